"""The FD sweep's Newton loops leave once their state repeats (ILQG_NT_REPLAY,
dcoop_impl.h): the records, and everything computed from them, stay the bits
the oracle computes by running every iteration up to the cap.

One shape throughout: hopper, 2 seeds (workloads.hopper_dmain(m, 2,
sigma=0.01)), H = 20, 8 line-search candidates, min-cost selection, two
iterations.  The first test shows on the CPU oracle that the second
iteration's sweep does contain replayed iterations, so the GPU comparisons
below are not vacuous.  Every GPU comparison is bit for bit.

fp32: the oracle is fp64 and cannot check the fp32 sweep bit for bit; the
switch test compares ILQG_NT_REPLAY=0 against 1 there.  Whether the rule fires
in fp32 at all is not visible from a test: it comes from the diagnostic
build's counters (tools/stamps.py, "Newton iterations skipped").
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, model_path

S, H, ITERS = 2, 20, 2
P = H + 1


def exact(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b, equal_nan=True):
        raise AssertionError(f"{what}: not bit-exact, max|diff|={np.nanmax(np.abs(a - b)):.3e}")


def test_oracle_sweep_has_replays(tmp_path):
    """Vacuity guard (CPU): the study library (the oracle's sources with
    -DORA_NT_STUDY and tools/ls_study/replay_study.c) over this file's shape;
    the second iteration's sweep contains at least one replayed iteration.
    Measured with this detector: 3,936 period-1 and 72 period-2 replays of
    9,096 iterations, 146 of 157 capped solves frozen.  It sees jar, Jv and
    alpha only, so it also counts steps that leave jar alone and still move
    qacc; the full (qacc, Ma, jar) comparison of an instrumented oracle gave
    2,882, 70 and 110 of 157."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "ls_study"))
    try:
        import replay_run
    finally:
        sys.path.pop(0)
    lib = replay_run.build(str(tmp_path / "liboracle_replaystudy.so"))
    rows = replay_run.sweep_counts(S, ITERS, H, lib)
    print(rows)
    second = rows[1]
    assert second["newton_iterations"] > 0
    assert second["period1_replays"] + second["period2_replays"] > 0, second


# ---- GPU ----------------------------------------------------------------

def _alphas():
    import workloads
    return workloads.LINESEARCH_ALPHAS


def _oracle_run(ora, om, dmain, s):
    om.lib.L.ora_set_nthread(1)
    d = om.make_data()
    d.set_state(time=dmain.time[s], qpos=dmain.qpos[s], qvel=dmain.qvel[s], warm=dmain.warm[s], ctrl=dmain.ctrl[s])
    il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
    il.set_dinit(d)
    for _ in range(ITERS):
        oc, osel = il.iterate_ls(_alphas(), "min_cost")
    return dict(traj=il.traj(), arr=il.arrays(), costs=oc, sel=osel)


def _gpu_run(ia, m, dmain, fdprec=None):
    g = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=_alphas(), select="min_cost")
    if fdprec:
        g.set_fd_precision(fdprec)
    for _ in range(ITERS):
        g.iterate()
    g.synchronize()
    V, v = g.value()
    K, k = g.gains()
    c, sel = g.costs()
    return dict(traj=g.traj(), deriv=g.deriv().copy(), K=K.copy(), k=k.copy(), V=V.copy(), v=v.copy(),
                costs=c.copy(), sel=sel.copy())


def _compare(run, refs):
    gt = run["traj"]
    for s, ref in enumerate(refs):
        ot, oa = ref["traj"], ref["arr"]
        for f in ("time", "qpos", "qvel", "warm", "ctrl"):
            exact(getattr(gt, f)[s * P:(s + 1) * P].reshape(ot[f].shape), ot[f], f"seed {s} traj.{f}")
        exact(run["deriv"][s], oa["deriv"], f"seed {s} records")
        for n in ("K", "k", "V", "v"):
            exact(run[n][s], oa[n], f"seed {s} {n}")
        exact(run["costs"][s], ref["costs"], f"seed {s} candidate costs")
        assert int(run["sel"][s]) == ref["sel"], (s, int(run["sel"][s]), ref["sel"])


@pytest.fixture(scope="module")
def hopper(ia, ora):
    """the bundled hopper: model, oracle model, start states and the oracle's two
    line-search iterations per seed (computed once, read-only)"""
    import workloads
    m = ia.Model.load(model_path("hopper"))
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(ia.HOPPER_COST, m.nq, m.nv, m.nu))
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    refs = [_oracle_run(ora, om, dmain, s) for s in range(S)]
    return m, om, dmain, refs


@pytest.mark.gpu
def test_fused_sweep_matches_oracle(ia, hopper):
    """the fused sweep (k_fd_fused_g, the compile-time hopper: fwd_constraint_u)"""
    m, om, dmain, refs = hopper
    assert m.static_id() != 0
    _compare(_gpu_run(ia, m, dmain), refs)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_fd_batch_matches_oracle(ia, ora, hopper, monkeypatch, fused):
    """ilqg_fd_batch on the 42 nominal points of the second iteration's sweep
    against ora_calcMJDerivatives: through the one-point fused launch, and
    (ILQG_FUSED=0) through the centre and column kernels"""
    m, om, dmain, refs = hopper
    monkeypatch.setenv("ILQG_FUSED", fused)
    tr = {f: np.concatenate([r["traj"][f] for r in refs]) for f in ("time", "qpos", "qvel", "warm", "ctrl")}
    st = ia.State(tr["time"], tr["qpos"], tr["qvel"], tr["warm"], tr["ctrl"])
    assert st.qpos.shape[0] == S * P == 42
    der = m.calc_derivatives(st, ia.HOPPER_COST)
    for i in range(S * P):
        d = om.make_data()
        d.set_state(qpos=st.qpos[i], qvel=st.qvel[i], warm=st.warm[i], ctrl=st.ctrl[i])
        exact(der[i], ora.calc_derivatives(om, d, cost_fn="ora_cost_desc_fn", nthread=1), f"point {i}")


@pytest.mark.gpu
def test_generic_kernels_match_oracle(ia, ora):
    """the same check on a model outside the compiled specialisations (the
    hopper on a frictionless floor): the generic kernels, fwd_constraint_fast"""
    import workloads
    with open(model_path("hopper")) as f:
        xml = f.read().replace('condim="3" name="floor"', 'condim="1" name="floor"')
    m = ia.Model.from_string(xml)
    assert m.static_id() == 0
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(ia.HOPPER_COST, m.nq, m.nv, m.nu))
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    refs = [_oracle_run(ora, om, dmain, s) for s in range(S)]
    _compare(_gpu_run(ia, m, dmain), refs)


@pytest.mark.gpu
def test_switch_hopper_fp64(ia, hopper, monkeypatch):
    """ILQG_NT_REPLAY=0 (every iteration runs) against 1, read at solver
    creation: the fused fp64 sweep's records and all that follows, bit for bit"""
    m, om, dmain, refs = hopper
    runs = {}
    for v in ("0", "1"):
        monkeypatch.setenv("ILQG_NT_REPLAY", v)
        runs[v] = _gpu_run(ia, m, dmain)
    for n in ("deriv", "K", "k", "V", "v", "costs", "sel"):
        exact(runs["0"][n], runs["1"][n], n)
    exact(runs["0"]["traj"].qpos, runs["1"]["traj"].qpos, "traj.qpos")
    _compare(runs["0"], refs)


@pytest.mark.gpu
def test_switch_humanoid_fp32(ia, monkeypatch):
    """the same switch on the fp32 FD sweep (humanoid, cfg 5's state, H = 10, one
    iteration; solver_newton with real = float): records bit-identical"""
    m = ia.Model.load(model_path("humanoid"))
    st = m.reset_state(1)
    st.qpos[0, 2] = 1.4
    rec = {}
    for v in ("0", "1"):
        monkeypatch.setenv("ILQG_NT_REPLAY", v)
        g = ia.ILQR(m, st, 10, ia.HUMANOID_COST)
        g.set_fd_precision("f32")
        g.iterate()
        g.synchronize()
        rec[v] = (g.deriv().copy(), g.gains()[0].copy())
    assert np.all(np.isfinite(rec["1"][0]))
    exact(rec["0"][0], rec["1"][0], "fp32 records")
    exact(rec["0"][1], rec["1"][1], "K")

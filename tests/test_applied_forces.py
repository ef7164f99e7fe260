"""qfrc_applied and xfrc_applied ("per-seed constants", include/ilqg_amd.h) through
every solver path, per seed, bit for bit against the oracle, whose physics
test_physics_reference.py holds to the independent longdouble reference with
the same kinds of forces.

The force sets (tests/applied_forces.py) give each of the four seeds of a solver
another kind of load -- none, qfrc_applied, xfrc_applied, both -- so one launch
has workgroups on the register fast paths of the compile-time models beside
workgroups on the general path, and a seed that reads another seed's forces gets
another trajectory.  The unmarked tests show on the oracle alone that every set
moves the trajectory and every block of the FD records, and that the world
body's row moves nothing.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import applied_forces as af
import cost_sched_ref as csr
from conftest import ROOT
from test_gpu_parity import FD32_EPS, MFMA_RTOL, _fd32_stats, _rel, exact, random_states

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ CPU: the inputs
_cpu = {}


def _hopper_oracle(ia, ora):
    """the oracle's iterate_ls on the hopper's four states, H = 6, 4 alphas, with the
    forces of every row of the set and with the world-only variant"""
    if not _cpu:
        m, om = af.oracle_model(ia, ora, "hopper")
        sts = af.hopper_states_oracle(ora, om, 4)
        qf, xf = af.force_set("hopper")
        wq, wx = af.world_only("hopper")

        def one(state, q, x):
            il = af.oracle_solver(ora, om, state, q, x, 6)
            return af.oracle_iterate(il, af.ALPHAS4, "min_cost"), il
        for s, state in enumerate(sts):
            for r in range(4):
                _cpu[s, r] = one(state, qf[r], xf[r])
            _cpu[s, "world"] = one(state, wq[s], wx[s])
        _cpu["m"] = m
    return _cpu


def test_every_force_set_moves_the_oracle(ia, ora):
    """hopper in contact, H = 6: against zero forces on the same state, every loaded
    row changes qpos at point 0 and entries of all three FD blocks (dq, dv, du);
    forces on the world body alone change nothing"""
    c = _hopper_oracle(ia, ora)
    m = c["m"]
    nv, nu = m.nv, m.nu
    blocks = {"dq": slice(0, nv * nv), "dv": slice(nv * nv, 2 * nv * nv), "du": slice(2 * nv * nv, 2 * nv * nv + nv * nu)}
    qf, xf = af.force_set("hopper")
    assert not qf[0].any() and not xf[0].any()
    assert qf[1].all() and not xf[1].any()
    assert not qf[2].any() and np.count_nonzero(np.any(xf[2] != 0, axis=1)) == 2 and not xf[2, 0].any()
    assert qf[3].all() and xf[3, 0].all() and xf[3, -1].all() and not xf[3, 1:-1].any()
    assert np.any(np.signbit(xf[3]) & (xf[3] == 0)), "the -0.0 entry"
    for s in range(4):
        zero = c[s, 0][0]
        for r in (1, 2, 3):
            got = c[s, r][0]
            assert not np.array_equal(got["qpos"][0], zero["qpos"][0]), (s, r)
            for b, sl in blocks.items():
                assert not np.array_equal(got["deriv"][:, sl], zero["deriv"][:, sl]), (s, r, b)
        for f in af.FIELDS:
            exact(c[s, "world"][0][f], zero[f], f"world-only forces, state {s}: {f}")


def test_oracle_points_carry_the_forces(ia, ora):
    """after iterate_ls every point of the oracle's trajectory still holds dmain's two arrays"""
    c = _hopper_oracle(ia, ora)
    qf, xf = af.force_set("hopper")
    for s in range(4):
        for r in range(4):
            il = c[s, r][1]
            for n in range(il.N + 1):
                pt = il.point(n)
                exact(pt.arr("qfrc_applied"), qf[r], f"state {s} row {r} point {n}: qfrc_applied")
                exact(pt.xfrc(), xf[r].ravel(), f"state {s} row {r} point {n}: xfrc_applied")
                assert np.array_equal(np.signbit(pt.xfrc()), np.signbit(xf[r].ravel()))


def test_humanoid_set_reaches_the_second_load_word(ia):
    """a loaded body of the humanoid's row 2 lies past the 64th double of its xfrc_applied"""
    _, xf = af.force_set("humanoid")
    assert xf.shape[1] * 6 > 64
    assert np.flatnonzero(xf[2].ravel()).max() >= 64 and np.flatnonzero(xf[3].ravel()).max() >= 64


# ------------------------------------------------------------------ GPU
def _same(dev, s, ref, what, fields=af.FIELDS):
    for f in fields:
        exact(dev[f][s], ref[f], f"{what}: {f}")


def _same_all(a, b, what, fields=None):
    for f in fields or a.keys():
        exact(a[f], b[f], f"{what}: {f}")


@gpu
@pytest.mark.parametrize("env", [{}, {"ILQG_FUSED": "0"}], ids=["built", "unfused"])
@pytest.mark.parametrize("name", af.MODELS)
def test_fd_batch(ia, ora, name, env, monkeypatch):
    """Model.calc_derivatives with forces against the oracle's calcMJDerivatives on an
    mjData that carries them: pendulum and chain in motion, hopper and humanoid
    (60 steps fallen) in contact; the fused sweep's one-point trajectories and
    the two-kernel sweep"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, om = af.oracle_model(ia, ora, name)
    if name == "humanoid":
        n = len(af.ROWS[name])
        st = m.reset_state(1)
        m.step(st, 60)
        st = random_states(m, n, np.random.default_rng(17), 0.01, af.sub(ia, st, [0] * n))
        q = st.qpos[:, 3:7]
        st.qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    else:
        st = af.states(ia, m, name)
    qf, xf = af.forces(name)
    c = af.cost(ia, name)
    der = m.calc_derivatives(st, c, qf, xf)
    zero = m.calc_derivatives(st, c)
    for i in range(st.qpos.shape[0]):
        d = af.oracle_data(om, dict(qpos=st.qpos[i], qvel=st.qvel[i], warm=st.warm[i], ctrl=st.ctrl[i]), qf[i], xf[i])
        exact(der[i], ora.calc_derivatives(om, d, cost_fn="ora_cost_desc_fn", nthread=1), f"{name} deriv[{i}]")
        assert (qf[i].any() or xf[i, 1:].any()) == (not np.array_equal(der[i], zero[i])), i


_oracle, _device = {}, {}


def _oracle_run(ia, ora, name):
    """the oracle's two iterations of every seed with its forces, computed once"""
    if name not in _oracle:
        m = af.model(ia, name)
        st = af.states(ia, m, name)
        qf, xf = af.forces(name)
        _oracle[name] = af.oracle_run(ia, ora, name, st, qf, xf, m=m)
    return _oracle[name]


def _device_run(ia, name):
    """the device's two iterations as built, no variable set, computed once"""
    if name not in _device:
        qf, xf = af.forces(name)
        _device[name] = af.run(ia, name, qf, xf)
    return _device[name]


def _child_run(name, env, tmp_path):
    """applied_forces.py in a process of its own under env"""
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "applied_forces.py"), name, out],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        return [{f: z[f"{f}{it}"] for f in af.FIELDS} for it in range(af.ITERS)]


@gpu
@pytest.mark.parametrize("name,env", [("inverted_pendulum", {}), ("hopper", {}), ("hopper", {"ILQG_FUSED": "0"}),
                                      ("hopper", {"ILQG_SNAP_POISON": "1"}), ("hopper", {"ILQG_DUAL": "0"}),
                                      ("chain", {})],
                         ids=["pendulum", "hopper", "hopper-unfused", "hopper-poison", "hopper-onewave", "chain"])
def test_iterate(ia, ora, name, env, monkeypatch, tmp_path):
    """4 seeds x 4 alphas, min-cost selection, two iterate() calls: after each, every
    seed's candidate costs, selection, trajectory, FD records, K, k, V, v are those
    of an oracle solver whose dmain carries that seed's forces.  The hopper also
    through the two-kernel sweep, with the snapshot's gaps poisoned, and on the
    one-wave rollout kernels (ILQG_DUAL=0, read once per process: a child)"""
    ref = _oracle_run(ia, ora, name)
    if "ILQG_DUAL" in env:
        dev = _child_run(name, env, tmp_path)
    elif env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dev = af.run(ia, name, *af.forces(name))
    else:
        dev = _device_run(ia, name)
    for it in range(af.ITERS):
        for s in range(len(af.ROWS[name])):
            _same(dev[it], s, ref[it][s], f"{name} iteration {it} seed {s}")
    # the loaded seeds are not the unloaded ones' copies
    zero = af.oracle_run(ia, ora, name, af.sub(ia, af.states(ia, af.model(ia, name), name), [1, 2, 3]), None, None,
                         iters=1)
    for s in (1, 2, 3):
        assert not np.array_equal(dev[0]["qpos"][s], zero[0][s - 1]["qpos"]), s


@gpu
def test_world_only_is_zero_force(ia):
    """xfrc_applied on body 0 alone: the results of a solver created without forces"""
    name = "hopper"
    a = af.run(ia, name, *af.world_only(name))
    b = af.run(ia, name, None, None)
    for it in range(af.ITERS):
        _same_all(a[it], b[it], f"iteration {it}")


@gpu
@pytest.mark.parametrize("G", [2, 3])
def test_seed_groups(ia, G):
    """hopper, 4 seeds as G ranges (G = 3: 1, 1, 2): the ungrouped solver's bits"""
    name = "hopper"
    ref = _device_run(ia, name)
    dev = af.run(ia, name, *af.forces(name), prepare=lambda g: g.set_groups(G))
    for it in range(af.ITERS):
        _same_all(dev[it], ref[it], f"G = {G} iteration {it}")


@gpu
@pytest.mark.parametrize("engine,chunk", [("exact", 0), ("exact", 3), ("mfma", 3)])
def test_humanoid_solver(ia, ora, engine, chunk, monkeypatch):
    """humanoid standing at z = 1.4, 2 seeds with rows 2 and 3 of its set (both load a
    body past the 64th double of xfrc_applied), H = 6.  The exact engine, unchunked
    and through the pipelined iterate in chunks of 3 points (two resumes from the
    carried state), two iterations: everything bit for bit.  The MFMA engine,
    pipelined, one iteration: trajectory and records bit for bit, gains and value
    within MFMA_RTOL"""
    name = "humanoid"
    monkeypatch.setenv("ILQG_PIPE_CHUNK", str(chunk))
    ref = _oracle_run(ia, ora, name)
    iters = 1 if engine == "mfma" else af.ITERS
    dev = af.run(ia, name, *af.forces(name), iters=iters, prepare=lambda g: g.set_riccati(engine))
    for it in range(iters):
        for s in range(2):
            what = f"humanoid {engine} chunk {chunk} iteration {it} seed {s}"
            if engine == "exact":
                _same(dev[it], s, ref[it][s], what)
                continue
            _same(dev[it], s, ref[it][s], what, ("costs", "sel", "qpos", "qvel", "warm", "ctrl", "deriv"))
            errs = {f: _rel(dev[it][f][s], ref[it][s][f]) for f in ("K", "k", "V", "v")}
            print(what, "MFMA deviation", errs)
            assert all(e <= MFMA_RTOL for e in errs.values()), errs
    assert not np.array_equal(dev[0]["deriv"][0], dev[0]["deriv"][1])   # same state, other forces


@gpu
@pytest.mark.parametrize("name", ["humanoid", "hopper"])
def test_range_and_sharded(ia, ora, name, monkeypatch):
    """One candidate per seed.  The whole sweep's records are the oracle's; the point
    blocks [0,1), [1,4), [4,P) of ilqg_fd_sweep_range write the same records, and so
    do the three ranks of ilqg_forward_sharded (chunks of 3 points) on the points
    each owns.  The last seed's records are not the ones its state gives with the
    first seed's forces (oracle): each seed's launch reads its own"""
    m = af.model(ia, name)
    st = af.states(ia, m, name)
    qf, xf = af.forces(name)
    S, P, H = st.qpos.shape[0], af.HORIZON[name] + 1, af.HORIZON[name]
    mk = lambda: af.solver(ia, m, name, st, qf, xf, alphas=(1.0,), select="reference")
    g = mk()
    g.forward_pass()
    g.fd_sweep()
    g.synchronize()
    D_full = g.deriv()
    _, om = af.oracle_model(ia, ora, name, m)
    for s in range(S):
        il = af.oracle_solver(ora, om, af.state_dict(st, s), qf[s], xf[s], H)
        il.iterate()
        exact(D_full[s], il.arrays()["deriv"], f"{name} seed {s}: the whole sweep against the oracle")
    il = af.oracle_solver(ora, om, af.state_dict(st, S - 1), qf[0], xf[0], H)
    il.iterate()
    assert not np.array_equal(D_full[S - 1], il.arrays()["deriv"])
    g.set_deriv(np.full_like(D_full, np.nan))
    for p0, p1 in ((0, 1), (1, 4), (4, P)):
        g.fd_sweep_range(p0, p1 - p0)
    g.synchronize()
    exact(g.deriv(), D_full, f"{name}: 3 blocks against the whole sweep")
    # the sharded, pipelined iteration: the unfused sweep behind rollout chunks
    monkeypatch.setenv("ILQG_PIPE_CHUNK", "3")
    monkeypatch.setenv("ILQG_FUSED", "0")
    world = 3
    ranks = [mk() for _ in range(world)]
    owner = ranks[0].point_owners(world)
    assert set(owner) == set(range(world))
    gathered = np.full_like(D_full, np.nan)
    for r, h in enumerate(ranks):
        h.set_deriv(np.full_like(D_full, np.nan))
        h.forward_sharded(r, world)
        h.synchronize()
        D, mine = h.deriv(), owner == r
        exact(D[:, mine], D_full[:, mine], f"{name}: rank {r}'s points")
        assert np.isnan(D[:, ~mine]).all(), f"{name}: rank {r} wrote points it does not own"
        exact(h.traj().qpos, g.traj().qpos, f"{name}: rank {r}'s trajectory")
        gathered[:, mine] = D[:, mine]
    exact(gathered, D_full, f"{name}: the ranks' records together")


def _stats(d, dref):
    e = np.abs(d - dref) / (1 + np.abs(dref))
    return dict(median=float(np.median(e)), p99=float(np.quantile(e, 0.99)), frac_big=float(np.mean(e > 0.1)),
                max=float(e.max()))


@gpu
@pytest.mark.parametrize("name", ["humanoid", "hopper"])
def test_fp32_sweep(ia, ora, name):
    """The fp32 sweep (load_state32's own casts of both arrays), one iterate().  Without
    a tolerance: seed s's records are those of a one-seed solver with its state and
    forces, and those at the mirrored index of the solver with seeds and forces
    reversed; the rollout ahead of the sweep is the fp64 oracle's bit for bit.
    Against the fp64 oracle at eps 1e-3 with the same forces:
    test_gpu_parity's _fd32_stats and its bounds, over all seeds' records.
    Measured on the MI355X (median, p99, fraction > 0.1, max), with / without forces:
      humanoid  8.4e-5, 3.8e-2, 1.8e-3, 0.38  /  6.4e-5, 3.7e-2, 1.4e-3, 0.26
      hopper    4.1e-5, 3.8e-3, 0, 2.2e-2     /  4.0e-5, 3.8e-3, 0, 1.4e-2
    (bounds: median 5e-4, p99 0.085, fraction 5.5e-3): the forces change nothing
    of note"""
    m = af.model(ia, name)
    st = af.states(ia, m, name)
    qf, xf = af.forces(name)
    S = st.qpos.shape[0]
    f32 = lambda g: g.set_fd_precision("f32")
    whole = lambda st_, q, x: af.run(ia, name, q, x, iters=1, prepare=f32, st=st_, m=m)[0]
    one = lambda st_, q, x: whole(st_, q, x)["deriv"]
    R = whole(st, qf, xf)
    D = R["deriv"]
    for s in range(S):
        exact(one(af.sub(ia, st, s), qf[s:s + 1], xf[s:s + 1])[0], D[s], f"{name} seed {s} alone")
    rev = list(range(S))[::-1]
    Dr = one(af.sub(ia, st, rev), qf[rev], xf[rev])
    exact(Dr[::-1], D, f"{name}: seeds and forces reversed")
    D0 = one(st, None, None)
    _, om = af.oracle_model(ia, ora, name, m)
    om.lib.L.ora_set_fd_eps(FD32_EPS)
    try:
        ref = af.oracle_run(ia, ora, name, st, qf, xf, iters=1, m=m)[0]
        O = np.stack([r["deriv"] for r in ref])
        O0 = np.stack([r["deriv"] for r in af.oracle_run(ia, ora, name, st, None, None, iters=1, m=m)[0]])
    finally:
        om.lib.L.ora_set_fd_eps(1e-6)
    for s in range(S):   # the rollout ahead of the sweep is the fp64 one
        _same(R, s, ref[s], f"{name} seed {s}", ("costs", "sel", "qpos", "qvel", "warm", "ctrl"))
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(D0))
    print(f"{name} fp32 FD against the fp64 oracle, with forces    {_stats(D, O)}")
    print(f"{name} fp32 FD against the fp64 oracle, without forces {_stats(D0, O0)}")
    _fd32_stats(f"{name} without forces", D0, O0)
    _fd32_stats(f"{name} with forces", D, O)


def _compose(ia, g, m, cfg):
    if cfg == "limits":
        g.set_ctrl_limits("model")
        return
    if cfg == "schedule_standard":
        g.set_layout("corrected")
    g.set_cost_schedule(csr.make_schedule(ia.HOPPER_COST, m, g.N))
    if cfg == "schedule_standard":
        g.set_recursion("standard")


@gpu
@pytest.mark.parametrize("cfg", ["limits", "schedule", "schedule_standard"])
def test_composition(ia, cfg):
    """hopper, 4 seeds, H = 8, mu = 1000, two iterations with control limits (the
    model's ctrlrange), a cost schedule, and the schedule with the corrected layout
    and the standard recursion: the clamp / sched instances of the rollout and the
    sweep and the other backward kernels.  Every result of seed s is a one-seed
    solver's with that seed's state and forces, and not the one its state gives
    without forces"""
    name = "hopper"
    m = af.model(ia, name)
    st = af.states(ia, m, name)
    qf, xf = af.forces(name)
    prep = lambda g: _compose(ia, g, m, cfg)
    multi = af.run(ia, name, qf, xf, prepare=prep, st=st, m=m)
    for s in range(4):
        one = af.run(ia, name, qf[s:s + 1], xf[s:s + 1], prepare=prep, st=af.sub(ia, st, s), m=m)
        for it in range(af.ITERS):
            for f in multi[it]:
                exact(multi[it][f][s], one[it][f][0], f"{cfg} iteration {it} seed {s}: {f}")
        if s:
            zero = af.run(ia, name, None, None, prepare=prep, st=af.sub(ia, st, s), m=m)
            for it in range(af.ITERS):   # (iteration 0's rollout has zero gains: the forces alone)
                for f in ("qpos", "deriv", "K"):
                    assert not np.array_equal(multi[it][f][s], zero[it][f][0]), (it, s, f)
    if cfg == "schedule_standard":
        assert multi[-1]["dV"].any()


@gpu
def test_reinit_null_forces_means_zero(ia):
    """ilqg_solver_init again on a solver created with forces, now with NULL force
    pointers ("applied forces may be NULL (zero)"): a fresh zero-force solver's
    results.  Failed before ilqg_solver_init zeroed the arrays for NULL: the
    solver kept the forces of its first initialisation"""
    name = "hopper"
    m = af.model(ia, name)
    st = af.states(ia, m, name)
    g = af.solver(ia, m, name, st, *af.forces(name))
    p = ia._ptr
    rc = ia.lib().ilqg_solver_init(g._h, p(st.time), p(st.qpos), p(st.qvel), p(st.warm), p(st.ctrl),
                                   ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_double)())
    assert rc == 0
    g.iterate()
    got = af.results(g)
    want = af.run(ia, name, None, None, iters=1, st=st, m=m)[0]
    _same_all(got, want, "re-initialised with NULL forces")

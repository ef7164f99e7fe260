"""HIP path vs the CPU oracle on the same seeded inputs, through the C ABI.

Tolerance contract (north star: "matching the reference CPU path to a stated
fp64 tolerance"): the device code follows the oracle's operation order with
FMA contraction off, so the stated tolerance is ZERO -- every comparison below
is bit-exact (np.array_equal).  SURVEY.md §8d's looser budgets (FD 1e-7 /
1e-5 relative, Riccati 1e-12) are therefore met with margin.
"""
import numpy as np
import pytest

from conftest import load_golden, model_path

pytestmark = pytest.mark.gpu


def exact(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b, equal_nan=True):
        err = np.nanmax(np.abs(a - b))
        raise AssertionError(f"{what}: not bit-exact, max|diff|={err:.3e}")


def setup(ia, ora, name, cost=None):
    m = ia.Model.load(model_path(name))
    om = ora.OModel(m.blob())
    if cost is not None:
        om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(cost, m.nq, m.nv, m.nu))
    return m, om


def random_states(m, n, rng, scale=0.05, base=None):
    st = m.reset_state(n) if base is None else base
    st.qpos = st.qpos + rng.normal(0, scale, st.qpos.shape)
    st.qvel = st.qvel + rng.normal(0, scale, st.qvel.shape)
    st.ctrl = st.ctrl + rng.normal(0, 0.3, st.ctrl.shape)
    return st


def oracle_steps(om, st, nstep):
    out = st.copy()
    for i in range(st.qpos.shape[0]):
        d = om.make_data()
        d.set_state(time=st.time[i], qpos=st.qpos[i], qvel=st.qvel[i], warm=st.warm[i], ctrl=st.ctrl[i])
        d.step(nstep)
        s = d.state()
        out.time[i], out.qpos[i], out.qvel[i], out.warm[i] = s["time"], s["qpos"], s["qvel"], s["warm"]
    return out


@pytest.mark.parametrize("name,nstep", [("inverted_pendulum", 25), ("hopper", 60), ("humanoid", 20)])
def test_step_batch_bitexact(ia, ora, name, nstep):
    m, om = setup(ia, ora, name)
    rng = np.random.default_rng(11)
    base = m.reset_state(1)
    m.step(base, 50)  # get into contact / motion first
    st = random_states(m, 24, rng, base=ia.State(*(np.repeat(getattr(base, k), 24, 0) for k in
                                                    ("time", "qpos", "qvel", "warm", "ctrl"))))
    ref = oracle_steps(om, st, nstep)
    m.step(st, nstep)
    for k in ("time", "qpos", "qvel", "warm"):
        exact(getattr(st, k), getattr(ref, k), f"{name} {k}")


@pytest.mark.parametrize("name", ["inverted_pendulum", "hopper", "humanoid"])
def test_forward_batch_bitexact(ia, ora, name):
    m, om = setup(ia, ora, name)
    rng = np.random.default_rng(5)
    st = m.reset_state(1)
    m.step(st, 100)
    sts = random_states(m, 16, rng, 0.02, ia.State(*(np.repeat(getattr(st, k), 16, 0) for k in
                                                     ("time", "qpos", "qvel", "warm", "ctrl"))))
    qacc = m.forward(sts.copy())
    for i in range(16):
        d = om.make_data()
        d.set_state(qpos=sts.qpos[i], qvel=sts.qvel[i], warm=sts.warm[i], ctrl=sts.ctrl[i])
        d.forward()
        exact(qacc[i], d.arr("qacc"), f"{name} qacc[{i}]")


@pytest.mark.parametrize("fixture,cost", [("fd_pendulum.npz", "PENDULUM"), ("fd_hopper.npz", "HOPPER"),
                                          ("fd_hopper_dummycost.npz", "DUMMY")])
def test_fd_batch_vs_reference_golden(ia, fixture, cost):
    """GPU FD sweep == vectors written by the reference's own calcMJDerivatives"""
    g = load_golden(fixture)
    m = ia.Model.load(model_path(str(g["model"])))
    c = {"PENDULUM": ia.PENDULUM_COST, "HOPPER": ia.HOPPER_COST, "DUMMY": ia.Cost(lq=[1.0])}[cost]
    st = ia.State(g["time"], g["qpos"], g["qvel"], g["warm"], g["ctrl"])
    exact(m.calc_derivatives(st, c), g["deriv"], fixture)


@pytest.mark.parametrize("name,cost,cfn", [("inverted_pendulum", "PENDULUM_COST", "ora_cost_pendulum"),
                                           ("hopper", "HOPPER_COST", "ora_cost_desc_fn"),
                                           ("humanoid", None, "ora_cost_desc_fn")])
def test_fd_batch_vs_oracle(ia, ora, name, cost, cfn):
    c = getattr(ia, cost) if cost else ia.Cost(wq=[1.0] * 28, wv=[0.1] * 27, wu=[0.01] * 21)
    m, om = setup(ia, ora, name, c)
    rng = np.random.default_rng(17)
    st = m.reset_state(1)
    m.step(st, 200 if name != "humanoid" else 60)  # humanoid falls onto the floor: contacts
    n = 8
    sts = random_states(m, n, rng, 0.01, ia.State(*(np.repeat(getattr(st, k), n, 0) for k in
                                                    ("time", "qpos", "qvel", "warm", "ctrl"))))
    if name == "humanoid":  # keep the free-joint quaternion normalised
        q = sts.qpos[:, 3:7]
        sts.qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    der = m.calc_derivatives(sts, c)
    for i in range(n):
        d = om.make_data()
        d.set_state(qpos=sts.qpos[i], qvel=sts.qvel[i], warm=sts.warm[i], ctrl=sts.ctrl[i])
        exact(der[i], ora.calc_derivatives(om, d, cost_fn=cfn, nthread=1), f"{name} deriv[{i}]")


def _oracle_ilqr(ora, om, dstate, H, cfn, iters):
    d = om.make_data()
    d.set_state(**dstate)
    il = ora.OILQR(om, d, H, cost_fn=cfn)
    il.set_dinit(d)
    for _ in range(iters):
        il.iterate()
    return il


def _state_dict(st, i):
    return dict(time=st.time[i], qpos=st.qpos[i], qvel=st.qvel[i], warm=st.warm[i], ctrl=st.ctrl[i])


@pytest.mark.parametrize("name,H,iters", [("inverted_pendulum", 20, 3), ("inverted_pendulum", 100, 2),
                                          ("inverted_pendulum", 200, 2), ("hopper", 500, 2)])
def test_iterate_bitexact(ia, ora, name, H, iters):
    """ILQR::iterate() (forwardPass; setDInit; backwardPass) -- trajectory, gains, value"""
    import workloads
    cost = ia.PENDULUM_COST if name == "inverted_pendulum" else ia.HOPPER_COST
    cfn = "ora_cost_pendulum" if name == "inverted_pendulum" else "ora_cost_desc_fn"
    m, om = setup(ia, ora, name, cost)
    dmain = workloads.pendulum_dmain(m) if name == "inverted_pendulum" else workloads.hopper_dmain(m)
    il = _oracle_ilqr(ora, om, _state_dict(dmain, 0), H, cfn, iters)
    g = ia.ILQR(m, dmain, H, cost)
    for _ in range(iters):
        g.iterate()
    g.synchronize()
    ot, oa, gt = il.traj(), il.arrays(), g.traj()
    for k in ("time", "qpos", "qvel", "warm", "ctrl"):
        exact(getattr(gt, k).reshape(ot[k].shape), ot[k], f"traj.{k}")
    K, k = g.gains()
    exact(K[0], oa["K"], "K")
    exact(k[0], oa["k"], "k")
    exact(g.deriv()[0], oa["deriv"], "deriv")
    V, v = g.value()
    exact(V[0], oa["V"], "V")
    exact(v[0], oa["v"], "v")


def test_multiseed_each_seed_matches_oracle(ia, ora):
    """cfg-4 style seeds (splitmix64 + Box-Muller perturbations): seeds are independent"""
    import workloads
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    S, H = 4, 60
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    g = ia.ILQR(m, dmain, H, ia.HOPPER_COST)
    g.iterate()
    g.iterate()
    g.synchronize()
    gt = g.traj()
    K, k = g.gains()
    P = H + 1
    for s in range(S):
        il = _oracle_ilqr(ora, om, _state_dict(dmain, s), H, "ora_cost_desc_fn", 2)
        exact(gt.qpos[s * P:(s + 1) * P], il.traj()["qpos"], f"seed {s} qpos")
        exact(K[s], il.arrays()["K"], f"seed {s} K")


def _traj_cost(cost, m, traj):
    """sum over n = N..0 of stepCost(x_n, u_n), accumulated in rollout order"""
    p = cost.packed(m.nq, m.nv, m.nu)
    c = 0.0
    for n in range(len(traj["time"]) - 1, -1, -1):
        s = 0.0
        for x, w, t, l in ((traj["qpos"][n], p["wq"], p["tq"], p["lq"]), (traj["qvel"][n], p["wv"], p["tv"], p["lv"]),
                           (traj["ctrl"][n], p["wu"], p["tu"], p["lu"])):
            for i in range(len(x)):
                if w[i] != 0:
                    dx = float(x[i]) - float(t[i])
                    s += float(w[i]) * dx * dx
                if l[i] != 0:
                    s += float(l[i]) * float(x[i])
        c += s
    return c


def test_linesearch_candidates(ia, ora):
    """cfg 3: 8 candidates alpha = 2^-i; alpha = 1 reproduces the reference rollout exactly"""
    import workloads
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    H = 80
    dmain = workloads.hopper_dmain(m)
    ref = ia.ILQR(m, dmain, H, ia.HOPPER_COST)  # reference semantics, 1 candidate
    ls = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=workloads.LINESEARCH_ALPHAS, select="reference")
    best = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=workloads.LINESEARCH_ALPHAS, select="min_cost")
    for _ in range(3):
        for s in (ref, ls, best):
            s.iterate()
    for s in (ref, ls, best):
        s.synchronize()
    rt, lt = ref.traj(), ls.traj()
    for k in ("qpos", "qvel", "ctrl", "warm"):
        exact(getattr(lt, k), getattr(rt, k), f"alpha=1 candidate {k}")
    costs, sel = ls.costs()
    assert sel[0] == 0
    il = _oracle_ilqr(ora, om, _state_dict(dmain, 0), H, "ora_cost_desc_fn", 3)
    # the third forward pass rolled out with the gains of the second iteration: its
    # alpha=1 cost equals the oracle's trajectory cost after 3 iterations
    assert costs[0, 0] == _traj_cost(ia.HOPPER_COST, m, il.traj())
    bc, bsel = best.costs()
    assert bc[0, bsel[0]] == bc[0].min() and np.all(np.isfinite(bc))


def test_full_size_properties(ia):
    """cfg 3/4 sizes (hopper H=500, 8 seeds x 8 candidates): finite, deterministic, argmin-consistent"""
    import workloads
    m = ia.Model.load(model_path("hopper"))
    dmain = workloads.hopper_dmain(m, 8, sigma=0.01)
    runs = []
    for _ in range(2):
        g = ia.ILQR(m, dmain, 500, ia.HOPPER_COST, alphas=workloads.LINESEARCH_ALPHAS, select="min_cost")
        g.iterate()
        g.iterate()
        g.synchronize()
        t = g.traj()
        c, sel = g.costs()
        runs.append((t.qpos.copy(), g.gains()[0].copy(), c.copy(), sel.copy()))
    exact(runs[0][0], runs[1][0], "determinism qpos")
    exact(runs[0][1], runs[1][1], "determinism K")
    assert np.all(np.isfinite(runs[0][0])) and np.all(np.isfinite(runs[0][1]))
    c, sel = runs[0][2], runs[0][3]
    assert np.all(c[np.arange(8), sel] == c.min(axis=1))


def test_edge_cases(ia, ora):
    """horizon 1, a NaN state (mj_checkPos reset semantics), zero-length-ish inputs"""
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    st = m.reset_state(2)
    st.qpos[1, 2] = np.nan
    ref = oracle_steps(om, st, 3)
    m.step(st, 3)
    exact(st.qpos, ref.qpos, "NaN reset qpos")
    assert np.all(np.isfinite(st.qpos))
    import workloads
    dmain = workloads.hopper_dmain(m)
    g = ia.ILQR(m, dmain, 1, ia.HOPPER_COST)
    g.iterate()
    g.synchronize()
    il = _oracle_ilqr(ora, om, _state_dict(dmain, 0), 1, "ora_cost_desc_fn", 1)
    exact(g.gains()[0][0], il.arrays()["K"], "H=1 K")
    with pytest.raises(ia.IlqgError):
        ia.ILQR(m, dmain, 0, ia.HOPPER_COST)


def test_generic_kernels_unbundled_model(ia, ora):
    """a model outside the compiled specialisations (hopper with a frictionless
    floor: different condim -> different key) runs the generic cooperative
    kernels and still matches the oracle bit for bit"""
    import workloads
    with open(model_path("hopper")) as f:
        xml = f.read().replace('condim="3" name="floor"', 'condim="1" name="floor"')
    m = ia.Model.from_string(xml)
    assert m.static_id() == 0
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(ia.HOPPER_COST, m.nq, m.nv, m.nu))
    dmain = workloads.hopper_dmain(m)
    il = _oracle_ilqr(ora, om, _state_dict(dmain, 0), 100, "ora_cost_desc_fn", 2)
    g = ia.ILQR(m, dmain, 100, ia.HOPPER_COST)
    g.iterate()
    g.iterate()
    g.synchronize()
    ot, oa, gt = il.traj(), il.arrays(), g.traj()
    exact(gt.qpos.reshape(ot["qpos"].shape), ot["qpos"], "traj.qpos")
    exact(g.gains()[0][0], oa["K"], "K")
    exact(g.deriv()[0], oa["deriv"], "deriv")


def test_humanoid_iterate_tangent_space(ia, ora):
    """humanoid iLQR (free joint, nq=28 != nv=27).  The
    state difference runs in the tangent space (quaternion dofs by the
    first-order log map, oracle ora_state_diff); FD, Riccati (nx=54, nu=21,
    unpadded LDS layout, FD records read from HBM) and rollout match the
    oracle bit for bit.  Parity vs a reference is unpinned by construction: the
    reference does not support nq != nv (inc/ilqr.h:90)."""
    m, om = setup(ia, ora, "humanoid", ia.HUMANOID_COST)
    st = m.reset_state(1)
    st.qpos[0, 2] = 1.4  # humanoid.xml:49-50 initial height
    m.step(st, 5)
    dstate = _state_dict(st, 0)
    il = _oracle_ilqr(ora, om, dstate, 6, "ora_cost_desc_fn", 1)
    g = ia.ILQR(m, st, 6, ia.HUMANOID_COST)
    g.iterate()
    g.synchronize()
    ot, oa, gt = il.traj(), il.arrays(), g.traj()
    for k in ("qpos", "qvel", "warm", "ctrl"):
        exact(getattr(gt, k).reshape(ot[k].shape), ot[k], f"traj.{k}")
    K, k = g.gains()
    exact(g.deriv()[0], oa["deriv"], "deriv")
    exact(K[0], oa["K"], "K")
    exact(k[0], oa["k"], "k")
    V, v = g.value()
    exact(V[0], oa["V"], "V")
    exact(v[0], oa["v"], "v")


def _humanoid_cfg5(ia, ora, H, iters, riccati, fdprec="f64"):
    """BASELINE.json configs[4] state: humanoid qpos0 standing at z = 1.4
    (humanoid.xml:49-50), qvel = 0, ctrl = 0; the GPU solver and the oracle
    iterate from it (fdprec "f32": the GPU's fp32 FD sweep at eps 1e-3, the
    oracle's fp64 FD at the same eps)"""
    m, om = setup(ia, ora, "humanoid", ia.HUMANOID_COST)
    st = m.reset_state(1)
    st.qpos[0, 2] = 1.4
    if fdprec == "f32":
        om.lib.L.ora_set_fd_eps(FD32_EPS)
    try:
        il = _oracle_ilqr(ora, om, _state_dict(st, 0), H, "ora_cost_desc_fn", iters)
    finally:
        om.lib.L.ora_set_fd_eps(1e-6)
    g = ia.ILQR(m, st, H, ia.HUMANOID_COST)
    g.set_riccati(riccati)
    g.set_fd_precision(fdprec)
    for _ in range(iters):
        g.iterate()
    g.synchronize()
    return g, il


def test_humanoid_cfg5_exact(ia, ora):
    """cfg 5 (humanoid, H = 200) on the cooperative kernels with the exact
    Riccati engine: two iterations, every trajectory field, FD record, K, k,
    V, v bit for bit against the oracle"""
    g, il = _humanoid_cfg5(ia, ora, 200, 2, "exact")
    ot, oa, gt = il.traj(), il.arrays(), g.traj()
    for k in ("qpos", "qvel", "warm", "ctrl"):
        exact(getattr(gt, k).reshape(ot[k].shape), ot[k], f"traj.{k}")
    K, k = g.gains()
    exact(g.deriv()[0], oa["deriv"], "deriv")
    exact(K[0], oa["K"], "K")
    exact(k[0], oa["k"], "k")
    V, v = g.value()
    exact(V[0], oa["V"], "V")
    exact(v[0], oa["v"], "v")


# MFMA Riccati tolerance: every matrix product sums in the matrix core's order,
# so each step's K, k, V, v differ from the oracle's by rounding (~1e-16
# relative), carried through the recursion; after one backward pass over
# H = 200 steps the gains and value function stay within 1e-9 relative to the
# largest entry of each array (SURVEY.md §8d asks 1e-12 per isolated step;
# tests/test_gpu_parity.py::test_riccati_mfma_step checks that)
MFMA_RTOL = 1e-9


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_humanoid_cfg5_mfma(ia, ora):
    """cfg 5 with the MFMA Riccati engine: one iteration (the FD records and
    the rollout before it are bit-exact; the backward pass runs on the matrix
    cores): K, k, V, v within MFMA_RTOL of the oracle"""
    g, il = _humanoid_cfg5(ia, ora, 200, 1, "mfma")
    oa = il.arrays()
    exact(g.deriv()[0], oa["deriv"], "deriv")
    K, k = g.gains()
    V, v = g.value()
    errs = {n: _rel(a, b) for n, a, b in (("K", K[0], oa["K"]), ("k", k[0], oa["k"]), ("V", V[0], oa["V"]),
                                          ("v", v[0], oa["v"]))}
    print("cfg5 MFMA Riccati max relative deviation:", errs)
    assert all(e <= MFMA_RTOL for e in errs.values()), errs


@pytest.mark.parametrize("fixture", ["riccati_pendulum.npz", "riccati_hopper.npz"])
def test_riccati_mfma_step(ia, fixture):
    """SURVEY.md §8d Riccati tolerance (rel <= 1e-12), stage-isolated: the MFMA
    engine on the committed Riccati fixtures (the oracle's K, k, V, v for
    seeded FD records and trajectory)"""
    g = load_golden(fixture)
    m = ia.Model.load(model_path(str(g["model"])))
    P = g["deriv"].shape[0]
    tr = _fixture_traj(ia, g, "traj_")
    s = ia.ILQR(m, ia.State(tr.time[:1], tr.qpos[:1], tr.qvel[:1], tr.warm[:1], tr.ctrl[:1]), P - 1,
                ia.HOPPER_COST if str(g["model"]) == "hopper" else ia.PENDULUM_COST)
    s.set_riccati("mfma")
    s.set_traj(tr)
    s.set_deriv(g["deriv"][None])
    s.riccati_pass()
    s.synchronize()
    K, k = s.gains()
    V, v = s.value()
    errs = {n: _rel(a, b) for n, a, b in (("K", K[0, 1:], g["K"][1:]), ("k", k[0, 1:], g["k"][1:]),
                                          ("V", V[0], g["V"]), ("v", v[0], g["v"]))}
    print(fixture, "MFMA Riccati max relative deviation:", errs)
    assert all(e <= 1e-12 for e in errs.values()), errs


def test_ldlt_reg_matches_lds(ia, monkeypatch):
    """The MFMA recursion's compile-time humanoid instance (nu = 21) factors
    Quu in registers (riccati.h ldlt_factor_reg_t: the pivot sequence replayed
    from the diagonal, one row per lane) or on LDS (ILQG_LDLT_REG=0,
    ldlt_factor_wave_t), with its pivot order from ranks of distinct keys or
    from the scan replayed (ILQG_LDLT_REG=2): the same operations in the same
    order, so K, k, V, v agree bit for bit (cfg 5's state, H = 200, after two
    iterations).  These are physical Quu matrices: whatever equal |diagonal|
    keys the symmetric standing pose presents, the three variants are compared
    with each other only, so a first-hit rule that is wrong in all of them
    passes here.  Crafted ties (at the maximum too), zero, denormal and NaN
    pivots, with step 1 anchored to the oracle at zero difference, are covered
    by tests/test_riccati_cases.py::test_mfma_engine."""
    m = ia.Model.load(model_path("humanoid"))
    st = m.reset_state(1)
    st.qpos[0, 2] = 1.4
    g = ia.ILQR(m, st, 200, ia.HUMANOID_COST)
    g.set_riccati("mfma")
    for _ in range(2):
        g.iterate()
    g.synchronize()
    out = {}
    for flag in ("0", "1", "2"):
        monkeypatch.setenv("ILQG_LDLT_REG", flag)
        g.riccati_pass()
        g.synchronize()
        out[flag] = g.gains() + g.value()
    for flag in ("1", "2"):
        for a, b, n in zip(out["0"], out[flag], ("K", "k", "V", "v")):
            assert np.isfinite(a).all(), n
            exact(b, a, f"{n} (ILQG_LDLT_REG={flag})")


@pytest.mark.parametrize("env", [{}, {"ILQG_FUSED": "0"}, {"ILQG_PLAN": "1"}, {"ILQG_PLAN": "1", "ILQG_FD_HALVES": "1"},
                                 {"ILQG_FD_HALVES": "1"},
                                 {"ILQG_FD_SNAP": "0"}, {"ILQG_FD_HALVES": "1", "ILQG_FD_SNAP": "0"},
                                 {"ILQG_FD_PRIO1": "500", "ILQG_FD_PRIO2": "800"},
                                 {"ILQG_SNAP_POISON": "1"}, {"ILQG_SNAP_POISON": "1", "ILQG_FD_HALVES": "1"}])
def test_fused_sweep_schedules(ia, ora, env, monkeypatch):
    """The fused FD sweep + streamed backward pass (k_fd_fused_g), the
    two-kernel sweep (ILQG_FUSED=0), the fused sweep with its tickets in the
    order planned from the previous launch's item durations (ILQG_PLAN=1, the
    second iteration's order is a non-trivial permutation), with every column
    as two teams, its + and - halves (ILQG_FD_HALVES=1) and with the qvel/ctrl
    teams computing their own position/velocity stages instead of loading the
    centre's (ILQG_FD_SNAP=0) give the oracle's iterate bit for bit (3 seeds x
    41 points x 16 column teams: the ticket order interleaves seeds).  With
    ILQG_SNAP_POISON=1 every workspace double the centre snapshot does not
    carry reads as NaN in the teams that load it: the trimmed snapshot holds
    everything they read"""
    import workloads
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    S, H = 3, 40
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    g = ia.ILQR(m, dmain, H, ia.HOPPER_COST)
    g.iterate()
    g.iterate()
    g.synchronize()
    gt, (K, k), D = g.traj(), g.gains(), g.deriv()
    V, v = g.value()
    P = H + 1
    for s in range(S):
        il = _oracle_ilqr(ora, om, _state_dict(dmain, s), H, "ora_cost_desc_fn", 2)
        oa = il.arrays()
        exact(gt.qpos[s * P:(s + 1) * P], il.traj()["qpos"], f"seed {s} qpos")
        exact(K[s], oa["K"], f"seed {s} K")
        exact(k[s], oa["k"], f"seed {s} k")
        exact(D[s], oa["deriv"], f"seed {s} deriv")
        exact(V[s], oa["V"], f"seed {s} V")
        exact(v[s], oa["v"], f"seed {s} v")
    if env.get("ILQG_PLAN") == "1":
        import ctypes
        n = ctypes.c_int(0)
        ia._check(ia.lib().ilqg_solver_debug_plan(g._h, None, None, ctypes.byref(n)), "debug_plan")
        order = np.zeros(n.value, dtype=np.uint32)
        dur = np.zeros(n.value, dtype=np.uint32)
        ia._check(ia.lib().ilqg_solver_debug_plan(g._h, order.ctypes.data_as(ctypes.c_void_p),
                                                  dur.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)),
                  "debug_plan")
        assert np.array_equal(np.sort(order), np.arange(n.value)), "planned order is a permutation"
        assert not np.array_equal(order, np.arange(n.value)), "the planner reordered the tickets"
        assert (dur > 0).all(), "every item's duration was recorded"
        # the deadlock-freedom invariant: every column item (each half, with
        # ILQG_FD_HALVES) holds a later ticket than its centre C(s,p) = p S + s
        nC = S * P
        nt = n.value // nC - 1
        pos = np.empty(n.value, dtype=np.int64)
        pos[order] = np.arange(n.value)
        cols = np.arange(nC, n.value)
        assert (pos[(cols - nC) // nt] < pos[cols]).all(), "a column is scheduled before its centre"
    # the sweep alone (no backward roles) writes the same records
    g.fd_sweep()
    g.synchronize()
    exact(g.deriv(), D, "fd_sweep alone vs iterate's fused records")


@pytest.mark.parametrize("bad", ["out_of_range", "repeated", "column_first"])
def test_invalid_schedule_is_reported(ia, ora, bad):
    """A fused sweep's ticket -> item map is validated on the device before the
    sweep reads it (launch_fd_order_check): an entry out of range, a repeated
    item, or a column ahead of its centre is replaced by the identity map,
    ilqg_synchronize reports ILQG_ERR_HIP once ("invalid ticket schedule")
    instead of the process dying on a memory fault or a hand-off deadlock,
    and the records stay the oracle's bit for bit -- on that iteration and the
    next (test hook ilqg_solver_debug_plant_schedule)"""
    import workloads
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    S, H = 2, 20
    P = H + 1
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    g = ia.ILQR(m, dmain, H, ia.HOPPER_COST)
    nC = S * P
    # slot nC holds item nC (the first column of C(0, 0)) in the identity map
    plants = {"out_of_range": [(nC, 1 << 30)], "repeated": [(nC, nC + 1)],
              "column_first": [(0, nC), (nC, 0)]}[bad]  # a permutation, C(0, 0) behind its column
    for slot, item in plants:
        g._debug_plant_schedule(slot, item)
    g.iterate()
    with pytest.raises(ia.IlqgError, match="invalid ticket schedule"):
        g.synchronize()
    g.synchronize()  # reported once
    g.iterate()
    g.synchronize()
    (K, k), D = g.gains(), g.deriv()
    for s in range(S):
        oa = _oracle_ilqr(ora, om, _state_dict(dmain, s), H, "ora_cost_desc_fn", 2).arrays()
        exact(D[s], oa["deriv"], f"seed {s} deriv")
        exact(K[s], oa["K"], f"seed {s} K")
        exact(k[s], oa["k"], f"seed {s} k")


@pytest.mark.parametrize("name,prec", [("hopper", "f64"), ("humanoid", "f32")])
def test_fd_sweep_range_blocks(ia, ora, name, prec):
    """ilqg_fd_sweep_range (one rank's block of a point-sharded sweep, cfg 5 on
    N GPUs): the blocks of a 3-way split together write exactly the records of
    the whole-trajectory sweep, and the recursion over them (after the
    single-rank RecordExchange over the solver's resident records) gives the
    gains of the unsharded iteration"""
    import workloads
    import torch
    from seed_shard import RecordExchange, point_range
    assert torch.cuda.is_available()  # torch's HIP runtime first (ilqg_amd.lib)
    m = ia.Model.load(workloads.model_file(name))
    if name == "hopper":
        dmain, H, cost = workloads.hopper_dmain(m, 2, sigma=0.01), 30, ia.HOPPER_COST
    else:
        dmain, H, cost = m.reset_state(1), 12, ia.HUMANOID_COST
        dmain.qpos[0, 2] = 1.4
    g = ia.ILQR(m, dmain, H, cost)
    if prec == "f32":
        g.set_fd_precision("f32")
    g.forward_pass()
    g.fd_sweep()
    g.riccati_pass()
    g.synchronize()
    D_full, (K_full, k_full) = g.deriv(), g.gains()
    P = H + 1
    g.set_deriv(np.full_like(D_full, np.nan))
    for r in range(3):
        p0, n = point_range(r, 3, P)
        g.fd_sweep_range(p0, n)
    g.synchronize()
    exact(g.deriv(), D_full, "3 blocks vs the whole sweep")
    RecordExchange.for_solver(g, 0, 1).exchange()
    g.riccati_pass()
    g.synchronize()
    K, k = g.gains()
    exact(K, K_full, "K")
    exact(k, k_full, "k")


@pytest.mark.parametrize("world", [3, 8])
def test_forward_sharded_interleaved(ia, ora, world, monkeypatch):
    """ilqg_forward_sharded (cfg 5 on N GPUs, one rank's share of the
    pipelined, point-sharded iteration), `world` ranks played by `world`
    solvers on one GPU: rank r's call writes exactly the records of the points
    point_owners gives it (the others stay as they were: NaN here), every rank
    rolls out the same trajectory, the owned records together are the
    unsharded pipelined sweep's, and the recursion over the gathered records
    gives the unsharded iteration's gains on every rank -- over two iterations
    (humanoid, fp32 FD, MFMA recursion, chunks of 5 points over H = 40:
    interleaved ownership)"""
    import workloads
    import torch
    assert torch.cuda.is_available()  # torch's HIP runtime first (ilqg_amd.lib)
    monkeypatch.setenv("ILQG_PIPE_CHUNK", "5")
    m = ia.Model.load(workloads.model_file("humanoid"))
    dmain, H = m.reset_state(1), 40
    dmain.qpos[0, 2] = 1.4
    P = H + 1

    def solver():
        g = ia.ILQR(m, dmain, H, ia.HUMANOID_COST)
        g.set_fd_precision("f32")
        g.set_riccati("mfma")
        return g
    ref, ranks = solver(), [solver() for _ in range(world)]
    owner = ranks[0].point_owners(world)
    assert np.array_equal(owner, ia.point_owners(P, 5, world))
    assert any(np.any(np.diff(np.nonzero(owner == r)[0]) > 1) for r in range(world))  # interleaved
    for it in range(2):
        ref.iterate()
        ref.synchronize()
        D_ref = ref.deriv().reshape(P, -1)
        gathered = np.full_like(D_ref, np.nan)
        for r, g in enumerate(ranks):
            g.set_deriv(np.full_like(D_ref, np.nan))
            g.forward_sharded(r, world)
            g.synchronize()
            D = g.deriv().reshape(P, -1)
            mine = owner == r
            exact(D[mine], D_ref[mine], f"iteration {it}: rank {r}'s points")
            assert np.isnan(D[~mine]).all(), f"iteration {it}: rank {r} wrote points it does not own"
            exact(g.traj().qpos, ref.traj().qpos, f"iteration {it}: rank {r}'s trajectory")
            gathered[mine] = D[mine]
        for r, g in enumerate(ranks):
            g.set_deriv(gathered)  # the all-gather's result on every rank
            g.riccati_pass()
            g.synchronize()
            for a, b, what in zip(g.gains(), ref.gains(), ("K", "k")):
                exact(a, b, f"iteration {it}: rank {r}'s {what}")


@pytest.mark.parametrize("name,prec,chunk", [("humanoid", "f32", 7), ("humanoid", "f64", 5), ("hopper", "f64", 16)])
def test_pipelined_iterate(ia, ora, name, prec, chunk, monkeypatch):
    """ilqg_iterate with one candidate per seed and the unfused sweep rolls out
    in chunks (ILQG_PIPE_CHUNK points each) with the FD sweep of every finished
    chunk on a second stream behind it: the trajectory, records, gains and
    value are the unchunked iteration's bit for bit (cfg 5: humanoid, fp32 FD,
    MFMA recursion; the hopper through the unfused path, ILQG_FUSED=0, also
    against the oracle)"""
    import workloads
    if name == "hopper":
        monkeypatch.setenv("ILQG_FUSED", "0")
        m, om = setup(ia, ora, name, ia.HOPPER_COST)
        dmain, H, cost = workloads.hopper_dmain(m, 2, sigma=0.01), 40, ia.HOPPER_COST
    else:
        m = ia.Model.load(workloads.model_file(name))
        dmain, H, cost = m.reset_state(1), 24, ia.HUMANOID_COST
        dmain.qpos[0, 2] = 1.4
    out = {}
    for ch in (0, chunk):
        monkeypatch.setenv("ILQG_PIPE_CHUNK", str(ch))
        g = ia.ILQR(m, dmain, H, cost)
        if prec == "f32":
            g.set_fd_precision("f32")
        if name == "humanoid":
            g.set_riccati("mfma")
        for _ in range(2):
            g.iterate()
        g.synchronize()
        t = g.traj()
        out[ch] = (t.qpos, t.qvel, t.ctrl, g.deriv(), *g.gains(), *g.value(), g.costs()[0])
    for a, b, what in zip(out[0], out[chunk], ("qpos", "qvel", "ctrl", "deriv", "K", "k", "V", "v", "costs")):
        exact(b, a, what)
    if name == "hopper":
        P = H + 1
        for s in range(2):
            il = _oracle_ilqr(ora, om, _state_dict(dmain, s), H, "ora_cost_desc_fn", 2)
            exact(out[chunk][4][s], il.arrays()["K"], f"seed {s} K vs oracle")
            exact(out[chunk][0][s * P:(s + 1) * P], il.traj()["qpos"], f"seed {s} qpos vs oracle")


@pytest.mark.parametrize("G", [2, 3, 4])
def test_seed_groups_bitexact(ia, ora, G):
    """ilqg_solver_set_groups: iterate() software-pipelines the seeds as G
    ranges (per group: rollout + selection on an XCD-masked stream, the fused
    sweep + recursion on a stream masked to the rest, staggered behind the
    previous group).  Every seed's trajectory, records, gains, value and costs
    equal the ungrouped iterate's bit for bit (G = 3 over 4 seeds: uneven
    ranges 1, 1, 2), through a switch back to one group and an API launch on
    the solver's stream (ilqg_fd_sweep) between grouped iterates."""
    import workloads
    m, _ = setup(ia, ora, "hopper", ia.HOPPER_COST)
    S, H = 4, 60
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    out = {}
    for grp in (1, G):
        g = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=workloads.LINESEARCH_ALPHAS[:4], select="min_cost")
        g.set_groups(grp)
        assert g.groups == grp
        if grp > 1:
            assert g.group_rollout_cus in (0, 32)
        for _ in range(3):
            g.iterate()
        g.fd_sweep()  # a launch on the solver's stream: the next grouped iterate joins it
        g.iterate()
        g.synchronize()
        g.set_groups(1)
        g.iterate()
        g.synchronize()
        t = g.traj()
        out[grp] = (t.qpos, t.qvel, t.ctrl, g.deriv(), *g.gains(), *g.value(), *g.costs())
    for a, b, what in zip(out[1], out[G], ("qpos", "qvel", "ctrl", "deriv", "K", "k", "V", "v", "costs", "sel")):
        exact(b, a, what)


@pytest.mark.parametrize("G", [2, 4])
def test_seed_groups_cost_exchange(ia, ora, G):
    """The bench's loop with seed groups: iterate(), then the cost exchange
    (CostExchange: argmin over the device costs on torch's stream, which is the
    solver's) and a torch copy of the selected costs, every iteration, with no
    host synchronisation in between.  The exchange joins the groups
    (ilqg_solver_join_stream), so no group's next rollout/selection overwrites
    the costs while torch still reads them: every iteration's copy and best
    seed equal the ungrouped run's (G = 4 over 4 seeds: one seed a group)."""
    import torch
    import workloads
    from seed_shard import CostExchange, device_view
    m, _ = setup(ia, ora, "hopper", ia.HOPPER_COST)
    S, H = 4, 60
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    out = {}
    for grp in (1, G):
        g = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=workloads.LINESEARCH_ALPHAS[:4], select="min_cost")
        stream = torch.cuda.Stream()
        g.set_stream(stream.cuda_stream)
        g.set_groups(grp)
        ex = CostExchange(device_view(g.device_costs_ptr(), S), 1, solver=g)
        seen, best = [], []
        with torch.cuda.stream(stream):
            for _ in range(5):
                g.iterate()
                best.append(ex())
                seen.append(ex.local.clone())
        torch.cuda.synchronize()
        g.synchronize()
        out[grp] = (torch.stack(seen).cpu().numpy(), torch.stack(best).cpu().numpy())
        g.set_groups(1)
    exact(out[G][0], out[1][0], "selected costs read by torch after every iterate")
    exact(out[G][1], out[1][1], "best seed per iterate")


def test_bench_workload_bitexact(ia, ora):
    """The exact timed workload of bench.py (cfg 4's per-GPU share: hopper H=500,
    8 seeds x 8 line-search candidates alpha = 2^-i, select='min_cost'), three
    iterations, against the oracle's line-search restatement
    (ora_ilqr_iterate_ls: u = K dx + alpha k + u*, inc/ilqr.h:126 with alpha
    scaling the feed-forward).  Iteration 2 selects a candidate other than
    alpha = 1, so iteration 3's rollout and every backward pass after it run
    from a non-reference nominal.  Compared bit for bit: every seed's
    trajectory, FD records, K, k, V, v, the cost matrix and the selection."""
    import workloads
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    om.lib.L.ora_set_nthread(1)
    S, H, iters = 8, 500, 3
    alphas = workloads.LINESEARCH_ALPHAS
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    g = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=alphas, select="min_cost")
    for _ in range(iters):
        g.iterate()
    g.synchronize()
    gt, (K, k), D = g.traj(), g.gains(), g.deriv()
    V, v = g.value()
    gc, gsel = g.costs()
    P = H + 1
    picked = set()
    for s in range(S):
        d = om.make_data()
        d.set_state(**_state_dict(dmain, s))
        il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
        il.set_dinit(d)
        for _ in range(iters):
            oc, osel = il.iterate_ls(alphas, "min_cost")
        picked.add(osel)
        ot, oa = il.traj(), il.arrays()
        for f in ("time", "qpos", "qvel", "warm", "ctrl"):
            exact(getattr(gt, f)[s * P:(s + 1) * P].reshape(ot[f].shape), ot[f], f"seed {s} traj.{f}")
        exact(D[s], oa["deriv"], f"seed {s} deriv")
        exact(K[s], oa["K"], f"seed {s} K")
        exact(k[s], oa["k"], f"seed {s} k")
        exact(V[s], oa["V"], f"seed {s} V")
        exact(v[s], oa["v"], f"seed {s} v")
        exact(gc[s], oc, f"seed {s} candidate costs")
        assert int(gsel[s]) == osel, (s, int(gsel[s]), osel)
    assert picked != {0}, "the workload must exercise a non-alpha=1 selection"


def test_cfg4_all_shards_one_gpu(ia, ora):
    """BASELINE.json configs[3]: all 64 cfg-4 seeds (the shares of ranks 0..7,
    seed_offset = 8 r) on one GPU as one S = 64 solver, two line-search
    iterations (8 alphas, min-cost).  One seed of every shard (seed 9 r) is
    compared bit for bit with the oracle's line-search iLQR; all 64 are finite
    and the whole run is deterministic (a second solver gives the same bits).
    Each rank's own solver (seed_offset = 8 r) starts from these same states
    (workloads.hopper_dmain), so this covers every rank's inputs."""
    import workloads
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    om.lib.L.ora_set_nthread(1)
    S, H, iters = 64, 500, 2
    alphas = workloads.LINESEARCH_ALPHAS
    dmain = workloads.hopper_dmain(m, S, sigma=0.01)
    for r in range(8):  # the shard of rank r is exactly hopper_dmain(..., seed_offset=8r)
        shard = workloads.hopper_dmain(m, 8, sigma=0.01, seed_offset=8 * r)
        assert np.array_equal(shard.qpos, dmain.qpos[8 * r:8 * r + 8])
        assert np.array_equal(shard.qvel, dmain.qvel[8 * r:8 * r + 8])
    runs = []
    for _ in range(2):
        g = ia.ILQR(m, dmain, H, ia.HOPPER_COST, alphas=alphas, select="min_cost")
        for _ in range(iters):
            g.iterate()
        g.synchronize()
        runs.append((g.traj(), g.gains(), g.costs()))
        del g
    (t1, (K1, k1), (c1, s1)), (t2, (K2, k2), (c2, s2)) = runs
    for a, b, nm in ((t1.qpos, t2.qpos, "qpos"), (t1.qvel, t2.qvel, "qvel"), (t1.ctrl, t2.ctrl, "ctrl"),
                     (K1, K2, "K"), (k1, k2, "k"), (c1, c2, "costs"), (s1, s2, "selection")):
        exact(a, b, f"determinism {nm}")
        assert np.all(np.isfinite(a)), nm
    P = H + 1
    for r in range(8):
        s = 9 * r  # rank r's local seed r
        d = om.make_data()
        d.set_state(**_state_dict(dmain, s))
        il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
        il.set_dinit(d)
        for _ in range(iters):
            oc, osel = il.iterate_ls(alphas, "min_cost")
        ot, oa = il.traj(), il.arrays()
        for f in ("qpos", "qvel", "warm", "ctrl"):
            exact(getattr(t1, f)[s * P:(s + 1) * P].reshape(ot[f].shape), ot[f], f"seed {s} traj.{f}")
        exact(K1[s], oa["K"], f"seed {s} K")
        exact(k1[s], oa["k"], f"seed {s} k")
        exact(c1[s], oc, f"seed {s} candidate costs")
        assert int(s1[s]) == osel


def test_fault_word_reported_once_then_cleared(ia, ora):
    """A tripped hand-off (preset fault word) is reported by synchronize()
    exactly once; the next iterate() runs every wait again and is bit-exact."""
    import workloads
    m, om = setup(ia, ora, "inverted_pendulum")
    dmain = workloads.pendulum_dmain(m)
    g = ia.ILQR(m, dmain, 20, ia.PENDULUM_COST)
    g.iterate()
    g.synchronize()
    g._debug_set_fault(1)
    with pytest.raises(ia.IlqgError):
        g.synchronize()
    g.synchronize()  # reported once: cleared by the read
    il = _oracle_ilqr(ora, om, _state_dict(dmain, 0), 20, "ora_cost_pendulum", 2)
    g.iterate()
    g.synchronize()
    exact(g.gains()[0][0], il.arrays()["K"], "K after a cleared fault")
    exact(g.traj().qpos, il.traj()["qpos"], "qpos after a cleared fault")


# ---- committed known-answer fixtures (tests/golden/make_golden_ilqr.py)
def _fixture_traj(ia, g, pre):
    return ia.State(*(g[pre + k] for k in ("time", "qpos", "qvel", "warm", "ctrl")))


@pytest.mark.parametrize("fixture", ["riccati_pendulum.npz", "riccati_hopper.npz"])
def test_riccati_vs_golden(ia, fixture):
    """initV + Riccati recursion (k_backward, inc/ilqr.h:100-107,144-175) on
    seeded synthetic FD records and trajectory == the committed fixture"""
    g = load_golden(fixture)
    m = ia.Model.load(model_path(str(g["model"])))
    P = g["deriv"].shape[0]
    tr = _fixture_traj(ia, g, "traj_")
    s = ia.ILQR(m, ia.State(tr.time[:1], tr.qpos[:1], tr.qvel[:1], tr.warm[:1], tr.ctrl[:1]), P - 1,
                ia.HOPPER_COST if str(g["model"]) == "hopper" else ia.PENDULUM_COST)
    s.set_traj(tr)
    s.set_deriv(g["deriv"][None])
    s.riccati_pass()
    s.synchronize()
    K, k = s.gains()
    V, v = s.value()
    exact(K[0, 1:], g["K"][1:], "K")
    exact(k[0, 1:], g["k"][1:], "k")
    exact(V[0], g["V"], "V")
    exact(v[0], g["v"], "v")


@pytest.mark.parametrize("fixture", ["iterate_pendulum_H20.npz", "iterate_pendulum_H100.npz"])
def test_iterate_vs_golden(ia, fixture):
    """ILQR::iterate() from the reference's initial state == the fixture written
    with the reference's own calcMJDerivatives (oracle/_ref)"""
    g = load_golden(fixture)
    m = ia.Model.load(model_path("inverted_pendulum"))
    s = ia.ILQR(m, _fixture_traj(ia, g, "dmain_"), int(g["horizon"]), ia.PENDULUM_COST)
    for _ in range(int(g["iters"])):
        s.iterate()
    s.synchronize()
    t = s.traj()
    for k in ("time", "qpos", "qvel", "warm", "ctrl"):
        exact(getattr(t, k).reshape(g["traj_" + k].shape), g["traj_" + k], "traj " + k)
    K, k = s.gains()
    V, v = s.value()
    exact(K[0], g["K"], "K")
    exact(k[0], g["k"], "k")
    exact(V[0], g["V"], "V")
    exact(v[0], g["v"], "v")
    exact(s.deriv()[0], g["deriv"], "deriv")


def test_fixed_gain_rollout_vs_golden(ia):
    """forwardPass with fixed seeded gains (inc/ilqr.h:116-130), hopper H=100
    from the cfg-3 state (contacts) == the committed fixture"""
    g = load_golden("rollout_hopper_H100.npz")
    m = ia.Model.load(model_path("hopper"))
    s = ia.ILQR(m, _fixture_traj(ia, g, "dmain_"), int(g["horizon"]), ia.HOPPER_COST)
    t = s.traj()
    for k in ("time", "qpos", "qvel", "warm", "ctrl"):
        exact(getattr(t, k).reshape(g["nominal_" + k].shape), g["nominal_" + k], "nominal " + k)
    s.set_gains(g["K"][None], g["k"][None])
    s.forward_pass()
    s.synchronize()
    t = s.traj()
    for k in ("time", "qpos", "qvel", "warm", "ctrl"):
        exact(getattr(t, k).reshape(g["traj_" + k].shape), g["traj_" + k], "traj " + k)


def test_split_division_is_ieee(ia):
    """dsmall.h's split fp64 division (the divisor's reciprocal refined ahead,
    used by the Newton Cholesky solve and the line search) equals IEEE a / b
    bit for bit, over 2M random operand pairs spanning the exponent range and
    the edge cases that take the ordinary division (zeros, denormals, Inf,
    NaN, |a / b| beyond 2^768)."""
    rng = np.random.default_rng(7)
    n = 1 << 21
    mant = rng.uniform(1.0, 2.0, (2, n)) * rng.choice([-1.0, 1.0], (2, n))
    ex = rng.integers(-60, 61, (2, n))
    ex[:, : n // 8] = rng.integers(-1074, 1024, (2, n // 8))  # the whole range
    a, b = np.ldexp(mant[0], ex[0]), np.ldexp(mant[1], ex[1])
    b[n // 8: n // 4] = rng.normal(size=n // 8)  # physics-like
    a[n // 8: n // 4] = rng.normal(size=n // 8) * 1e-3
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308,
                        1.7976931348623157e308, 1.0, -1.0, 3.0, 1e-300, 1e300, 2.0 ** 800, 2.0 ** -800])
    sa, sb = np.meshgrid(special, special)
    a = np.concatenate([a, sa.ravel()])
    b = np.concatenate([b, sb.ravel()])
    with np.errstate(all="ignore"):
        want = a / b
    for got in ia.selftest_div(a, b):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        bad = np.flatnonzero(got[~nan].view(np.int64) != want[~nan].view(np.int64))
        assert bad.size == 0, (bad.size, a[~nan][bad[:4]], b[~nan][bad[:4]], got[~nan][bad[:4]])


# fp32 FD (BASELINE.json configs[4]: "fp32 FD with fp64 Riccati").  The FD step
# is 1e-3; the oracle runs the same central differences in
# fp64 at the same step, so the difference is fp32 rounding of qacc (~6e-8
# relative) amplified by 1/(2 eps) = 500 and by the conditioning of the
# constrained dynamics -- and, at the few evaluations where a perturbed fp32
# state sits on the other side of a contact or limit activation than the fp64
# one, by the jump of the dynamics there (isolated entries of order 1-10).
# Stated tolerances on e = |d - d_ref| / (1 + |d_ref|) over every record entry
# (measured on MI355X):
FD32_EPS = 1e-3
# ~2x the measured deviations (round 3, MI355X): records of the humanoid at
# cfg 5's state, H = 200 -- median e 2.2e-4, p99 4.2e-2, 0.27 % of entries
# with e > 0.1 (max 15: evaluations where the fp32 perturbed state lands on
# the other side of a contact or limit activation than the fp64 one); hopper
# after 500 passive steps, H = 40 -- median 3.4e-5, p99 2.6e-3, max 7.3e-3
FD32_MEDIAN = 5e-4     # median e
FD32_P99 = 0.085       # 99th percentile of e
FD32_FRAC_BIG = 5.5e-3  # fraction of entries with e > 0.1
# after the H = 200 recursion, max deviation relative to each array's max:
# measured K 3.7e-2, k 1.03e-2, v 1.15e-2, V 6.8e-5
FD32_GAIN_RTOL = {"K": 0.075, "k": 0.025, "v": 0.025}
FD32_V_RTOL = 1.5e-4


def _fd32_stats(what, d, dref):
    assert np.all(np.isfinite(d))
    e = np.abs(d - dref) / (1 + np.abs(dref))
    st = dict(median=float(np.median(e)), p99=float(np.quantile(e, 0.99)), frac_big=float(np.mean(e > 0.1)),
              max=float(e.max()))
    print(f"{what} fp32 FD vs fp64 oracle (eps 1e-3): {st}")
    assert st["median"] <= FD32_MEDIAN and st["p99"] <= FD32_P99 and st["frac_big"] <= FD32_FRAC_BIG, st
    return st


def test_humanoid_cfg5_fp32_fd(ia, ora):
    """cfg 5 with fp32 FD and the fp64 MFMA Riccati engine (one iteration,
    H = 200): the rollout is the fp64 one (bit-exact); the FD records and the
    gains agree with the fp64 oracle at eps = 1e-3 to the stated tolerances"""
    g, il = _humanoid_cfg5(ia, ora, 200, 1, "mfma", "f32")
    oa, ot, gt = il.arrays(), il.traj(), g.traj()
    exact(gt.qpos.reshape(ot["qpos"].shape), ot["qpos"], "traj.qpos")
    _fd32_stats("humanoid H=200", g.deriv()[0], oa["deriv"])
    K, k = g.gains()
    V, v = g.value()
    errs = {n: _rel(a, b) for n, a, b in (("K", K[0], oa["K"]), ("k", k[0], oa["k"]), ("V", V[0], oa["V"]),
                                          ("v", v[0], oa["v"]))}
    print("cfg5 fp32 FD gains, max relative deviation:", errs)
    assert errs["V"] <= FD32_V_RTOL and all(errs[n] <= FD32_GAIN_RTOL[n] for n in ("K", "k", "v")), errs


def test_fp32_fd_hopper_contacts(ia, ora):
    """The fp32 FD sweep on a contact-rich model (hopper after 500 passive
    steps, cfg 3's state; the generic kernels): records within the stated
    tolerances of the fp64 oracle at eps = 1e-3"""
    m, om = setup(ia, ora, "hopper", ia.HOPPER_COST)
    st = m.reset_state(1)
    st.ctrl[:] = -0.1
    m.step(st, 500)
    om.lib.L.ora_set_fd_eps(FD32_EPS)
    try:
        il = _oracle_ilqr(ora, om, _state_dict(st, 0), 40, "ora_cost_desc_fn", 1)
    finally:
        om.lib.L.ora_set_fd_eps(1e-6)
    g = ia.ILQR(m, st, 40, ia.HOPPER_COST)
    g.set_fd_precision("f32")
    g.iterate()
    g.synchronize()
    _fd32_stats("hopper H=40", g.deriv()[0], il.arrays()["deriv"])


# multi-iteration fp32-FD runs: the line-search iLQR with the
# fp32 FD sweep tracks the fp64 oracle run at the same eps iteration by
# iteration.  (The reference iLQR -- fixed mu = 1000, the Q1 column-major B,
# no regularization schedule -- does not lower the cost on these models: from
# cfg 3's hopper state the oracle's own selected cost rises 110 -> 1.2e5 ->
# 1.8e5 -> 3.6e5, so "the cost decreases" is not a property of the path being
# reproduced; the fp32 run must follow the fp64 one instead.)  Iteration 1's
# cost is the fp64 rollout of the initial trajectory (bit-exact); the gap then
# grows with the iterations as the model's dynamics amplify it.
# per iteration, ~2x measured (hopper 0, 2.3e-4, 1.2e-2; humanoid 0, 6.5e-3 --
# its third iteration is past the point where the reference iLQR diverges:
# the fp64 oracle's own cost there is 1.6e8)
FD32_COST_RTOL = {"hopper": (1e-12, 5e-4, 3e-2), "humanoid": (1e-12, 1.3e-2)}


def _fp32_cost_run(ia, ora, name, cost, st, H, iters, riccati):
    import workloads
    m, om = setup(ia, ora, name, cost)
    alphas = workloads.LINESEARCH_ALPHAS
    om.lib.L.ora_set_fd_eps(FD32_EPS)
    try:
        d = om.make_data()
        d.set_state(**_state_dict(st, 0))
        il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
        il.set_dinit(d)
        oc = []
        for _ in range(iters):
            c, sel = il.iterate_ls(alphas, "min_cost")
            oc.append(float(c[sel]))
    finally:
        om.lib.L.ora_set_fd_eps(1e-6)
    g = ia.ILQR(m, st, H, cost, alphas=alphas, select="min_cost")
    g.set_riccati(riccati)
    g.set_fd_precision("f32")
    gcs = []
    for _ in range(iters):
        g.iterate()
        g.synchronize()
        c, sel = g.costs()
        gcs.append(float(c[0][int(sel[0])]))
    return np.array(gcs), np.array(oc)


@pytest.mark.parametrize("name", ["hopper", "humanoid"])
def test_fp32_fd_multi_iteration_cost(ia, ora, name):
    """fp32 FD sweep (eps 1e-3) + fp64 Riccati, line-search iterations (8
    alphas, min-cost; 3 for the hopper, 2 for the humanoid): the selected
    trajectory cost of every iteration is
    finite and within FD32_COST_RTOL of the fp64 oracle's at the same eps
    (hopper: cfg 3's state, H = 100, exact Riccati; humanoid: cfg 5's state,
    H = 50, MFMA Riccati)"""
    import workloads
    if name == "hopper":
        m, _ = setup(ia, ora, "hopper", ia.HOPPER_COST)
        st = workloads.hopper_dmain(m, 1)
        gc, oc = _fp32_cost_run(ia, ora, "hopper", ia.HOPPER_COST, st, 100, len(FD32_COST_RTOL[name]), "exact")
    else:
        m, _ = setup(ia, ora, "humanoid", ia.HUMANOID_COST)
        st = m.reset_state(1)
        st.qpos[0, 2] = 1.4
        gc, oc = _fp32_cost_run(ia, ora, "humanoid", ia.HUMANOID_COST, st, 50, len(FD32_COST_RTOL[name]), "mfma")
    rel = np.abs(gc - oc) / np.abs(oc)
    print(f"{name} fp32-FD selected costs {gc.tolist()}, fp64 oracle {oc.tolist()}, relative gaps {rel.tolist()}")
    assert np.all(np.isfinite(gc))
    assert np.all(rel <= np.array(FD32_COST_RTOL[name])), (rel, FD32_COST_RTOL[name])

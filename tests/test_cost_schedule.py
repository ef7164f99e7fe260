"""Cost schedule (ilqg_solver_set_cost_schedule): one cost row per trajectory
point in the rollout and the FD sweep.

The reference is tests/cost_sched_ref.py, the oracle composed piecewise; the
CPU tests pin it against OILQR.iterate_ls.  GPU comparisons are bit for bit
unless a tolerance is stated.
"""
import os
import re

import numpy as np
import pytest

import boxqp_ref as bq
import cost_sched_ref as cs
from conftest import model_path

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = (1.0, 0.5, 0.25)
NAMES = ("ilqg_solver_set_cost_schedule", "ilqg_solver_get_cost_schedule", "ilqg_solver_shift_cost_schedule")
SETUPS = {"inverted_pendulum": 8, "hopper": 12}


def exact(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b, equal_nan=True):
        raise AssertionError(f"{what}: not bit-exact, max|diff|={np.nanmax(np.abs(a - b)):.3e}")


def _cost(ia, name):
    return {"inverted_pendulum": ia.PENDULUM_COST, "hopper": ia.HOPPER_COST, "humanoid": ia.HUMANOID_COST}[name]


def _state_dict(st, i):
    return dict(time=st.time[i], qpos=st.qpos[i], qvel=st.qvel[i], warm=st.warm[i], ctrl=st.ctrl[i])


def _cpu_dmain(ia, ora, m, name):
    """workloads.*_dmain with the oracle's physics (the GPU's bit for bit): no device needed"""
    om = ora.OModel(m.blob())
    d = om.make_data()
    d.set_state(time=0.0, qpos=m.qpos0, qvel=np.zeros(m.nv), warm=np.zeros(m.nv), ctrl=np.zeros(m.nu))
    d.step(10 if name == "inverted_pendulum" else 500)
    s = d.state()
    if name != "inverted_pendulum":
        s["ctrl"] = s["ctrl"] - 0.1
    return ia.State(np.array([s["time"]]), s["qpos"][None], s["qvel"][None], s["warm"][None], s["ctrl"][None])


# ---------------------------------------------------------------- CPU ----
@pytest.mark.parametrize("name", sorted(SETUPS))
def test_reference_is_iterate_ls(ia, ora, name):
    """every row equal to one cost: the composed reference is OILQR.iterate_ls
    itself -- costs, selection, trajectory, records, K, k, V, v, two iterations"""
    m = ia.Model.load(model_path(name))
    H, cost = SETUPS[name], _cost(ia, name)
    dm = _state_dict(_cpu_dmain(ia, ora, m, name), 0)
    om = ora.OModel(m.blob())
    ref = cs.SchedRef(ora, m, om, dm, H, cs.constant_schedule(cost, m, H), ALPHAS)
    om2 = ora.OModel(m.blob())
    om2.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(cost, m.nq, m.nv, m.nu))
    d = om2.make_data()
    d.set_state(**dm)
    il = ora.OILQR(om2, d, H, cost_fn="ora_cost_desc_fn")
    il.set_dinit(d)
    for it in range(2):
        c, sel = ref.iterate()
        om2.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(cost, m.nq, m.nv, m.nu))
        c2, sel2 = il.iterate_ls(ALPHAS, "min_cost")
        exact(c, c2, f"{name} it{it} costs")
        assert sel == sel2
        a, b, ta, tb = ref.arrays(), il.arrays(), ref.traj(), il.traj()
        for f in cs.FIELDS:
            exact(ta[f], tb[f], f"{name} it{it} traj.{f}")
        for f in ("deriv", "K", "k", "V", "v"):
            exact(a[f], b[f], f"{name} it{it} {f}")
    assert np.any(il.arrays()["K"] != 0)


def test_row_layout(ia):
    """Cost.row is Cost.packed's arrays in order: wq tq lq wv tv lv wu tu lu"""
    nq, nv, nu = 3, 2, 2
    c = ia.Cost(wq=[1, 2, 3], tq=[4, 5, 6], lq=[7, 8, 9], wv=[10, 11], tv=[12, 13], lv=[14, 15], wu=[16, 17],
                tu=[18, 19], lu=[20, 21])
    exact(c.row(nq, nv, nu), np.arange(1.0, 22.0), "row")
    p = c.packed(nq, nv, nu)
    assert list(p) == ["wq", "tq", "lq", "wv", "tv", "lv", "wu", "tu", "lu"]
    exact(c.row(nq, nv, nu), np.concatenate(list(p.values())), "row vs packed")
    exact(ia.Cost(wq=[1.0]).row(2, 1, 1), np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]), "short arrays are zero-padded")

    class M:
        pass
    M.nq, M.nv, M.nu = nq, nv, nu
    sl = cs.row_slices(M)
    for k, v in p.items():
        exact(c.row(nq, nv, nu)[sl[k]], v, k)


def test_header_and_exports(ia):
    with open(os.path.join(ROOT, "include", "ilqg_amd.h")) as f:
        hdr = f.read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert n in ia.EXPORTS
        assert hasattr(ia.lib(), n)


def test_generated_schedule_properties(ia):
    """what the generator promises: weights >= 0 with exact zeros, an all-zero
    row, a linear-only row with negative terms, moving targets, a heavier terminal row"""
    m = ia.Model.load(model_path("hopper"))
    rows = cs.make_schedule(ia.HOPPER_COST, m, 12)
    sl = cs.row_slices(m)
    w = np.concatenate([rows[:, sl["w" + x]] for x in "qvu"], axis=1)
    l = np.concatenate([rows[:, sl["l" + x]] for x in "qvu"], axis=1)
    t = np.concatenate([rows[:, sl["t" + x]] for x in "qvu"], axis=1)
    assert np.all(w >= 0) and np.any(w[3:] == 0) and np.any(w[3:] > 0)
    assert not rows[1].any()
    assert not w[2].any() and not t[2].any() and np.any(l[2] < 0) and np.any(l[2] > 0)
    assert np.all(np.ptp(t[3:], axis=0) > 0)
    assert w[0].sum() > 3 * np.median(w[3:].sum(axis=1))
    exact(rows, cs.make_schedule(ia.HOPPER_COST, m, 12), "deterministic")


# ---------------------------------------------------------------- GPU ----
def _dmain(ia, m, name, S=1):
    import workloads
    return workloads.pendulum_dmain(m, S) if name == "inverted_pendulum" else workloads.hopper_dmain(m, S)


def _snapshot(g):
    g.synchronize()
    t = g.traj()
    K, k = g.gains()
    V, v = g.value()
    c, sel = g.costs()
    out = {f: getattr(t, f).copy() for f in cs.FIELDS}
    out.update(K=K, k=k, V=V, v=v, deriv=g.deriv(), costs=c, sel=sel)
    return out


def _same(a, b, what, keys=None):
    for f in keys or a:
        exact(a[f], b[f], f"{what} {f}")


def _vs_ref(snap, ref, c, sel, s, what):
    """seed s of a device snapshot against the composed reference's state"""
    P = ref.N + 1
    exact(snap["costs"][s], c, f"{what} costs")
    assert snap["sel"][s] == sel, (what, snap["sel"][s], sel)
    rt, ra = ref.traj(), ref.arrays()
    for f in cs.FIELDS:
        exact(snap[f][s * P:(s + 1) * P].reshape(rt[f].shape), rt[f], f"{what} traj.{f}")
    exact(snap["deriv"][s], ra["deriv"], f"{what} records")
    exact(snap["K"][s], ra["K"], f"{what} K")
    exact(snap["k"][s], ra["k"], f"{what} k")
    exact(snap["V"][s], ra["V"], f"{what} V")
    exact(snap["v"][s], ra["v"], f"{what} v")


@gpu
@pytest.mark.parametrize("name", sorted(SETUPS))
def test_constant_schedule_is_noop(ia, name):
    """1: rows all equal to the creation cost change nothing; nor does switching it off again"""
    m = ia.Model.load(model_path(name))
    H, cost, S = SETUPS[name], _cost(ia, name), 2
    dm = _dmain(ia, m, name, S)
    a = ia.ILQR(m, dm, H, cost, alphas=ALPHAS, select="min_cost")
    b = ia.ILQR(m, dm, H, cost, alphas=ALPHAS, select="min_cost")
    assert b.cost_schedule() is None
    b.set_cost_schedule(cs.constant_schedule(cost, m, H))
    exact(b.cost_schedule(), cs.constant_schedule(cost, m, H), "get")
    for it in range(2):
        a.iterate()
        b.iterate()
        _same(_snapshot(a), _snapshot(b), f"{name} it{it}")
    assert np.any(_snapshot(a)["K"] != 0)
    b.set_cost_schedule(None)
    assert b.cost_schedule() is None
    a.iterate()
    b.iterate()
    _same(_snapshot(a), _snapshot(b), f"{name} after off")


def _varying(ia, ora, m, name, dm, H, rows, iters=2, alphas=ALPHAS, jac_check=True):
    """assertions of test 2: the scheduled solver against the composed reference
    (seed 0), and against an unscheduled solver where they must and must not agree"""
    cost = _cost(ia, name)
    om = ora.OModel(m.blob())
    ref = cs.SchedRef(ora, m, om, _state_dict(dm, 0), H, rows, alphas)
    g = ia.ILQR(m, dm, H, cost, alphas=alphas, select="min_cost")
    g.set_cost_schedule(rows)
    u = ia.ILQR(m, dm, H, cost, alphas=alphas, select="min_cost")
    G = 2 * m.nv * m.nv + m.nv * m.nu
    for it in range(iters):
        g.iterate()
        snap = _snapshot(g)
        c, sel = ref.iterate()
        _vs_ref(snap, ref, c, sel, 0, f"{name} it{it}")
        if it == 0:
            # K = k = 0: both replay the constructor's trajectory
            u.iterate()
            us = _snapshot(u)
            exact(snap["deriv"][..., :G], us["deriv"][..., :G], f"{name} Jacobian blocks")
            if jac_check:
                assert np.all(np.any(snap["deriv"][..., G:] != us["deriv"][..., G:], axis=-1)), "cost gradients"
            assert np.all(snap["costs"] != us["costs"]), "candidate costs"
    return g, ref


@gpu
@pytest.mark.parametrize("env", [{}, {"ILQG_FUSED": "0"}, {"ILQG_PLAN": "1", "ILQG_FD_HALVES": "1"}],
                         ids=["fused", "unfused", "plan_halves"])
@pytest.mark.parametrize("name", sorted(SETUPS))
def test_varying_schedule(ia, ora, name, env, monkeypatch):
    """2: a schedule that varies over the horizon, on the static-model kernels"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = ia.Model.load(model_path(name))
    H = SETUPS[name]
    dm = _dmain(ia, m, name, 2)
    g, _ = _varying(ia, ora, m, name, dm, H, cs.make_schedule(_cost(ia, name), m, H))
    # both seeds start from the same state: the same results
    s = _snapshot(g)
    exact(s["K"][0], s["K"][1], "seed 1")


@gpu
def test_generic_kernels_hopper(ia, ora):
    """3a: the condim-1 hopper (no compiled specialisation): generic two-wave rollout, generic sweep"""
    import workloads
    with open(model_path("hopper")) as f:
        xml = f.read().replace('condim="3" name="floor"', 'condim="1" name="floor"')
    m = ia.Model.from_string(xml)
    assert m.static_id() == 0
    H = 6
    _varying(ia, ora, m, "hopper", workloads.hopper_dmain(m), H, cs.make_schedule(ia.HOPPER_COST, m, H))


@gpu
def test_generic_kernels_humanoid(ia, ora):
    """3b: the humanoid (nv = 27 > 8, exact engine, 228-double rows: 4 prefetch registers a lane)"""
    m = ia.Model.load(model_path("humanoid"))
    st = m.reset_state(1)
    st.qpos[0, 2] = 1.4
    m.step(st, 5)
    H = 3
    _varying(ia, ora, m, "humanoid", st, H, cs.make_schedule(ia.HUMANOID_COST, m, H))


@gpu
def test_chunked_rollout(ia, ora, monkeypatch):
    """4: the pipelined iterate (one candidate, unfused sweep, chunks 5 + 5 + 3):
    the cost carried across chunks and the rows staged on resume"""
    monkeypatch.setenv("ILQG_FUSED", "0")
    monkeypatch.setenv("ILQG_PIPE_CHUNK", "5")
    name, H = "hopper", 12
    m = ia.Model.load(model_path(name))
    dm = _dmain(ia, m, name)
    _varying(ia, ora, m, name, dm, H, cs.make_schedule(ia.HOPPER_COST, m, H), alphas=(1.0,))


def _row_cost(ia, m, row):
    sl = cs.row_slices(m)
    return ia.Cost(**{k: row[v] for k, v in sl.items()})


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_per_point_equivalence(ia, prec):
    """5: record p of a scheduled sweep is record p of a solver whose stationary
    cost is row p, on the same trajectory (fp32 sweep; once fp64, the fused sweep)"""
    name, H = "hopper", 12
    m = ia.Model.load(model_path(name))
    dm = _dmain(ia, m, name)
    rows = cs.make_schedule(ia.HOPPER_COST, m, H)
    g = ia.ILQR(m, dm, H, ia.HOPPER_COST)
    g.set_fd_precision(prec)
    g.set_cost_schedule(rows)
    g.iterate()
    g.iterate()
    g.synchronize()
    t, rec = g.traj(), g.deriv()
    for p in (0, 5, H):
        one = ia.ILQR(m, dm, H, _row_cost(ia, m, rows[p]))
        one.set_fd_precision(prec)
        one.set_traj(t)
        one.fd_sweep()
        one.synchronize()
        exact(one.deriv()[0, p], rec[0, p], f"{prec} record {p}")
    assert np.all(np.isfinite(rec))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.longdouble(1e-300)))


def _box_deviation(g, m, lo, hi, H):
    """the device's K, k, V, v against boxqp_ref's recursion over the device's own
    records and trajectory -> (largest relative deviation, reference)"""
    g.synchronize()
    t = g.traj()
    ref = bq.recursion(g.deriv()[0], t.qpos, t.qvel, t.ctrl, m.nv, m.nu, m.timestep, 1000.0, lo, hi, layout=0)
    K, k = g.gains()
    V, v = g.value()
    out = dict(K=K[0, 1:], k=k[0, 1:], V=V[0], v=v[0])
    dev = 0.0
    for n in ("K", "k", "V", "v"):
        want = ref[n][1:] if n in ("K", "k") else ref[n]
        dev = max(dev, _rel(out[n].reshape(np.shape(want)), want))
    return dev, ref


@gpu
def test_with_limits(ia, ora):
    """6: schedule + control limits (pendulum H = 8, seeded gains, limits the
    rollout runs into): candidate costs are the reference's sums over the
    clamped trajectories, records are the scheduled ones, and the boxed gains
    agree with boxqp_ref's recursion on those records as test_ctrl_limits.py
    asserts it: the same clamped sets, deviation <= max(1e-12, 10 E0), E0 the
    unboxed engine's deviation over the same horizon"""
    name, H = "inverted_pendulum", 8
    m = ia.Model.load(model_path(name))
    dm = _dmain(ia, m, name)
    rows = cs.make_schedule(ia.PENDULUM_COST, m, H)
    # limits and seeded gains chosen on the CPU reference alone: the selected
    # rollout clamps 6 of its 9 controls and one backward step leaves the fast
    # path, its margin 2e-2 of the step's scale
    lo, hi = np.array([-0.004]), np.array([0.006])
    rng = np.random.default_rng(20261020)
    P = H + 1
    K0 = rng.standard_normal((1, P, m.nu * 2 * m.nv)) * 0.5
    k0 = rng.standard_normal((1, P, m.nu)) * 0.05
    inf = np.full(m.nu, np.inf)

    free = ia.ILQR(m, dm, H, ia.PENDULUM_COST, alphas=ALPHAS, select="min_cost")
    free.set_cost_schedule(rows)
    free.set_gains(K0, k0)
    free.iterate()
    E0, _ = _box_deviation(free, m, -inf, inf, H)

    g = ia.ILQR(m, dm, H, ia.PENDULUM_COST, alphas=ALPHAS, select="min_cost")
    g.set_cost_schedule(rows)
    g.set_ctrl_limits(lo, hi)
    g.set_gains(K0, k0)
    g.iterate()
    snap = _snapshot(g)

    om = ora.OModel(m.blob())
    ref = cs.SchedRef(ora, m, om, _state_dict(dm, 0), H, rows, ALPHAS, lo=lo, hi=hi)
    ref.il.set_gains(K0[0], k0[0])
    c, sel = ref.forward()
    recs = ref.sweep()
    assert 0 < ref.clamped < P, "the limits must bind in the selected rollout, and not everywhere"
    exact(snap["costs"][0], c, "candidate costs over the clamped trajectories")
    assert snap["sel"][0] == sel
    rt = ref.traj()
    for f in cs.FIELDS:
        exact(snap[f].reshape(rt[f].shape), rt[f], f"traj.{f}")
    assert np.any(snap["ctrl"] == lo[0]) or np.any(snap["ctrl"] == hi[0])
    assert np.all(snap["ctrl"] >= lo[0]) and np.all(snap["ctrl"] <= hi[0])
    exact(snap["deriv"][0], recs, "scheduled records")
    dev, bref = _box_deviation(g, m, lo, hi, H)
    mask, info = g.clamped()
    tol = max(1e-12, 10 * E0)
    print(f"schedule + limits: E0 = {E0:.3e}, tol = {tol:.3e}, boxed deviation = {dev:.3e}, "
          f"clamped steps {int(np.count_nonzero(mask[0, 1:]))} of {H}, rollout clamps {ref.clamped}")
    # the input condition of test_ctrl_limits.py: no step decided by rounding
    assert np.all(bref["margin"][1:] > 1e-6 * bref["scale"][1:]), float(np.min(bref["margin"][1:] / bref["scale"][1:]))
    assert bref["mask"].any(), "a backward step must leave the fast path"
    assert np.array_equal(mask[0], bref["mask"]), (mask[0], bref["mask"])
    assert not (info >> 31).any()
    assert dev <= tol, (dev, tol, E0)


@gpu
def test_seed_groups(ia):
    """7: two seed groups read the same schedule: everything equals the ungrouped scheduled run"""
    import workloads
    name, H = "hopper", 12
    m = ia.Model.load(model_path(name))
    dm = workloads.hopper_dmain(m, 2, sigma=0.01)
    rows = cs.make_schedule(ia.HOPPER_COST, m, H)
    a = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS, select="min_cost")
    b = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS, select="min_cost")
    for g in (a, b):
        g.set_cost_schedule(rows)
    b.set_groups(2)
    assert b.groups == 2
    for it in range(2):
        a.iterate()
        b.iterate()
        _same(_snapshot(a), _snapshot(b), f"groups it{it}")
    s = _snapshot(a)
    assert np.any(s["K"][0] != s["K"][1])


@gpu
def test_shift(ia):
    """8: the receding-horizon tick: shift by 1 and by 3, then iterate as a solver given the shifted array"""
    name, H = "hopper", 12
    m = ia.Model.load(model_path(name))
    dm = _dmain(ia, m, name)
    rows = cs.make_schedule(ia.HOPPER_COST, m, H)
    new = cs.make_schedule(ia.HOPPER_COST, m, H, seed=7)[3:7]
    g = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS, select="min_cost")
    g.set_cost_schedule(rows)
    g.iterate()
    g.shift_cost_schedule(new[0], 1)
    want = np.concatenate([new[:1], rows[:-1]])
    exact(g.cost_schedule(), want, "shift 1")
    g.shift_cost_schedule(new[1:], 3)
    want = np.concatenate([new[1:], want[:-3]])
    exact(g.cost_schedule(), want, "shift 3")
    h = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS, select="min_cost")
    h.set_cost_schedule(rows)
    h.iterate()
    h.set_cost_schedule(want)
    g.iterate()
    h.iterate()
    _same(_snapshot(g), _snapshot(h), "after the shifts")
    full = cs.make_schedule(ia.HOPPER_COST, m, H, seed=9)
    g.shift_cost_schedule(full, H + 1)
    exact(g.cost_schedule(), full, "shift by the whole window")


@gpu
def test_arguments(ia):
    """9: refused arguments (ILQG_ERR_ARG = 1) and the getter while off"""
    name, H = "inverted_pendulum", 8
    m = ia.Model.load(model_path(name))
    g = ia.ILQR(m, _dmain(ia, m, name), H, ia.PENDULUM_COST)
    rows = cs.make_schedule(ia.PENDULUM_COST, m, H)
    C = rows.shape[1]
    on = np.zeros(1, dtype=np.int32)
    got = np.full((H + 1, C), np.nan)
    L = ia.lib()
    import ctypes
    ip = ctypes.POINTER(ctypes.c_int)
    assert L.ilqg_solver_get_cost_schedule(g._h, ia._ptr(got), on.ctypes.data_as(ip)) == 0
    assert on[0] == 0
    exact(got, cs.constant_schedule(ia.PENDULUM_COST, m, H), "get while off: the creation cost")
    assert L.ilqg_solver_get_cost_schedule(g._h, None, None) == 0
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule(rows[0], 1)  # off
    for bad in (np.nan, np.inf, -np.inf):
        r = rows.copy()
        r[H, C - 1] = bad
        with pytest.raises(ia.IlqgError, match="code 1"):
            g.set_cost_schedule(r)
        assert g.cost_schedule() is None
    g.set_cost_schedule(rows)
    assert L.ilqg_solver_get_cost_schedule(g._h, None, on.ctypes.data_as(ip)) == 0 and on[0] == 1
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule(rows[:1], 0)
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule(np.concatenate([rows, rows[:1]]), H + 2)
    assert L.ilqg_solver_shift_cost_schedule(g._h, 1, None) == 1
    r = rows[:2].copy()
    r[1, 0] = np.nan
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule(r, 2)
    exact(g.cost_schedule(), rows, "refused calls change nothing")
    with pytest.raises(ia.IlqgError):
        g.set_cost_schedule(rows[:-1])
    g.set_cost_schedule([_row_cost(ia, m, r) for r in rows])
    exact(g.cost_schedule(), rows, "a sequence of Costs")

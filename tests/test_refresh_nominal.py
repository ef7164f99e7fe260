"""The nominal refresh (ilqg_solver_refresh_nominal): the stored nominal's cost
recomputed on the device -- or the stored policy rolled out again from dinit --
so that the regularisation mode's accept test, its mu schedule and its stop
survive a receding-horizon tick.

CPU: the Python restatement of the charge (nominal_ref.traj_cost) pinned
against the oracle's rollout under a schedule; the symbol and its refusal of a
null solver.  GPU: COST against the rollout's own charge and the restatement,
after a shift, with the accept test alive; REROLL against a twin solver of one
candidate with feed-forward scale 0; RESUME; asynchrony; arguments; the off
path.  Bit for bit throughout: every comparison is of the same additions on the
same operands, so there is no tolerance to state.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import applied_forces as af
import cost_sched_ref as cs
import nominal_ref as nr
import reg_ref as rr
import sched_seeds as ss
import test_std_recursion as tsr
from conftest import ROOT
from sched_seeds import exact

gpu = pytest.mark.gpu
NAME = "ilqg_solver_refresh_nominal"
ERR_ARG = 1
ALPHAS4 = (1.0, 0.5, 0.25, 0.125)
FIELDS = cs.FIELDS
H = 20
# the kernel charges NOMC_TILE = 256 points per pass (kernels_shift.hip): 301
# points are one full pass and a part of one, the carry between them included
H_TILES = 300


# ---------------------------------------------------------------- CPU ----
@pytest.mark.parametrize("sched", ("schedule", "constant"))
def test_restatement_is_the_rollouts_charge(ia, ora, sched):
    """hopper H = 8 on the oracle: traj_cost of a rolled-out candidate is the
    candidate cost SchedRef returns, after an iterate() (gains and a nominal
    that the candidates leave)"""
    N = 8
    m = tsr._model(ia, "hopper")
    om, st = tsr._oracle_state(ora, m, "hopper")
    rows = cs.make_schedule(ia.HOPPER_COST, m, N) if sched == "schedule" else cs.constant_schedule(ia.HOPPER_COST, m, N)
    ref = cs.SchedRef(ora, m, om, st, N, rows, alphas=ALPHAS4)
    ref.iterate()
    seen = []
    for alpha in (1.0, 0.25, 0.0):
        rec, c, _ = ref.rollout(alpha)
        got = nr.traj_cost(rows, np.array(rec["qpos"]), np.array(rec["qvel"]), np.array(rec["ctrl"]))
        print(f"{sched} alpha {alpha}: oracle {c!r} restatement {got!r}")
        assert np.float64(got).tobytes() == np.float64(c).tobytes(), (alpha, got, c)
        seen.append(c)
    assert len(set(seen)) == 3 and all(np.isfinite(seen))


def test_symbol_and_null_refusal(ia):
    """fails without the feature: the declaration, the binding's list, the library's symbol"""
    with open(os.path.join(ROOT, "include", "ilqg_amd.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(ilqg_solver\*\s*\w+,\s*int\s+\w+,\s*unsigned\s+\w+\);", hdr)
    for d, v in (("ILQG_NOMINAL_COST", "0"), ("ILQG_NOMINAL_REROLL", "1"), ("ILQG_NOMINAL_RESUME", "1u")):
        assert re.search(r"#define\s+" + d + r"\s+" + v + r"\b", hdr), d
    assert NAME in ia.EXPORTS
    L = ia.lib()
    assert hasattr(L, NAME)
    assert L.ilqg_solver_refresh_nominal(None, 0, 0) == ERR_ARG        # before any device call
    assert ia.NOMINAL_MODES == {"cost": 0, "reroll": 1} and ia.NOMINAL_RESUME == 1
    with pytest.raises(ia.IlqgError, match="mode"):
        ia.ILQR.refresh_nominal(object.__new__(ia.ILQR), "bogus")


# ---------------------------------------------------------------- GPU ----
def _seedwise(g):
    t = g.traj()
    return {f: getattr(t, f).reshape(g.S, g.P, -1).copy() for f in FIELDS}


def _sel_costs(g):
    """the selected-cost buffer (ilqg_solver_device_costs), copied to the host"""
    from seed_shard import device_view
    g.synchronize()
    return device_view(g.device_costs_ptr(), g.S).cpu().numpy().copy()


def _poison_sel_costs(g):
    """NaN into the selected-cost buffer: whatever reads right afterwards was written afterwards"""
    import torch
    from seed_shard import device_view
    g.synchronize()
    device_view(g.device_costs_ptr(), g.S).fill_(float("nan"))
    torch.cuda.synchronize()


def _nominal_costs(g, t=None):
    """traj_cost of every seed's stored nominal under the rows in force"""
    rows, _ = g.cost_schedule_seeds()
    t = t or _seedwise(g)
    return np.array([nr.traj_cost(rows[s], t["qpos"][s], t["qvel"][s], t["ctrl"][s]) for s in range(g.S)])


def _hopper(ia, S=2):
    import workloads
    m = tsr._model(ia, "hopper")
    return m, workloads.hopper_dmain(m, S, sigma=0.01)


def _reg_solver(ia, m, dm, alphas=ALPHAS4, **opts):
    """STANDARD, corrected layout, mu = 1000, the regularisation mode on"""
    g = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=alphas, select="min_cost", mu=1000.0)
    g.set_layout("corrected")
    g.set_recursion("standard")
    g.set_regularization(True, **opts)
    return g


COST_CASES = ("hopper", "hopper_sched", "hopper_seeds", "hopper_limits", "pendulum", "humanoid", "pendulum_tiles")


def _cost_case(ia, case):
    name = {"pendulum": "inverted_pendulum", "pendulum_tiles": "inverted_pendulum", "humanoid": "humanoid"}.get(
        case, "hopper")
    N = {"humanoid": 4, "pendulum_tiles": H_TILES}.get(case, H)
    m = af.model(ia, name)
    if name == "hopper":
        st = _hopper(ia)[1]
    elif name == "humanoid":
        st = m.reset_state(1)
        st.qpos[:, 2] = 1.4
    else:
        st = tsr._dmain(ia, m, name, 2)
    c = af.cost(ia, name)

    def make():
        g = ia.ILQR(m, st, N, c, alphas=ALPHAS4, select="min_cost")
        if case == "hopper_sched":
            g.set_cost_schedule(cs.make_schedule(c, m, N))
        if case == "hopper_seeds":
            g.set_cost_schedule_seeds(ss.seed_rows(c, m, N, S=2))
        if case == "hopper_limits":
            g.set_ctrl_limits("model")
        return g
    return m, make


@gpu
@pytest.mark.parametrize("case", COST_CASES)
def test_cost_is_the_rollouts_charge(ia, case):
    """after forward_pass(), refresh_nominal('cost') writes costs()[s, sel[s]] and
    traj_cost(traj()) into the (poisoned) selected-cost buffer and changes nothing
    else; dinit through a second forward_pass() beside a solver that never refreshed"""
    m, make = _cost_case(ia, case)
    g, plain = make(), make()
    # (the long horizon is about the sum's carry from pass to pass: the passive
    # nominal, whose candidates coincide, serves; elsewhere an iterate() first
    # gives gains, so that the candidates differ)
    tiles = case == "pendulum_tiles"
    for x in (g, plain):
        if not tiles:
            x.iterate()
        x.forward_pass()
    costs, sel = g.costs()
    t0, (K0, k0) = _seedwise(g), g.gains()
    assert case != "humanoid" or m.nq != m.nv
    assert np.all(np.isfinite(costs)) and (tiles or all(len(set(row)) > 1 for row in costs.tolist()))
    assert not tiles or (g.P > 256 and g.P % 256 != 0)
    want = np.array([costs[s, sel[s]] for s in range(g.S)])
    exact(_sel_costs(g), want, f"{case}: the selection's own store")
    _poison_sel_costs(g)
    g.refresh_nominal("cost")
    got = _sel_costs(g)
    ref = _nominal_costs(g)
    print(f"{case}: device {got.tolist()} rollout {want.tolist()} restatement {ref.tolist()}")
    exact(got, want, f"{case}: refresh against the rollout's charge")
    exact(got, ref, f"{case}: refresh against traj_cost")
    t1, (K1, k1) = _seedwise(g), g.gains()
    for f in FIELDS:
        exact(t1[f], t0[f], f"{case}: trajectory {f}")
    exact(K1, K0, "K")
    exact(k1, k0, "k")
    c1, s1 = g.costs()
    exact(c1, costs, "candidate costs")
    exact(s1, sel, "sel")
    for x in (g, plain):
        x.forward_pass()
    exact(g.costs()[0], plain.costs()[0], f"{case}: the next rollout's costs (dinit)")
    exact(g.traj().qpos, plain.traj().qpos, f"{case}: the next rollout's qpos (dinit)")


def _state_dicts(st, S):
    return [dict(mu=float(st["mu"][s]), dmu=float(st["dmu"][s]), cost_nom=float(st["cost_nom"][s]),
                 valid=int(st["valid"][s]), status=int(st["status"][s])) for s in range(S)]


def _iterate_against_decide(g, opts, alphas=ALPHAS4):
    """one iterate(); the decision recomputed on the host (reg_ref.decide) from the
    state before, the device's own candidate costs and the last pass's dV"""
    before = _state_dicts(g.reg_state(), g.S)
    dV, _ = g.expected()
    g.iterate()
    costs, sel = g.costs()
    st = g.reg_state()
    o = rr.options(**opts)
    picks = []
    for s in range(g.S):
        d = before[s]
        pick, _, _ = rr.decide(o, d, costs[s], alphas, dV[s], 1)
        for _ in range(int(st["retries"][s])):
            d["mu"], d["dmu"], d["status"] = rr.increase(o, d["mu"], d["dmu"], d["status"])
        assert sel[s] == pick, (s, sel[s], pick)
        for f in ("mu", "dmu", "cost_nom", "status", "valid"):
            assert np.float64(st[f][s]).tobytes() == np.float64(d[f]).tobytes(), (s, f, st[f][s], d[f])
        picks.append(pick)
    return picks, st


@gpu
def test_after_a_shift(ia):
    """two iterate(), shift_horizon(1): valid 0 (pinned today).  refresh_nominal('cost'):
    valid 1, cost_nom = traj_cost of the shifted nominal, the rest of the state and
    the trace untouched.  The next iterate() decides as reg_ref.decide does and its
    trace slot carries the refreshed cost."""
    m, dm = _hopper(ia)
    opts = dict(trace_len=8)
    g = _reg_solver(ia, m, dm, **opts)
    g.iterate()
    g.iterate()
    g.shift_horizon(1)
    s0 = g.reg_state()
    n0 = len(g.reg_trace())
    assert not s0["valid"].any() and n0 == 2
    _poison_sel_costs(g)
    g.refresh_nominal("cost")
    s1 = g.reg_state()
    want = _nominal_costs(g)
    assert s1["valid"].all()
    exact(s1["cost_nom"], want, "cost_nom against traj_cost of the shifted nominal")
    exact(_sel_costs(g), want, "selected costs")
    for f in ("mu", "dmu", "status", "retries"):
        exact(s1[f], s0[f], f"reg {f}")
    assert len(g.reg_trace()) == n0
    picks, st = _iterate_against_decide(g, opts)
    tr = g.reg_trace()
    assert len(tr) == n0 + 1
    exact(tr[-1][:, 0], want, "trace field 0: the refreshed cost")
    print("picks", picks, "mu", st["mu"].tolist(), "nominal", want.tolist())


@gpu
def test_accept_test_is_alive_after_a_tick(ia):
    """zmin = 1e6: no step can be accepted.  With the refresh the tick's step is
    rejected, the nominal keeps its bits and mu takes the increase; without it the
    step is taken whatever it costs and mu stays (today's behaviour)."""
    m, dm = _hopper(ia)
    opts = dict(trace_len=8, zmin=1e6)
    o = rr.options(**opts)
    out = {}
    for refresh in (True, False):
        g = _reg_solver(ia, m, dm, **opts)
        g.iterate()
        g.iterate()
        dV, bad = g.expected()
        assert np.all(bad == -1)
        assert all(rr.expected(a, dV[s]) > 0 for s in range(g.S) for a in ALPHAS4), dV
        g.shift_horizon(1)
        if refresh:
            g.refresh_nominal("cost")
        before, t0 = g.reg_state(), _seedwise(g)
        g.iterate()
        out[refresh] = (before, t0, g.costs()[1].copy(), g.reg_state(), _seedwise(g))
    before, t0, sel, st, t1 = out[True]
    assert list(sel) == [-1, -1]
    for f in FIELDS:
        exact(t1[f], t0[f], f"rejected: nominal {f}")
    for s in range(2):
        mu, dmu, status = rr.increase(o, float(before["mu"][s]), float(before["dmu"][s]), int(before["status"][s]))
        assert st["mu"][s] == mu and st["dmu"][s] == dmu and st["status"][s] == status == 0
        assert mu > before["mu"][s]
    before, t0, sel, st, t1 = out[False]
    assert np.all(sel >= 0)
    exact(st["mu"], before["mu"], "without the refresh mu stays")
    assert np.any(t1["ctrl"] != t0["ctrl"])


REROLL_CASES = ("plain", "limits", "seeds", "reg")
LIM = 0.12      # tighter than the hopper's ctrlrange: the optimised controls reach it


def _reroll_configure(ia, g, m, case, twin=False):
    if case == "limits":
        g.set_ctrl_limits(-LIM, LIM)
    if case == "seeds":
        g.set_cost_schedule_seeds(ss.seed_rows(ia.HOPPER_COST, m, H, S=2))
    if case == "reg":
        g.set_layout("corrected")
        g.set_recursion("standard")
        if not twin:
            g.set_regularization(True, trace_len=8)


@gpu
@pytest.mark.parametrize("case", REROLL_CASES)
def test_reroll_against_twin(ia, case):
    """two iterate(), set_dinit(a displaced state), refresh_nominal('reroll') against
    a solver of one candidate, alphas (0.0,), select 'reference', given the same
    nominal, gains and dinit, after forward_pass(): the five fields and the selected
    cost.  dinit (no getter): a second reroll / forward_pass() starts from it."""
    m, dm = _hopper(ia)
    g = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS4, select="min_cost", mu=1000.0)
    _reroll_configure(ia, g, m, case)
    g.iterate()
    g.iterate()
    t0, (K0, k0) = g.traj(), g.gains()
    assert np.any(K0 != 0) and np.any(k0 != 0)
    d = dm.copy()
    d.qpos[:, 1] += 0.05
    g.set_dinit(d)
    n0 = len(g.reg_trace()) if case == "reg" else None
    _poison_sel_costs(g)
    g.refresh_nominal("reroll")
    twin = ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=(0.0,), select="reference", mu=1000.0)
    _reroll_configure(ia, twin, m, case, twin=True)
    twin.set_traj(t0)
    twin.set_gains(K0, k0)
    twin.set_dinit(d)
    twin.forward_pass()
    for rnd in (0, 1):
        a, b = _seedwise(g), _seedwise(twin)
        for f in FIELDS:
            exact(a[f], b[f], f"{case} round {rnd}: {f}")
        exact(_sel_costs(g), _sel_costs(twin), f"{case} round {rnd}: selected cost")
        exact(_sel_costs(g), twin.costs()[0][:, 0], f"{case} round {rnd}: the twin's candidate cost")
        exact(_sel_costs(g), _nominal_costs(g), f"{case} round {rnd}: traj_cost")
        K1, k1 = g.gains()
        exact(K1, K0, "K")
        exact(k1, k0, "k")
        if rnd == 0:
            first = a
            exact(a["qpos"][:, -1], d.qpos, "the rollout starts from dinit")
            assert np.any(a["qpos"] != t0.qpos.reshape(a["qpos"].shape))
            if case == "limits":
                assert np.any(np.abs(a["ctrl"]) == LIM), "no limit binds"
                assert np.all(np.abs(a["ctrl"]) <= LIM)
            if case == "reg":
                st = g.reg_state()
                assert st["valid"].all() and len(g.reg_trace()) == n0
                exact(st["cost_nom"], _sel_costs(g), "cost_nom")
            g.refresh_nominal("reroll")
            twin.forward_pass()
    print(f"{case}: selected costs {_sel_costs(g).tolist()}; max |ctrl| {np.abs(first['ctrl']).max():.4g}")


@gpu
def test_resume(ia):
    """tol_cost = 1e9: status 1 after the second iterate(), the third is frozen.
    refresh_nominal('cost') keeps the status; resume=True sets it to 0 with mu and
    dmu untouched, and the next iterate() decides as reg_ref.decide does.  A seed
    at status 2 stays there."""
    m, dm = _hopper(ia)
    opts = dict(trace_len=8, tol_cost=1e9)
    g = _reg_solver(ia, m, dm, **opts)
    g.iterate()
    g.iterate()
    st = g.reg_state()
    assert list(st["status"]) == [1, 1] and list(g.costs()[1] >= 0) == [True, True]
    g.iterate()
    assert list(g.costs()[1]) == [-1, -1]
    s0 = g.reg_state()
    g.refresh_nominal("cost")
    s1 = g.reg_state()
    assert list(s1["status"]) == [1, 1]
    g.refresh_nominal("cost", resume=True)
    s2 = g.reg_state()
    assert list(s2["status"]) == [0, 0] and s2["valid"].all()
    for f in ("mu", "dmu", "cost_nom"):
        exact(s1[f], s0[f], f"refresh: {f}")
        exact(s2[f], s0[f], f"resume: {f}")
    picks, _ = _iterate_against_decide(g, opts)
    assert all(p >= 0 for p in picks)       # running again: the accepting schedule goes on
    # status 2: mu_max reached on the second iterate's rejection
    opts2 = dict(mu_max=1500.0, zmin=1e6)
    g2 = _reg_solver(ia, m, dm, **opts2)
    g2.iterate()
    g2.iterate()
    assert list(g2.reg_state()["status"]) == [2, 2]
    g2.refresh_nominal("cost", resume=True)
    st = g2.reg_state()
    mu2 = rr.increase(rr.options(**opts2), 1000.0, 1.0, 0)[0]
    assert list(st["status"]) == [2, 2] and list(st["mu"]) == [mu2, mu2] and mu2 >= 1500.0
    g2.refresh_nominal("reroll", resume=True)
    assert list(g2.reg_state()["status"]) == [2, 2]


@gpu
def test_ticks_without_host_sync(ia):
    """three ticks of shift_horizon(1); refresh_nominal('cost', resume=True); iterate()
    enqueued back to back equal the same ticks with synchronize() after every call"""
    m, dm = _hopper(ia)
    out = []
    for sync in (False, True):
        g = _reg_solver(ia, m, dm, trace_len=8)
        g.iterate()
        g.iterate()
        for _ in range(3):
            for call in (lambda: g.shift_horizon(1), lambda: g.refresh_nominal("cost", resume=True), g.iterate):
                call()
                if sync:
                    g.synchronize()
        tr = g.reg_trace()      # read once
        out.append((af.results(g), g.reg_state(), tr, _sel_costs(g)))
    (ra, sa, ta, ca), (rb, sb, tb, cb) = out
    for f in af.FIELDS + ("dV", "first_bad"):
        exact(ra[f], rb[f], f"ticks {f}")
    for f in sa:
        exact(sa[f], sb[f], f"ticks reg {f}")
    exact(ca, cb, "selected costs")
    assert ta.shape[0] == 5 and np.array_equal(ta, tb, equal_nan=True)
    assert not np.isnan(ta[2:, :, 0]).any() and np.isnan(ta[0, :, 0]).all()


@gpu
def test_arguments(ia):
    m, dm = _hopper(ia)
    mk = lambda: ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS4, select="min_cost")
    g, fresh = mk(), mk()
    L = ia.lib()
    for mode, flags in ((2, 0), (-1, 0), (0, 2), (1, 3), (0, 1), (1, 1)):     # (RESUME: the mode is off)
        assert L.ilqg_solver_refresh_nominal(g._h, mode, flags) == ERR_ARG, (mode, flags)
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.refresh_nominal("cost", resume=True)
    with pytest.raises(ia.IlqgError):
        g.refresh_nominal("again")
    # a solver that was created but never initialised
    alphas = np.ones(1)
    o = ia._Opts(horizon=H, nseed=2, nalpha=1, alphas=ia._ptr(alphas), select_mode=0, mu=1000.0, device=0)
    c = ia.HOPPER_COST.struct(m.nq, m.nv, m.nu)
    h = ctypes.c_void_p()
    assert L.ilqg_solver_create(m._h, ctypes.byref(o), ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        assert L.ilqg_solver_refresh_nominal(h, 0, 0) == ERR_ARG
        assert L.ilqg_solver_refresh_nominal(h, 1, 0) == ERR_ARG
    finally:
        L.ilqg_solver_free(h)
    # the refused calls changed nothing
    g.iterate()
    fresh.iterate()
    ra, rb = af.results(g), af.results(fresh)
    for f in af.FIELDS:
        exact(ra[f], rb[f], f"after refused calls {f}")
    exact(_sel_costs(g), _sel_costs(fresh), "selected costs")


@gpu
def test_off_path(ia):
    """the reference recursion: forward_pass(); refresh_nominal('cost'); two iterate()
    equal a solver that never made the call, on the fused sweep; the cost kernel is
    timed under 'select', the reroll's rollout under 'rollout'; with two seed groups
    iterate(); shift_horizon(1); refresh_nominal('cost'); iterate() is the ungrouped solver's"""
    m, dm = _hopper(ia)
    mk = lambda: ia.ILQR(m, dm, H, ia.HOPPER_COST, alphas=ALPHAS4, select="min_cost")
    out = []
    for call in (True, False):
        g = mk()
        g.forward_pass()
        g.set_timing(True)
        if call:
            g.refresh_nominal("cost")
            tm = g.timing()
            assert tm["select"][1] == 1 and tm["rollout"][1] == 0, tm
        g.iterate()
        g.iterate()
        r = af.results(g)
        tm = g.timing()
        assert tm["fd_backward"][1] == 2 and tm["backward"][1] == 0, tm
        out.append(r)
    for f in af.FIELDS:
        exact(out[0][f], out[1][f], f"off path {f}")
    g.refresh_nominal("reroll")
    tm = g.timing()
    assert tm["rollout"][1] == 1 and tm["select"][1] == 1, tm
    a, b = mk(), mk()
    a.set_groups(2)
    assert a.groups == 2
    for x in (a, b):
        x.iterate()
        x.shift_horizon(1)
        x.refresh_nominal("cost")
        x.iterate()
    ra, rb = af.results(a), af.results(b)
    for f in af.FIELDS:
        exact(ra[f], rb[f], f"groups {f}")
    exact(_sel_costs(a), _sel_costs(b), "groups: selected costs")

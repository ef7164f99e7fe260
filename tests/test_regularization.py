"""The regularisation mode (ilqg_solver_set_regularization): per-seed mu / dmu
schedule, step acceptance and the restarting backward pass on the device.

The reference is tests/reg_ref.py: the schedule and the acceptance rule in
Python floats in the header's order, composed with std_ref.StdRef's oracle
rollout and recursions.  Decisions, mu and trajectories are compared bit for
bit (in replay mode the reference is driven with the device's gains and dV, as
test_std_recursion.test_end_to_end does); gains, V, v, dV within
std_ref.tol(E64), the reference's own fp64-against-longdouble deviation.

The unmarked tests pin the reference: the decisions the loop takes on the oracle
and the margins that make those decisions meaningful -- every |actual| at least
1e-6 of the nominal cost, every pivot of the restart case at least 1e-6 of the
largest diagonal entry -- are asserted before anything is compared."""
import ctypes
import os
import re

import numpy as np
import pytest

import cost_sched_ref as csr
import reg_ref as rr
import riccati_cases as rc
import std_ref as sr
import test_std_recursion as tsr
from conftest import ROOT

gpu = pytest.mark.gpu
UNSUPPORTED, ERR_ARG = 4, 1
ALPHAS4 = tsr.ALPHAS4
INC = [1e-6, 2.56e-6, 1.049e-5, 6.872e-5, 7.206e-4, 0.01209, 0.3245, 13.94, 957.8, 1.053e5]
DEC = [625.0, 244.1, 59.6, 9.095, 0.8674, 0.0517, 0.001926]
RESTART_C, RESTART_WU = 1e-3, 1e-12


def _seq(n, mu, up, o=None):
    o, dmu, st, out = o or rr.options(), 1.0, 0, []
    for _ in range(n):
        if up:
            mu, dmu, st = rr.increase(o, mu, dmu, st)
        else:
            mu, dmu = rr.decrease(o, mu, dmu)
        out.append(mu)
    return out


# ------------------------------------------------------------------ CPU --
def test_exports(ia):
    """fails on the parent: no such entry points"""
    L = ia.lib()
    hdr = open(os.path.join(ROOT, "include", "ilqg_amd.h")).read()
    for name in ("ilqg_solver_set_regularization", "ilqg_solver_get_regularization", "ilqg_solver_get_reg_state",
                 "ilqg_solver_set_reg_mu", "ilqg_solver_get_reg_trace"):
        assert hasattr(L, name), name
        assert name in ia.EXPORTS
        assert re.search(r"int\s+" + name + r"\(ilqg_solver\*", hdr), name
    assert re.search(r"#define\s+ILQG_REG_MAXRETRY\s+16", hdr)
    assert "typedef struct ilqg_reg_opts" in hdr
    for fld in ("factor", "mu_min", "mu_max", "zmin", "tol_cost", "max_retry", "trace_len"):
        assert re.search(r"(double|int)\s+" + fld + r";", hdr), fld
    for meth in ("set_regularization", "reg_state", "reg_trace", "set_reg_mu"):
        assert hasattr(ia.ILQR, meth), meth


def test_schedule_alone():
    up = _seq(10, 0.0, True)
    down = _seq(7, 1000.0, False)
    print("increases from 0:", " ".join(f"{x:.4g}" for x in up))
    print("decreases from 1000:", " ".join(f"{x:.4g}" for x in down))
    assert np.allclose(up, INC, rtol=2e-3, atol=0) and up[0] == 1e-6
    assert np.allclose(down, DEC, rtol=2e-3, atol=0) and down[0] == 625.0
    # below mu_min the decrease lands on 0, and the next increase on mu_min
    o = rr.options()
    assert rr.decrease(o, 1.5e-6, 1.0 / 1.6)[0] == 0.0
    assert rr.increase(o, 0.0, 1.0, 0) == (1e-6, 1.6, 0)
    assert rr.increase(rr.options(mu_max=1e3), 900.0, 1.0, 0)[2] == 2
    # a NaN is never acceptable
    st = dict(mu=1.0, dmu=1.0, cost_nom=2.0, valid=1, status=0)
    assert rr.decide(o, st, [float("nan")], (1.0,), [-1.0, 0.5], 1)[0] == -1
    st = dict(mu=1.0, dmu=1.0, cost_nom=2.0, valid=1, status=0)
    assert rr.decide(o, st, [1.0], (1.0,), [float("nan"), 0.5], 1)[0] == -1


def _loop(ia, ora, name, H, alphas, mu, opts, iters):
    ref = tsr._std_ref(ia, ora, name, H, alphas=alphas, mu=mu)
    g = rr.RegRef(ref, opts, mu)
    log = []
    for _ in range(iters):
        nom_before = g.traj()
        cn = g.st["cost_nom"] if g.st["valid"] else None
        costs, pick = g.iterate()
        log.append(dict(pick=pick, costs=costs, cost_nom=cn, ratio=g.ratios[-1], mu=g.st["mu"], status=g.st["status"],
                        retries=g.retries, unchanged=all(np.array_equal(nom_before[f], g.traj()[f])
                                                         for f in ("qpos", "qvel", "ctrl"))))
    return g, log


def _meaningful(log):
    """|actual| >= 1e-6 cost_nom at every decision (the first step has no nominal cost)"""
    worst = min(abs(e["cost_nom"] - min(e["costs"])) / e["cost_nom"] for e in log[1:])
    assert worst >= 1e-6, worst
    return worst


def test_reference_accepting_schedule(ia, ora):
    """hopper H = 20, four alphas, mu = 1000: every step accepted at alpha = 1 with
    actual / expected in 1.001 .. 1.002, mu down DEC, cost 1.67467 -> 0.399106"""
    g, log = _loop(ia, ora, "hopper", 20, ALPHAS4, 1000.0, rr.options(), 8)
    w = _meaningful(log)
    ratios = [e["ratio"] for e in log[1:]]
    noms = [round(float(e["cost_nom"]), 6) for e in log[1:]] + [round(g.st["cost_nom"], 6)]
    mus = [float("%.4g" % e["mu"]) for e in log]
    print(f"margin {w:.3g}; ratios {min(ratios):.5f} .. {max(ratios):.5f}; nominal costs {noms}; mu {mus}")
    assert all(e["pick"] == 0 and e["retries"] == 0 for e in log)
    assert all(1.001 <= r <= 1.002 for r in ratios)
    assert log[0]["mu"] == 1000.0 and np.allclose([e["mu"] for e in log[1:]], DEC, rtol=2e-3)
    assert abs(log[0]["costs"][0] - 1.67467) < 1e-5 and abs(g.st["cost_nom"] - 0.399106) < 1e-6


def test_reference_forced_rejection(ia, ora):
    """pendulum H = 20, alphas (1,), mu = 0, zmin = 2, mu_max = 1e3: every step
    rejected with actual / expected in 1.002 .. 1.014 (< 1.5), status 2 on the tenth"""
    o = rr.options(zmin=2.0, mu_max=1e3)
    g, log = _loop(ia, ora, "inverted_pendulum", 20, (1.0,), 0.0, o, 12)
    w = _meaningful(log[:11])
    ratios = [e["ratio"] for e in log[1:11]]
    print(f"margin {w:.3g}; ratios {min(ratios):.5f} .. {max(ratios):.5f}")
    assert all(e["pick"] == -1 and e["unchanged"] for e in log[1:])
    assert all(1.0 < r < 1.5 for r in ratios)
    assert [e["mu"] for e in log[1:11]] == _seq(10, 0.0, True, o)
    assert [e["status"] for e in log[:11]] == [0] * 10 + [2] and log[11]["mu"] == log[10]["mu"]


def test_reference_natural_rejections(ia, ora):
    """hopper H = 100, alphas (1,), mu = 0, sixteen iterations: 1-8 rejected, 9, 10
    accepted, 11 rejected, 12-15 accepted; 109.553 -> 21.151, final mu 0.04952"""
    g, log = _loop(ia, ora, "hopper", 100, (1.0,), 0.0, rr.options(), 16)
    w = _meaningful(log)
    picks = [e["pick"] for e in log]
    print(f"margin {w:.3g}; picks {picks}; ratios {[round(e['ratio'], 4) for e in log[1:]]}; "
          f"cost {log[0]['costs'][0]:.6g} -> {g.st['cost_nom']:.6g}; mu {g.st['mu']:.4g}")
    assert picks == [0] + [-1] * 8 + [0, 0, -1, 0, 0, 0, 0]
    assert all(e["unchanged"] == (e["pick"] < 0) for e in log[1:])   # (the first rollout repeats the passive one)
    assert abs(log[0]["costs"][0] - 109.553) < 1e-3 and abs(g.st["cost_nom"] - 21.151) < 1e-3
    assert abs(g.st["mu"] - 0.04952) < 1e-5


def _restart_case(ia, name):
    """family-D dense records, V0 = -c I, wu tiny: Quu_r ~ (mu - c) B'B is
    indefinite until mu > c.  -> (model, cost, records (2, 3, D), V0, v0, lxx, luu)"""
    m = tsr._model(ia, name)
    c0 = tsr._gcost(ia, name)
    cost = ia.Cost(wq=c0.wq, tq=c0.tq, wv=c0.wv, wu=[RESTART_WU] * m.nu)
    cases = [c for c in rc.make_cases(m.nv, m.nu, m.timestep) if c.family == "D"]
    rec = np.stack([c.rec for c in cases])
    nx = 2 * m.nv
    V0 = np.tile((-RESTART_C * np.eye(nx)).ravel(), (2, 1))
    v0 = np.random.default_rng(20261020).standard_normal((2, nx))
    lxx, luu = sr.hessians(csr.constant_schedule(cost, m, rc.H), m.nq, m.nv, m.nu)
    return m, cost, rec, V0, v0, lxx, luu


def _restart_ref(m, rec, V0, v0, lxx, luu, s, opts):
    st = dict(mu=0.0, dmu=1.0, status=0)
    out, retries, tried, margin = rr.backward_restart(opts, st, rec[s], m.nv, m.nu, m.timestep, "reference", lxx, luu,
                                                      V0[s], v0[s])
    return st, out, retries, tried, margin


@pytest.mark.parametrize("name", ["inverted_pendulum", "hopper", "chain"])
def test_reference_restart(ia, name):
    """c = 1e-3: six restarts (mu 0 -> 0.01209); measured margins are printed"""
    m, _, rec, V0, v0, lxx, luu = _restart_case(ia, name)
    for s in range(2):
        st, out, retries, tried, margin = _restart_ref(m, rec, V0, v0, lxx, luu, s, rr.options())
        print(f"{name} seed {s}: retries {retries}, mu tried {[f'{x:.3g}' for x in tried]}, pivot margin {margin:.3g}")
        assert 3 <= retries <= 8 and out["first_bad"] == -1 and st["status"] == 0
        assert margin >= 1e-6
        assert tried[-1] == _seq(retries, 0.0, True)[-1]
        # max_retry = 1: the fallback
        st1, out1, r1, _, _ = _restart_ref(m, rec, V0, v0, lxx, luu, s, rr.options(max_retry=1))
        assert r1 == 1 and out1["first_bad"] >= 1 and st1["mu"] == 1e-6


# ------------------------------------------------------------------ GPU --
def _solver(ia, m, dm, H, cost, alphas, mu, select="min_cost", **opts):
    g = ia.ILQR(m, dm, H, cost, alphas=alphas, select=select, mu=mu)
    g.set_layout("corrected")
    g.set_recursion("standard")
    g.set_regularization(True, **opts)
    return g


def _state_of(dm, s):
    return dict(time=dm.time[s], qpos=dm.qpos[s], qvel=dm.qvel[s], warm=dm.warm[s], ctrl=dm.ctrl[s])


def _replays(ia, ora, m, dm, name, H, alphas, mu, opts):
    om = ora.OModel(m.blob())
    rows = csr.constant_schedule(tsr._cost_of(ia, name), m, H)
    return [rr.RegRef(sr.StdRef(ora, m, om, _state_of(dm, s), H, rows, alphas=alphas, select="min_cost",
                                layout="corrected", mu=mu), rr.options(**opts), mu, replay=True)
            for s in range(dm.qpos.shape[0])]


def _step_and_check(ia, g, refs, m, name, H, it, gains=False):
    """one iterate() on the device, the same on every seed's replay: candidate
    costs, decision, trajectory and the schedule state bit for bit"""
    S = len(refs)
    g.iterate()
    dev = tsr._device(g)
    costs, sel = g.costs()
    t, st = g.traj(), g.reg_state()
    for s in range(S):
        oc, pick = refs[s].forward()
        assert np.array_equal(costs[s], oc) and sel[s] == pick, (it, s, costs[s], oc, sel[s], pick)
        ot = refs[s].traj()
        for f in ("qpos", "qvel", "ctrl"):
            assert np.array_equal(getattr(t, f).reshape(S, H + 1, -1)[s], ot[f]), (it, s, f)
        refs[s].backward(dict(K=dev["K"][s], k=dev["k"][s], dV=dev["dV"][s], retries=st["retries"][s]))
        for f in ("mu", "dmu", "cost_nom", "status", "valid"):
            assert st[f][s] == refs[s].st[f], (it, s, f, st[f][s], refs[s].st[f])
        assert st["retries"][s] == 0 and dev["first_bad"][s] == -1
        if gains:
            lxx, luu = tsr._hess(ia, m, name, H + 1)
            ref, E = sr.both(g.deriv()[s], m.nv, m.nu, m.timestep, st["mu"][s], "corrected", lxx, luu)
            tsr._compare(dev, s, ref, E, f"{name} H={H} iteration {it} seed {s} mu {st['mu'][s]:.4g}")
    return costs, sel, t, st


def _trace_of(refs):
    return np.array([[r.trace[i] for r in refs] for i in range(len(refs[0].trace))])


@gpu
@pytest.mark.parametrize("name", ["inverted_pendulum", "hopper", "chain"])
def test_restart_parity(ia, name):
    """k_backward_std_reg<2,1>, <6,3>, <0,0>, horizon 2, two seeds: the restart case
    through set_deriv + set_value.  retries, mu, dmu, first_bad exact; K, k, V, v,
    dV within tol(E64) of the reference at the final mu; max_retry = 1 ends in the fallback.
    MI355X: six restarts, mu 0 -> 0.0120893 at every size; E64 <= 6.5e-15, device
    deviation <= 2.4e-15 (both on the chain's second seed); max_retry = 1: mu 1e-6, first_bad 1."""
    m, cost, rec, V0, v0, lxx, luu = _restart_case(ia, name)
    S = 2
    g = ia.ILQR(m, tsr._dmain(ia, m, name, S), rc.H, cost, mu=0.0)
    g.set_recursion("standard")
    for max_retry in (rr.DEFAULTS["max_retry"], 1):
        g.set_regularization(True, max_retry=max_retry)
        g.set_deriv(rec)
        g.set_value(V0, v0)
        g.riccati_pass()
        dev, st = tsr._device(g), g.reg_state()
        for s in range(S):
            rst, out, retries, tried, margin = _restart_ref(m, rec, V0, v0, lxx, luu, s, rr.options(max_retry=max_retry))
            assert margin >= 1e-6
            print(f"{name} seed {s} max_retry {max_retry}: retries {st['retries'][s]} (reference {retries}), "
                  f"mu {st['mu'][s]:.6g}, first_bad {dev['first_bad'][s]}")
            assert st["retries"][s] == retries and st["mu"][s] == rst["mu"] and st["dmu"][s] == rst["dmu"]
            assert st["status"][s] == rst["status"] == 0 and dev["first_bad"][s] == out["first_bad"]
            assert all(np.all(np.isfinite(dev[a][s])) for a in sr.ARRAYS)
            if max_retry == 1:
                b = dev["first_bad"][s]
                assert b >= 1 and not dev["K"][s, b].any() and not dev["k"][s, b].any()
            else:
                assert 3 <= retries <= 8
                ref, E = sr.both(rec[s], m.nv, m.nu, m.timestep, rst["mu"], "reference", lxx, luu, V0[s], v0[s])
                tsr._compare(dev, s, ref, E, f"{name} restart seed {s}")


@gpu
def test_exhaustion_is_bounded(ia):
    """test_std_recursion.test_fallback's records (hopper, horizon 3, wu = 0):
    seed 0 has Quu_r = 0 at step 2 for every mu, seed 1 a NaN in record 1.
    Both use every restart and end with the fallback.
    MI355X: retries 5 / 5 and 16 / 16, first_bad 2 / 1, the run ends normally."""
    name, H, S, bad_step, MR = "hopper", 3, 2, 2, 5
    m = tsr._model(ia, name)
    c0 = ia.HOPPER_COST
    cost = ia.Cost(wq=c0.wq, tq=c0.tq, wv=c0.wv, wu=[0.0] * m.nu)
    rng = np.random.default_rng(20261020)
    rec = rng.standard_normal((S, H + 1, m.D))
    o = 2 * m.nv * m.nv
    rec[0, bad_step, o:o + m.nv * m.nu] = 0.0
    rec[1] = rec[0]
    rec[1, bad_step] = rng.standard_normal(m.D)
    rec[1, 1, 3] = np.nan
    g = ia.ILQR(m, tsr._dmain(ia, m, name, S), H, cost, mu=0.0)
    g.set_layout("corrected")
    g.set_recursion("standard")
    for mr in (MR, ia.REG_MAXRETRY):
        g.set_regularization(True, max_retry=mr, mu_max=1e30)    # (sixteen increases from 0 end at 2.1e20)
        g.set_deriv(rec)
        g.riccati_pass()
        dev, st = tsr._device(g), g.reg_state()
        assert list(st["retries"]) == [mr, mr] and list(dev["first_bad"]) == [bad_step, 1]
        assert list(st["mu"]) == [_seq(mr, 0.0, True)[-1]] * 2 and not st["status"].any()
        assert all(np.all(np.isfinite(dev[a][0])) for a in sr.ARRAYS)
        assert not dev["K"][0, bad_step].any() and not dev["K"][1].any() and not dev["dV"][1].any()


@gpu
def test_forced_rejection(ia, ora):
    """pendulum H = 20, alphas (1,), mu = 0, zmin = 2, mu_max = 1e3, two seeds: after
    every iterate the trajectory and the selected cost are the first iterate's,
    sel = -1, mu follows the reference and stops moving once status is 2.  (dinit
    has no getter: the next rollout starts from it, and its cost is the replay's.)"""
    from seed_shard import device_view
    name, H, S = "inverted_pendulum", 20, 2
    opts = dict(zmin=2.0, mu_max=1e3)
    m = tsr._model(ia, name)
    dm = tsr._dmain(ia, m, name, S)
    g = _solver(ia, m, dm, H, ia.PENDULUM_COST, (1.0,), 0.0, **opts)
    refs = _replays(ia, ora, m, dm, name, H, (1.0,), 0.0, opts)
    first = None
    for it in range(13):
        costs, sel, t, st = _step_and_check(ia, g, refs, m, name, H, it)
        csel = device_view(g.device_costs_ptr(), S).cpu().numpy().copy()
        if it == 0:
            first = (t, csel)
            assert list(sel) == [0, 0] and np.array_equal(csel, costs[:, 0])
            continue
        assert list(sel) == [-1, -1]
        for f in ("time", "qpos", "qvel", "warm", "ctrl"):
            assert np.array_equal(getattr(t, f), getattr(first[0], f)), (it, f)
        assert np.array_equal(csel, first[1])
        want = _seq(min(it, 10), 0.0, True, rr.options(**opts))[-1]
        assert list(st["mu"]) == [want, want] and list(st["status"]) == [2 if it >= 10 else 0] * 2


@gpu
def test_accepting_schedule(ia, ora):
    """hopper H = 20, two bench seeds x four alphas, mu = 1000: eight iterations in
    replay mode, costs, decisions, mu, trajectories bit for bit; gains on the first two.
    MI355X: E64 <= 1.0e-15, device deviation <= 1.1e-15 (mu 1000 and 625)."""
    name, H, S = "hopper", 20, 2
    m = tsr._model(ia, name)
    dm = tsr._dmain(ia, m, name, S)
    g = _solver(ia, m, dm, H, ia.HOPPER_COST, ALPHAS4, 1000.0, trace_len=8)
    refs = _replays(ia, ora, m, dm, name, H, ALPHAS4, 1000.0, {})
    for it in range(8):
        costs, sel, t, st = _step_and_check(ia, g, refs, m, name, H, it, gains=it < 2)
        assert (sel >= 0).all()
    assert list(st["mu"]) == [_seq(7, 1000.0, False)[-1]] * 2
    assert np.array_equal(g.reg_trace(), _trace_of(refs), equal_nan=True)


def _two_seeds(m):
    """the hopper's cfg-3 state and a bench seed"""
    import workloads
    dm = workloads.hopper_dmain(m, 2, sigma=0.01)
    d0 = workloads.hopper_dmain(m, 1)
    for f in ("time", "qpos", "qvel", "warm", "ctrl"):
        getattr(dm, f)[0] = getattr(d0, f)[0]
    return dm


@gpu
def test_natural_rejections(ia, ora):
    """hopper H = 100, alphas (1,), mu = 0, two seeds (the cfg-3 state and a bench
    seed).  One solver is stepped with the replay (gains compared on iterations 0
    and 9); a second one enqueues sixteen iterates without a sync and its trace,
    read once, is the first solver's and the replay's.  The two seeds' mu differ.
    MI355X: E64 <= 2.4e-15, device deviation <= 2.1e-15 (mu 0 and 8.711); mu after
    the decision parts at iteration 11, 5.445 against 0.8308, and ends 0.04952 / 2.684e-05."""
    name, H, S, N = "hopper", 100, 2, 16
    m = tsr._model(ia, name)
    dm = _two_seeds(m)
    g = _solver(ia, m, dm, H, ia.HOPPER_COST, (1.0,), 0.0, trace_len=N)
    refs = _replays(ia, ora, m, dm, name, H, (1.0,), 0.0, {})
    picks = []
    for it in range(N):
        costs, sel, t, st = _step_and_check(ia, g, refs, m, name, H, it, gains=it in (0, 9))
        picks.append([int(x) for x in sel])
    want = _trace_of(refs)
    tr = g.reg_trace()
    assert np.array_equal(tr, want, equal_nan=True)
    print("decisions per iteration (seed 0, seed 1):", picks)
    print("mu after the decision:", [[float("%.4g" % x) for x in row] for row in tr[:, :, 5]])
    assert [p[0] for p in picks] == [0] + [-1] * 8 + [0, 0, -1, 0, 0, 0, 0]     # the cfg-3 seed: the CPU test's
    assert np.any(tr[:, 0, 5] != tr[:, 1, 5])
    # no sync between the iterates
    g2 = _solver(ia, m, dm, H, ia.HOPPER_COST, (1.0,), 0.0, trace_len=N)
    for _ in range(N):
        g2.iterate()
    assert np.array_equal(g2.reg_trace(), want, equal_nan=True)
    assert np.array_equal(g2.traj().qpos, g.traj().qpos)
    # a shorter ring keeps the newest iterations, oldest first
    g2.set_regularization(True, trace_len=4)
    for _ in range(6):
        g2.iterate()
    t4 = g2.reg_trace()
    assert t4.shape == (4, S, ia.REG_TRACE) and np.all(t4[1:, :, 4] == t4[:-1, :, 6])


@gpu
def test_convergence(ia, ora):
    """hopper H = 50, four alphas, mu = 0, tol_cost = 1e-6: status 1 at the
    iteration the replay says (prototype: the fourth rollout); later iterates
    leave the trajectory and mu untouched.  MI355X: status 1 at the fourth rollout on both seeds."""
    name, H, S = "hopper", 50, 2
    opts = dict(tol_cost=1e-6)
    m = tsr._model(ia, name)
    dm = _two_seeds(m)
    g = _solver(ia, m, dm, H, ia.HOPPER_COST, ALPHAS4, 0.0, **opts)
    refs = _replays(ia, ora, m, dm, name, H, ALPHAS4, 0.0, opts)
    when, frozen = [None] * S, [None] * S
    for it in range(10):
        costs, sel, t, st = _step_and_check(ia, g, refs, m, name, H, it)
        for s in range(S):
            q = t.qpos.reshape(S, H + 1, -1)[s].copy()
            if when[s] is None and st["status"][s] == 1:
                when[s], frozen[s] = it, (q, st["mu"][s])
            elif when[s] is not None:
                assert sel[s] == -1 and st["status"][s] == 1
                assert np.array_equal(q, frozen[s][0]) and st["mu"][s] == frozen[s][1]
    print("status 1 at rollout (0-based):", when)
    assert when[0] is not None and when[0] <= 8      # the cfg-3 seed (prototype: 3)


@gpu
def test_invalidation(ia, ora):
    """after set_dinit to a new state the next rollout is taken unconditionally and mu stays"""
    name, H, S = "hopper", 20, 2
    m = tsr._model(ia, name)
    dm = tsr._dmain(ia, m, name, S)
    g = _solver(ia, m, dm, H, ia.HOPPER_COST, (1.0,), 1000.0)
    refs = _replays(ia, ora, m, dm, name, H, (1.0,), 1000.0, {})
    for it in range(2):
        _step_and_check(ia, g, refs, m, name, H, it)
    mu = g.reg_state()["mu"].copy()
    d2 = dm.copy()
    d2.qpos[:, 1] += 0.3                # higher: the cost rises, a valid nominal would reject
    g.set_dinit(d2)
    assert not g.reg_state()["valid"].any()
    for s, r in enumerate(refs):
        d = r.ref.om.make_data()
        d.set_state(**_state_of(d2, s))
        r.ref.il.set_dinit(d)
        r.invalidate()
    costs, sel, t, st = _step_and_check(ia, g, refs, m, name, H, 2)
    assert list(sel) == [0, 0] and np.array_equal(st["mu"], mu) and st["valid"].all()
    assert np.isnan(refs[0].trace[2][0])


@gpu
def test_off_path(ia):
    """set_regularization(opts) then None: in STANDARD two iterates are a fresh
    STANDARD solver's bit for bit; after set_recursion('reference') a fresh
    solver's on the fused path"""
    import workloads
    m = tsr._model(ia, "hopper")
    mk = lambda al: ia.ILQR(m, workloads.hopper_dmain(m, 2, sigma=0.01), 20, ia.HOPPER_COST, alphas=al,
                            select="min_cost")
    for al in ((1.0,), ALPHAS4):
        for std in (True, False):
            out = []
            for toggle in (False, True):
                g = mk(al)
                if toggle:
                    g.set_recursion("standard")
                    g.set_regularization(True, trace_len=4)
                    g.set_regularization(None)
                    assert g.regularization() is None
                    if not std:
                        g.set_recursion("reference")
                elif std:
                    g.set_recursion("standard")
                g.set_timing(True)
                g.iterate()
                g.iterate()
                d = tsr._device(g)
                tm = g.timing()
                if std:
                    assert tm["backward"][1] == 2 and tm["fd_backward"][1] == 0
                else:
                    assert tm["fd_backward"][1] == 2 and tm["backward"][1] == 0     # the fused sweep
                d["costs"], d["sel"] = g.costs()
                d["qpos"], d["ctrl"] = g.traj().qpos, g.traj().ctrl
                out.append(d)
            for a in out[0]:
                assert np.array_equal(out[0][a], out[1][a]), (al, std, a)
            assert (out[1]["sel"] >= 0).all()


def _set(ia, g, **kw):
    o = ia._RegOpts(**rr.options(**kw))
    return ia.lib().ilqg_solver_set_regularization(g._h, ctypes.byref(o))


@gpu
def test_refusals(ia):
    import workloads
    L = ia.lib()
    m = tsr._model(ia, "hopper")
    g = ia.ILQR(m, workloads.hopper_dmain(m, 2, sigma=0.01), 4, ia.HOPPER_COST)
    # needs STANDARD, both orders
    assert _set(ia, g) == UNSUPPORTED
    g.set_recursion("standard")
    assert _set(ia, g) == 0
    assert L.ilqg_solver_set_recursion(g._h, 0) == UNSUPPORTED
    assert L.ilqg_forward_sharded(g._h, 0, 1) == UNSUPPORTED
    # the options
    for bad in (dict(factor=1.0), dict(factor=float("nan")), dict(mu_min=-1.0), dict(mu_max=1e-6), dict(zmin=-0.1),
                dict(tol_cost=-1.0), dict(max_retry=17), dict(max_retry=-1), dict(trace_len=1025), dict(trace_len=-1)):
        assert _set(ia, g, **bad) == ERR_ARG, bad
    assert g.regularization()["factor"] == 1.6        # a refused call changes nothing
    # set_mu / set_reg_mu reset dmu and status
    g.iterate()
    g.iterate()
    g.set_mu(3.0)
    st = g.reg_state()
    assert list(st["mu"]) == [3.0, 3.0] and list(st["dmu"]) == [1.0, 1.0] and not st["status"].any()
    g.set_reg_mu([0.5, 2.0])
    assert list(g.reg_state()["mu"]) == [0.5, 2.0]
    # off: REFERENCE is allowed again, the getters refuse
    g.set_regularization(None)
    assert L.ilqg_solver_set_recursion(g._h, 0) == 0
    assert L.ilqg_solver_get_reg_state(g._h, None, None, None, None, None, None) == ERR_ARG


@gpu
@pytest.mark.parametrize("variant", ["select0", "schedule_f32", "reference_layout"])
def test_composition(ia, variant):
    """select_mode 0 (candidate 0 alone is tested), a cost schedule with the fp32 FD
    sweep, the reference layout: hopper H = 8, two seeds, four alphas, zmin = 0.5.
    No oracle here: the decision is recomputed by reg_ref.decide from the device's
    own candidate costs and dV and must be the device's, with mu, dmu, cost_nom and
    status, bit for bit; a rejected seed's trajectory is untouched; restarts of the
    backward pass (the schedule's weight-free rows at mu = 0) move mu by the
    increase, retries times.  MI355X: select0 rejects from the fourth iteration on;
    schedule_f32 restarts once in the first pass and twelve times in a later one
    (mu 1.049e-05 -> 5.468e10 >= mu_max: status 2, frozen from there)."""
    name, H, S = "hopper", 8, 2
    m = tsr._model(ia, name)
    select = "reference" if variant == "select0" else "min_cost"
    g = ia.ILQR(m, tsr._dmain(ia, m, name, S), H, ia.HOPPER_COST, alphas=ALPHAS4, select=select, mu=0.0)
    if variant != "reference_layout":
        g.set_layout("corrected")
    g.set_recursion("standard")
    if variant == "schedule_f32":
        g.set_cost_schedule(csr.make_schedule(ia.HOPPER_COST, m, H))
        g.set_fd_precision("f32")
    o = rr.options(zmin=0.5)
    g.set_regularization(True, zmin=0.5)
    sts = [dict(mu=0.0, dmu=1.0, cost_nom=0.0, valid=0, status=0) for _ in range(S)]
    dV = np.zeros((S, 2))
    seen = []
    for it in range(8):
        before = g.traj()
        g.iterate()
        costs, sel = g.costs()
        st, t = g.reg_state(), g.traj()
        for s in range(S):
            pick, _, _ = rr.decide(o, sts[s], costs[s], ALPHAS4, dV[s], 1 if select == "min_cost" else 0)
            assert sel[s] == pick, (it, s, sel[s], pick)
            assert select == "min_cost" or pick in (0, -1)
            if pick < 0:
                for f in ("time", "qpos", "qvel", "warm", "ctrl"):
                    assert np.array_equal(getattr(t, f).reshape(S, H + 1, -1)[s], getattr(before, f).reshape(S, H + 1, -1)[s])
            for _ in range(int(st["retries"][s])):
                sts[s]["mu"], sts[s]["dmu"], sts[s]["status"] = rr.increase(o, sts[s]["mu"], sts[s]["dmu"], sts[s]["status"])
            for f in ("mu", "dmu", "cost_nom", "status", "valid"):
                assert st[f][s] == sts[s][f], (it, s, f, st[f][s], sts[s][f])
        seen.append(([int(x) for x in sel], [int(x) for x in st["retries"]], [float("%.4g" % x) for x in st["mu"]]))
        dV, _ = g.expected()
    print(variant, "(chosen, retries, mu) per iteration:", seen)

"""The standard recursion (ilqg_solver_set_recursion STANDARD, ilqg_solver_get_expected):
the textbook iLQR backward step with the exact diagonal cost Hessians, mu in
Quu / Qux only and an expected reduction, in place of inc/ilqr.h:157-174.

The reference is tests/std_ref.py: the step written in np.longdouble (Gaussian
elimination) and again in fp64 with sequential loops.  Tolerance of every
comparison with the device (K, k, V, v, dV, each relative to the array's
maximum): tol = max(1e-12, 10 E64), E64 the largest such deviation of the
reference's own fp64 evaluation from its longdouble one on the same records --
a property of the reference, not of the code under test.  Every test prints E64
and what it observed.

The unmarked tests pin the reference itself: on a linear-quadratic problem the
cost changes by exactly dV1 + dV2, and on the hopper and the pendulum the
recursion optimises (the figures are beside the bounds)."""
import ctypes
import os
import re

import numpy as np
import pytest

import cost_sched_ref as csr
import riccati_cases as rc
import std_ref as sr
import test_riccati_cases as trc
from conftest import ROOT, model_path

gpu = pytest.mark.gpu
LD = np.longdouble
H20 = 20
ALPHAS8 = tuple(2.0 ** -i for i in range(8))
ALPHAS4 = ALPHAS8[:4]
UNSUPPORTED, ERR_ARG = 4, 1


# ------------------------------------------------------------------ CPU --
def _lq_problem(seed, zero_last=False):
    """records and Hessians of a linear system x_{n-1} = A x_n + B u_n
    (nv = 2, nu = 2, P = 6 points, point P-1 first) under a diagonal quadratic cost"""
    nv, nu, P, dt = 2, 2, 6, 0.05
    nx = 2 * nv
    rng = np.random.default_rng([20261020, seed])
    body = rng.standard_normal(nv * (2 * nv + nu))
    wx, tx = rng.uniform(0.2, 2.0, (P, nx)), rng.standard_normal((P, nx))
    wu, tu = rng.uniform(0.2, 2.0, (P, nu)), rng.standard_normal((P, nu))
    bodies = np.tile(body, (P, 1))
    if zero_last:  # the step of point P-1: nothing to gain from its control, and no curvature
        bodies[P - 1, 2 * nv * nv:] = 0.0
        wx[P - 1] = 0.0
        wu[P - 1] = 0.0
    AB = [tuple(x.astype(LD) for x in sr.assemble_AB(bodies[n], nv, nu, dt, "corrected")) for n in range(P)]
    x, u = np.zeros((P, nx), dtype=LD), rng.standard_normal((P, nu)).astype(LD)
    x[P - 1] = rng.standard_normal(nx)
    for n in range(P - 1, 0, -1):
        x[n - 1] = AB[n][0] @ x[n] + AB[n][1] @ u[n]
    rec = np.zeros((P, rc.record_size(nv, nu)))
    for n in range(P):
        rec[n, :len(body)] = bodies[n]
        rec[n, len(body):len(body) + nx] = (2 * wx[n] * (x[n] - tx[n])).astype(np.float64)   # exact gradients,
        rec[n, len(body) + nx:] = (2 * wu[n] * (u[n] - tu[n])).astype(np.float64)            # rounded to fp64
    return dict(nv=nv, nu=nu, P=P, dt=dt, rec=rec, lxx=2 * wx, luu=2 * wu, AB=AB)


def _lq_apply(p, out):
    """the cost change of u = K dx + k on the linear system from dx = 0, with the
    recorded (fp64-rounded) gradients standing for the exact ones"""
    P, nx, nu = p["P"], 2 * p["nv"], p["nu"]
    dx, dJ = np.zeros(nx, dtype=LD), LD(0)
    q = lambda n: p["rec"][n, -(nx + nu):-nu].astype(LD)
    r = lambda n: p["rec"][n, -nu:].astype(LD)
    for n in range(P - 1, 0, -1):
        K = np.asarray(out["K"][n], dtype=LD).reshape(nu, nx, order="F")
        du = K @ dx + np.asarray(out["k"][n], dtype=LD)
        dJ += q(n) @ dx + r(n) @ du + (dx * p["lxx"][n]) @ dx / 2 + (du * p["luu"][n]) @ du / 2
        dx = p["AB"][n][0] @ dx + p["AB"][n][1] @ du
    return dJ + q(0) @ dx + (dx * p["lxx"][0]) @ dx / 2


def test_reference_is_exact_on_lq():
    """measured: |dJ - (dV1 + dV2)| / |dV1 + dV2| <= 1.1e-19 (longdouble), E64 <= 4.0e-16"""
    for seed in range(4):
        p = _lq_problem(seed)
        ld, E = sr.both(p["rec"], p["nv"], p["nu"], p["dt"], 0.0, "corrected", p["lxx"], p["luu"])
        assert ld["first_bad"] == -1
        dJ, pred = _lq_apply(p, ld), ld["dV"][0] + ld["dV"][1]
        err = float(abs(dJ - pred) / abs(pred))
        print(f"LQ seed {seed}: dJ {float(dJ):.6g} predicted {float(pred):.6g} rel {err:.2e} E64 {E:.2e}")
        assert pred < 0 and err <= 1e-12
        assert E <= 1e-12


def test_reference_fallback_on_lq():
    """lxx = 0, B = 0 and luu = 0 at the last step: Quu_r = 0 there, and only there"""
    p = _lq_problem(7, zero_last=True)
    n = p["P"] - 1
    for f in (sr.recursion_ld, sr.recursion_f64):
        out = f(p["rec"], p["nv"], p["nu"], p["dt"], 0.0, "corrected", p["lxx"], p["luu"])
        assert out["first_bad"] == n
        assert not np.any(out["K"][n]) and not np.any(out["k"][n])
        assert all(np.any(out["k"][j]) and np.any(out["K"][j]) for j in range(1, n))
        assert all(np.all(np.isfinite(np.asarray(out[a], dtype=np.float64))) for a in sr.ARRAYS)
    # with a control cost at that step, no step falls back
    p["luu"][n] = 0.5
    assert sr.recursion_f64(p["rec"], p["nv"], p["nu"], p["dt"], 0.0, "corrected", p["lxx"], p["luu"])["first_bad"] == -1


def _oracle_state(ora, m, name):
    """cfg-3 hopper state (reset, 500 passive steps, ctrl -= 0.1) / the pendulum's 10 passive steps, on the oracle"""
    om = ora.OModel(m.blob())
    d = om.make_data()
    if name == "hopper":
        d.step(500)
        d.arr("ctrl")[:] -= 0.1
    else:
        d.step(10)
    return om, d.state()


def _cost_of(ia, name):
    return ia.PENDULUM_COST if name == "inverted_pendulum" else ia.HOPPER_COST


def _std_ref(ia, ora, name, H, alphas=ALPHAS8, mu=0.0):
    m = ia.Model.load(model_path(name))
    om, st = _oracle_state(ora, m, name)
    rows = csr.constant_schedule(_cost_of(ia, name), m, H)
    return sr.StdRef(ora, m, om, st, H, rows, alphas=alphas, select="min_cost", layout="corrected", mu=mu)


# measured with this reference: (cost ratio of the first update, |actual - predicted| / |predicted|)
#   hopper            0.2254   1.5e-3   (1.67467 -> 0.377552, predicted reduction 1.29522, actual 1.29712)
#   inverted_pendulum 0.0143   2.1e-3   (0.280083 -> 0.00401143, predicted 0.275506, actual 0.276071)
# The bound on the second figure, 1e-2, is about 6x the hopper's, for the FD gradients' one-sided bias.
@pytest.mark.parametrize("name", ["hopper", "inverted_pendulum"])
def test_reference_optimises_h20(ia, ora, name):
    ref = _std_ref(ia, ora, name, H20)
    c0, s0 = ref.iterate()
    dV = ref.out["dV"]
    c1, s1 = ref.forward()
    ratio = c1[s1] / c0[s0]
    pred = -(dV[0] + dV[1])
    err = abs((c0[s0] - c1[s1]) - pred) / abs(pred)
    print(f"{name} H=20: cost {c0[s0]:.6g} -> {c1[s1]:.6g} (x{ratio:.4f}), alpha index {s1}, predicted reduction "
          f"{pred:.6g}, actual {c0[s0] - c1[s1]:.6g}, rel {err:.2e}")
    assert ref.out["first_bad"] == -1
    assert s1 == 0                      # the full step
    assert ratio < 0.5
    assert err <= 1e-2


def test_reference_optimises_hopper_h100(ia, ora):
    """measured: 109.55 -> 90.31 -> 3.03 -> 1.89 -> 1.78 (x0.016)"""
    ref = _std_ref(ia, ora, "hopper", 100)
    costs = []
    for _ in range(5):
        c, s = ref.iterate()
        costs.append(float(c[s]))
    print("hopper H=100 selected costs:", " -> ".join(f"{c:.5g}" for c in costs), f"(x{costs[-1] / costs[0]:.4f})")
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert costs[-1] < 0.05 * costs[0]


def test_exports(ia):
    """fails on the parent: no such entry points"""
    L = ia.lib()
    for name in ("ilqg_solver_set_recursion", "ilqg_solver_get_expected"):
        assert hasattr(L, name), name
        assert name in ia.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ilqg_amd.h")).read()
    assert re.search(r"int\s+ilqg_solver_set_recursion\(ilqg_solver\*\s*\w*,\s*int\s+\w+\);", hdr)
    assert re.search(r"int\s+ilqg_solver_get_expected\(ilqg_solver\*\s*\w*,\s*double\*\s*\w+,\s*int\*\s*\w+\);", hdr)
    assert re.search(r"#define\s+ILQG_RECURSION_REFERENCE\s+0", hdr)
    assert re.search(r"#define\s+ILQG_RECURSION_STANDARD\s+1", hdr)
    assert hasattr(ia.ILQR, "set_recursion") and hasattr(ia.ILQR, "expected")


# ------------------------------------------------------------------ GPU --
def _model(ia, name):
    return ia.Model.from_string(trc.chain_xml()) if name == "chain" else ia.Model.load(model_path(name))


def _gcost(ia, name):
    return ia.Cost(wq=[1.0] * 9, wv=[0.1] * 9, wu=[0.01] * 7) if name == "chain" else _cost_of(ia, name)


def _dmain(ia, m, name, S):
    import workloads
    if name == "inverted_pendulum":
        st = workloads.pendulum_dmain(m, S)
        st.qpos[:, 1] += 0.01 * np.arange(S)
        return st
    if name == "hopper":
        return workloads.hopper_dmain(m, S, sigma=0.01)   # the bench's seeds
    st = m.reset_state(S)
    st.qpos[:] = 0.05 * (1 + np.arange(m.nq)) + 0.01 * np.arange(S)[:, None]
    return st


def _device(g):
    """K, k, V, v, dV, first_bad of the last backward pass, per seed"""
    g.synchronize()
    K, k = g.gains()
    V, v = g.value()
    dV, bad = g.expected()
    return dict(K=K, k=k, V=V, v=v, dV=dV, first_bad=bad)


def _compare(dev, s, ref, E, what, steps=None):
    t, worst = sr.tol(E), 0.0
    for a in sr.ARRAYS:
        x, y = np.asarray(dev[a][s]), np.asarray(ref[a])
        if steps is not None and a in ("K", "k"):
            x, y = x[steps], y[steps]
        assert np.all(np.isfinite(x)), (what, a)
        worst = max(worst, sr.rel(x, y))
    print(f"{what}: E64 {E:.2e} tol {t:.2e} device deviation {worst:.2e}")
    assert worst <= t, (what, worst, t)
    return worst


def _hess(ia, m, name, P, rows=None):
    rows = csr.constant_schedule(_gcost(ia, name), m, P - 1) if rows is None else rows
    return sr.hessians(rows, m.nq, m.nv, m.nu)


@gpu
@pytest.mark.parametrize("mu", [0.0, 1000.0])
@pytest.mark.parametrize("layout", ["reference", "corrected"])
@pytest.mark.parametrize("name", ["inverted_pendulum", "hopper", "chain"])
def test_stage_parity(ia, name, layout, mu):
    """k_backward_std<2,1>, <6,3>, <0,0> on the device's own records and trajectory.
    MI355X, largest over the 2 seeds x 2 layouts x 2 mu (E64, device deviation):
    pendulum 1.2e-15, 6.3e-16; hopper 1.5e-15, 1.1e-15; chain 2.1e-15, 1.8e-15
    but for corrected / mu = 1000: 2.1e-13, 2.2e-13 (tol 1.9e-12)."""
    S = 2
    m = _model(ia, name)
    g = ia.ILQR(m, _dmain(ia, m, name, S), H20, _gcost(ia, name), mu=mu)
    g.set_layout(layout)
    g.iterate()
    g.set_recursion("standard")
    g.backward_pass()
    dev, rec = _device(g), g.deriv()
    lxx, luu = _hess(ia, m, name, H20 + 1)
    for s in range(S):
        ref, E = sr.both(rec[s], m.nv, m.nu, m.timestep, mu, layout, lxx, luu)
        assert dev["first_bad"][s] == ref["first_bad"] == -1
        _compare(dev, s, ref, E, f"{name} {layout} mu={mu:g} seed {s}")
    # a REFERENCE pass reports nothing
    g.set_recursion("reference")
    g.backward_pass()
    dV, bad = g.expected()
    assert not dV.any() and (bad == -1).all()


@gpu
@pytest.mark.parametrize("name", ["inverted_pendulum", "hopper", "chain"])
def test_dense_records(ia, name):
    """family-D records of riccati_cases (horizon 2) through set_deriv, mu = 1000 and 0.
    MI355X: E64 <= 7.6e-16, device deviation <= 6.7e-16 over the three sizes."""
    m = _model(ia, name)
    cases = [c for c in rc.make_cases(m.nv, m.nu, m.timestep) if c.family == "D"]
    assert len(cases) == 2
    S, P = len(cases), rc.H + 1
    g = ia.ILQR(m, _dmain(ia, m, name, S), rc.H, _gcost(ia, name), mu=rc.MU)
    g.set_recursion("standard")
    lxx, luu = _hess(ia, m, name, P)
    for mu in (rc.MU, 0.0):
        g.set_mu(mu)
        g.set_deriv(np.stack([c.rec for c in cases]))
        g.riccati_pass()
        dev = _device(g)
        for s, c in enumerate(cases):
            ref, E = sr.both(c.rec, m.nv, m.nu, m.timestep, mu, "reference", lxx, luu)
            assert dev["first_bad"][s] == ref["first_bad"]
            _compare(dev, s, ref, E, f"{name} {c.name} mu={mu:g}")


@gpu
def test_fallback(ia):
    """hopper, horizon 3, records through set_deriv, wu = 0 and mu = 0: seed 0 has
    fu = 0 at step 2 (Quu_r = 0 exactly), seed 1 a NaN in record 1.
    MI355X: E64 4.4e-16, device deviation 6.4e-16 on steps 1 and 3."""
    name, H, S, bad_step = "hopper", 3, 2, 2
    m = _model(ia, name)
    c0 = ia.HOPPER_COST
    cost = ia.Cost(wq=c0.wq, tq=c0.tq, wv=c0.wv, wu=[0.0] * m.nu)
    rng = np.random.default_rng(20261020)
    rec = rng.standard_normal((S, H + 1, m.D))
    o = 2 * m.nv * m.nv
    rec[0, bad_step, o:o + m.nv * m.nu] = 0.0
    rec[1] = rec[0]
    rec[1, bad_step] = rng.standard_normal(m.D)
    rec[1, 1, 3] = np.nan
    g = ia.ILQR(m, _dmain(ia, m, name, S), H, cost, mu=0.0)
    g.set_layout("corrected")
    g.set_recursion("standard")
    g.set_deriv(rec)
    g.riccati_pass()
    dev = _device(g)
    lxx, luu = sr.hessians(csr.constant_schedule(cost, m, H), m.nq, m.nv, m.nu)
    ref, E = sr.both(rec[0], m.nv, m.nu, m.timestep, 0.0, "corrected", lxx, luu)
    assert ref["first_bad"] == bad_step and dev["first_bad"][0] == bad_step
    assert not dev["K"][0, bad_step].any() and not dev["k"][0, bad_step].any()
    assert all(np.all(np.isfinite(dev[a][0])) for a in sr.ARRAYS)
    others = [n for n in range(1, H + 1) if n != bad_step]
    assert all(dev["k"][0, n].any() for n in others)
    _compare(dev, 0, ref, E, "hopper fallback seed 0", steps=others)
    # the NaN: step 1 falls back and the pass ends; V is NaN from there on, so every later step does too
    assert dev["first_bad"][1] == 1
    assert not dev["K"][1].any() and not dev["k"][1].any()
    assert not dev["dV"][1].any()


@gpu
def test_schedule(ia):
    """hopper, horizon 8: the Hessians of step n come from row n of the schedule.
    mu = 1000, the library's default: make_schedule's all-zero row 1 and
    weight-free row 2 leave Quu_r = B'VB alone at mu = 0, singular to rounding
    (the reference's own E64 is then 3e-3 on one seed and the other falls back).
    MI355X: E64 3.6e-16 / 7.5e-16, device deviation 1.5e-15 / 6.2e-16; the gains
    differ from the constant-cost Hessians' by 9.5e-3 / 2.6e-2."""
    name, H, S, MU = "hopper", 8, 2, 1000.0
    m = _model(ia, name)
    rows = csr.make_schedule(ia.HOPPER_COST, m, H)
    g = ia.ILQR(m, _dmain(ia, m, name, S), H, ia.HOPPER_COST, mu=MU)
    g.set_layout("corrected")
    g.set_cost_schedule(rows)
    g.iterate()
    g.set_recursion("standard")
    g.backward_pass()
    dev, rec = _device(g), g.deriv()
    lxx, luu = sr.hessians(rows, m.nq, m.nv, m.nu)
    tols = []
    for s in range(S):
        ref, E = sr.both(rec[s], m.nv, m.nu, m.timestep, MU, "corrected", lxx, luu)
        assert dev["first_bad"][s] == ref["first_bad"] == -1
        _compare(dev, s, ref, E, f"hopper schedule seed {s}")
        tols.append(sr.tol(E))
    # the same records under the creation cost's Hessians: other gains
    g.set_cost_schedule(None)
    g.set_deriv(rec)
    g.riccati_pass()
    const = _device(g)
    for s in range(S):
        d = max(sr.rel(const[a][s], dev[a][s]) for a in ("K", "k"))
        print(f"hopper schedule seed {s}: gains differ from the constant-cost run by {d:.2e}")
        assert d > 100 * tols[s]


@gpu
def test_end_to_end(ia, ora):
    """hopper H = 20, 2 seeds x 4 alphas, corrected layout, mu = 0, three iterate() calls
    in STANDARD: the rollouts are the oracle's driven with the device's gains, the
    gains the reference's on the device's records, and the cost falls as in
    test_reference_optimises_h20.
    MI355X (E64, device deviation), worst seed per iteration: 1.4e-15, 7.2e-16;
    5.9e-14, 9.5e-14; 3.5e-12, 2.1e-12 (tol 3.5e-11).  Selected costs 1.5918 ->
    0.37542 and 1.9207 -> 0.59432 at alpha = 1, actual against predicted
    reduction 1.4e-3 and 2.3e-3."""
    name, S = "hopper", 2
    m = _model(ia, name)
    dm = _dmain(ia, m, name, S)
    g = ia.ILQR(m, dm, H20, ia.HOPPER_COST, alphas=ALPHAS4, select="min_cost", mu=0.0)
    g.set_layout("corrected")
    g.set_recursion("standard")
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(ia.HOPPER_COST, m.nq, m.nv, m.nu))
    ils = []
    for s in range(S):
        d = om.make_data()
        d.set_state(time=dm.time[s], qpos=dm.qpos[s], qvel=dm.qvel[s], warm=dm.warm[s], ctrl=dm.ctrl[s])
        il = ora.OILQR(om, d, H20, cost_fn="ora_cost_desc_fn")
        il.set_dinit(d)
        ils.append(il)
    lxx, luu = _hess(ia, m, name, H20 + 1)
    sel_cost, exp = [], []
    for it in range(3):
        g.iterate()
        dev, rec = _device(g), g.deriv()
        costs, sel = g.costs()
        t = g.traj()
        for s in range(S):
            oc, osel = ils[s].forward_candidates(ALPHAS4, "min_cost")
            ot = ils[s].traj()
            assert np.array_equal(costs[s], oc) and sel[s] == osel, (it, s)
            for f in ("qpos", "qvel", "ctrl"):
                assert np.array_equal(getattr(t, f).reshape(S, H20 + 1, -1)[s], ot[f]), (it, s, f)
            ref, E = sr.both(rec[s], m.nv, m.nu, m.timestep, 0.0, "corrected", lxx, luu)
            assert dev["first_bad"][s] == ref["first_bad"] == -1
            _compare(dev, s, ref, E, f"hopper end-to-end iteration {it} seed {s}")
            ils[s].set_gains(dev["K"][s], dev["k"][s])
        sel_cost.append(costs[np.arange(S), sel].copy())
        exp.append((sel.copy(), dev["dV"].copy()))
    for s in range(S):
        c0, c1 = sel_cost[0][s], sel_cost[1][s]
        a = ALPHAS4[exp[1][0][s]]
        dV = exp[0][1][s]
        pred = -(a * dV[0] + a * a * dV[1])
        err = abs((c0 - c1) - pred) / abs(pred)
        print(f"seed {s}: selected costs {' -> '.join(f'{c[s]:.5g}' for c in sel_cost)}, first update alpha {a:g}, "
              f"predicted reduction {pred:.5g}, actual {c0 - c1:.5g}, rel {err:.2e}")
        assert a == 1.0 and c1 < 0.5 * c0 and err <= 1e-2


@gpu
@pytest.mark.parametrize("case", ["hopper_h20", "bench_seeds"])
def test_off_path(ia, case):
    """set_recursion('standard') then 'reference': iterate() is a fresh solver's, on the fused path"""
    import workloads
    m = _model(ia, "hopper")
    if case == "hopper_h20":
        mk = lambda: ia.ILQR(m, workloads.hopper_dmain(m), H20, ia.HOPPER_COST)
    else:
        mk = lambda: ia.ILQR(m, workloads.hopper_dmain(m, 2, sigma=0.01), H20, ia.HOPPER_COST, alphas=ALPHAS8,
                             select="min_cost")
    out = []
    for toggle in (False, True):
        g = mk()
        if toggle:
            g.set_recursion("standard")
            g.set_recursion("reference")
        g.set_timing(True)
        g.iterate()
        g.iterate()
        d = _device(g)
        tm = g.timing()
        assert tm["fd_backward"][1] == 2 and tm["backward"][1] == 0     # the fused sweep
        d["costs"], d["sel"] = g.costs()
        d["qpos"], d["ctrl"] = g.traj().qpos, g.traj().ctrl
        out.append(d)
    for a in out[0]:
        assert np.array_equal(out[0][a], out[1][a]), a
    assert not out[1]["dV"].any()


def _rc(ia, g, mode):
    return ia.lib().ilqg_solver_set_recursion(g._h, ctypes.c_int(mode))


@gpu
def test_refusals(ia):
    import workloads
    L = ia.lib()
    m = _model(ia, "hopper")
    mk = lambda: ia.ILQR(m, workloads.hopper_dmain(m, 2, sigma=0.01), 4, ia.HOPPER_COST)
    g = mk()
    assert _rc(ia, g, 2) == ERR_ARG and _rc(ia, g, -1) == ERR_ARG
    # the MFMA engine, both orders
    g.set_riccati("mfma")
    assert _rc(ia, g, 1) == UNSUPPORTED
    g.set_riccati("exact")
    assert _rc(ia, g, 1) == 0
    assert L.ilqg_solver_set_riccati(g._h, 1) == UNSUPPORTED
    # control limits, both orders
    lo, hi = -np.ones(m.nu), np.ones(m.nu)
    dp = ctypes.POINTER(ctypes.c_double)
    assert L.ilqg_solver_set_ctrl_limits(g._h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp)) == UNSUPPORTED
    assert _rc(ia, g, 0) == 0
    g.set_ctrl_limits(lo, hi)
    assert _rc(ia, g, 1) == UNSUPPORTED
    g.set_ctrl_limits(None, None)
    # seed groups, both orders
    g.set_groups(2)
    assert _rc(ia, g, 1) == UNSUPPORTED
    g.set_groups(1)
    assert _rc(ia, g, 1) == 0
    assert L.ilqg_solver_set_groups(g._h, 2) == UNSUPPORTED
    assert _rc(ia, g, 0) == 0
    # nq != nv
    hm = ia.Model.load(model_path("humanoid"))
    st = hm.reset_state(1)
    st.qpos[:, 2] = 1.4
    h = ia.ILQR(hm, st, 2, ia.HUMANOID_COST)
    assert _rc(ia, h, 1) == UNSUPPORTED
    assert _rc(ia, h, 0) == 0

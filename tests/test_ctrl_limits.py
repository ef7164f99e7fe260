"""Control limits: the box-constrained backward pass and the clamped rollout
(ilqg_solver_set_ctrl_limits; the reference has no counterpart).

The reference of a boxed step is tests/boxqp_ref.py: np.longdouble, the QP
solved by enumerating all 3^nu active sets and keeping the KKT point -- nothing
in common with the device's projected Newton.  The unmarked tests pin that
reference (against a plain projected Newton) and the inputs of the GPU tests
(every boxed step non-degenerate, 20 % .. 80 % of the (step, control) pairs
clamped, all-free, all-clamped and mixed steps present), so the GPU tests
cannot pass vacuously.

Tolerance of the boxed comparisons (K, k, V, v relative to each array's
maximum): tol = max(1e-12, 10 E0), E0 the largest such deviation of the exact
engine WITHOUT limits from the same longdouble recursion without the box on the
same cases -- the parent's own rounding against this reference.  1e-12 is the
per-step Riccati budget (test_riccati_cases.MFMA_STEP_RTOL); the 10x allows for
the boxed step's extra factor + solve on a principal sub-block (by eigenvalue
interlacing no worse conditioned than the full block) and a handful of Newton
iterations.  Each test prints E0 and the deviation it observed."""
import numpy as np
import pytest

import boxqp_ref as bq
import riccati_cases as rc
import test_riccati_cases as trc
from test_riccati_cases import bundle  # noqa: F401  (the four-model fixture)
from conftest import model_path

gpu = pytest.mark.gpu
ARRAYS = ("K", "k", "V", "v")
INF = np.inf
NONDEGENERATE = 1e-6


def exact(a, b, what=""):
    trc.exact(a, b, what)


def _bundle(ia, ora, name):
    if name not in trc._bundles:
        trc._bundles[name] = trc.Bundle(ia, ora, name)
    return trc._bundles[name]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.longdouble(1e-300)))


def _tol(E0):
    return max(1e-12, 10 * E0)


# ---- CPU: the model's control ranges (fails on the parent: no such call)
def test_model_ctrlrange(ia):
    lo, hi = ia.Model.load(model_path("hopper")).ctrlrange()
    assert lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0] * 3
    lo, hi = ia.Model.load(model_path("humanoid")).ctrlrange()
    assert lo.tolist() == [-0.4] * 21 and hi.tolist() == [0.4] * 21
    lo, hi = ia.Model.load(model_path("inverted_pendulum")).ctrlrange()
    assert lo.tolist() == [-INF] and hi.tolist() == [INF]
    assert "ilqg_solver_set_ctrl_limits" in ia.EXPORTS and hasattr(ia.lib(), "ilqg_solver_get_clamped")


# ---- CPU: the reference against a plain projected Newton
@pytest.mark.parametrize("nu", [1, 3, 7])
def test_boxqp_ref_against_projected_newton(nu):
    rng = np.random.default_rng([20261019, nu])
    nclamped = 0
    for trial in range(6 if nu == 7 else 24):
        M = rng.standard_normal((nu, nu + 2))
        H = M @ M.T + 0.1 * np.eye(nu)
        g = rng.standard_normal(nu) * 2
        kunc = -np.linalg.solve(H, g)
        ctr = kunc * rng.choice([0.0, 1.0, 1.0], nu) + rng.standard_normal(nu)
        w = rng.uniform(0.1, 1.5, nu)
        bl, bh = ctr - w, ctr + w
        if trial % 5 == 4:
            bh = np.where(rng.random(nu) < 0.5, INF, bh)
            bl = np.where(rng.random(nu) < 0.5, -INF, bl)
        k, st, mg = bq.solve(H, g, bl, bh)
        kn, stn, it = bq.newton(H, g, bl, bh)
        assert mg > 0, (nu, trial, mg)
        assert np.array_equal(st, stn), (nu, trial, st, stn)
        scale = max(float(np.max(np.abs(g))), 1.0)
        assert bq.kkt_residual(H, g, bl, bh, k, st) <= 1e-16 * scale * nu * 10
        assert float(np.max(np.abs(k - kn))) <= 1e-15 * max(float(np.max(np.abs(k))), 1.0) * nu * 10
        nclamped += int(np.count_nonzero(st))
    assert nclamped > 0


# ---- the boxed horizon-2 cases (GPU item 3): seeded dense records, one case per
# seed of one solver.  The limits are solver-wide (lo = -W/2, hi = +W/2 per
# control), so each case places its box on k through its own nominal control:
# bl = lo - u*, bh = hi - u*.  Step 1 of a case is built from its KKT point: the
# controls of `clamp` are held at k_unconstrained + 0.75 W `sign`, the others
# re-solved on the free block and their boxes centred there, and each clamped
# control sits at the bound its gradient points out of.
def _patterns(nu, rng):
    a0 = int(rng.integers(nu))
    one = np.arange(nu) == a0
    sg = lambda: rng.choice([-1, 1], nu)
    out = [("free", np.zeros(nu, bool), sg()), ("lo", one, np.ones(nu, int)), ("hi", one, -np.ones(nu, int)),
           ("all", np.ones(nu, bool), sg())]
    if nu > 1:
        out.append(("mixed", np.arange(nu) % 2 == 1, sg()))
        sub = rng.random(nu) < 0.5
        sub[a0], sub[(a0 + 1) % nu] = True, False
        out.append(("mixed2", sub, sg()))
    out.append(("excl", None, None))  # placed below: one control's box excludes 0
    return out


class BoxCases:
    """records, nominal controls, limits and the longdouble references (boxed and unboxed) of one model size"""

    def __init__(self, b):
        self.b = b
        nv, nu, D = b.nv, b.nu, b.m.D
        rng = np.random.default_rng([20261019, nv, nu, 3])
        t = b.traj
        self.q, self.v = t["qpos"], t["qvel"]
        kinds = _patterns(nu, rng)
        self.names = [k for k, _, _ in kinds]
        S = len(kinds)
        self.rec = rng.standard_normal((S, rc.H + 1, D))
        free = [self._ref(s, np.zeros((rc.H + 1, nu)), -INF, INF) for s in range(S)]
        kunc = np.stack([f["kunc"] for f in free])          # (S, P, nu) of the unboxed recursion
        self.W = W = np.median(np.abs(kunc[:, 1]), axis=0) + 1e-3
        self.lo, self.hi = -W / 2, W / 2
        self.ctrl = np.zeros((S, rc.H + 1, nu))
        for s, (kind, cl, sg) in enumerate(kinds):
            if cl is None:  # the control with the largest |k| / W held beyond its k, away from 0
                a = int(np.argmax(np.abs(kunc[s, 1]) / W))
                cl = np.arange(nu) == a
                sg = np.where(kunc[s, 1] > 0, 1, -1)
            H, g = free[s]["H"][1], free[s]["g"][1]
            k = np.array(kunc[s, 1], dtype=np.longdouble)
            k[cl] += 0.75 * W[cl] * sg[cl]
            fr = ~cl
            if fr.any():
                k[fr] = bq.gauss_solve(H[np.ix_(fr, fr)], -g[fr] - (H[np.ix_(fr, cl)] @ k[cl] if cl.any() else 0))
            grad = H @ k + g
            # at lo (gradient > 0): lo - u* = k; at hi: hi - u* = k; free: the box centred on k
            self.ctrl[s, 1] = np.where(cl, np.where(grad > 0, self.lo, self.hi), 0.0) - k.astype(np.float64)
            # step 2: boxes shifted off the unboxed recursion's k by the same pattern, rotated
            self.ctrl[s, 2] = -(kunc[s, 2] - 0.75 * W * np.roll(np.where(cl, sg, 0), 1))
        self.free = free
        self.ref = [self._ref(s, self.ctrl[s], self.lo, self.hi) for s in range(S)]

    def _ref(self, s, ctrl, lo, hi):
        b = self.b
        return bq.recursion(self.rec[s], self.q, self.v, ctrl, b.nv, b.nu, b.dt, rc.MU,
                            np.broadcast_to(lo, (b.nu,)), np.broadcast_to(hi, (b.nu,)))


_box = {}


def _boxcases(ia, ora, name):
    if name not in _box:
        _box[name] = BoxCases(_bundle(ia, ora, name))
    return _box[name]


def _conditions(refs, nu, what):
    """the input conditions, on the reference alone: refs = one recursion per case"""
    states = np.concatenate([r["state"][1:] for r in refs])
    margin = np.concatenate([r["margin"][1:] for r in refs])
    scale = np.concatenate([r["scale"][1:] for r in refs])
    assert np.all(margin > NONDEGENERATE * scale), (what, float(np.min(margin / scale)))
    cl = states != 0
    frac = cl.mean()
    print(f"{what}: {cl.sum()} of {cl.size} (step, control) pairs clamped ({100 * frac:.0f} %), "
          f"smallest margin / scale {float(np.min(margin / scale)):.2e}")
    assert 0.2 <= frac <= 0.8, (what, frac)
    per = cl.sum(axis=1)
    assert (per == 0).any() and (per == nu).any(), (what, per)
    if nu > 1:
        assert ((per > 0) & (per < nu)).any(), (what, per)
    return states


BOX_MODELS = ("inverted_pendulum", "hopper", "chain")


@pytest.mark.parametrize("name", BOX_MODELS)
def test_boxed_case_conditions(ia, ora, name):
    bc = _boxcases(ia, ora, name)
    st = _conditions(bc.ref, bc.b.nu, name)
    assert (st == 1).any() and (st == 2).any()                      # a control at lo, one at hi
    i = bc.names.index("excl")
    u = bc.ctrl[i, 1]
    assert ((u < bc.lo) | (u > bc.hi)).any()                         # u* outside [lo, hi]: the box on k excludes 0
    assert np.count_nonzero(bc.ref[bc.names.index("lo")]["state"][1] == 1) >= 1
    assert np.count_nonzero(bc.ref[bc.names.index("hi")]["state"][1] == 2) >= 1
    assert not bc.ref[bc.names.index("free")]["state"][1].any()
    assert bc.ref[bc.names.index("all")]["state"][1].all()


# ---- the horizon-20 recursions (GPU item 4): the first iterate() rolls out with
# zero gains, so its trajectory is the constructor's passive one and its FD
# records are the oracle's first sweep -- available without a GPU
HORIZON = {"hopper": "corrected", "inverted_pendulum": "reference"}
H20 = 20
C_CHOICES = (0.25, 0.5, 1.0, 2.0)


def _dmain(ia, m, name):
    import workloads
    return workloads.pendulum_dmain(m) if name == "inverted_pendulum" else workloads.hopper_dmain(m)


class Horizon:
    def __init__(self, ia, ora, name, dmain=None, recs=None, traj=None):
        """on the CPU the records and the trajectory are the oracle's; a GPU test passes the device's own"""
        self.name, self.layout = name, HORIZON[name]
        self.m = m = ia.Model.load(model_path(name))
        self.cost = ia.PENDULUM_COST if name == "inverted_pendulum" else ia.HOPPER_COST
        self.recs, self.traj = recs, traj
        if recs is None:
            om = ora.OModel(m.blob())
            om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(self.cost, m.nq, m.nv, m.nu))
            d = om.make_data()
            d.set_state(time=dmain.time[0], qpos=dmain.qpos[0], qvel=dmain.qvel[0], warm=dmain.warm[0],
                        ctrl=dmain.ctrl[0])
            il = ora.OILQR(om, d, H20, cost_fn="ora_cost_desc_fn")
            il.set_dinit(d)
            il.iterate()
            self.recs, self.traj = il.arrays()["deriv"], il.traj()
        self.ustar = self.traj["ctrl"][0].copy()
        assert np.all(self.traj["ctrl"] == self.ustar)  # zero gains: the constant control of the passive rollout

    def recursion(self, lo, hi):
        m, t = self.m, self.traj
        return bq.recursion(self.recs, t["qpos"], t["qvel"], t["ctrl"], m.nv, m.nu, m.timestep, rc.MU, lo, hi,
                            layout=1 if self.layout == "corrected" else 0)

    def limits(self, c, free):
        """u* -+ c median|k_unconstrained|, the median per control over the horizon's steps"""
        med = np.median(np.abs(free["kunc"][1:]), axis=0)
        return self.ustar - c * med, self.ustar + c * med

    def choose(self):
        """the first c of C_CHOICES for which the input conditions hold -> (c, lo, hi, boxed reference)"""
        free = self.recursion(np.full(self.m.nu, -INF), np.full(self.m.nu, INF))
        why = []
        for c in C_CHOICES:
            lo, hi = self.limits(c, free)
            ref = self.recursion(lo, hi)
            try:
                _conditions([ref], self.m.nu, f"{self.name} H={H20} c={c}")
            except AssertionError as e:
                why.append(str(e))
                continue
            return c, lo, hi, ref, free
        raise AssertionError(f"no c of {C_CHOICES} meets the input conditions: {why}")


_hor = {}


def _horizon(ia, ora, name):
    if name not in _hor:
        m = ia.Model.load(model_path(name))
        h = Horizon(ia, ora, name, dmain=_cpu_dmain(ia, ora, m, name))
        _hor[name] = (h, h.choose())
    return _hor[name]


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


@pytest.mark.parametrize("name", sorted(HORIZON))
def test_horizon_conditions(ia, ora, name):
    h, (c, lo, hi, ref, free) = _horizon(ia, ora, name)
    assert c in C_CHOICES and np.all(lo < hi)


# ---- GPU
def _results(g):
    g.synchronize()
    K, k = g.gains()
    V, v = g.value()
    return dict(K=K[:, 1:], k=k[:, 1:], V=V, v=v)


@gpu
def test_infinite_limits_are_the_exact_engine(ia, bundle):
    """1a: the crafted cases of riccati_cases (ties, zero, denormal and NaN
    pivots) through k_backward_box with +-inf limits: the oracle's K, k, V, v
    bit for bit (families and mu as test_exact_engine_bitexact), mask all zero"""
    b = bundle
    g = trc._solver(ia, b, "exact")
    g.set_ctrl_limits(-INF, INF)
    lim = g.ctrl_limits()
    assert lim is not None and np.all(lim[0] == -INF) and np.all(lim[1] == INF)
    for kw, mu, what, fam in ((dict(vinit=False), rc.MU, "initV", "TD"), ({}, rc.MU, "set_value", "TSD"),
                              (dict(mu=0.0), 0.0, "mu = 0", "TSD")):
        trc._against_oracle(b, trc._pass(g, b, **kw), mu, what + ", infinite limits", fam)
        mask, info = g.clamped()
        assert not mask.any() and not info.any(), what
    g.set_mu(rc.MU)


@gpu
@pytest.mark.parametrize("name", sorted(HORIZON))
def test_infinite_limits_iterate(ia, name):
    """1b: two iterate() with +-inf limits (the unfused order, the clamped rollout
    kernel, k_backward_box) against a solver without limits: the same bits"""
    m = ia.Model.load(model_path(name))
    cost = ia.PENDULUM_COST if name == "inverted_pendulum" else ia.HOPPER_COST
    out = []
    for lim in (False, True):
        g = ia.ILQR(m, _dmain(ia, m, name), H20, cost)
        if lim:
            g.set_ctrl_limits(-INF, INF)
        g.iterate()
        g.iterate()
        g.synchronize()
        t = g.traj()
        out.append((t.time, t.qpos, t.qvel, t.warm, t.ctrl, *g.gains(), *g.value(), g.costs()[0]))
        if lim:
            assert not g.clamped()[0].any()
    for a, b_, n in zip(out[1], out[0], ("time", "qpos", "qvel", "warm", "ctrl", "K", "k", "V", "v", "cost")):
        exact(a, b_, f"{name} {n}")


@gpu
@pytest.mark.parametrize("name", BOX_MODELS)
def test_loose_finite_limits(ia, ora, name):
    """2: finite limits wider than every control the pass produces: the fast path, the exact engine's bits, mask zero"""
    b = _bundle(ia, ora, name)
    g = trc._solver(ia, b, "exact")
    base = trc._pass(g, b)
    big = 4 * max(float(np.nanmax(np.abs(base["k"]))), 1.0)
    g.set_ctrl_limits(-big, big)
    out = trc._pass(g, b)
    for n in ARRAYS:
        exact(out[n], base[n], f"{name} {n} (loose limits)")
    trc._against_oracle(b, out, rc.MU, "loose limits")
    mask, info = g.clamped()
    assert not mask.any() and not info.any()


def _box_solver(ia, bc):
    b = bc.b
    S = len(bc.names)
    g = ia.ILQR(b.m, b.state(S), rc.H, b.cost)
    t = b.traj
    g.set_traj(ia.State(*(np.concatenate([t[k]] * S) for k in ("time", "qpos", "qvel", "warm")),
                        bc.ctrl.reshape(S * (rc.H + 1), b.nu)))
    g.set_deriv(bc.rec)
    g.set_mu(rc.MU)
    return g


def _deviation(out, refs, what):
    """largest deviation per array, relative to the array's maximum, over the cases"""
    worst = dict.fromkeys(ARRAYS, 0.0)
    for s, r in enumerate(refs):
        for n in ARRAYS:
            want = r[n][1:] if n in ("K", "k") else r[n]
            worst[n] = max(worst[n], _rel(out[n][s].reshape(np.shape(want)), want))
    print(f"{what}: {worst}")
    return max(worst.values())


@gpu
@pytest.mark.parametrize("name", BOX_MODELS)
def test_boxed_steps_against_kkt_reference(ia, ora, name):
    """3: horizon 2, one boxed case per seed (one control at lo, one at hi, all
    clamped, mixed, a box that excludes 0).  mask is the reference's active set
    exactly; K, k, V, v within tol = max(1e-12, 10 E0) of it.

    Measured on MI355X (E0 = exact engine without limits against the unboxed
    longdouble recursion; then the boxed deviation):
      pendulum  E0 = 6.8e-16  boxed 3.4e-16  (QP iterations 0: one control)
      hopper    E0 = 1.4e-14  boxed 7.4e-15  (QP iterations <= 4)
      chain     E0 = 7.2e-14  boxed 3.0e-14  (QP iterations <= 7)
    so tol = 1e-12 in all three; no fallback."""
    bc = _boxcases(ia, ora, name)
    g = _box_solver(ia, bc)
    g.riccati_pass()
    E0 = _deviation(_results(g), bc.free, f"{name} E0 (no limits)")
    g.set_ctrl_limits(bc.lo, bc.hi)
    g.riccati_pass()
    out = _results(g)
    mask, info = g.clamped()
    dev = _deviation(out, bc.ref, f"{name} boxed")
    tol = _tol(E0)
    print(f"{name}: E0 = {E0:.3e}, tol = {tol:.3e}, boxed deviation = {dev:.3e}, QP iterations up to "
          f"{int((info & 0x7fffffff).max())}, fallbacks {int((info >> 31).sum())}")
    for s, r in enumerate(bc.ref):
        assert np.array_equal(mask[s], r["mask"]), (name, bc.names[s], mask[s], r["mask"])
    assert not mask[:, 0].any() and not info[:, 0].any()
    assert not (info >> 31).any()
    assert dev <= tol, (name, dev, tol, E0)


@gpu
@pytest.mark.parametrize("name", ("hopper", "chain"))
def test_rank_one_takes_the_fallback(ia, ora, name):
    """3, mu = 0: family T's rank-one case (Mm = -2 r r').  The limits cut the
    one non-zero entry of the unconstrained k in half and leave the others (0)
    free, so the free block is a singular rank-one block of two or more
    controls: bit 31 of info, finite outputs, k within the bounds.  (With one
    control -- the pendulum -- a rank-one Mm is a regular 1 x 1 matrix and the
    step has no reason to fall back; it is covered by the boxed cases above.)"""
    b = _bundle(ia, ora, name)
    s = [c.kind for c in b.cases].index("rank1")
    kunc = b.ref[0.0][s]["k"][1]
    assert np.count_nonzero(kunc) == 1
    half = float(np.max(np.abs(kunc))) / 2
    g = trc._solver(ia, b, "exact")
    g.set_ctrl_limits(-half, half)
    out = trc._pass(g, b, mu=0.0)
    mask, info = g.clamped()
    assert info[s, 1] >> 31 == 1, hex(int(info[s, 1]))
    assert mask[s, 1] == 1 << int(np.argmax(np.abs(kunc)))
    for n in ARRAYS:
        assert np.isfinite(out[n][s]).all(), n
    ustar = b.traj["ctrl"][1:]
    assert np.all(out["k"][s] >= -half - ustar) and np.all(out["k"][s] <= half - ustar)
    assert np.array_equal(out["k"][s][0], np.clip(kunc, -half, half))
    g.set_mu(rc.MU)


@gpu
@pytest.mark.parametrize("name", sorted(HORIZON))
def test_boxed_recursion_over_a_horizon(ia, ora, name):
    """4: iterate() with limits u* -+ c median|k_unconstrained| (c chosen on the
    CPU), then the recursion recomputed by boxqp_ref from the device's own
    deriv() and traj(): the same masks, K, k, V, v within tol, E0 over the
    same horizon.

    Measured on MI355X:
      hopper (corrected layout), c = 1     E0 = 3.0e-15  boxed 1.5e-15
      pendulum (reference layout), c = 1   E0 = 2.6e-15  boxed 1.6e-15
    so tol = 1e-12 in both; 10 of 20 steps left the fast path in each."""
    h, (c, lo, hi, _, _) = _horizon(ia, ora, name)
    m = h.m
    g = ia.ILQR(m, _dmain(ia, m, name), H20, h.cost)
    g.set_layout(h.layout)
    g.iterate()
    t = g.traj()
    traj = {k: getattr(t, k) for k in ("time", "qpos", "qvel", "warm", "ctrl")}
    dev_h = Horizon(ia, ora, name, recs=g.deriv()[0], traj=traj)
    free = dev_h.recursion(np.full(m.nu, -INF), np.full(m.nu, INF))
    E0 = _deviation(_results(g), [free], f"{name} H={H20} E0 (no limits)")
    g2 = ia.ILQR(m, _dmain(ia, m, name), H20, h.cost)
    g2.set_layout(h.layout)
    g2.set_ctrl_limits(lo, hi)
    g2.iterate()
    out = _results(g2)
    t2 = g2.traj()
    for k in ("qpos", "qvel", "ctrl"):
        exact(getattr(t2, k), getattr(t, k), f"{name} {k}: zero gains, u* inside the limits")
    exact(g2.deriv(), g.deriv(), "deriv")
    ref = dev_h.recursion(lo, hi)
    _conditions([ref], m.nu, f"{name} H={H20} c={c} (device records)")
    mask, info = g2.clamped()
    dev = _deviation(out, [ref], f"{name} H={H20} boxed")
    tol = _tol(E0)
    left = int(np.count_nonzero(mask[0, 1:]))
    print(f"{name} H={H20} c={c}: E0 = {E0:.3e}, tol = {tol:.3e}, boxed deviation = {dev:.3e}; {left} of {H20} "
          f"steps left the fast path, QP iterations up to {int((info & 0x7fffffff).max())}")
    assert np.array_equal(mask[0], ref["mask"]), (mask[0], ref["mask"])
    assert not (info >> 31).any()
    assert dev <= tol, (name, dev, tol, E0)


def _step_cost(p, q, v, u):
    s = 0.0
    for x, w, t, l in ((q, p["wq"], p["tq"], p["lq"]), (v, p["wv"], p["tv"], p["lv"]), (u, p["wu"], p["tu"], p["lu"])):
        for i in range(len(x)):
            if w[i] != 0:
                dx = float(x[i]) - float(t[i])
                s += float(w[i]) * dx * dx
            if l[i] != 0:
                s += float(l[i]) * float(x[i])
    return s


class ClampedRollout:
    """the inputs of GPU item 5 (pendulum, H = 20, 8 alpha candidates, seeded
    gains, tight limits) and the restatement of the clamped rollout: per point
    n = N .. 0, u = clip((seq-dot K dx + alpha k) + u*), the record, the step
    cost, then the oracle's mj_step"""
    lo, hi = np.array([-0.02]), np.array([0.03])

    def __init__(self, ia, ora):
        import workloads
        self.alphas = workloads.LINESEARCH_ALPHAS
        self.m = m = ia.Model.load(model_path("inverted_pendulum"))
        self.om = ora.OModel(m.blob())
        self.dmain = _cpu_dmain(ia, ora, m, "inverted_pendulum")
        rng = np.random.default_rng(20261019)
        P = H20 + 1
        self.K = rng.standard_normal((1, P, m.nu * 2 * m.nv)) * 2.0
        self.k = rng.standard_normal((1, P, m.nu)) * 1.0
        self.cost = ia.PENDULUM_COST.packed(m.nq, m.nv, m.nu)

    def nominal(self, ora):
        """the constructor's passive rollout (what a fresh solver's traj() holds)"""
        d = self.om.make_data()
        dm = self.dmain
        d.set_state(time=dm.time[0], qpos=dm.qpos[0], qvel=dm.qvel[0], warm=dm.warm[0], ctrl=dm.ctrl[0])
        return ora.OILQR(self.om, d, H20, cost_fn="ora_cost_pendulum").traj()

    def restate(self, nom):
        """-> per candidate: trajectory dict, cost, number of controls the clamp changed"""
        m, dm, K, k, lo, hi = self.m, self.dmain, self.K, self.k, self.lo, self.hi
        P, nu, nx, nv = H20 + 1, m.nu, 2 * m.nv, m.nv
        out = []
        for alpha in self.alphas:
            d = self.om.make_data()
            d.set_state(time=dm.time[0], qpos=dm.qpos[0], qvel=dm.qvel[0], warm=dm.warm[0], ctrl=dm.ctrl[0])
            tr = dict(time=np.zeros(P), qpos=np.zeros((P, m.nq)), qvel=np.zeros((P, nv)), warm=np.zeros((P, nv)),
                      ctrl=np.zeros((P, nu)))
            c, hit = 0.0, 0
            for n in range(P - 1, -1, -1):
                s = d.state()
                dx = np.concatenate([s["qpos"] - nom["qpos"][n], s["qvel"] - nom["qvel"][n]])
                u = np.zeros(nu)
                for i in range(nu):
                    acc = 0.0
                    for j in range(nx):
                        acc += float(K[0, n, i + j * nu]) * float(dx[j])
                    cv = (acc + float(alpha) * float(k[0, n, i])) + float(nom["ctrl"][n, i])
                    hit += bool(cv < lo[i] or cv > hi[i])
                    u[i] = lo[i] if cv < lo[i] else (hi[i] if cv > hi[i] else cv)
                for f in ("time", "qpos", "qvel", "warm"):
                    tr[f][n] = s[f]
                tr["ctrl"][n] = u
                c += _step_cost(self.cost, s["qpos"], s["qvel"], u)
                d.set_state(ctrl=u)
                d.step()
            out.append((tr, c, hit))
        return out


def test_clamped_rollout_inputs_bind(ia, ora):
    """the limits of GPU item 5 do change controls: in at least half of the
    candidates, and on average at least one control in four of those rollouts"""
    cr = ClampedRollout(ia, ora)
    hits = [h for _, _, h in cr.restate(cr.nominal(ora))]
    print("controls changed by the clamp, per alpha candidate:", hits)
    bind = [h for h in hits if h]
    assert len(bind) >= len(hits) // 2 and sum(bind) >= len(bind) * (H20 + 1) // 4, hits


@gpu
def test_clamped_rollout_bitexact(ia, ora):
    """5: pendulum (no ctrllimited motor: the physics clips nothing, so the clamp
    changes the dynamics): forward_pass() with gains from set_gains and tight
    limits gives the selected candidate's ctrl, qpos, qvel, warm, time and every
    candidate's cost bit-identical to the restatement (ClampedRollout)"""
    cr = ClampedRollout(ia, ora)
    m = cr.m
    g = ia.ILQR(m, cr.dmain, H20, ia.PENDULUM_COST, alphas=cr.alphas, select="min_cost")
    t = g.traj()
    nom = {f: getattr(t, f) for f in ("time", "qpos", "qvel", "warm", "ctrl")}
    ref = cr.nominal(ora)
    for f in nom:
        exact(nom[f].reshape(ref[f].shape), ref[f], f"nominal {f}")
    g.set_gains(cr.K, cr.k)
    g.set_ctrl_limits(cr.lo, cr.hi)
    g.forward_pass()
    g.synchronize()
    res = cr.restate(nom)
    costs = [c for _, c, _ in res]
    gc, gsel = g.costs()
    exact(gc[0], np.array(costs), "candidate costs")
    best = int(np.argmin(costs))
    assert gsel[0] == best
    t = g.traj()
    for f in ("time", "qpos", "qvel", "warm", "ctrl"):
        exact(getattr(t, f).reshape(res[best][0][f].shape), res[best][0][f], f)
    assert np.all(t.ctrl >= cr.lo) and np.all(t.ctrl <= cr.hi)
    print(f"selected candidate {best}: the clamp changed {res[best][2]} of its {H20 + 1} controls")


@gpu
def test_clamp_under_a_clipping_model(ia):
    """6: hopper (ctrllimited motors: mj_fwdActuation clips to ctrlrange
    already), limits = ctrlrange, saturating gains: the states are the
    unlimited rollout's bit for bit, ctrl is its clip, the cost differs"""
    import workloads
    m = ia.Model.load(model_path("hopper"))
    dmain = workloads.hopper_dmain(m)
    rng = np.random.default_rng(20261020)
    P = H20 + 1
    K = rng.standard_normal((1, P, m.nu * 2 * m.nv)) * 5.0
    k = rng.standard_normal((1, P, m.nu)) * 3.0
    out = []
    for lim in (False, True):
        g = ia.ILQR(m, dmain, H20, ia.HOPPER_COST)
        g.set_gains(K, k)
        if lim:
            g.set_ctrl_limits("model")
            lo, hi = g.ctrl_limits()
            assert lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0] * 3
        g.forward_pass()
        g.synchronize()
        out.append((g.traj(), g.costs()[0]))
    (t0, c0), (t1, c1) = out
    for f in ("time", "qpos", "qvel", "warm"):
        exact(getattr(t1, f), getattr(t0, f), f)
    assert np.count_nonzero(np.abs(t0.ctrl) > 1.0) >= P // 4  # the gains do saturate
    exact(t1.ctrl, np.clip(t0.ctrl, -1.0, 1.0), "ctrl")
    assert c0[0, 0] != c1[0, 0] and np.isfinite(c1).all()


@gpu
@pytest.mark.parametrize("name", ("chain", "humanoid"))
def test_generic_rollout_clamps(ia, ora, name):
    """the clamped variants of the generic rollout kernel (k_rollout2_coop<MT, true>:
    the run-time instance for the chain, the 27-dof one for the humanoid), H = 5.
    With K = 0 the control law is alpha k + u* whatever the state, so the
    limited run's ctrl is exactly the clip of the unlimited run's.  The chain's
    motors are not ctrllimited (the states then differ); the humanoid's are, and
    with limits = its ctrlrange the states are the unlimited run's bit for bit."""
    b = _bundle(ia, ora, name)
    H = 5
    rng = np.random.default_rng([20261021, b.nu])
    K = np.zeros((1, H + 1, b.nu * b.nx))
    k = rng.standard_normal((1, H + 1, b.nu))
    out = []
    for lim in (False, True):
        g = ia.ILQR(b.m, b.state(1), H, b.cost)
        g.set_gains(K, k)
        if lim:
            g.set_ctrl_limits("model" if name == "humanoid" else 0.3 * np.linspace(-1, -2, b.nu),
                              None if name == "humanoid" else 0.3 * np.linspace(2, 1, b.nu))
            lo, hi = g.ctrl_limits()
        g.forward_pass()
        g.synchronize()
        out.append((g.traj(), g.costs()[0]))
    (t0, c0), (t1, c1) = out
    assert np.count_nonzero((t0.ctrl < lo) | (t0.ctrl > hi)) >= t0.ctrl.size // 4
    exact(t1.ctrl, np.clip(t0.ctrl, lo, hi), f"{name} ctrl")
    assert np.isfinite(c1).all() and c1[0, 0] != c0[0, 0]
    same = all(np.array_equal(getattr(t1, f), getattr(t0, f)) for f in ("qpos", "qvel", "warm"))
    assert same == (name == "humanoid")


@gpu
def test_closed_loop_stays_within_limits(ia):
    """7: pendulum, corrected layout, 5 iterations with limits on"""
    m = ia.Model.load(model_path("inverted_pendulum"))
    g = ia.ILQR(m, _dmain(ia, m, "inverted_pendulum"), H20, ia.PENDULUM_COST,
                alphas=(1.0, 0.5, 0.25, 0.125), select="min_cost")
    g.set_layout("corrected")
    lo, hi = np.array([-0.002]), np.array([0.005])  # the first pass's unconstrained k is 0.01 .. 0.03
    g.set_ctrl_limits(lo, hi)
    nclamped = 0
    for _ in range(5):
        g.iterate()
        g.synchronize()
        t = g.traj()
        K, k = g.gains()
        V, v = g.value()
        for a in (t.qpos, t.qvel, t.ctrl, t.warm, K, k, V, v, g.costs()[0]):
            assert np.isfinite(a).all()
        assert np.all(t.ctrl >= lo) and np.all(t.ctrl <= hi)
        nclamped += int(np.count_nonzero(g.clamped()[0]))
    assert nclamped > 0


@gpu
def test_combinations_and_arguments(ia):
    """8: MFMA + limits and groups > 1 + limits are unsupported in either order;
    bad arguments are refused; switching the limits off restores the fused iterate"""
    m = ia.Model.load(model_path("hopper"))
    dmain = _dmain(ia, m, "hopper")
    two = ia.State(*(np.repeat(getattr(dmain, f), 2, 0) for f in ("time", "qpos", "qvel", "warm", "ctrl")))
    g = ia.ILQR(m, two, H20, ia.HOPPER_COST)
    UNSUPPORTED, ARG = "code 4", "code 1"
    g.set_ctrl_limits("model")
    with pytest.raises(ia.IlqgError, match=UNSUPPORTED):
        g.set_riccati("mfma")
    with pytest.raises(ia.IlqgError, match=UNSUPPORTED):
        g.set_groups(2)
    g.set_ctrl_limits(None, None)
    assert g.ctrl_limits() is None
    g.set_riccati("mfma")
    with pytest.raises(ia.IlqgError, match=UNSUPPORTED):
        g.set_ctrl_limits("model")
    g.set_riccati("exact")
    g.set_groups(2)
    with pytest.raises(ia.IlqgError, match=UNSUPPORTED):
        g.set_ctrl_limits("model")
    g.set_groups(1)
    assert g.ctrl_limits() is None
    for lo, hi in (([0.5, -1, -1], [0.4, 1, 1]), ([np.nan, -1, -1], [1, 1, 1]), ([-1, -1, -1], [1, np.nan, 1]),
                   ([-1, -1, -1], None), (None, [1, 1, 1])):
        with pytest.raises(ia.IlqgError, match=ARG):
            g.set_ctrl_limits(lo, hi)
    assert g.ctrl_limits() is None
    g.set_ctrl_limits([-1, -INF, 0.25], [1, INF, 0.25])  # one-sided, unbounded and lo == hi are fine
    lo, hi = g.ctrl_limits()
    assert lo.tolist() == [-1, -INF, 0.25] and hi.tolist() == [1, INF, 0.25]
    # limits on: the unfused order; off again: the fused launch, and a fresh solver's bits
    g.set_timing(True)
    g.iterate()
    tm = g.timing()
    assert tm["backward"][1] == 1 and tm["fd_backward"][1] == 0, tm
    g2 = ia.ILQR(m, two, H20, ia.HOPPER_COST)
    g2.set_ctrl_limits(-0.5, 0.5)
    g2.set_ctrl_limits(None, None)
    g2.set_timing(True)
    fresh = ia.ILQR(m, two, H20, ia.HOPPER_COST)
    res = []
    for s in (g2, fresh):
        s.iterate()
        s.iterate()
        s.synchronize()
        t = s.traj()
        res.append((t.qpos, t.qvel, t.ctrl, t.warm, *s.gains(), *s.value(), s.costs()[0]))
    for a, b_ in zip(*res):
        exact(a, b_, "limits switched off against a fresh solver")
    tm = g2.timing()
    assert tm["fd_backward"][1] == 2 and tm["backward"][1] == 0, tm
    assert not g2.clamped()[0].any() and not g2.clamped()[1].any()

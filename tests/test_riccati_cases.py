"""Riccati edge-case parity: tied, zero and tiny LDLT pivots, odd sizes.

Crafted FD records (tests/riccati_cases.py) run through the backward pass of
four model sizes -- the bundled pendulum (nv 2, nu 1), hopper (6, 3) and
humanoid (27, 21), and a 9-hinge chain with 7 motors (9, 7) that drives the
generic k_backward<0,0> / k_backward_mfma<0,0> through their padded-LX,
prefetch and runtime-n LDLT branches -- at horizon 2, every case one seed of one
solver.  The oracle (OILQR.backward_from_records) is the reference, bit for
bit for the exact engine.

The unmarked tests pin the generator against the oracle alone, so the GPU
tests cannot pass vacuously: the cases do present pivot ties whose scan-and-swap
order differs from the index-stable one, the single-term claim of family T
holds, and a restated LDLT with the stable tie rule gives other bits of k."""
import numpy as np
import pytest

import riccati_cases as rc
from conftest import model_path

gpu = pytest.mark.gpu
MODELS = ("inverted_pendulum", "hopper", "chain", "humanoid")
ARRAYS = ("K", "k", "V", "v")
# SURVEY.md §8d's per-step Riccati budget, as tests/test_gpu_parity.py::test_riccati_mfma_step
MFMA_STEP_RTOL = 1e-12


def exact(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b, equal_nan=True):
        with np.errstate(all="ignore"):
            err = np.nanmax(np.abs(a - b))
        raise AssertionError(f"{what}: not bit-exact, max|diff|={err:.3e}")


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def chain_xml(nlink=9, nmotor=7, length=0.2):
    """a serial chain of hinges about y hanging from the world, the first nmotor of them driven"""
    s = ['<mujoco model="chain">',
         '<compiler angle="radian" coordinate="global" inertiafromgeom="true"/>',
         '<option integrator="Euler" timestep="0.002"/>', "<worldbody>"]
    for i in range(nlink):
        z0, z1 = 2.0 - length * i, 2.0 - length * (i + 1)
        s += [f'<body name="link{i}" pos="0 0 {z0:.3f}">',
              f'<joint name="hinge{i}" type="hinge" axis="0 1 0" pos="0 0 {z0:.3f}" armature="0.1" damping="0.5" '
              'limited="false"/>',
              f'<geom name="cap{i}" type="capsule" fromto="0 0 {z0:.3f} 0 0 {z1:.3f}" size="0.03" contype="0" '
              'conaffinity="0"/>']
    s += ["</body>"] * nlink + ["</worldbody>", "<actuator>"]
    s += [f'<motor joint="hinge{i}" gear="{10 + 5 * i}" ctrllimited="false"/>' for i in range(nmotor)]
    s += ["</actuator>", "</mujoco>"]
    return "\n".join(s)


class Bundle:
    """one model size: the model, its cases, the nominal trajectory and the
    oracle's K, k, V, v of every case (computed once, shared by every test)"""

    def __init__(self, ia, ora, name):
        self.name = name
        self.m = m = ia.Model.from_string(chain_xml()) if name == "chain" else ia.Model.load(model_path(name))
        self.cost = {"inverted_pendulum": ia.PENDULUM_COST, "hopper": ia.HOPPER_COST, "humanoid": ia.HUMANOID_COST,
                     "chain": ia.Cost(wq=[1.0] * 9, wv=[0.1] * 9, wu=[0.01] * 7)}[name]
        self.nv, self.nu, self.nx, self.dt = m.nv, m.nu, 2 * m.nv, m.timestep
        self.cases = rc.make_cases(m.nv, m.nu, m.timestep)
        self.om = om = ora.OModel(m.blob())
        st = self.state(1)
        d = om.make_data()
        d.set_state(time=st.time[0], qpos=st.qpos[0], qvel=st.qvel[0], warm=st.warm[0], ctrl=st.ctrl[0])
        self.il = il = ora.OILQR(om, d, rc.H, cost_fn="ora_cost_desc_fn")
        self.traj = t = il.traj()
        # c of step 1: x*_0 (-) x*_1
        self.c1 = ora.state_diff(om, t["qpos"][0], t["qvel"][0], t["qpos"][1], t["qvel"][1])
        self.ref = {}
        for mu in (rc.MU, 0.0):
            il.set_mu(mu)
            self.ref[mu] = []
            for c in self.cases:
                il.backward_from_records(c.rec, c.V0, c.v0)
                a = il.arrays()
                self.ref[mu].append({n: a[n] for n in ARRAYS})
        il.set_mu(rc.MU)

    def state(self, n):
        st = self.m.reset_state(n)
        if self.name == "humanoid":
            st.qpos[:, 2] = 1.4  # humanoid.xml:49-50 initial height, as cfg 5
        if self.name == "chain":
            st.qpos[:] = 0.05 * (1 + np.arange(self.m.nq))
        return st

    def start(self, c):
        """V0, v0 the recursion of case c starts from (initV: v = q_0, V = v v')"""
        if c.V0 is not None:
            return c.V0, c.v0
        q0 = rc.unpack(c.rec[0], self.nv, self.nu)[3]
        return np.outer(q0, q0), q0.copy()

    def keys(self, c):
        """|diag(Mm)| of step 1 in the oracle's loop order"""
        V0, v0 = self.start(c)
        return np.abs(np.diag(rc.step_inputs(c.rec[1], self.nv, self.nu, self.dt, rc.MU, V0, v0, self.c1)[0]))


_bundles = {}


@pytest.fixture(params=MODELS)
def bundle(request, ia, ora):
    if request.param not in _bundles:
        _bundles[request.param] = Bundle(ia, ora, request.param)
    return _bundles[request.param]


def test_chain_is_generic(ia):
    m = ia.Model.from_string(chain_xml())
    assert (m.nq, m.nv, m.nu, m.D) == (9, 9, 7, 250)
    assert m.static_id() == 0


def test_case_counts(bundle):
    kinds = [c.kind for c in bundle.cases]
    assert len(bundle.cases) <= 40
    assert all(c.rec.shape == (rc.H + 1, bundle.m.D) for c in bundle.cases)
    if bundle.nu == 21:
        assert kinds.count("ties") + kinds.count("zero") >= 24
    elif bundle.nu == 7:
        assert kinds.count("ties") + kinds.count("zero") >= 12
    elif bundle.nu == 3:
        assert kinds.count("enum") == 27
        assert len({c.name for c in bundle.cases if c.kind == "enum"}) == 27
    if bundle.nu > 1:
        for k in ("alltie", "allzero", "rank1", "denorm", "nan", "S", "D"):
            assert k in kinds, k
    else:
        assert {"T-zero", "T-denorm", "T-normal"} <= {c.name for c in bundle.cases}
    # a second call gives the same records: seeded
    again = rc.make_cases(bundle.nv, bundle.nu, bundle.dt)
    assert all(np.array_equal(a.rec, b.rec, equal_nan=True) for a, b in zip(again, bundle.cases))


# at least this many tie cases must have a scan-and-swap pivot order other than
# the index-stable one.  nu = 3: the enumeration of {zero, lo, hi} is exhaustive,
# so the count is a fact of Eigen's scan, not of a draw: the orders differ
# exactly where two equal keys stand in front of a larger one -- (lo, lo, hi),
# (zero, zero, hi), (zero, zero, lo) -- the only patterns where the first swap
# carries row 0 behind its equal; 3 of 27, asserted as an equality
MIN_ORDER_DIFFERS = {21: (20, 24), 7: (8, 12), 3: (3, 27)}
ENUM_ORDER_DIFFERS = {"T-enum-llh", "T-enum-zzh", "T-enum-zzl"}


def test_tie_order_differs_from_stable(bundle):
    """4a, 4b: the tie cases do tie, the maximum key included, and Eigen's
    scan-and-swap order is not the index-stable descending order"""
    if bundle.nu == 1:
        return  # one control: no pivot choice
    tie =[c for c in bundle.cases if c.tie_case]
    need, of = MIN_ORDER_DIFFERS[bundle.nu]
    assert len(tie) >= of
    differs = maxtied = anytie = 0
    for c in tie:
        ky = bundle.keys(c)
        d = rc.eigen_order(ky) != rc.stable_order(ky)
        differs += d
        if bundle.nu == 3:
            assert d == (c.name in ENUM_ORDER_DIFFERS), c.name
        maxtied += int(np.sum(ky == ky.max()) >= 2)
        anytie += len(set(ky.tolist())) < len(ky)
    print(f"{bundle.name}: pivot order differs from the stable one in {differs} of {len(tie)} tie cases; "
          f"the maximum key is tied in {maxtied} of the {anytie} cases with a tie")
    assert differs >= need, (differs, len(tie))
    # (the exhaustive hopper enumeration includes the 6 patterns without a tie)
    assert 2 * maxtied >= anytie, (maxtied, anytie)
    if bundle.nu >= 7:
        assert anytie == len(tie)


def test_family_T_is_single_term(bundle):
    """4c: Mm, T3 and B'w + r of family T have the same bits with every sum reversed"""
    for c in bundle.cases:
        if c.family != "T":
            continue
        V0, v0 = bundle.start(c)
        assert not V0.any() and not v0.any()
        fwd = rc.step_inputs(c.rec[1], bundle.nv, bundle.nu, bundle.dt, rc.MU, V0, v0, bundle.c1)
        rev = rc.step_inputs(c.rec[1], bundle.nv, bundle.nu, bundle.dt, rc.MU, V0, v0, bundle.c1, reverse=True)
        for a, b, n in zip(fwd, rev, ("Mm", "T3", "B'w + r")):
            assert rc.same_bits(a, b), (bundle.name, c.name, n)


def test_oracle_results_are_what_the_cases_claim(bundle):
    """4d: finite everywhere but T-nan; the structurally zero and the denormal
    controls get zero gain rows and zero feed-forward"""
    nu, nx = bundle.nu, bundle.nx
    for c, r in zip(bundle.cases, bundle.ref[rc.MU]):
        fin = all(np.isfinite(r[n]).all() for n in ARRAYS)
        assert fin == c.finite, (bundle.name, c.name)
        K1, k1 = r["K"][1].reshape(nx, nu).T, r["k"][1]  # K is nu x nx, column-major
        if c.kind in ("zero", "enum", "enum1", "allzero", "denorm"):
            for a in c.special:
                assert not K1[a].any() and k1[a] == 0, (bundle.name, c.name, a)
        if c.kind == "denorm":
            ky = bundle.keys(c)
            assert all(0 < ky[a] <= rc.DBL_MIN for a in c.special), ky[list(c.special)]
        if c.kind == "allzero":
            assert not K1.any() and not k1.any()
        if c.kind == "nan":  # (one control: the NaN pivot is the early exit's, the solve writes 0)
            assert np.isnan(k1).any() or nu == 1
    for c, r in zip(bundle.cases, bundle.ref[0.0]):
        if c.kind == "rank1":
            assert all(np.isfinite(r[n]).all() for n in ARRAYS)


def test_restated_ldlt_is_sensitive_to_the_tie_rule(bundle):
    """4e: the Python restatement of ora_ldlt_factor / ora_ldlt_solve gives the
    oracle's k of step 1 bit for bit in every case; with the index-stable tie
    rule it gives other bits wherever that changes the order of the non-zero
    pivots (a permutation among all-zero rows changes nothing) -- in every such
    humanoid case, so a bit-for-bit GPU comparison sees a wrong tie order"""
    changed = other = 0
    for c, r in zip(bundle.cases, bundle.ref[rc.MU]):
        V0, v0 = bundle.start(c)
        Mm, _, rhs = rc.step_inputs(c.rec[1], bundle.nv, bundle.nu, bundle.dt, rc.MU, V0, v0, bundle.c1)
        L, tr = rc.ldlt_factor(Mm)
        assert rc.same_bits(rc.ldlt_solve(L, tr, rhs), r["k"][1]), (bundle.name, c.name)
        if not c.tie_case:
            continue
        ky = np.abs(np.diag(Mm))
        nz = [[i for i in order(ky) if ky[i] > 0] for order in (rc.eigen_order, rc.stable_order)]
        if nz[0] == nz[1]:
            continue
        changed += 1
        L, tr = rc.ldlt_factor(Mm, rule="stable")
        other += not rc.same_bits(rc.ldlt_solve(L, tr, rhs), r["k"][1])
    print(f"{bundle.name}: the stable tie rule changes the non-zero pivot order in {changed} tie cases "
          f"and the bits of k in {other} of them")
    if bundle.nu == 21:
        assert changed >= 20 and other == changed, (changed, other)
    elif bundle.nu > 1:
        assert other >= 1, (changed, other)


# ---- GPU
def _solver(ia, b, engine):
    S = len(b.cases)
    g = ia.ILQR(b.m, b.state(S), rc.H, b.cost)
    t = b.traj
    g.set_traj(ia.State(*(np.concatenate([t[k]] * S) for k in ("time", "qpos", "qvel", "warm", "ctrl"))))
    g.set_riccati(engine)
    g.set_deriv(np.stack([c.rec for c in b.cases]))
    return g


def _pass(g, b, mu=rc.MU, vinit=True):
    """one backward pass over every case; vinit: from each case's own V0, v0
    (set_value is one-shot), else through the kernel's initV"""
    g.set_mu(mu)
    if vinit:
        st = [b.start(c) for c in b.cases]
        g.set_value(np.stack([V for V, _ in st]), np.stack([v for _, v in st]))
    g.riccati_pass()
    g.synchronize()
    K, k = g.gains()
    V, v = g.value()
    return dict(K=K[:, 1:], k=k[:, 1:], V=V, v=v)


def _against_oracle(b, out, mu, what, families="TSD"):
    for s, (c, r) in enumerate(zip(b.cases, b.ref[mu])):
        if c.family not in families:
            continue
        for n in ARRAYS:
            exact(out[n][s], r[n][1:] if n in ("K", "k") else r[n], f"{b.name} {c.name} {n} ({what})")


@gpu
def test_exact_engine_bitexact(ia, bundle):
    """the exact engine on every case of every size: K, k, V, v of both steps
    are the oracle's bit for bit -- through the kernel's own initV (families T
    and D), from each case's V0 (set_value, every family), and at mu = 0 (Mm
    rank one: after the first pivot every Schur entry is an exact zero)"""
    g = _solver(ia, bundle, "exact")
    _against_oracle(bundle, _pass(g, bundle, vinit=False), rc.MU, "initV", "TD")
    _against_oracle(bundle, _pass(g, bundle), rc.MU, "set_value")
    _against_oracle(bundle, _pass(g, bundle, mu=0.0), 0.0, "mu = 0")


def _mfma_checks(b, out, what):
    """family T: step 1's K and k have zero difference from the oracle (+-0
    equal, NaN in the same places) -- every product there has one term, so the
    matrix core's summation order cannot show and the pivot order must be the
    oracle's.  Every finite case but T-rank1: both steps within the per-step
    budget, relative to each array's maximum."""
    worst = dict.fromkeys(ARRAYS, 0.0)
    for s, (c, r) in enumerate(zip(b.cases, b.ref[rc.MU])):
        if c.family == "T":
            for n in ("K", "k"):
                got, want = out[n][s, 0], r[n][1]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (b.name, c.name, n, what)
                ok = ~np.isnan(want)
                assert np.all(got[ok] - want[ok] == 0), (b.name, c.name, n, what,
                                                         float(np.max(np.abs(got[ok] - want[ok]))))
        if c.finite and c.kind != "rank1":
            for n in ARRAYS:
                e = _rel(out[n][s], r[n][1:] if n in ("K", "k") else r[n])
                worst[n] = max(worst[n], e)
                assert e <= MFMA_STEP_RTOL, (b.name, c.name, n, e, what)
    print(f"{b.name} MFMA Riccati ({what}), max relative deviation over the finite cases, two steps:", worst)


@gpu
def test_mfma_engine(ia, bundle, monkeypatch):
    """the MFMA engine on the same cases (k_backward_mfma<0,0> for the chain,
    hopper and pendulum; the compile-time humanoid instance with its LDLT on
    LDS, in registers, and in registers with the pivot replay forced --
    ILQG_LDLT_REG 0, 1, 2 -- which must agree bit for bit on all four arrays)"""
    g = _solver(ia, bundle, "mfma")
    if bundle.nu != 21:
        _mfma_checks(bundle, _pass(g, bundle), "generic")
        return
    out = {}
    for flag in ("0", "1", "2"):
        monkeypatch.setenv("ILQG_LDLT_REG", flag)
        out[flag] = _pass(g, bundle)
    for flag in ("1", "2"):
        for n in ARRAYS:
            exact(out[flag][n], out["0"][n], f"{n} (ILQG_LDLT_REG={flag} against 0)")
    for flag in ("0", "1", "2"):
        _mfma_checks(bundle, out[flag], f"ILQG_LDLT_REG={flag}")

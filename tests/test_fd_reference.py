"""The FD derivative records (calcMJDerivatives at a trajectory point) against an
independent reference: tests/fd_ref.py differentiates tests/rigid_ref.py (np.longdouble,
no recursion shared with the oracle or the kernels) by the record's own definition,
central differences of qacc and forward differences of the step cost at eps = 1e-6
(mjderivative.cpp:39), the qpos columns stepped in the tangent space.  Every other FD
test compares the kernels with oracle/ilqr_ora.c bit for bit; here the oracle is held to
the reference without a GPU and the kernels with one, so a convention the two share (a
quaternion column in the wrong frame, a stale stage, a dropped load, a cost column on a
quaternion dof) has somewhere to show.

The target is the longdouble record at the project's eps, not the eps -> 0 Jacobian: the
record is by definition a finite difference.

States: the airborne batches of test_physics_reference.py (all six models, with their
qfrc_applied / xfrc_applied and clipped motors) and its literal contact cases (all seven
models), a seeded qfrc_applied added to every second case of a model so that loads and
constraints meet.  The humanoid runs its first four airborne states and three contact
cases.  The cost is dense and seeded: every w, t, l non-zero, quaternion components too.

Tolerance, per block (dq, dv, du, cost), deviations relative to the block's largest
reference magnitude at that state: bound = max(2 nv E64, floor).  E64 is the largest
deviation over the batch of fd_ref run in float64 from fd_ref in longdouble (the rule of
test_physics_reference.py: two backward-stable evaluations in different operation
orders).  The floor is the rounding of one record entry: 2^-52 max|qacc| / eps for the
dynamics blocks (an entry is a difference of two float64 accelerations over 2 eps),
2^-52 |c| / eps for the cost block (a difference of two float64 costs over eps),
relative to the block at that state.  A block whose reference is all zero (a clipped
motor's column where it is the only motor) must be exactly zero.

A contact case is compared only if fd_ref.same_active_set holds, a condition on the
reference alone; at most two cases in all and one per model may fail it (asserted;
none does).

Building the reference (longdouble and float64 records of every state, CPU seconds,
measured): airborne pendulum 0.1, hopper 0.5, humanoid 9.1, chain 1.2, ballarm 0.6,
floatarm 0.5; contact hopper 0.3, pendulum 0.1, humanoid 14.2, cross 0.3, parallel 0.1,
ballarm 0.4 (REFERENCE_SECONDS below; each build is asserted to stay inside three times
its figure plus two seconds for a loaded machine).  Every record is built once per
process and shared by the tests that need it.

Out of scope: the fp32 sweep (its statistical envelope in test_gpu_parity.py stays as it
is), and the discrete-time A, B of the corrected layout against the Jacobian of Ref.step
(quirk Q10's explicit top block and the implicit damping are documented deviations).
"""
import time

import numpy as np
import pytest

import fd_ref as fr
from test_physics_reference import (CONTACT_MODELS, LD, MODELS, batch, cbatch, contact_product, product_model, report)

EPS = 1e-6
HUMANOID_AIRBORNE = 4
HUMANOID_CONTACT = ("on its back", "capsule-capsule edge", "sphere-sphere")
# static_id() == 0: the generic cooperative kernels (the humanoid too: only the pendulum and
# the hopper have compile-time instances, test_model_compile.py)
GENERIC = ("humanoid", "chain", "ballarm", "floatarm", "cross", "parallel")
# measured on the CPU: seconds to build (kind, model)'s reference, longdouble and float64
REFERENCE_SECONDS = {("airborne", "inverted_pendulum"): 0.1, ("airborne", "hopper"): 0.5, ("airborne", "humanoid"): 9.1,
                     ("airborne", "chain"): 1.2, ("airborne", "ballarm"): 0.6, ("airborne", "floatarm"): 0.5,
                     ("contact", "hopper"): 0.3, ("contact", "inverted_pendulum"): 0.1, ("contact", "humanoid"): 14.2,
                     ("contact", "cross"): 0.3, ("contact", "parallel"): 0.1, ("contact", "ballarm"): 0.4}


# ------------------------------------------------------------------ inputs
def dense_cost(ia, C, name):
    """every weight, target and linear term non-zero, seeded per model"""
    rng = np.random.default_rng([31, sorted(set(MODELS + CONTACT_MODELS)).index(name)])
    nu = len(C.act)

    def w(n):
        return rng.uniform(0.5, 2.0, n)

    def t(n):
        return rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return ia.Cost(wq=w(C.nq), tq=t(C.nq), lq=t(C.nq), wv=w(C.nv), tv=t(C.nv), lv=t(C.nv),
                   wu=w(nu), tu=t(nu), lu=t(nu))


def _states(kind, name):
    if kind == "airborne":
        S = batch(name).states[:HUMANOID_AIRBORNE if name == "humanoid" else None]
        return [dict(what=f"state {k}", q=s["q"], v=s["v"], ctrl=s["ctrl"], qf=s["qf"], xf=s["xf"], contact=False)
                for k, s in enumerate(S)]
    B = cbatch(name)
    S = B.states
    if name == "humanoid":
        S = [s for s in S if any(h in s["what"] for h in HUMANOID_CONTACT)]
        assert len(S) == len(HUMANOID_CONTACT)
    rng = np.random.default_rng(4100 + CONTACT_MODELS.index(name))
    out = []
    for k, s in enumerate(S):
        qf = rng.normal(0, 0.5, B.C.nv) * (0.3 if name == "humanoid" else 1.0) if k % 2 == 1 else np.zeros(B.C.nv)
        out.append(dict(what=s["what"], q=s["q"], v=s["v"], ctrl=s["ctrl"], qf=qf, xf=np.zeros((B.C.nbody, 6)),
                        contact=True))
    assert any(np.all(s["qf"] != 0) for s in out) and any(not np.any(s["qf"]) for s in out)
    return out


class Records:
    """the states of one model of one kind and the reference's records at them, computed once"""

    def __init__(self, ia, kind, name):
        self.kind, self.name = kind, name
        B = batch(name) if kind == "airborne" else cbatch(name)
        self.B, self.C, self.R, self.R64 = B, B.C, B.R, B.R64
        self.nv, self.nu = B.C.nv, len(B.C.act)
        self.sl = fr.block_slices(self.nv, self.nu)
        self.cost = dense_cost(ia, B.C, name)
        self.row = self.cost.row(B.C.nq, self.nv, self.nu)
        assert np.all(self.row != 0)
        states = _states(kind, name)
        t0 = time.perf_counter()
        self.excluded = [s for s in states if kind == "contact" and not fr.same_active_set(self.R, s, EPS)]
        assert len(self.excluded) <= 1, [s["what"] for s in self.excluded]
        self.states = [s for s in states if not any(s is x for x in self.excluded)]
        for s in self.states:
            s["ref"] = fr.record(self.R, self.row, s, EPS)
            s["ref64"] = fr.record(self.R64, self.row, s, EPS)
            # the sizes that one rounding of a record entry scales with
            s["scale"] = dict.fromkeys(("dq", "dv", "du"), float(np.max(np.abs(fr.qacc(self.R, s)))))
            s["scale"]["cost"] = float(abs(fr.step_cost(self.R, self.row, s["q"], s["v"], s["ctrl"])))
        self.seconds = time.perf_counter() - t0
        self.e64 = {b: max(dev(s["ref64"][sl], s["ref"][sl]) for s in self.states) for b, sl in self.sl.items()}

    def floor(self, s, b):
        big = float(np.max(np.abs(s["ref"][self.sl[b]])))
        return 2.0 ** -52 * s["scale"][b] / EPS / big if big > 0 else 0.0

    def bound(self, s, b):
        return max(2 * self.nv * self.e64[b], self.floor(s, b))

    def check(self, what, got):
        """got[i] against the reference record of state i, block by block; prints the batch's
        figures, then asserts every state's bound"""
        worst = {}
        for b, sl in self.sl.items():
            devs = [dev(got[i][sl], s["ref"][sl]) for i, s in enumerate(self.states)]
            worst[b] = max(0.0 if d == 0 else float("inf") if self.bound(s, b) == 0 else d / self.bound(s, b)
                           for d, s in zip(devs, self.states))
            report(what, self.name, b, self.e64[b], max(devs), min(self.bound(s, b) for s in self.states))
        for b, r in worst.items():
            assert r <= 1, (self.name, b, r)

    def arrays(self, ia, m):
        S = self.states
        n = len(S)
        st = ia.State(time=np.zeros(n), qpos=np.array([s["q"] for s in S]), qvel=np.array([s["v"] for s in S]),
                      warm=np.zeros((n, m.nv)), ctrl=np.array([s["ctrl"] for s in S]).reshape(n, m.nu))
        return st, np.array([s["qf"] for s in S]), np.array([s["xf"].ravel() for s in S])


def dev(got, ref):
    """largest deviation relative to the reference's largest magnitude; an all-zero
    reference admits only an all-zero result"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    big = np.max(np.abs(ref))
    if big == 0:
        return 0.0 if not np.any(got) else float("inf")
    return float(np.max(np.abs(got - ref)) / big)


_records = {}


def records(ia, kind, name):
    if (kind, name) not in _records:
        _records[kind, name] = Records(ia, kind, name)
    return _records[kind, name]


def product(ia, kind, name):
    return product_model(ia, name) if kind == "airborne" else contact_product(ia, name)


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", MODELS)
def test_reference_records_are_derivatives(ia, name):
    """the reference on itself.  The eps = 1e-6 longdouble blocks of the first three airborne
    states (the humanoid's take eight seconds: 150 evaluations a block set) against the Richardson
    pair (4 D(5e-4) - D(1e-3)) / 3 of the same central differences: 1e-10 of the block's largest
    entry (the pair's own error is h^4 f^(5) / 480, the record's eps^2 f''' / 6).  The cost
    columns of the scalar dofs (slide, hinge, a free joint's position, every qvel and ctrl)
    of every state against the closed form 2 w (x - t) + l: they differ by eps w, the exact
    second-order term of a forward difference of a quadratic, to 1e-3 of it.
    Measured on the CPU (three states each): pendulum 4.8e-13, hopper 3.7e-12, humanoid
    1.8e-11, chain 3.0e-12, ballarm 1.7e-12, floatarm 4.1e-12."""
    rec = records(ia, "airborne", name)
    R, nv, nu = rec.R, rec.nv, rec.nu
    worst = 0.0
    for s in rec.states[:3]:
        D1, D2 = fr.dyn_blocks(R, s, 1e-3), fr.dyn_blocks(R, s, 5e-4)
        for b, d1, d2 in zip(("dq", "dv", "du"), D1, D2):
            worst = max(worst, dev(s["ref"][rec.sl[b]], (4 * d2 - d1) / 3))
    print(f"eps = 1e-6 blocks against Richardson, {name}: {worst:.2e}")
    assert worst <= 1e-10
    (wq, tq, lq), (wv, tv, lv), (wu, tu, lu) = fr.split_cost_row(R, rec.row)
    scalar = [(R.jq[ji] + k, R.jd[ji] + k) for ji, j in enumerate(rec.C.joints)
              for k in range({"free": 3, "ball": 0}.get(j["type"], 1))]
    for s in rec.states:
        col = s["ref"][rec.sl["cost"]]
        q, v, u = R.T(s["q"]), R.T(s["v"]), R.T(s["ctrl"])
        pairs = [(col[d], 2 * wq[a] * (q[a] - tq[a]) + lq[a], wq[a]) for a, d in scalar]
        pairs += [(col[nv + i], 2 * wv[i] * (v[i] - tv[i]) + lv[i], wv[i]) for i in range(nv)]
        pairs += [(col[2 * nv + a], 2 * wu[a] * (u[a] - tu[a]) + lu[a], wu[a]) for a in range(nu)]
        for got, grad, w in pairs:
            assert abs(got - grad - EPS * w) <= 1e-3 * EPS * w, (name, s["what"])


# ------------------------------------------------------------------ the oracle
def _oracle_records(ia, ora, rec):
    m = product(ia, rec.kind, rec.name)
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(rec.cost, m.nq, m.nv, m.nu))
    out = []
    for s in rec.states:
        d = om.make_data()
        d.set_state(qpos=s["q"], qvel=s["v"], ctrl=s["ctrl"])
        d.arr("qfrc_applied")[:] = s["qf"]
        d.xfrc()[:] = s["xf"].ravel()
        out.append(ora.calc_derivatives(om, d, cost_fn="ora_cost_desc_fn", nthread=1))
    return out


def _within_time(rec):
    print(f"reference build {rec.kind} {rec.name}: {rec.seconds:.1f} s")
    assert rec.seconds <= 3 * REFERENCE_SECONDS[rec.kind, rec.name] + 2


@pytest.mark.parametrize("name", MODELS)
def test_oracle_records_airborne(ia, ora, name):
    """ora_calcMJDerivatives against the reference record on the moving airborne states.
    Measured on the CPU, E64 / deviation (the batch's smallest bound is 2 nv E64 in every block):
                         dq               dv               du               cost
      inverted_pendulum  4.5e-11/1.4e-10  2.1e-09/6.1e-10  4.3e-11/1.5e-11  4.8e-10/7.9e-10
      hopper             1.2e-08/1.3e-08  2.1e-08/3.0e-08  1.0e-10/1.2e-10  2.0e-09/2.6e-09
      humanoid           3.9e-08/6.7e-08  3.9e-09/9.9e-09  1.2e-11/4.2e-11  4.6e-09/3.2e-09
      chain              4.9e-09/9.6e-09  1.4e-08/2.1e-08  3.3e-10/4.5e-10  2.6e-09/2.1e-09
      ballarm            5.2e-09/4.3e-09  4.0e-09/6.7e-09  9.7e-11/1.4e-10  1.9e-09/1.7e-09
      floatarm           9.8e-09/8.7e-09  4.9e-09/1.6e-08  4.2e-11/7.3e-11  3.3e-09/2.5e-09
    The largest deviation / bound is the pendulum's dq, 0.8 (nv = 2 leaves the least room)."""
    rec = records(ia, "airborne", name)
    _within_time(rec)
    rec.check("oracle fd", _oracle_records(ia, ora, rec))


@pytest.mark.parametrize("name", CONTACT_MODELS)
def test_oracle_records_contact(ia, ora, name):
    """ora_calcMJDerivatives against the reference record on the contact cases (none excluded).
    Measured on the CPU, E64 / deviation:
                         dq               dv               du               cost
      hopper             7.5e-11/1.6e-10  2.5e-09/1.4e-09  1.4e-09/5.4e-10  8.1e-10/6.1e-10
      inverted_pendulum  9.2e-11/8.2e-11  5.5e-11/3.3e-11  1.1e-08/8.5e-10  2.4e-10/2.4e-10
      humanoid           7.2e-09/3.4e-08  7.0e-09/5.0e-09  1.5e-10/8.3e-11  2.9e-09/3.2e-09
      cross              1.5e-10/1.3e-10  6.4e-10/9.6e-10  4.6e-09/7.1e-09  4.1e-10/5.0e-10
      parallel           4.5e-12/4.1e-12  1.6e-10/1.2e-10  1.2e-08/6.3e-09  1.4e-10/3.0e-10
      ballarm            6.1e-10/5.4e-10  5.7e-10/4.4e-10  7.2e-10/3.5e-10  6.6e-10/7.1e-10"""
    rec = records(ia, "contact", name)
    _within_time(rec)
    rec.check("oracle fd contact", _oracle_records(ia, ora, rec))


def test_exclusion_cap(ia):
    """same_active_set, on the reference alone, leaves out at most two contact cases in
    all and at most one per model (the latter asserted where the records are built)"""
    out = [(n, s["what"]) for n in CONTACT_MODELS for s in records(ia, "contact", n).excluded]
    print(f"contact cases excluded by same_active_set: {len(out)} {out}")
    assert len(out) <= 2


def test_comparison_is_sensitive(ia):
    """host arrays only: each wrong convention, applied to the reference's own record,
    exceeds the bound of its block by a factor of at least 1e3 at some state.
    Measured, deviation / bound: dq transposed 7.3e6, two ball-dof columns swapped 1.1e7, one
    negated 2.2e7, an unclipped motor's column zero 8.0e8, the world-frame quaternion step
    1.1e7 in dq and 3.9e6 in the cost columns, xfrc_applied dropped 1.0e6."""
    hop, arm = records(ia, "airborne", "hopper"), records(ia, "airborne", "ballarm")

    def ratio(rec, b, mutate):
        """the largest deviation / bound over the states; mutate(s) gives the wrong record or None"""
        out = 0.0
        for s in rec.states:
            got = mutate(s)
            if got is not None:
                out = max(out, dev(got[rec.sl[b]], s["ref"][rec.sl[b]]) / rec.bound(s, b))
        return out

    def on_block(rec, b, shape, f):
        def mutate(s):
            got = np.array(s["ref"], np.float64)
            got[rec.sl[b]] = f(got[rec.sl[b]].reshape(shape).copy(), s).ravel()
            return got
        return mutate

    ball = [d for ji, j in enumerate(arm.C.joints) if j["type"] == "ball" for d in range(arm.R.jd[ji], arm.R.jd[ji] + 3)]
    assert len(ball) >= 3
    first = [s["what"] for s in arm.states[:2]]
    nv, nu = hop.nv, hop.nu
    lim = [(a["ctrlrange"] if a["ctrllimited"] else (-np.inf, np.inf)) for a in hop.C.act]

    def swap(M, s):
        M[:, [ball[0], ball[1]]] = M[:, [ball[1], ball[0]]]
        return M

    def negate(M, s):
        M[:, ball[2]] = -M[:, ball[2]]
        return M

    def zero_motor(M, s):
        free = [a for a in range(nu) if lim[a][0] < s["ctrl"][a] < lim[a][1]]
        M[:, free[0]] = 0
        return M

    found = {
        "dq transposed (quirk Q1 read as the record)":
            ratio(hop, "dq", on_block(hop, "dq", (nv, nv), lambda M, s: M.T)),
        "two ball-dof columns swapped": ratio(arm, "dq", on_block(arm, "dq", (arm.nv, arm.nv), swap)),
        "one ball-dof column negated": ratio(arm, "dq", on_block(arm, "dq", (arm.nv, arm.nv), negate)),
        "an unclipped motor's column zero": ratio(hop, "du", on_block(hop, "du", (nv, nu), zero_motor)),
        "world-frame quaternion step, dq": ratio(
            arm, "dq", lambda s: fr.record(arm.R, arm.row, s, EPS, frame="world") if s["what"] in first else None),
        "world-frame quaternion step, cost": ratio(
            arm, "cost", lambda s: np.concatenate([np.zeros(arm.sl["cost"].start, LD),
                                                   fr.cost_columns(arm.R, arm.row, s, EPS, frame="world")])),
        "xfrc_applied dropped from the perturbed evaluations": ratio(
            hop, "dq", lambda s: fr.record(hop.R, hop.row, s, EPS, drop_xf=True) if np.any(s["xf"]) else None),
    }
    for what, r in found.items():
        print(f"mutation: {what:55s} deviation / bound {r:.2e}")
    for what, r in found.items():
        assert r >= 1e3, what


# ------------------------------------------------------------------ the kernels
def _gpu_batch(ia, kind, name):
    rec = records(ia, kind, name)
    m = product(ia, kind, name)
    assert (m.static_id() == 0) == (name in GENERIC), m.static_id()
    st, qf, xf = rec.arrays(ia, m)
    rec.check(f"gpu fd {kind}", m.calc_derivatives(st, rec.cost, qf, xf))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_gpu_fd_batch_airborne(ia, name):
    """Model.calc_derivatives (ilqg_fd_batch) against the reference record on the airborne
    states: pendulum and hopper on their compile-time instances, humanoid, chain, ballarm and
    floatarm on the generic cooperative kernels (asserted).
    Measured on the MI355X: E64, deviation and bound of test_oracle_records_airborne to every
    printed digit, all six models and four blocks (the kernels are the oracle's bits)."""
    _gpu_batch(ia, "airborne", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONTACT_MODELS)
def test_gpu_fd_batch_contact(ia, name):
    """Model.calc_derivatives against the reference record on the contact cases; cross and
    parallel on the generic kernels too.
    Measured on the MI355X: the figures of test_oracle_records_contact to every printed digit."""
    _gpu_batch(ia, "contact", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("hopper", "1"), ("hopper", "0"), ("humanoid", "1"), ("ballarm", "1")],
                         ids=["hopper", "hopper-unfused", "humanoid", "ballarm"])
def test_gpu_solver_sweep(ia, name, fused, monkeypatch):
    """the solver's own sweep: one seed per state (airborne and contact together), each seed
    with its own qfrc_applied / xfrc_applied, N = 1, the state at both points (set_traj), then
    fd_sweep() and deriv(): both records of every seed against the reference.  The hopper
    through the fused ticket queue and (ILQG_FUSED=0) the centre and column kernels.
    Measured on the MI355X: at both points of every seed the figures of the two oracle tests to
    every printed digit (largest: humanoid airborne dq, E64 3.9e-08, deviation 6.7e-08, bound
    2.1e-06; humanoid contact dq 7.2e-09 / 3.4e-08 / 3.9e-07)."""
    if fused == "0":
        monkeypatch.setenv("ILQG_FUSED", "0")
    recs = [records(ia, kind, name) for kind in ("airborne", "contact")]
    m = product_model(ia, name)
    parts = [rec.arrays(ia, m) for rec in recs]
    st = ia.State(*(np.concatenate([getattr(p[0], f) for p in parts]) for f in ("time", "qpos", "qvel", "warm", "ctrl")))
    qf, xf = (np.concatenate([p[k] for p in parts]) for k in (1, 2))
    g = ia.ILQR(m, st, 1, recs[0].cost, qfrc_applied=qf, xfrc_applied=xf)
    g.set_traj(ia.State(*(np.repeat(getattr(st, f), 2, axis=0) for f in ("time", "qpos", "qvel", "warm", "ctrl"))))
    g.fd_sweep()
    g.synchronize()
    D = g.deriv()
    assert D.shape == (len(st.time), 2, m.D)
    at = 0
    for rec in recs:
        n = len(rec.states)
        for p in (0, 1):
            rec.check(f"gpu sweep {rec.kind} point {p}", D[at:at + n, p])
        at += n

"""Ball joints through every kernel path against the CPU oracle, bit for bit, on
the two models of tests/ball_models.py (neither is bundled: static_id() == 0, the
generic kernels; ball_model asserts it).

The device code has a ball branch in the kinematics, the motion axes, the velocity
recursion, integrate_pos, the tangent-space state difference and the quaternion
perturbation of every FD kernel; the oracle has the matching cases.  The oracle
itself is held to the independent reference on these models in
tests/test_physics_reference.py; here the kernels are held to the oracle.

States: 8 seeded ones per model, batch 8, horizon 20, every ball (and free)
quaternion a unit one far from the identity, every dof moving.  ballarm: states 0
and 1 are floor-contact poses of test_physics_reference.CONTACT_CASES, state 2 is
reached by stepping the oracle until the arm has swung into the floor (its warm
start is the solver's own); floatarm: state 2 likewise after its fall.  What the
states have to show is asserted on the oracle alone, in tests that need no GPU,
and so are the two vacuity guards: the FD record changes grossly when a ball dof's
qpos column is perturbed with a plain += eps instead of the quaternion step, and
the ball quaternions turn by more than 0.1 rad over the solver's horizon.

The cost has non-zero quadratic and linear weights on every qpos entry, quaternion
components included, so the cost columns of the ball dofs are live.
"""
import ctypes

import numpy as np
import pytest

import shift_ref as sr
from ball_models import BALL_XML, ball_model
from test_gpu_parity import (FD32_EPS, FD32_FRAC_BIG, FD32_MEDIAN, FD32_P99, _fd32_stats, _oracle_ilqr, _state_dict,
                             exact, random_states)
from test_model_compile import _fields
from test_physics_reference import CONTACT_CASES

gpu = pytest.mark.gpu
MODELS = list(BALL_XML)
B, H, P = 8, 20, 21
ALPHAS4 = [1.0, 0.5, 0.25, 0.125]
_dp = ctypes.POINTER(ctypes.c_double)


def _unit_quat(rng):
    """far from the identity, every component away from 0, as numpy rounds it"""
    axis = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.6, 2.6)
    quat = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
    return quat / np.linalg.norm(quat)


def _angle(qa, qb):
    """the rotation angle between two unit quaternions"""
    return 2 * np.arccos(min(1.0, abs(float(np.dot(qa, qb)))))


class Case:
    """one model: the product's compile, the oracle's model, the cost, the 8 states"""

    def __init__(self, ia, ora, name):
        self.ia, self.ora, self.name = ia, ora, name
        self.m = m = ball_model(ia, name)
        assert m.static_id() == 0   # the generic kernels, not a specialisation
        self.om = ora.OModel(m.blob())
        self.f = f = _fields(m.blob())
        self.dof_of_free = {int(a): int(d) for t, a, d in zip(f["jnt_type"], f["jnt_qposadr"], f["jnt_dofadr"]) if t == 0}
        self.balls = [(int(a), int(d)) for t, a, d in zip(f["jnt_type"], f["jnt_qposadr"], f["jnt_dofadr"]) if t == 1]
        self.quats = sorted([a for a, _ in self.balls] + [int(a) + 3 for t, a in zip(f["jnt_type"], f["jnt_qposadr"])
                                                           if t == 0])
        self.free = [int(a) for t, a in zip(f["jnt_type"], f["jnt_qposadr"]) if t == 0]
        w = 0.5 + 0.25 * np.arange(m.nq)
        self.cost = ia.Cost(wq=w, tq=0.1 * np.cos(np.arange(m.nq)), lq=0.2 * np.sin(1 + np.arange(m.nq)) + 0.3,
                            wv=[0.05] * m.nv, wu=[0.01] * m.nu)
        assert all(np.all(np.asarray(getattr(self.cost, k))[a:a + 4] != 0) for k in ("wq", "lq") for a in self.quats)
        self.install()
        self.st = self._states()
        self.ncon, self.nefc = [], []
        for i in range(B):
            d = self.data(i)
            d.forward()
            self.ncon.append(d.ncon())
            self.nefc.append(d.nefc())
        self.free_states = [i for i in range(3, B) if self.nefc[i] == 0]   # no contact, no limit row
        # the solver's two seeds: one in floor contact, one unconstrained
        self.seeds = (0 if name == "ballarm" else 2, self.free_states[0])

    def install(self):
        """the oracle's descriptor cost is one global: install this model's before the oracle evaluates it"""
        L = self.om.lib.L
        L.ora_set_cost_desc(self.ora.CostDesc.from_cost(self.cost, self.m.nq, self.m.nv, self.m.nu))
        L.ora_set_nthread(1)

    def _states(self):
        ia, m = self.ia, self.m
        rng = np.random.default_rng(611 + MODELS.index(self.name))
        st = random_states(m, B, rng, 0.3)
        st.qvel = rng.normal(0, 3.0, st.qvel.shape)
        for i in range(B):
            for a in self.free:
                st.qpos[i, a:a + 3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.9, 1.3)]
            for a in self.quats:
                st.qpos[i, a:a + 4] = _unit_quat(rng)
        if self.name == "ballarm":
            for i, case in ((0, 0), (1, 2)):
                st.qpos[i] = CONTACT_CASES["ballarm"][case][1]
        # state 2: stepped into the floor on the oracle, then three steps more
        d = self.om.make_data()
        d.set_state(**_state_dict(st, 2))
        for _ in range(1500):
            d.step()
            if d.ncon():
                break
        d.step(3)
        s = d.state()
        st.time[2], st.qpos[2], st.qvel[2], st.warm[2] = s["time"], s["qpos"], s["qvel"], s["warm"]
        return st

    def data(self, i):
        d = self.om.make_data()
        d.set_state(**_state_dict(self.st, i))
        return d

    def refs(self, layout):
        """the oracle's two line-search iterations from the solver's two seeds (computed once)"""
        if layout not in _refs.setdefault(self.name, {}):
            self.install()
            out = []
            with self.ora.layout(layout):
                for s in self.seeds:
                    d = self.data(s)
                    il = self.ora.OILQR(self.om, d, H, cost_fn="ora_cost_desc_fn")
                    il.set_dinit(d)
                    for _ in range(2):
                        oc, osel = il.iterate_ls(ALPHAS4, "min_cost")
                    out.append(dict(traj=il.traj(), arr=il.arrays(), costs=oc, sel=osel))
            _refs[self.name][layout] = out
        return _refs[self.name][layout]

    def dmain(self):
        idx = list(self.seeds)
        st = self.st
        return self.ia.State(st.time[idx], st.qpos[idx], st.qvel[idx], st.warm[idx], st.ctrl[idx])


_cases, _refs = {}, {}


@pytest.fixture
def case(request, ia, ora):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(ia, ora, name)
    _cases[name].install()
    return _cases[name]


both = pytest.mark.parametrize("case", MODELS, indirect=True)
ballarm = pytest.mark.parametrize("case", ["ballarm"], indirect=True)


# ------------------------------------------------------------------ what the states show (oracle alone)
@both
def test_states(case):
    """unit quaternions at least 0.5 rad from the identity with no component near 0, every
    dof moving; floor contact where the docstring says so (ncon > 0 on the oracle)"""
    st = case.st
    for i in range(B):
        for a in case.quats:
            q = st.qpos[i, a:a + 4]
            assert abs(np.linalg.norm(q) - 1) <= 1e-15
            if i != 2 and not (case.name == "ballarm" and i < 2):   # drawn here, not found by a search or a fall
                assert _angle(q, np.array([1.0, 0, 0, 0])) >= 0.5 and np.all(np.abs(q[1:]) > 0.05)
        assert np.all(st.qvel[i] != 0)
    ncon = case.ncon
    print(case.name, "ncon per state:", ncon, "nefc:", case.nefc, "seeds:", case.seeds)
    assert ncon[2] > 0 and np.any(st.warm[2] != 0)
    if case.name == "ballarm":
        assert ncon[0] == 1 and ncon[1] == 3
    assert ncon[case.seeds[0]] > 0 and case.nefc[case.seeds[1]] == 0 and len(case.free_states) >= 2


@both
def test_quaternion_branch_matters(case, ora):
    """vacuity guard: the qacc block of a ball dof's qpos column, formed with a plain
    += eps on the qpos entry the slide / hinge branch would address instead of the
    quaternion step, differs from the record's column by more than 1e-3 of its size at
    every state, while the same central difference formed here with the oracle's
    mju_quatIntegrate reproduces the record's column to 1e-6 (the record's own solver
    settings differ from mj_forward's in the iteration cap only)"""
    m, om, L = case.m, case.om, case.om.lib.L
    L.mju_quatIntegrate.argtypes = [_dp, _dp, ctypes.c_double]
    L.mju_quatIntegrate.restype = None
    nv, eps = m.nv, 1e-6

    def qacc(i, q):
        d = case.data(i)
        d.arr("qpos")[:] = q
        d.forward()
        return d.arr("qacc").copy()

    for i in case.free_states[:2]:   # no constraint row: no activation flips in the difference
        rec = ora.calc_derivatives(om, case.data(i), cost_fn="ora_cost_desc_fn", nthread=1)
        J = rec[:nv * nv].reshape(nv, nv)   # row-major by output: J[j, dof]
        for qa, da in case.balls:
            for k in range(3):
                cols = {}
                for kind in ("quat", "plain"):
                    side = []
                    for sg in (1.0, -1.0):
                        q = np.array(case.st.qpos[i])
                        if kind == "quat":
                            quat, vel = np.ascontiguousarray(q[qa:qa + 4]), np.zeros(3)
                            vel[k] = sg * eps
                            L.mju_quatIntegrate(quat.ctypes.data_as(_dp), vel.ctypes.data_as(_dp), 1.0)
                            q[qa:qa + 4] = quat
                        else:
                            q[qa + k] += sg * eps
                        side.append(qacc(i, q))
                    cols[kind] = (side[0] - side[1]) / (2 * eps)
                scale = np.max(np.abs(J[:, da + k]))
                assert np.max(np.abs(cols["quat"] - J[:, da + k])) <= 1e-6 * scale
                assert np.max(np.abs(cols["plain"] - J[:, da + k])) > 1e-3 * scale


@both
@pytest.mark.parametrize("layout", ["reference", "corrected"])
def test_trajectory_quaternions_move(case, layout):
    """vacuity guard: over the horizon of the oracle's second iteration every ball
    quaternion of every seed turns by more than 0.1 rad"""
    for ref in case.refs(layout):
        q = ref["traj"]["qpos"]
        for a, _ in case.balls:
            assert _angle(q[0, a:a + 4], q[H, a:a + 4]) > 0.1
        assert np.all(np.isfinite(ref["arr"]["K"]))
    # gains at every step in the unconstrained seed (the seed in contact may drive a motor past its
    # ctrlrange, where the clipped control's column of B, and with it K, is zero)
    assert np.all(np.any(case.refs(layout)[1]["arr"]["K"][1:] != 0, axis=1))


# ------------------------------------------------------------------ forward, step, FD batches
@gpu
@both
def test_forward_batch(case):
    qacc = case.m.forward(case.st.copy())
    for i in range(B):
        d = case.data(i)
        d.forward()
        exact(qacc[i], d.arr("qacc"), f"{case.name} qacc[{i}]")


@gpu
@both
@pytest.mark.parametrize("nstep", [1, 10])
def test_step_batch(case, nstep):
    st = case.st.copy()
    case.m.step(st, nstep)
    qacc = case.m.forward(st.copy())
    for i in range(B):
        d = case.data(i)
        d.step(nstep)
        s = d.state()
        for f in ("time", "qpos", "qvel", "warm"):
            exact(getattr(st, f)[i], s[f], f"{case.name} state {i} {f} after {nstep}")
        d.forward()
        exact(qacc[i], d.arr("qacc"), f"{case.name} state {i} qacc after {nstep}")


@gpu
@both
@pytest.mark.parametrize("fused", ["1", "0"])
def test_fd_batch(case, ora, fused, monkeypatch):
    """ilqg_fd_batch, the whole record of all 8 states: through the one-point launch of
    the fused kernel, and (ILQG_FUSED=0) through the centre and column kernels"""
    monkeypatch.setenv("ILQG_FUSED", fused)
    der = case.m.calc_derivatives(case.st.copy(), case.cost)
    for i in range(B):
        exact(der[i], ora.calc_derivatives(case.om, case.data(i), cost_fn="ora_cost_desc_fn", nthread=1),
              f"{case.name} record {i}")


# ------------------------------------------------------------------ the solver
def _solver(case, layout):
    g = case.ia.ILQR(case.m, case.dmain(), H, case.cost, alphas=ALPHAS4, select="min_cost")
    g.set_layout(layout)
    return g


def _compare(g, refs, what):
    g.synchronize()
    gt, (K, k), (V, v), D = g.traj(), g.gains(), g.value(), g.deriv()
    costs, sel = g.costs()
    for s, ref in enumerate(refs):
        ot, oa = ref["traj"], ref["arr"]
        for f in ("time", "qpos", "qvel", "warm", "ctrl"):
            exact(getattr(gt, f)[s * P:(s + 1) * P].reshape(ot[f].shape), ot[f], f"{what} seed {s} traj.{f}")
        exact(D[s], oa["deriv"], f"{what} seed {s} records")
        for n, a in (("K", K), ("k", k), ("V", V), ("v", v)):
            exact(a[s], oa[n], f"{what} seed {s} {n}")
        exact(costs[s], ref["costs"], f"{what} seed {s} candidate costs")
        assert int(sel[s]) == ref["sel"], (what, s, int(sel[s]), ref["sel"])


@gpu
@both
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("layout", ["reference", "corrected"])
def test_iterate(case, layout, fused, monkeypatch):
    """ILQR(m, 2 seeds, 20, cost) with 4 alphas, two iterate() calls, in both layouts,
    with the fused sweep and (ILQG_FUSED=0) the two-kernel sweep: every trajectory field
    (the rollout's tangent-space state difference, nx = 2 nv != nq + nv), the FD records,
    K, k, V, v, the candidate costs and the selection, per seed; then the sweep alone"""
    monkeypatch.setenv("ILQG_FUSED", fused)
    refs = case.refs(layout)
    g = _solver(case, layout)
    g.iterate()
    g.iterate()
    _compare(g, refs, f"{case.name} {layout} fused={fused}")
    D = g.deriv().copy()
    g.fd_sweep()
    g.synchronize()
    exact(g.deriv(), D, "fd_sweep alone against iterate's records")


@gpu
@both
def test_standard_recursion_is_refused(case):
    """the standard recursion's cost Hessian is diagonal in qpos, which a quaternion term
    is not in the tangent space: with nq != nv it is refused (ILQG_ERR_UNSUPPORTED), not run
    with a wrong Hessian, and the solver goes on in the reference recursion"""
    g = _solver(case, "corrected")
    with pytest.raises(case.ia.IlqgError, match=r"code 4\).*nq != nv"):
        g.set_recursion("standard")
    g.iterate()
    g.iterate()
    _compare(g, case.refs("corrected"), f"{case.name} after the refusal")


@gpu
@ballarm
def test_shift_horizon(case, ora):
    """one shift_horizon(1, hold) tick after two iterations against tests/shift_ref.py driven
    by the oracle's step and sweep: the moved columns are nq = 10 and nv = 8 wide"""
    g = _solver(case, "reference")
    g.iterate()
    g.iterate()
    before = sr.solver_arrays(g)
    g.shift_horizon(1)
    after = sr.solver_arrays(g)
    want = sr.shift(before, 1, sr.oracle_step(case.om, None, None), sr.oracle_sweep(ora, case.om, None, None))
    for f in sr.ARRAYS:
        assert sr.bits_equal(after[f], want[f]), f
    assert np.any(after["qpos"][:, 0] != before["qpos"][:, 0])


# ------------------------------------------------------------------ the fp32 sweep
FP32_SCALE = 0.01   # of the batch's velocities and controls
FP32_QACC = 0.5     # rad/s^2 (m/s^2): the joints' accelerations at an fp32 state


def _joint_qacc(case, s):
    """the oracle's qacc at a state, a free joint's translation left out (free fall is its rest)"""
    d = case.om.make_data()
    d.set_state(**s)
    d.forward()
    keep = np.ones(case.m.nv, bool)
    for a in case.free:
        keep[case.dof_of_free[a]:case.dof_of_free[a] + 3] = False
    return d.arr("qacc")[keep].copy(), d.nefc()


def _move(case, q, p):
    """q (+) p: the tangent increment p (nv) applied with the oracle's quaternion step"""
    L, f, q = case.om.lib.L, case.f, np.array(q)
    L.mju_quatIntegrate.argtypes = [_dp, _dp, ctypes.c_double]
    L.mju_quatIntegrate.restype = None
    for j, (t, qa, da) in enumerate(zip(f["jnt_type"], f["jnt_qposadr"], f["jnt_dofadr"])):
        if t >= 2:
            q[qa] += p[da]
            continue
        if t == 0:
            q[qa:qa + 3] += p[da:da + 3]
            qa, da = qa + 3, da + 3
        quat, vel = np.ascontiguousarray(q[qa:qa + 4]), np.ascontiguousarray(p[da:da + 3])
        L.mju_quatIntegrate(quat.ctypes.data_as(_dp), vel.ctypes.data_as(_dp), 1.0)
        q[qa:qa + 4] = quat
    return q


def _airborne(case, scale=FP32_SCALE):
    """two seeded airborne states close to an equilibrium of the joints, found on the oracle
    alone: from a seeded pose (every quaternion far from the identity) a Gauss-Newton
    iteration on the joints' accelerations, the batch's velocities and controls scaled by
    `scale`; kept if the accelerations end within FP32_QACC, every quaternion is still at
    least 0.5 rad from the identity, and the whole passive horizon has no constraint row
    (no activation can flip between the fp32 and the fp64 run)"""
    rng = np.random.default_rng(977 + MODELS.index(case.name))
    nv, found = case.m.nv, []
    for _ in range(400):
        s = _state_dict(case.st, int(rng.integers(B)))
        s["qpos"], s["warm"] = np.array(s["qpos"]), np.zeros(nv)
        s["qvel"], s["ctrl"] = scale * np.array(s["qvel"]), scale * np.array(s["ctrl"])
        for a in case.free:   # within 1.5 m of the origin, where fp32 resolves a position to 1.2e-7 m
            s["qpos"][a:a + 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.2 + rng.uniform(0, 0.3)]
        for a in case.quats:
            s["qpos"][a:a + 4] = _unit_quat(rng)
        for _ in range(30):
            r, _ = _joint_qacc(case, s)
            if np.abs(r).max() <= 0.1 * FP32_QACC:
                break
            J = np.array([(_joint_qacc(case, dict(s, qpos=_move(case, s["qpos"], 1e-6 * e)))[0] - r) / 1e-6
                          for e in np.eye(nv)]).T
            dp = np.linalg.lstsq(J, -r, rcond=1e-6)[0]   # a turn about the vertical changes nothing
            s["qpos"] = _move(case, s["qpos"], dp * min(1.0, 0.5 / max(np.linalg.norm(dp), 1e-300)))
        r, _ = _joint_qacc(case, s)
        if np.abs(r).max() > FP32_QACC:
            continue
        if any(_angle(s["qpos"][a:a + 4], np.array([1.0, 0, 0, 0])) < 0.5 for a in case.quats):
            continue
        d = case.om.make_data()
        d.set_state(**s)
        clear = True
        for _ in range(H + 2):
            d.forward()
            clear = clear and d.nefc() == 0
            d.step()
        if clear:
            found.append(s)
        if len(found) == 2:
            return found
    raise AssertionError("no airborne states found")


def _fp32_records(case, ora, s):
    """(the fp32 sweep's records over the horizon from state s, the fp64 oracle's at the same step)"""
    ia = case.ia
    case.install()
    case.om.lib.L.ora_set_fd_eps(FD32_EPS)
    try:
        il = _oracle_ilqr(ora, case.om, s, H, "ora_cost_desc_fn", 1)
    finally:
        case.om.lib.L.ora_set_fd_eps(1e-6)
    st = ia.State(np.array([s["time"]]), s["qpos"][None], s["qvel"][None], s["warm"][None], s["ctrl"][None])
    g = ia.ILQR(case.m, st, H, case.cost)
    g.set_fd_precision("f32")
    g.iterate()
    g.synchronize()
    exact(g.traj().qpos, il.traj()["qpos"], "the rollout is the fp64 one")
    return g.deriv()[0], il.arrays()["deriv"]


def _ball_column_medians(case, d, dref):
    """per ball dof: the median of e over its qpos column (its qacc block and its cost entry, all points)"""
    nv, nu = case.m.nv, case.m.nu
    e = np.abs(d - dref) / (1 + np.abs(dref))
    out = {}
    for _, da in case.balls:
        for k in range(3):
            i = da + k
            col = np.concatenate([e[:, i:nv * nv:nv], e[:, 2 * nv * nv + nv * nu + i][:, None]], axis=1)
            out[i] = (float(np.median(col)), float(col.max()))
    return out


_fp32 = {}


def _fp32_runs(case, ora):
    """[(fp32 records, fp64 oracle records)] of the model's two airborne states, computed once"""
    if case.name not in _fp32:
        out = []
        for s in _airborne(case):
            assert np.abs(_joint_qacc(case, s)[0]).max() <= FP32_QACC
            assert np.all(s["qvel"] != 0) and np.all(s["ctrl"] != 0)
            out.append(_fp32_records(case, ora, s))
        _fp32[case.name] = out
    return _fp32[case.name]


@gpu
@both
def test_fp32_ball_columns(case, ora):
    """set_fd_precision("f32") on airborne states against the fp64 oracle at the fp32 step
    (FD32_EPS): the median of e = |d - d_ref| / (1 + |d_ref|) over each single ball-dof qpos
    column (its qacc block and its cost entry, all 21 points) is within FD32_P99, and so are
    the 99th percentile over every entry and FD32_FRAC_BIG.  A wrong quaternion branch makes a
    whole column wrong by its own size, e of order 1.
    Measured on the MI355X (bound 0.085): column medians 5.5e-5 .. 4.6e-4 (ballarm), 6.6e-5 ..
    8.8e-4 (floatarm), column maxima at most 1.9e-2; p99 over every entry 2.4e-3 .. 1.0e-2;
    no entry above 0.1."""
    for n, (d, dref) in enumerate(_fp32_runs(case, ora)):
        assert np.all(np.isfinite(d))
        e = np.abs(d - dref) / (1 + np.abs(dref))
        for i, (med, big) in _ball_column_medians(case, d, dref).items():
            print(f"{case.name} state {n} ball dof {i}: median e of its qpos column {med:.2e}, max {big:.2e}")
            assert med <= FD32_P99, (i, med)
        assert float(np.quantile(e, 0.99)) <= FD32_P99 and float(np.mean(e > 0.1)) <= FD32_FRAC_BIG


@gpu
@both
def test_fp32_sweep_airborne(case, ora):
    """the same records under _fd32_stats, the project's three bounds unchanged: FD32_MEDIAN
    5e-4, FD32_P99 0.085, FD32_FRAC_BIG 5.5e-3.

    Which states: e is the fp32 rounding of the pipeline behind qacc, a few 2^-24 of the
    largest term it sums, times 1 / (2 eps) = 500, so it grows with the forces that act in
    the state.  The three bounds were measured where those nearly cancel: the humanoid
    standing at rest, the hopper settled on the floor.  An arm that swings under gravity and
    its motors accelerates at 20 to 130 rad/s^2 (links of 0.01 kg m^2), and there the median
    is what the format gives, not what the bound was made for.  Measured on the MI355X on
    ballarm, airborne, no constraint row, same horizon:
      the batch's velocities and controls      |qacc| <= 88    median 8.5e-4 .. 9.2e-4
      both scaled by 0.1                       |qacc| <= 20    median 7.6e-4 .. 8.2e-4
      at rest, no control, gravity alone       |qacc| <= 20    median 7.7e-4 .. 8.1e-4
      near an equilibrium (the states here)    |qacc| <= 0.33  median 4.4e-5 .. 6.6e-5
    (rounding the oracle's qacc to fp32 and nothing else: 2.4e-5 .. 3.8e-5 at |qacc| <= 20.)
    So the states here are airborne poses close to an equilibrium of the joints, found on the
    oracle alone (_airborne): every joint acceleration within FP32_QACC = 0.5 rad/s^2, every
    quaternion at least 0.5 rad from the identity, slowly moving, lightly driven, and a free
    body within 1.5 m of the origin, where fp32 resolves its position to 1.2e-7 m.  A free
    body still carries its weight through the pipeline (qfrc_bias 88 N against joint inertias
    of 0.02 kg m^2), which is why floatarm stays closer to the bound than ballarm.
    Measured on the MI355X, per state:
                 median     p99      e > 0.1   max
      ballarm    4.4e-5   2.9e-3    0        1.8e-2
                 6.6e-5   2.4e-3    0        1.2e-2
      floatarm   4.6e-4   9.6e-3    0        2.2e-2
                 3.6e-4   1.0e-2    0        1.9e-2"""
    for n, (d, dref) in enumerate(_fp32_runs(case, ora)):
        stats = _fd32_stats(f"{case.name} airborne state {n} H={H}", d, dref)
        assert stats["median"] <= FD32_MEDIAN and stats["p99"] <= FD32_P99 and stats["frac_big"] <= FD32_FRAC_BIG

"""The physics against an independent reference (tests/rigid_ref.py: np.longdouble,
world-frame product of exponentials, dense Jacobian sums, no recursion shared
with oracle/mjsub.c or the device code), away from rest: velocities (Coriolis,
gyroscopic terms), a rotated free joint, springs, dampers, clipped motors,
qfrc_applied and xfrc_applied.  The oracle is held to it without a GPU, the
kernels with one.

Tolerance of every comparison: E64 is the largest deviation of the reference
run in float64 from the reference in longdouble on the same states, relative to
the array's largest magnitude; the bound is 2 nv E64 with a floor of 1e-14 (both
solvers are backward stable, errors scale with cond(M) eps, and the sparse LDL
and the dense elimination differ in order, worth about a factor nv).
"""
import io

import numpy as np
import pytest

import mjcf_indep as mi
import rigid_ref as rr
from ball_models import BALL_XML, ball_file, ball_model
from conftest import model_path
from test_riccati_cases import chain_xml

LD = np.longdouble
MODELS = ["inverted_pendulum", "hopper", "humanoid", "chain", "ballarm", "floatarm"]
NSTATE = 8


def compiled(name):
    if name in BALL_XML:
        return mi.compile_mjcf(ball_file(name))
    return mi.compile_mjcf(io.StringIO(chain_xml())) if name == "chain" else mi.compile_mjcf(model_path(name))


def product_model(ia, name):
    if name in BALL_XML:
        return ball_model(ia, name)
    return ia.Model.from_string(chain_xml()) if name == "chain" else ia.Model.load(model_path(name))


def _far_quat(rng):
    """a unit quaternion far from the identity, every component away from 0"""
    axis = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.6, 2.6)
    quat = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
    return quat / np.linalg.norm(quat)


def rel(a, b):
    """largest deviation of a from b relative to b's largest magnitude"""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


# ------------------------------------------------------------------ states
def _candidate(name, C, rng, k):
    """one seeded state: inside every joint range, airborne, moving"""
    q = np.array(C.qpos0, float)
    v = np.zeros(C.nv)
    aq = ad = 0
    for j in C.joints:
        if j["type"] == "free":
            q[aq:aq + 3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), 3.0 + rng.uniform(0, 1)]
            axis = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
            axis /= np.linalg.norm(axis)
            ang = rng.uniform(0.6, 2.6)
            quat = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
            q[aq + 3:aq + 7] = quat / np.linalg.norm(quat)
            v[ad:ad + 3] = rng.normal(0, 1.0, 3)
            v[ad + 3:ad + 6] = rng.normal(0, 4.0, 3)
            aq, ad = aq + 7, ad + 6
            continue
        if j["type"] == "ball":
            q[aq:aq + 4] = _far_quat(rng)
            v[ad:ad + 3] = rng.normal(0, 3.0, 3)
            aq, ad = aq + 4, ad + 3
            continue
        if j["limited"]:
            lo, hi = j["range"]
            w = 0.3 * (hi - lo)
            q[aq] = rng.uniform(lo + w, hi - w)
        elif name == "hopper" and j["name"] == "rootz":
            q[aq] = 2.5 + rng.uniform(0, 1)
        else:
            q[aq] = rng.uniform(-1.2, 1.2)
        v[ad] = rng.normal(0, 3.0 if name != "humanoid" else 1.5)
        aq, ad = aq + 1, ad + 1
    nu = len(C.act)
    ctrl = rng.uniform(-0.1, 0.1, nu)
    if name == "humanoid":
        ctrl *= 0.3
    limited = [i for i, a in enumerate(C.act) if a["ctrllimited"]]
    if limited and k % 2 == 0:  # one motor driven past its ctrlrange
        i = limited[int(rng.integers(len(limited) if name != "humanoid" else 3))]
        ctrl[i] = C.act[i]["ctrlrange"][1] * 1.5 * rng.choice([-1.0, 1.0])
    qf = rng.normal(0, 0.5, C.nv) if k % 2 == 1 else np.zeros(C.nv)
    xf = np.zeros((C.nbody, 6))
    if k >= NSTATE // 2:  # a leaf (force and torque) and one more body
        leaves = [b for b in range(1, C.nbody) if b not in [x["parent"] for x in C.bodies[1:]]]
        leaf = leaves[int(rng.integers(len(leaves)))]
        other = [b for b in range(1, C.nbody) if b != leaf]
        xf[leaf] = np.concatenate([rng.normal(0, 3.0, 3), rng.normal(0, 0.2, 3)])
        xf[other[int(rng.integers(len(other)))], :3] = rng.normal(0, 5.0, 3)
    return dict(q=q, v=v, ctrl=ctrl, qf=qf, xf=xf)


class Batch:
    """the states of one model and the reference's results on them, computed once"""

    def __init__(self, name):
        self.name = name
        self.C = C = compiled(name)
        self.R, self.R64 = rr.Ref(C, LD), rr.Ref(C, np.float64)
        rng = np.random.default_rng(20240 + MODELS.index(name))
        self.states = []
        tries = 0
        while len(self.states) < NSTATE:
            tries += 1
            assert tries < 200, "state search exhausted"
            s = _candidate(name, C, rng, len(self.states))
            try:
                self._check(s)
                s["ref"] = self._run(self.R, s)
            except AssertionError:
                continue
            s["ref64"] = self._run(self.R64, s)
            self.states.append(s)
        # batch-wide conditions, on the reference alone (the pendulum's and the chain's
        # motors are not ctrllimited: nothing there can be clipped)
        lim = [(i, a) for i, a in enumerate(C.act) if a["ctrllimited"]]
        if lim:
            clipped = [abs(s["ctrl"][i]) > a["ctrlrange"][1] for s in self.states for i, a in lim]
            assert any(clipped) and not all(clipped)
        assert sum(np.any(s["qf"] != 0) for s in self.states) == NSTATE // 2
        assert sum(np.count_nonzero(np.any(s["xf"] != 0, axis=1)) == 2 for s in self.states) == NSTATE // 2

    def _check(self, s):
        """the conditions a state must meet, by the reference's own geometry"""
        R, C = self.R, self.C
        clear = R.limit_clearance(s["q"])
        assert clear is None or clear >= 0.05
        cons, sep = R.contacts(s["q"])
        assert not cons and (sep is None or sep > 0)
        K = R.kin(s["q"])
        c, c0 = R.bias(K, s["v"]), R.bias(K, np.zeros(C.nv))
        assert np.sqrt((c - c0) @ (c - c0)) >= 0.1 * np.sqrt(c @ c), "velocity terms too small"
        aq = 0
        for j in C.joints:
            if j["type"] == "free":
                quat = s["q"][aq + 3:aq + 7]
                assert abs(np.linalg.norm(quat) - 1) <= 2.3e-16
                assert 2 * np.arccos(abs(quat[0])) >= 0.5 and np.all(np.abs(quat[1:]) > 0.05)
            if j["type"] == "ball":
                quat = s["q"][aq:aq + 4]
                assert abs(np.linalg.norm(quat) - 1) <= 2.3e-16
                assert 2 * np.arccos(abs(quat[0])) >= 0.5 and np.all(np.abs(quat[1:]) > 0.05)
            aq += {"free": 7, "ball": 4}.get(j["type"], 1)

    @staticmethod
    def _run(R, s):
        f = R.forward(s["q"], s["v"], s["ctrl"], s["qf"], s["xf"])
        q1, v1 = R.step(s["q"], s["v"], s["ctrl"], s["qf"], s["xf"], 1)
        q10, v10 = R.step(q1, v1, s["ctrl"], s["qf"], s["xf"], 9)   # asserts: no constraint in ten steps
        return dict(xpos=f.xpos, qM=f.M, qfrc_bias=f.bias, qacc_smooth=f.qacc_smooth, qacc=f.qacc_smooth,
                    q1=q1, v1=v1, q10=q10, v10=v10)

    def e64(self, key):
        return max(rel(s["ref64"][key], s["ref"][key]) for s in self.states)

    def tol(self, key):
        return max(2 * self.C.nv * self.e64(key), 1e-14)

    def arrays(self):
        S = self.states
        return (np.array([s["q"] for s in S]), np.array([s["v"] for s in S]), np.array([s["ctrl"] for s in S]),
                np.array([s["qf"] for s in S]), np.array([s["xf"].ravel() for s in S]))


_batches = {}


def batch(name):
    if name not in _batches:
        _batches[name] = Batch(name)
    return _batches[name]


def report(what, name, key, e64, dev, tol):
    print(f"{what} {name:18s} {key:12s} E64 {e64:.2e}  deviation {dev:.2e}  bound {tol:.2e}")


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", MODELS)
def test_jacobian_rate_against_richardson(name):
    """closed-form Jp_dot v and Jr_dot v at every body COM against Richardson-extrapolated
    central differences of J(q (+) t v) v, steps 1e-3 and 5e-4, in longdouble: 1e-10 relative.
    The extrapolation's own error is h^4 f^(5) / 480, which grows with the fifth power of
    the velocity (nine chained hinges at 3 rad/s each reach 3e-10), so the batch's
    velocities are scaled by a quarter here; the closed form is exact at any speed.
    Measured: pendulum 1.7e-15, hopper 2.1e-13, humanoid 2.1e-13, chain 1.1e-12
    (3e-10 for the chain at full speed, all of it the extrapolation's), ballarm 2.5e-13,
    floatarm 1.8e-13 (ball joints: the rate of the body axes under the ball's own rotation)."""
    B = batch(name)
    R = B.R
    worst = 0.0
    for s in B.states[:3]:
        q, v = LD(1) * s["q"], LD(0.25) * s["v"]
        K = R.kin(q)
        rates = R.axis_rates(K, v)

        def Jv(t):
            Kt = R.kin(R.integrate_pos(q, v, LD(t)))
            return np.array([np.concatenate([J @ v for J in R.jac(Kt, b, Kt.com[b])]) for b in range(1, R.nb)])

        def D(h):
            return (Jv(h) - Jv(-h)) / (2 * LD(h))

        fd = (4 * D(5e-4) - D(1e-3)) / 3
        cf = np.array([np.concatenate([Jd @ v for Jd in R.jac_dot(K, rates, b, K.com[b], R.jac(K, b, K.com[b])[0] @ v)])
                       for b in range(1, R.nb)])
        worst = max(worst, rel(cf, fd))
    print(f"Jdot v against Richardson, {name}: {worst:.2e}")
    assert worst <= 1e-10


def test_newtons_second_law_humanoid():
    """airborne humanoid with the reference's qacc: sum m_b a_b = (sum m_b) g + applied
    forces, and the rate of angular momentum about the origin equals the applied moment.
    Armature, springs, dampers and motors are internal and cancel; qfrc_applied on the
    free joint is a force at the root body's origin and a body-frame torque.  1e-14 of
    the largest term (longdouble).  Measured over the eight states: at most 5.6e-18 linear,
    1.9e-17 angular."""
    B = batch("humanoid")
    R, C = B.R, B.C
    assert all(a == 0 for a in R.armature[:6])
    for s in B.states:
        f = R.forward(s["q"], s["v"], s["ctrl"], s["qf"], s["xf"])
        K, v, a = f.K, f.v, f.qacc_smooth
        rates = R.axis_rates(K, v)
        lin, ang, terms = np.zeros(3, LD), np.zeros(3, LD), [LD(0)]
        F, Tq = np.zeros(3, LD), np.zeros(3, LD)
        xf = np.asarray(s["xf"], LD)
        for b in range(1, R.nb):
            Jp, Jr = R.jac(K, b, K.com[b])
            Jpd, Jrd = R.jac_dot(K, rates, b, K.com[b], Jp @ v)
            acc, alpha, w = Jp @ a + Jpd @ v, Jr @ a + Jrd @ v, Jr @ v
            lin += R.mass[b] * acc
            ang += rr.cross(K.com[b], R.mass[b] * acc) + K.I[b] @ alpha + rr.cross(w, K.I[b] @ w)
            fb = R.mass[b] * R.grav + xf[b, :3]
            F += fb
            Tq += rr.cross(K.com[b], fb) + xf[b, 3:]
            terms += [np.max(np.abs(R.mass[b] * acc)), np.max(np.abs(rr.cross(K.com[b], fb)))]
        qf = np.asarray(s["qf"], LD)
        root = np.asarray(s["q"][:3], LD)
        F += qf[:3]
        Tq += rr.cross(root, qf[:3]) + mi.qmat(np.asarray(s["q"][3:7], LD)) @ qf[3:6]
        big = max(terms)
        dl, da = float(np.max(np.abs(lin - F)) / big), float(np.max(np.abs(ang - Tq)) / big)
        print(f"Newton II humanoid: linear {dl:.2e} angular {da:.2e}")
        assert dl <= 1e-14 and da <= 1e-14


def test_capsule_enumeration_against_grid():
    """segment-segment closest points by enumeration against a 401 x 401 grid over
    the two parameters: the grid's minimum is never below the enumeration's, and not
    above it by more than the grid's resolution (half a cell in each parameter moves a
    point by at most |a|/400).  Every one of the nine regions wins in some seeded case."""
    rng = np.random.default_rng(7)
    g = np.linspace(-1, 1, 401).astype(LD)
    seen = set()
    for case in range(60):
        c1, c2 = (rng.normal(0, 0.6, 3).astype(LD) for _ in range(2))
        a1, a2 = (rng.normal(0, 1, 3) for _ in range(2))
        a1, a2 = (LD(1) * a / np.linalg.norm(a) * rng.uniform(0.2, 0.8) for a in (a1, a2))
        cosang = abs(float(a1 @ a2)) / float(np.sqrt((a1 @ a1) * (a2 @ a2)))
        if np.arccos(min(cosang, 1.0)) < 0.1:
            continue
        s, t, region = rr.segment_segment(c1, a1, c2, a2)
        kind, _, sign = region.partition("_")
        assert (abs(s) == 1) == (kind == "corner" or region.startswith("edge_s"))
        assert (abs(t) == 1) == (kind == "corner" or region.startswith("edge_t"))
        r = c1 + s * a1 - (c2 + t * a2)
        dist = np.sqrt(r @ r)
        P1 = c1[None, :] + g[:, None] * a1[None, :]
        P2 = c2[None, :] + g[:, None] * a2[None, :]
        dd = P1[:, None, :] - P2[None, :, :]
        grid = np.sqrt(np.min(np.sum(dd * dd, axis=2)))
        res = (np.sqrt(a1 @ a1) + np.sqrt(a2 @ a2)) / 400
        assert dist <= grid * (1 + LD(1e-15)) and grid - dist <= res, (case, region, float(dist), float(grid))
        seen.add(region)
    assert len(seen) == 9, sorted(seen)


# ------------------------------------------------------------------ smooth dynamics: the oracle
def _oracle_forward(om, s, extra=()):
    d = om.make_data()
    d.set_state(qpos=s["q"], qvel=s["v"], ctrl=s["ctrl"])
    d.arr("qfrc_applied")[:] = s["qf"]
    d.xfrc()[:] = s["xf"].ravel()
    d.forward()
    return d


def _oracle_array(om, d, key):
    L = om.lib.L
    if key == "xpos":
        return np.ctypeslib.as_array(L.ora_d_field(d.d, 12), shape=(om.nbody, 3)).copy()
    if key == "qM":
        return np.ctypeslib.as_array(L.ora_d_field(d.d, 9), shape=(om.nv, om.nv)).copy()
    return d.arr(key).copy()


@pytest.mark.parametrize("key", ["xpos", "qM", "qfrc_bias", "qacc_smooth", "qacc"])
@pytest.mark.parametrize("name", MODELS)
def test_oracle_smooth_dynamics(ia, ora, name, key):
    """oracle/mjsub.c against the reference, stage by stage, on moving airborne states.
    Measured on the CPU, E64 / deviation (bound 2 nv E64, floor 1e-14):
                         xpos             qM               qfrc_bias        qacc_smooth = qacc
      inverted_pendulum  0 / 0            5.7e-17/5.7e-17  5.4e-16/7.4e-16  5.1e-16/6.5e-16
      hopper             1.7e-16/2.7e-16  3.9e-16/4.0e-16  3.1e-15/1.4e-15  1.6e-15/1.7e-15
      humanoid           2.9e-16/5.7e-16  5.1e-16/5.6e-16  2.8e-15/1.9e-15  1.5e-14/2.0e-14
      chain              3.0e-16/1.9e-16  6.4e-16/6.3e-16  1.8e-15/8.1e-16  3.7e-15/5.6e-15
      ballarm            5.2e-16/4.6e-16  1.5e-15/1.6e-15  1.5e-15/6.6e-15  2.5e-15/3.5e-15
      floatarm           1.2e-16/2.1e-16  3.2e-16/2.2e-16  2.3e-15/5.0e-15  9.8e-15/1.0e-14
    (no constraint is active, so qacc is qacc_smooth)"""
    B = batch(name)
    om = ora.OModel(product_model(ia, name).blob())
    dev = 0.0
    for s in B.states:
        d = _oracle_forward(om, s)
        assert d.nefc() == 0 and d.ncon() == 0
        dev = max(dev, rel(_oracle_array(om, d, key), s["ref"][key]))
    report("oracle", name, key, B.e64(key), dev, B.tol(key))
    assert dev <= B.tol(key)


@pytest.mark.parametrize("name", MODELS)
def test_oracle_steps(ia, ora, name):
    """mj_step once and ten times against the reference integrator (Euler with implicit
    damping; RK4 for the pendulum), qpos and qvel.
    Measured on the CPU, E64 / deviation:
                         qpos 1 step      qvel 1 step      qpos 10 steps    qvel 10 steps
      inverted_pendulum  2.5e-16/1.7e-16  8.4e-17/1.4e-16  1.8e-16/1.6e-16  3.5e-16/5.5e-16
      hopper             7.3e-17/7.3e-17  1.2e-16/1.8e-16  1.4e-16/1.5e-16  5.2e-16/4.5e-16
      humanoid           7.8e-17/2.1e-16  1.4e-14/3.7e-14  5.7e-16/8.7e-16  2.9e-15/2.7e-15
      chain              9.4e-17/9.4e-17  2.3e-16/1.9e-16  2.5e-16/2.5e-16  8.4e-16/1.0e-15
      ballarm            3.4e-16/3.4e-16  1.4e-16/2.8e-16  5.3e-16/6.5e-16  1.1e-15/6.1e-16
      floatarm           6.3e-17/6.3e-17  2.6e-16/3.9e-16  1.5e-16/1.5e-16  1.1e-15/2.5e-15"""
    B = batch(name)
    om = ora.OModel(product_model(ia, name).blob())
    devs = dict(q1=0.0, v1=0.0, q10=0.0, v10=0.0)
    for s in B.states:
        d = _oracle_forward(om, s)
        d.step(1)
        devs["q1"] = max(devs["q1"], rel(d.arr("qpos"), s["ref"]["q1"]))
        devs["v1"] = max(devs["v1"], rel(d.arr("qvel"), s["ref"]["v1"]))
        d.step(9)
        devs["q10"] = max(devs["q10"], rel(d.arr("qpos"), s["ref"]["q10"]))
        devs["v10"] = max(devs["v10"], rel(d.arr("qvel"), s["ref"]["v10"]))
    for k, dev in devs.items():
        report("oracle step", name, k, B.e64(k), dev, B.tol(k))
    for k, dev in devs.items():
        assert dev <= B.tol(k), k


# ------------------------------------------------------------------ smooth dynamics: the kernels
def _gpu_state(ia, m, B):
    q, v, ctrl, qf, xf = B.arrays()
    n = q.shape[0]
    return ia.State(time=np.zeros(n), qpos=q, qvel=v, warm=np.zeros((n, m.nv)), ctrl=ctrl), qf, xf


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_gpu_forward(ia, name):
    """Model.forward(states, qfrc_applied, xfrc_applied) against the reference qacc.
    Measured on the MI355X, E64 / deviation: pendulum 5.1e-16/6.5e-16, hopper 1.6e-15/1.7e-15,
    humanoid 1.5e-14/2.0e-14, chain 3.7e-15/5.6e-15 (the oracle's figures to every digit)"""
    B = batch(name)
    m = product_model(ia, name)
    st, qf, xf = _gpu_state(ia, m, B)
    qacc = m.forward(st, qf, xf)
    dev = max(rel(qacc[i], s["ref"]["qacc"]) for i, s in enumerate(B.states))
    report("gpu forward", name, "qacc", B.e64("qacc"), dev, B.tol("qacc"))
    assert dev <= B.tol("qacc")


@pytest.mark.gpu
@pytest.mark.parametrize("nstep", [1, 10])
@pytest.mark.parametrize("name", MODELS)
def test_gpu_step(ia, name, nstep):
    """Model.step(states, 1) and Model.step(states, 10) against the reference integrator.
    Measured on the MI355X: the figures of test_oracle_steps to every digit (largest:
    humanoid qvel after one step, E64 1.4e-14, deviation 3.7e-14, bound 7.3e-13)"""
    B = batch(name)
    m = product_model(ia, name)
    st, qf, xf = _gpu_state(ia, m, B)
    m.step(st, nstep, qf, xf)
    for key, got in ((f"q{nstep}", st.qpos), (f"v{nstep}", st.qvel)):
        dev = max(rel(got[i], s["ref"][key]) for i, s in enumerate(B.states))
        report(f"gpu step {nstep}", name, key, B.e64(key), dev, B.tol(key))
        assert dev <= B.tol(key), key


# ------------------------------------------------------------------ contact geometry and the constraint solve
CROSS_XML = """<mujoco model="cross">
  <compiler angle="radian" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom condim="3" friction="0.7" margin="0.001"/></default>
  <worldbody>
    <body name="a" pos="0 0 1">
      <joint name="az" type="slide" axis="0 0 1"/>
      <joint name="ay" type="hinge" axis="0 1 0" pos="0.1 0 0"/>
      <geom name="ca" type="capsule" fromto="-0.3 0 0 0.3 0 0" size="0.05"/>
    </body>
    <body name="b" pos="0 0 1.2">
      <joint name="bx" type="slide" axis="1 0 0"/>
      <joint name="by" type="slide" axis="0 1 0"/>
      <joint name="bz" type="slide" axis="0 0 1"/>
      <joint name="bh" type="hinge" axis="1 0 0" pos="0 0.05 0"/>
      <geom name="cb" type="capsule" fromto="-0.1 -0.2 0 0.1 0.2 0" size="0.04"/>
    </body>
  </worldbody>
  <actuator><motor joint="az" gear="10"/><motor joint="bh" gear="2"/></actuator>
</mujoco>"""
# both axes are exactly (0, 0, 1) and both half lengths powers of two: det == 0 exactly
PARALLEL_XML = """<mujoco model="parallel">
  <compiler angle="radian" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom condim="3" friction="0.7"/></default>
  <worldbody>
    <body name="a" pos="0 0 1">
      <joint name="ax" type="slide" axis="1 0 0"/>
      <geom name="ca" type="capsule" pos="0 0 0" size="0.05 0.25"/>
    </body>
    <body name="b" pos="0.085 0 1.125">
      <joint name="bz" type="slide" axis="0 0 1"/>
      <joint name="by" type="slide" axis="0 1 0"/>
      <geom name="cb" type="capsule" pos="0 0 0" size="0.04 0.5"/>
    </body>
  </worldbody>
  <actuator><motor joint="ax" gear="10"/></actuator>
</mujoco>"""
TEST_XML = {"cross": CROSS_XML, "parallel": PARALLEL_XML}
_H = [0.0, 0.0, 3.0, 1.0, 0.0, 0.0, 0.0]  # humanoid root: airborne, for the self-collision poses

# every state was found by a seeded search with the reference (float64) and is fixed
# here as a literal; what each one has to show is asserted in ContactBatch, on the
# reference alone.  (name of the case, qpos)
CONTACT_CASES = {
    "hopper": [
        ("one end sphere", [0.0, 0.965652, 0.2, -0.4, -0.7, 0.35]),
        ("both end spheres sliding, foot_joint past its limit", [0.0, 1.038122, -0.01, -0.3, -0.5, 0.79]),
    ],
    "inverted_pendulum": [
        ("slider past its upper end", [1.004, 0.3]),
        ("slider past its lower end", [-1.006, -0.2]),
    ],
    "humanoid": [
        ("on its back: head, butt and four foot capsules on the floor, knees past their limit",
         [0.0, 0.0, 0.089819, 0.6924048490274763, 0.0, -0.7215091995555134, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.060444,
          0.0, 0.0, 0.0, 0.0, 0.0, 0.060444, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
        ("lower arm across both feet (capsule-capsule edge)",
         _H + [-0.027263, -0.7582, -0.161644, -0.072153, -0.374349, -1.4382, -1.86909, -0.044506, 0.71769, -0.349346,
               0.474322, -0.924114, -2.442822, -0.01714, -0.333547, 0.054782, 0.146286, -0.964958, -0.063651,
               0.716969, 0.074252]),
        ("upper arm end on a foot end (capsule-capsule corner)",
         _H + [-0.553842, -1.103307, 0.098021, -0.276162, -0.818154, -1.763267, -1.600552, -0.283711, -0.007791,
               -0.039911, -0.35525, -1.531413, -1.280303, -0.672253, -0.233505, -0.753395, -0.426205, -1.249745,
               0.445268, 0.45306, 0.241485]),
        ("hand on the ends of two foot capsules (sphere-capsule end)",
         _H + [0.416936, -1.086289, 0.269794, -0.049445, 0.148142, -1.60899, -1.295587, 0.359702, -0.169468, -0.03052,
               -0.655537, -0.877917, -1.399804, 0.318362, -0.159262, -0.69092, 0.214243, -1.037297, 0.093483,
               0.172729, 0.187602]),
        ("head against a hand (sphere-sphere)",
         _H + [-0.315124, -0.631597, -0.279292, -0.116229, -0.257398, -1.049962, -1.198937, -0.401116, -0.091938,
               -0.150512, -0.037165, -1.177303, -0.752579, 0.517231, 0.581094, 0.059153, 0.692682, 0.610859,
               0.459476, -0.509072, -0.182822]),
        ("hand on the side of a thigh (sphere-capsule interior)",
         _H + [0.245863, -0.881226, -0.077361, -0.261651, -0.257919, -0.299016, -2.3386, 0.088666, 0.040125,
               -0.226084, 0.315802, -1.198126, -0.593973, -0.608425, -0.135983, -1.07628, 0.528613, 0.026974,
               -0.375048, -0.076816, -1.140423]),
    ],
    "cross": [
        ("interior", [0.0, 0.09142146695279263, -0.23894081849715845, -0.04553671344240057, -0.079841,
                      0.4741861932592554]),
        ("edge, first capsule's end", [0.0, -0.10503441325463636, 0.2755937979243392, -0.1284835388168569, -0.083957,
                                       -0.3509614164664442]),
        ("edge, second capsule's end", [0.0, 0.2152529414759124, -0.1464322448261709, 0.2055581694310592, -0.067397,
                                        -0.10101274691195616]),
        ("corner +-", [0.0, 0.2646005851455611, 0.4425090452911767, 0.1565733782555574, -0.1144, 0.3088438090346699]),
        ("corner -+", [0.0, 0.17369566654539986, -0.4001468452380013, -0.23466797395621297, -0.122073,
                       0.3828722599610608]),
    ],
    "parallel": [
        ("rest pose", [0.0, 0.0, 0.0]),
        ("shifted along the axis", [0.003, -0.2, 0.0]),
    ],
    "ballarm": [
        ("the hand sphere on the floor",
         [0.9474701826353175, -0.036599007054861875, 0.31103605995562766, -0.06494101251809571, 0.697937,
          0.7901337836246584, 0.41084788749075934, 0.3936028922132403, -0.2279679375717867, -0.07322]),
        ("the finger capsule flat on the floor: two contacts",
         [0.755206759905838, 0.48578584555971727, 0.1976859371519934, -0.3931858749989563, -0.542051,
          0.8951127601317426, -0.16334595622729153, 0.36204490298084907, 0.20252094572935556, 1.348883]),
        ("the hand sphere and both ends of the finger capsule on the floor, the arm moving",
         [-0.6810432623263374, 0.4687011805357616, -0.5625602166886736, 0.005028001936701243, -0.103403,
          0.6302000459586005, -0.436061031800624, -0.15752001148746228, -0.6228050454193053, -0.921498]),
    ],
}
CONTACT_MODELS = list(CONTACT_CASES)
REQUIRED_KINDS = ["plane-sphere", "plane-capsule one contact", "plane-capsule two contacts", "sphere-capsule end",
                  "sphere-capsule interior", "capsule-capsule interior", "capsule-capsule edge",
                  "capsule-capsule corner", "capsule-capsule parallel", "limit"]


def contact_compiled(name):
    return mi.compile_mjcf(io.StringIO(TEST_XML[name])) if name in TEST_XML else compiled(name)


def contact_product(ia, name):
    return ia.Model.from_string(TEST_XML[name]) if name in TEST_XML else product_model(ia, name)


class ContactBatch:
    """the literal states of one model, seeded velocities and controls, the reference's
    problem and minimiser at each (longdouble) and the problem again in float64"""

    def __init__(self, name):
        self.name, self.C = name, contact_compiled(name)
        C = self.C
        self.R, self.R64 = rr.Ref(C, LD), rr.Ref(C, np.float64)
        rng = np.random.default_rng(977 + CONTACT_MODELS.index(name))
        assert len(CONTACT_CASES[name]) <= 12
        self.states, self.kinds = [], set()
        for what, q in CONTACT_CASES[name]:
            q = np.array(q, float)
            v = rng.normal(0, 0.5, C.nv)
            if "sliding" in what:
                v[0] = 0.6
            s = dict(what=what, q=q, v=v, ctrl=rng.uniform(-0.3, 0.3, len(C.act)))
            s["P"] = P = self.R.problem(q, v, s["ctrl"])
            s["P64"] = self.R64.problem(q, v, s["ctrl"])
            assert len(P.D) == len(s["P64"].D) > 0, what
            s["astar"] = self.R.minimise(P)
            per_pair = {}
            for c in P.contacts:
                assert 0 < -c["dist"] <= 0.02, (what, float(c["dist"]))  # every depth in (0, 2 cm]
                per_pair.setdefault((c["g1"], c["g2"]), []).append(c)
            for cs in per_pair.values():
                k = cs[0]["kind"]
                self.kinds.add(k if k != "plane-capsule" else
                               "plane-capsule one contact" if len(cs) == 1 else "plane-capsule two contacts")
            if "limit" in P.kind:
                self.kinds.add("limit")
            s["nlimit"], s["ncon"] = P.kind.count("limit"), len(P.contacts)
            self.states.append(s)
        self._conditions()

    def _conditions(self):
        """what the cases of this model have to show, by the reference"""
        S, R, C = self.states, self.R, self.C
        if self.name == "hopper":
            assert S[0]["ncon"] == 1 and S[0]["nlimit"] == 0
            assert S[1]["ncon"] == 2 and S[1]["nlimit"] == 1 and {"limit", "contact"} <= set(S[1]["P"].kind)
            foot = [i for i, j in enumerate(C.joints) if j["name"] == "foot_joint"][0]
            assert S[1]["q"][R.jq[foot]] > C.joints[foot]["range"][1]
            for c in S[1]["P"].contacts:  # sliding: tangential speed of the foot at the contact
                vel = R.jac(S[1]["P"].f.K, C.geoms[c["g2"]]["body"], c["pos"])[0] @ S[1]["P"].f.v
                assert np.sqrt(vel @ vel - (vel @ c["normal"]) ** 2) >= 0.1
        if self.name == "inverted_pendulum":
            assert [s["nlimit"] for s in S] == [1, 1] and S[0]["P"].J[0, 0] == -1 and S[1]["P"].J[0, 0] == 1
        if self.name == "humanoid":
            floor = S[0]["P"].contacts
            types = {C.geoms[c["g2"]]["type"] for c in floor if C.geoms[c["g1"]]["type"] == "plane"}
            assert len({c["g2"] for c in floor}) >= 3 and types == {"sphere", "capsule"}
            for s in S[1:]:  # self-collision inside every joint range
                assert s["nlimit"] == 0 and R.limit_clearance(s["q"]) > 0
                assert all(C.geoms[c["g1"]]["type"] != "plane" for c in s["P"].contacts)
            assert {"sphere-capsule end", "sphere-capsule interior", "capsule-capsule edge"} <= self.kinds
        if self.name == "ballarm":
            pairs = [sorted((C.geoms[c["g2"]]["type"], c["kind"]) for c in s["P"].contacts) for s in S]
            assert pairs[0] == [("sphere", "plane-sphere")]
            assert pairs[1] == [("capsule", "plane-capsule")] * 2 and len({c["g2"] for c in S[1]["P"].contacts}) == 1
            assert pairs[2] == [("capsule", "plane-capsule")] * 2 + [("sphere", "plane-sphere")]
            assert all(C.geoms[c["g1"]]["type"] == "plane" for s in S for c in s["P"].contacts)
            for s in S:  # inside the elbow's range, both ball quaternions at least 0.5 rad from the identity
                assert s["nlimit"] == 0 and R.limit_clearance(s["q"]) > 0
                for a in (0, 5):
                    assert abs(np.linalg.norm(s["q"][a:a + 4]) - 1) <= 2.3e-16
                    assert 2 * np.arccos(abs(s["q"][a])) >= 0.5
            for c in S[2]["P"].contacts:  # moving: the speed of the arm's point at each contact
                vel = R.jac(S[2]["P"].f.K, C.geoms[c["g2"]]["body"], c["pos"])[0] @ S[2]["P"].f.v
                assert np.sqrt(vel @ vel) >= 0.1
        if self.name in TEST_XML:
            for s in S:
                K = s["P"].f.K
                z1, z2 = R.geom_pose(K, 0)[1], R.geom_pose(K, 1)[1]
                ang = float(np.arccos(min(abs(z1 @ z2), LD(1))))
                assert (ang == 0.0) if self.name == "parallel" else (ang >= 0.1)
                assert s["ncon"] == (2 if self.name == "parallel" else 1)

    def e64(self, key):
        return max(rel(self.value(s["P64"], key), self.value(s["P"], key)) for s in self.states)

    @staticmethod
    def value(P, key):
        if key in ("dist", "normal", "pos"):
            return np.array([c[key] for c in P.contacts], dtype=P.D.dtype) if P.contacts else np.zeros(1, P.D.dtype)
        return {"efc_J": P.J, "efc_D": P.D, "efc_aref": P.aref, "efc_pos": P.pos}[key]

    def tol(self, key):
        return max(2 * self.C.nv * self.e64(key), 1e-14)

    def gap(self, s, qacc):
        """(scaled cost gap to the minimiser, |qacc - a*| in the M norm), in longdouble"""
        R, P = self.R, s["P"]
        qacc = np.asarray(qacc, LD)
        e = qacc - s["astar"]
        return float(P.scale * (R.cost(P, qacc) - R.cost(P, s["astar"]))), float(np.sqrt(e @ (P.M @ e)))


_cbatches = {}


def cbatch(name):
    if name not in _cbatches:
        _cbatches[name] = ContactBatch(name)
    return _cbatches[name]


def test_contact_cases_cover_every_branch():
    """across all cases, by the reference: every pair kind, every capsule-capsule region
    class, one and two plane-capsule contacts, and a limit row"""
    kinds = set().union(*(cbatch(n).kinds for n in CONTACT_MODELS))
    print(sorted(kinds))
    assert set(REQUIRED_KINDS) <= kinds, sorted(set(REQUIRED_KINDS) - kinds)


def test_reference_minimiser_is_stationary():
    """the reference's a*: its gradient is at the rounding of its own terms (the cost is
    strictly convex, so a stationary point is the minimiser), and no seeded perturbation
    lowers the cost"""
    rng = np.random.default_rng(3)
    for name in CONTACT_MODELS:
        B = cbatch(name)
        for s in B.states:
            P, a = s["P"], s["astar"]
            g = B.R.grad(P, a)
            assert np.all(np.abs(g) <= 64 * np.finfo(LD).eps * B.R.grad_scale(P, a)), (name, s["what"])
            c0 = B.R.cost(P, a)
            for _ in range(4):
                assert B.R.cost(P, a + LD(1e-6) * rng.normal(0, 1, B.C.nv) * np.max(np.abs(a))) >= c0


@pytest.mark.parametrize("name", CONTACT_MODELS)
def test_oracle_contacts_and_rows(ia, ora, name):
    """the oracle's contacts (distance, normal, point; sorted by geom pair) and constraint
    rows (efc_J, efc_D, efc_aref, efc_pos) against the reference: ncon and nefc exactly,
    the arrays at 2 nv E64 (floor 1e-14).
    Measured on the CPU, E64 / deviation (the distance is a difference of positions a hundred
    times its size, hence its larger figures):
                 dist             normal           pos              efc_J            efc_D            efc_aref
      hopper     3.0e-14/2.0e-14  0 / 0            2.2e-16/2.2e-16  9.3e-17/1.1e-16  2.9e-17/4.2e-16  2.0e-15/1.5e-15
      pendulum   (no contacts)                                      0 / 0            7.2e-17/3.0e-16  1.4e-16/1.4e-16
      humanoid   8.5e-14/8.4e-14  3.4e-15/8.3e-15  1.4e-16/2.6e-16  5.8e-15/8.6e-15  2.2e-16/2.1e-15  9.5e-14/9.9e-14
      cross      1.3e-14/3.5e-14  1.2e-15/2.0e-15  1.6e-16/2.1e-16  1.2e-15/2.0e-15  2.9e-16/2.9e-16  4.3e-15/9.2e-15
      parallel   3.3e-16/3.3e-16  0 / 0            2.8e-18/2.8e-18  0 / 0            9.6e-17/3.5e-16  8.2e-17/2.0e-16
      ballarm    2.5e-14/3.2e-14  0 / 0            8.1e-16/8.1e-16  5.6e-16/7.1e-16  8.9e-17/7.4e-16  1.1e-14/9.7e-15
    efc_pos follows dist."""
    B = cbatch(name)
    om = ora.OModel(contact_product(ia, name).blob())
    devs = {}
    for s in B.states:
        P = s["P"]
        d = om.make_data()
        d.set_state(qpos=s["q"], qvel=s["v"], ctrl=s["ctrl"])
        d.forward()
        assert (d.ncon(), d.nefc()) == (len(P.contacts), len(P.D)), s["what"]
        got = sorted(d.contacts(), key=lambda c: (c["geom1"], c["geom2"]))
        ref = sorted(P.contacts, key=lambda c: (c["g1"], c["g2"]))
        for g, r in zip(got, ref):
            assert (g["geom1"], g["geom2"], g["dim"]) == (r["g1"], r["g2"], r["dim"]), s["what"]
        for key in ("dist", "normal", "pos"):
            if ref:
                devs[key] = max(devs.get(key, 0.0), rel([g[key] for g in got], [r[key] for r in ref]))
        for key in ("efc_J", "efc_D", "efc_aref", "efc_pos"):
            devs[key] = max(devs.get(key, 0.0), rel(d.efc(key), B.value(P, key)))
    for key, dev in devs.items():
        report("oracle contact", name, key, B.e64(key), dev, B.tol(key))
    for key, dev in devs.items():
        assert dev <= B.tol(key), key


@pytest.mark.parametrize("name", CONTACT_MODELS)
def test_oracle_constraint_solve(ia, ora, name):
    """mj_forward's qacc is the minimiser of the reference's problem:
    scale (cost(qacc) - cost(a*)) <= 10 opt.tolerance, scale = 1 / (meaninertia max(1, nv)),
    evaluated in longdouble.  The solver stops when its last step improved the scaled cost
    by less than opt.tolerance or the scaled gradient is below it; after a converging
    Newton step the remaining gap is no larger than that improvement, 10x allows for it.
    Measured on the CPU: the gap is between -4.1e-16 and 1.2e-16 in every case (zero at the
    rounding of the two costs in longdouble), |qacc - a*|_M at most 1.1e-11 (humanoid, head
    against a hand), one to four iterations, never the cap (ballarm: gap within -2.1e-16 ..
    4.2e-16, |qacc - a*|_M at most 1.0e-12, two to four iterations)."""
    B = cbatch(name)
    om = ora.OModel(contact_product(ia, name).blob())
    worst = 0.0
    for s in B.states:
        d = om.make_data()
        d.set_state(qpos=s["q"], qvel=s["v"], ctrl=s["ctrl"])
        d.forward()
        gap, dist = B.gap(s, d.arr("qacc"))
        print(f"oracle solve {name:18s} {s['what'][:40]:40s} gap {gap:.2e} |qacc - a*|_M {dist:.2e} "
              f"iterations {d.solver_iter()}")
        assert d.solver_iter() < B.C.iterations, "ended on the iteration cap"
        worst = max(worst, gap)
    assert worst <= 10 * B.C.tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONTACT_MODELS)
def test_gpu_constraint_solve(ia, name):
    """Model.forward's qacc on the contact cases: the same bound as the oracle's.
    Measured on the MI355X: the oracle's figures to every digit (gap within -4.1e-16 .. 1.2e-16,
    |qacc - a*|_M at most 1.1e-11)."""
    B = cbatch(name)
    m = contact_product(ia, name)
    n = len(B.states)
    st = ia.State(time=np.zeros(n), qpos=np.array([s["q"] for s in B.states]),
                  qvel=np.array([s["v"] for s in B.states]), warm=np.zeros((n, m.nv)),
                  ctrl=np.array([s["ctrl"] for s in B.states]).reshape(n, m.nu))
    qacc = m.forward(st)
    worst = 0.0
    for i, s in enumerate(B.states):
        gap, dist = B.gap(s, qacc[i])
        print(f"gpu solve {name:18s} {s['what'][:40]:40s} gap {gap:.2e} |qacc - a*|_M {dist:.2e}")
        worst = max(worst, gap)
    assert worst <= 10 * B.C.tolerance

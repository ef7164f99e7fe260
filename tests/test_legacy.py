"""Legacy C++ boundary: include/legacy (mujoco.h subset,
mjderivative.h, util.h, update.h, differentiator.h, ilqr.h) over
libilqg_mujoco.so.

CPU: the library exports the reference's C++ symbols with the reference's
mangling and the MuJoCo C API subset; the reference's own controller
(src/inverted_pendulum/inverted_pendulum.cpp) compiles unmodified against the
headers and links (when /root/reference is present); without a GPU the path
fails loudly.
GPU: the headless cmd/basic.cpp loop (ilqg_headless, host-callback cost and
registered device cost) and the reference's controller linked against the
product reproduce the oracle's MPC loop bit for bit.

Off the pendulum (models with quaternion dofs: the humanoid's free joint, the
ball joints of tests/ball_models.py): the library's mju_quatIntegrate and the
cost columns that host_cost_columns forms with it against the oracle bit for
bit on the CPU, and calcMJDerivatives's whole record with a host callback and
with a registered descriptor on the GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ball_models import BALL_XML, ball_model
from conftest import ROOT, model_path
from test_model_compile import _fields

LIB = os.path.join(ROOT, "ilqg-mujoco_amd", "lib", "libilqg_mujoco.so")
HEADLESS = os.path.join(ROOT, "ilqg-mujoco_amd", "bin", "ilqg_headless")
REF_LOOP = os.path.join(ROOT, "oracle", "_ref", "ref_pendulum_legacy")
MEMBERS = os.path.join(ROOT, "ilqg-mujoco_amd", "bin", "legacy_members")

REF_SYMBOLS = [
    "_Z17calcMJDerivativesP8_mjModelP7_mjDataPdPFdPKS1_E",  # inc/mjderivative.h:7
    "_Z8cpMjDataPK8_mjModelP7_mjDataPKS2_",  # inc/util.h:6
    "_Z11forwardStepP8_mjModelP7_mjData",  # inc/update.h:6
    "_Z12forwardFrameP8_mjModelP7_mjData",  # inc/update.h:8
]
MJ_API = ["mj_activate", "mj_deactivate", "mj_loadXML", "mj_deleteModel", "mj_makeData", "mj_deleteData",
          "mj_resetData", "mj_stackAlloc", "mj_step", "mj_forward", "mj_forwardSkip", "mju_copy", "mju_zero",
          "mju_malloc", "mju_free", "mju_error", "mju_error_s", "mju_quatIntegrate"]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_legacy_exports_reference_symbols():
    syms = _exports(LIB)
    for s in REF_SYMBOLS + MJ_API:
        assert s in syms, s


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="/root/reference not present (GPU box)")
def test_reference_controller_compiles_against_legacy_headers():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "legacy"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(REF_LOOP)


def test_legacy_members_caller_compiles():
    """tests/legacy_members.cpp -- a caller touching every public type, member
    and method of Differentiator<nv,nu> and ILQR<nv,nu,N> that SURVEY.md §8b
    lists (inc/differentiator.h:14-93, inc/ilqr.h:19-186), and an ILQR
    subclass overriding the virtual initV -- compiles warning-free (-Wall
    -Wextra) against include/legacy and links against libilqg_mujoco.so"""
    src = os.path.join(ROOT, "tests", "legacy_members.cpp")
    pkg = os.path.join(ROOT, "ilqg-mujoco_amd")
    out = os.path.join(pkg, "build", "legacy_members_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "legacy"),
                        "-o", out, src, "-L" + os.path.join(pkg, "lib"), "-lilqg_mujoco", "-lilqg_amd",
                        "-Wl,-rpath," + os.path.join(pkg, "lib")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(src) as f:
        text = f.read()
    # every public member / method named in SURVEY.md §8b is touched
    for name in ("->m", "->d", "->deriv", "->dqaccdq", "->dqaccdqvel", "->dqaccdctrl", "->dgdx", "->dgdu",
                 "->x", "->u", "->A", "->B", "->stepCostFn", "setMJData", "updateDerivatives", "->differentiator",
                 "->dArray", "->V", "->v", "->K", "->xStar", "->uStar", "->mu", "initV", "setDInit",
                 "forwardPass", "backwardPass", "iterate"):
        assert name in text, name


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is visible")
def test_headless_fails_loudly_without_gpu():
    r = subprocess.run([HEADLESS, model_path("inverted_pendulum"), "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR" in r.stderr


# ------------------------------------------------------------------ quaternion dofs, CPU
QUAT_CASES = 3072   # 6 kinds of quaternion x 8 kinds of velocity x 64


def test_quat_integrate_matches_oracle(ora):
    """the library's mju_quatIntegrate (what host_cost_columns perturbs ball and free
    quaternions with) against the oracle's, bit for bit, on seeded cases printed by
    legacy_members: a third exactly the identity, unit quaternions, quaternions whose
    norm is off 1 by 1e-16..1e-15 (inside or at the edge of the window in which the
    oracle leaves a quaternion unnormalised) and by 1e-12, each with +-1e-6 e_k (the FD
    perturbation) and with general velocities at scales 0.002 and 1.
    Before the fix (host sin / cos, division by the norm, unconditional normalisation)
    1485 of the 3072 cases differed: 143 at the identity, all of those with a general
    velocity (host sin / cos); none at the identity with +-1e-6 e_k, which is why tests
    at the rest pose could not see it."""
    r = subprocess.run([MEMBERS, "-", "quat", "20241", str(QUAT_CASES)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = _hex_rows(r.stdout)
    cases, out = rows["case"], rows["out"]
    assert cases.shape == (QUAT_CASES, 8) and out.shape == (QUAT_CASES, 4)
    norm_off = np.abs(np.linalg.norm(cases[:, :4].astype(np.longdouble), axis=1) - 1)
    ident = np.all(cases[:, :4] == [1, 0, 0, 0], axis=1)
    assert QUAT_CASES >= 3000 and ident.sum() == QUAT_CASES // 3
    assert np.sum((norm_off >= 1e-16) & (norm_off <= 1e-15)) >= QUAT_CASES // 6
    assert np.sum((norm_off > 5e-13) & (norm_off < 2e-12)) >= QUAT_CASES // 8
    fd_pert = np.sum(np.abs(cases[:, 4:7]) == 1e-6, axis=1) == 1
    assert fd_pert.sum() == QUAT_CASES * 3 // 4 and set(cases[~fd_pert, 7]) == {0.002, 1.0}
    L = ora.oracle_lib().L
    dp = ctypes.POINTER(ctypes.c_double)
    L.mju_quatIntegrate.argtypes = [dp, dp, ctypes.c_double]
    L.mju_quatIntegrate.restype = None
    want = np.ascontiguousarray(cases[:, :4].copy())
    for i in range(QUAT_CASES):
        vel = np.ascontiguousarray(cases[i, 4:7])
        L.mju_quatIntegrate(want[i].ctypes.data_as(dp), vel.ctypes.data_as(dp), float(cases[i, 7]))
    differ = np.any(out.view(np.int64) != want.view(np.int64), axis=1)
    print(f"mju_quatIntegrate: {int(differ.sum())} of {QUAT_CASES} cases differ from the oracle "
          f"({int((differ & ident).sum())} at the identity)")
    assert not differ.any(), (int(differ.sum()), cases[differ][:3], out[differ][:3], want[differ][:3])


LEGACY_MODELS = ["humanoid", "ballarm", "floatarm"]


def _legacy_model(ia, name):
    return ball_model(ia, name) if name in BALL_XML else ia.Model.load(model_path(name))


def _legacy_xml(name, tmp_path):
    if name not in BALL_XML:
        return model_path(name)
    path = tmp_path / (name + ".xml")
    path.write_text(BALL_XML[name])
    return str(path)


def _quat_addresses(f):
    """qpos address of every quaternion (free joints' and ball joints')"""
    return [int(a) + (3 if t == 0 else 0) for t, a in zip(f["jnt_type"], f["jnt_qposadr"]) if t in (0, 1)]


def _legacy_states(m, n, seed):
    """n seeded states: every quaternion a unit one away from the identity as numpy
    rounds it, a free joint's body well above the floor, the other joints near qpos0,
    moving, with controls"""
    rng = np.random.default_rng(seed)
    f = _fields(m.blob())
    out = []
    for _ in range(n):
        q = np.array(m.qpos0, float)
        for t, a in zip(f["jnt_type"], f["jnt_qposadr"]):
            if t == 0:
                q[a:a + 3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), 3.0 + rng.uniform(0, 1)]
            elif t >= 2:
                q[a] += rng.uniform(-0.2, 0.2)
        for a in _quat_addresses(f):
            quat = rng.normal(0, 1, 4)
            q[a:a + 4] = quat / np.linalg.norm(quat)
        out.append(dict(time=0.0, qpos=q, qvel=rng.normal(0, 0.5, m.nv), warm=np.zeros(m.nv),
                        ctrl=rng.uniform(-0.2, 0.2, m.nu)))
    return out


def _lq_cost(ia, m):
    """linear weights on every quaternion component and nothing else on qpos: then
    (cost(perturbed) - cost(centre)) / eps keeps every bit of the perturbed quaternion
    (a quadratic cost of size 100 rounds most of a 1e-16 difference away); quadratic
    terms on qvel and ctrl so that every column is live"""
    lq = np.zeros(m.nq)
    for k, a in enumerate(_quat_addresses(_fields(m.blob()))):
        lq[a:a + 4] = np.array([0.7, -1.3, 0.9, 1.1]) * (1 + 0.25 * k)
    return ia.Cost(lq=lq, wv=[0.05] * m.nv, tv=[0.1] * m.nv, wu=[0.01] * m.nu, lu=[0.3] * m.nu)


def _write_cases(path, cost, m, states):
    rows = [tag + " " + " ".join(float(x).hex() for x in v) for tag, v in cost.packed(m.nq, m.nv, m.nu).items()]
    for s in states:
        vals = [s["time"], *s["qpos"], *s["qvel"], *s["warm"], *s["ctrl"]]
        rows.append("state " + " ".join(float(x).hex() for x in vals))
    path.write_text("\n".join(rows) + "\n")
    return str(path)


def _oracle_records(ora, m, cost, states):
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(cost, m.nq, m.nv, m.nu))
    recs, ncon = [], []
    for s in states:
        d = om.make_data()
        d.set_state(**s)
        recs.append(ora.calc_derivatives(om, d, cost_fn="ora_cost_desc_fn", nthread=1))
        d.set_state(**s)
        d.forward()
        ncon.append(d.ncon())
    return np.array(recs), ncon


@pytest.mark.parametrize("name", LEGACY_MODELS)
def test_host_cost_columns_match_oracle(ia, ora, name, tmp_path):
    """host_cost_columns (the cost entries of a legacy calcMJDerivatives with a host
    stepCostFn_t) on 16 seeded states per model against the cost entries of the oracle's
    calcMJDerivatives, bit for bit; the callback restates the descriptor cost's expression
    order.  Runs without a GPU: the columns are host arithmetic.
    Before the fix of mju_quatIntegrate the quaternion columns differed, by up to 4.4e-10:
    humanoid 10 entries in 5 of 16 states, ballarm 18 entries in 8 states, floatarm 18
    entries in 8 states."""
    m = _legacy_model(ia, name)
    cost, states = _lq_cost(ia, m), _legacy_states(m, 16, 4100 + LEGACY_MODELS.index(name))
    r = subprocess.run([MEMBERS, _legacy_xml(name, tmp_path), "costcols",
                        _write_cases(tmp_path / "cases.txt", cost, m, states)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    got = _hex_rows(r.stdout)["g"]
    ref, _ = _oracle_records(ora, m, cost, states)
    want = ref[:, m.nv * (2 * m.nv + m.nu):]
    assert got.shape == want.shape == (16, 2 * m.nv + m.nu)
    differ = got.view(np.int64) != want.view(np.int64)
    print(f"host_cost_columns {name}: {int(differ.sum())} entries differ in {int(differ.any(axis=1).sum())} of 16 "
          f"states, columns {sorted(set(np.nonzero(differ)[1].tolist()))}, max {np.abs(got - want).max():.2e}")
    # the quaternion columns are live: none of them is zero in every state
    f = _fields(m.blob())
    qdofs = [int(d) + k + (3 if t == 0 else 0) for t, d in zip(f["jnt_type"], f["jnt_dofadr"]) if t in (0, 1)
             for k in range(3)]
    assert len(qdofs) >= 3 and np.all(np.any(want[:, qdofs] != 0, axis=0))
    assert not differ.any()


# ------------------------------------------------------------------ GPU
FRAMES = 3


def _parse(out):
    rows = []
    for line in out.splitlines():
        if line.startswith("frame "):
            rows.append([float.fromhex(x) for x in line.split()[2:]])
    return np.array(rows)


def _oracle_loop(ora, frames):
    """InvertedPendulum (src/inverted_pendulum/inverted_pendulum.cpp:7-30) on the oracle:
    10 passive steps, ILQR<2,1,20>; per frame setDInit, 10 iterate, first control, mj_step."""
    import ilqg_amd as ia
    m = ia.Model.load(model_path("inverted_pendulum"))
    om = ora.OModel(m.blob())
    d = om.make_data()
    d.step(10)
    il = ora.OILQR(om, d, 20, cost_fn="ora_cost_pendulum")

    def row():
        return [d.time] + list(d.arr("qpos")) + list(d.arr("qvel")) + list(d.arr("ctrl"))
    rows = [row()]
    for _ in range(frames):
        il.set_dinit(d)
        for _ in range(10):
            il.iterate()
        d.arr("ctrl")[:] = il.traj()["ctrl"][20]
        d.step(1)
        rows.append(row())
    return np.array(rows)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return _parse(r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("device_cost", [False, True])
def test_headless_loop_bitexact(ora, device_cost):
    cmd = [HEADLESS, model_path("inverted_pendulum"), str(FRAMES)] + (["--device-cost"] if device_cost else [])
    got = _run(cmd)
    ref = _oracle_loop(ora, FRAMES)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), np.abs(got - ref).max()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_LOOP), reason="oracle/_ref/ref_pendulum_legacy not built")
def test_reference_controller_on_gpu_bitexact(ora):
    got = _run([REF_LOOP, model_path("inverted_pendulum"), str(FRAMES)])
    ref = _oracle_loop(ora, FRAMES)
    assert np.array_equal(got, ref), np.abs(got - ref).max()


@pytest.mark.gpu
def test_legacy_members_semantics():
    """the public members keep the reference's meaning on the GPU path: x / u
    on d, xStar / uStar left on dArray[0] by forwardPass, d one step past the
    terminal point after the ctor, the differentiator left at dArray[N] with
    its A / B after backwardPass (inc/ilqr.h:82-93,121-129,153-154)"""
    r = subprocess.run([MEMBERS, model_path("inverted_pendulum"), "members"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "members ok" in r.stdout, r.stderr


def _hex_rows(out):
    rows = {}
    for line in out.splitlines():
        tag, *vals = line.split()
        rows.setdefault(tag, []).append([float.fromhex(x) for x in vals])
    return {k: np.array(v) for k, v in rows.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2])
def test_initv_override_drives_recursion(ora, iters):
    """virtual initV (inc/ilqr.h:100,142): an ILQR subclass whose initV sets
    its own V0 / v0 gets the recursion started from them (uploaded through
    ilqg_solver_set_value) -- K, k, V, v and the trajectory bit-exact against
    the oracle's backwardPass seeded with the same V0 / v0"""
    import ilqg_amd as ia
    r = subprocess.run([MEMBERS, model_path("inverted_pendulum"), "initv", str(iters)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = _hex_rows(r.stdout)
    m = ia.Model.load(model_path("inverted_pendulum"))
    om = ora.OModel(m.blob())
    d = om.make_data()
    d.step(10)
    il = ora.OILQR(om, d, 20, cost_fn="ora_cost_pendulum")
    il.set_dinit(d)
    nx = 4
    V0 = np.array([[(0.5 * (i + 1) if i == j else 0.0) + 0.125 * (i + j) for i in range(nx)] for j in range(nx)])
    v0 = np.arange(nx) - 1.5
    for _ in range(iters):
        il.iterate_v0(V0.ravel(), v0)  # V0 column-major: V0[j][i] = V(i, j)
    a, t = il.arrays(), il.traj()
    assert np.array_equal(got["K"], a["K"]) and np.array_equal(got["k"], a["k"])
    assert np.array_equal(got["V"][0], a["V"]) and np.array_equal(got["v"][0], a["v"])
    assert np.array_equal(got["qpos"], t["qpos"]) and np.array_equal(got["ctrl"], t["ctrl"])
    # and the override mattered: the default initV gives other gains
    il2 = ora.OILQR(om, d, 20, cost_fn="ora_cost_pendulum")
    il2.set_dinit(d)
    for _ in range(iters):
        il2.iterate()
    assert not np.array_equal(il2.arrays()["K"], a["K"])


@pytest.mark.gpu
def test_initv_override_changing_a_point(ora):
    """an initV override that changes a later point (dArray[N/2]->qvel[0] +=
    1e-3 after the default initV): the reference differentiates dArray[n]
    inside its loop, after initV (inc/ilqr.h:142-154), so the recursion sees
    the changed state -- the legacy backwardPass re-sweeps when an override
    changed the trajectory.  K, k, V, v and the trajectory bit-exact against
    the oracle's backwardPass run on the changed trajectory"""
    import ilqg_amd as ia
    r = subprocess.run([MEMBERS, model_path("inverted_pendulum"), "mutate"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    got = _hex_rows(r.stdout)
    m = ia.Model.load(model_path("inverted_pendulum"))
    om = ora.OModel(m.blob())
    d = om.make_data()
    d.step(10)
    N = 20
    il = ora.OILQR(om, d, N, cost_fn="ora_cost_pendulum")
    il.set_dinit(d)
    il.forward_pass()  # iterate(): forwardPass; setDInit(dArray[N]); backwardPass
    il.set_dinit(il.point(N))
    il.point(N // 2).arr("qvel")[0] += 1e-3  # what the override does after the default initV
    il.backward_pass()
    a, t = il.arrays(), il.traj()
    assert np.array_equal(got["K"], a["K"]) and np.array_equal(got["k"], a["k"])
    assert np.array_equal(got["V"][0], a["V"]) and np.array_equal(got["v"][0], a["v"])
    assert np.array_equal(got["qvel"], t["qvel"]) and np.array_equal(got["ctrl"], t["ctrl"])


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2])
def test_legacy_mu_is_live(ora, iters):
    """the public ILQR::mu (inc/ilqr.h:65) is read by every backward pass
    (inc/ilqr.h:166): a caller setting il.mu = 10 before iterate() gets the
    oracle's recursion at mu = 10 bit for bit, and mu = 1000 gives other gains"""
    import ilqg_amd as ia
    m = ia.Model.load(model_path("inverted_pendulum"))
    om = ora.OModel(m.blob())
    d = om.make_data()
    d.step(10)
    runs = {}
    for mu in (10.0, 1000.0):
        r = subprocess.run([MEMBERS, model_path("inverted_pendulum"), "mu", repr(mu), str(iters)], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        got = _hex_rows(r.stdout)
        il = ora.OILQR(om, d, 20, cost_fn="ora_cost_pendulum")
        il.set_mu(mu)
        il.set_dinit(d)
        for _ in range(iters):
            il.iterate()
        a, t = il.arrays(), il.traj()
        assert np.array_equal(got["K"], a["K"]) and np.array_equal(got["k"], a["k"]), mu
        assert np.array_equal(got["V"][0], a["V"]) and np.array_equal(got["v"][0], a["v"]), mu
        assert np.array_equal(got["qpos"], t["qpos"]) and np.array_equal(got["ctrl"], t["ctrl"]), mu
        runs[mu] = got
    assert not np.array_equal(runs[10.0]["K"], runs[1000.0]["K"])


@pytest.mark.gpu
@pytest.mark.parametrize("device_cost", [False, True])
@pytest.mark.parametrize("name", ["humanoid", "ballarm"])
def test_calc_derivatives_quaternion_models(ia, ora, name, device_cost, tmp_path):
    """legacy calcMJDerivatives off the pendulum (legacy_members fd: nothing tied to nv 2,
    nu 1): 4 seeded states, with the host callback (the physics blocks from the device, the
    cost entries from host_cost_columns) and with the descriptor registered for it (all of
    it from the device): the whole record is ora_calcMJDerivatives's bit for bit.  The
    humanoid's states are the first four of test_host_cost_columns_match_oracle's that touch
    nothing (airborne, no self-collision, by the oracle); ballarm's fourth is the
    hand-on-the-floor pose of test_physics_reference.CONTACT_CASES"""
    from test_physics_reference import CONTACT_CASES
    m = _legacy_model(ia, name)
    cost, states = _lq_cost(ia, m), _legacy_states(m, 16, 4100 + LEGACY_MODELS.index(name))
    if name == "humanoid":
        om = ora.OModel(m.blob())
        free = []
        for s in states:
            d = om.make_data()
            d.set_state(**s)
            d.forward()
            if d.ncon() == 0:
                free.append(s)
        states = free
    states = states[:4]
    assert len(states) == 4
    if name == "ballarm":
        states[3]["qpos"] = np.array(CONTACT_CASES["ballarm"][0][1])
    ref, ncon = _oracle_records(ora, m, cost, states)
    assert (ncon[3] > 0) if name == "ballarm" else (ncon == [0, 0, 0, 0])
    cmd = [MEMBERS, _legacy_xml(name, tmp_path), "fd", _write_cases(tmp_path / "cases.txt", cost, m, states)]
    r = subprocess.run(cmd + (["--device-cost"] if device_cost else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _hex_rows(r.stdout)["deriv"]
    assert got.shape == ref.shape == (4, m.nv * (2 * m.nv + m.nu) + 2 * m.nv + m.nu)
    differ = got.view(np.int64) != ref.view(np.int64)
    assert not differ.any(), (int(differ.sum()), sorted(set(np.nonzero(differ)[1].tolist()))[:10])

"""The receding-horizon shift (ilqg_solver_shift_horizon): the nominal
trajectory, the gains and the FD records move n points toward "now" in place on
the device, the tail continues the rollout with the terminal control held, its
records are swept, dinit takes the new point N.

CPU: the ABI, and the numpy restatement (shift_ref.py) pinned against the
oracle.  GPU: the device against a longer passive rollout, against the
restatement driven by the oracle's step and by Model.step, against a twin
solver loaded with the shifted arrays from the host, and against itself
(composition, asynchrony, seed groups).  Bit for bit throughout.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import applied_forces as af
import cost_sched_ref as cs
import shift_ref as sr
from conftest import model_path

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ilqg_solver_shift_horizon"
MODELS = ("inverted_pendulum", "hopper", "chain", "humanoid")
HORIZON = {"inverted_pendulum": 8, "hopper": 8, "chain": 6, "humanoid": 4}
ERR_ARG = 1
REG = dict(factor=1.6, mu_min=1e-6, mu_max=1e10, zmin=0.0, tol_cost=0.0, max_retry=4, trace_len=16)


def exact(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not sr.bits_equal(a, b):
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        raise AssertionError(f"{what}: not bit-exact at {len(bad)} entries, first {bad[0].tolist()}: "
                             f"{a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def exact_arrays(a, b, what, names=sr.ARRAYS):
    for f in names:
        exact(a[f], b[f], f"{what} {f}")


# ---------------------------------------------------------------- CPU ----
def test_header_and_exports(ia):
    """fails without the feature: the declaration, the binding's list, the library's symbol"""
    with open(os.path.join(ROOT, "include", "ilqg_amd.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    assert re.search(r"#define\s+ILQG_TAIL_HOLD\s+0\b", hdr)
    assert NAME in ia.EXPORTS
    assert hasattr(ia.lib(), NAME)
    assert ia.lib().ilqg_solver_shift_horizon.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert ia.TAIL_MODES == {"hold": 0}
    assert ia.lib().ilqg_solver_shift_horizon(None, 1, 0) == ERR_ARG  # a null solver, before any device call


def _cpu_setup(ia, ora, name):
    """(m, om, two state dicts) with the oracle's physics alone; the model's cost installed"""
    m = ia.Model.load(model_path(name))
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(af.cost(ia, name), m.nq, m.nv, m.nu))
    om.lib.L.ora_set_nthread(1)
    d = om.make_data()
    d.set_state(time=0.0, qpos=m.qpos0, qvel=np.zeros(m.nv), warm=np.zeros(m.nv), ctrl=np.zeros(m.nu))
    d.step(10 if name == "inverted_pendulum" else 500)
    base = d.state()
    if name != "inverted_pendulum":
        base["ctrl"] = base["ctrl"] - 0.1
    sts = []
    for s in range(2):
        st = {k: np.copy(v) for k, v in base.items()}
        st["qpos"] = st["qpos"] + 0.01 * s
        st["ctrl"] = st["ctrl"] + 0.05 * s
        sts.append(st)
    return m, om, sts


def _oracle_passive(ora, om, sts, qf, xf, H):
    """the constructor's passive rollout of every seed: shift()'s layout, the trajectory alone"""
    out = {f: [] for f in sr.FIELDS}
    for s, st in enumerate(sts):
        il = ora.OILQR(om, af.oracle_data(om, st, qf[s], xf[s]), H, cost_fn="ora_cost_desc_fn")
        t = il.traj()
        for f in sr.FIELDS:
            out[f].append(t[f])
    return {f: np.stack(v) for f, v in out.items()}


def _cpu_forces(name):
    """seed 0 without forces, seed 1 with qfrc_applied and xfrc_applied"""
    qf, xf = af.force_set(name)
    return np.ascontiguousarray(qf[[0, 3]]), np.ascontiguousarray(xf[[0, 3]])


@pytest.mark.parametrize("name", ("inverted_pendulum", "hopper"))
def test_restatement_composes(ia, ora, name):
    """shift(a) then shift(b) is shift(a + b), bit for bit, in every array"""
    H = 8
    m, om, sts = _cpu_setup(ia, ora, name)
    qf, xf = _cpu_forces(name)
    h = _oracle_passive(ora, om, sts, qf, xf, H)
    rng = np.random.default_rng(20261021)
    h["K"] = rng.normal(size=(2, H + 1, m.nu * 2 * m.nv))
    h["k"] = rng.normal(size=(2, H + 1, m.nu))
    h["deriv"] = rng.normal(size=(2, H + 1, m.D))
    step, sweep = sr.oracle_step(om, qf, xf), sr.oracle_sweep(ora, om, qf, xf)
    for a, b in ((1, 1), (2, 3), (5, 3)):
        two = sr.shift(sr.shift(h, a, step, sweep), b, step, sweep)
        one = sr.shift(h, a + b, step, sweep)
        exact_arrays(two, one, f"{name} shift({a}) shift({b}) vs shift({a + b})")
        for f in sr.FIELDS:
            exact(two["dinit"][f], one["dinit"][f], f"dinit.{f}")
        assert not np.any(one["K"][:, :a + b]) and not np.any(one["k"][:, :a + b])
        exact(one["deriv"][:, a + b:], h["deriv"][:, :H + 1 - a - b], "moved records")
        assert np.all(np.isfinite(one["deriv"])) and np.any(one["deriv"][:, :a + b] != 0)


@pytest.mark.parametrize("name", ("inverted_pendulum", "hopper"))
def test_restatement_is_longer_rollout(ia, ora, name):
    """after a passive rollout, shift(n) is points 0 .. N of the passive rollout of horizon N + n"""
    H = 8
    m, om, sts = _cpu_setup(ia, ora, name)
    qf, xf = _cpu_forces(name)
    h = _oracle_passive(ora, om, sts, qf, xf, H)
    step = sr.oracle_step(om, qf, xf)
    for n in (1, 2, H // 2 + 1, H):
        long = _oracle_passive(ora, om, sts, qf, xf, H + n)
        got = sr.shift(h, n, step)
        for f in sr.FIELDS:
            exact(got[f], long[f][:, :H + 1], f"{name} n={n} {f}")
            exact(got["dinit"][f], long[f][:, H], f"{name} n={n} dinit.{f}")
    assert np.any(h["qvel"][1] != h["qvel"][0])


# ---------------------------------------------------------------- GPU ----
def _states(ia, m, name):
    """two seeds started from different states"""
    import workloads
    if name == "inverted_pendulum":
        st = workloads.pendulum_dmain(m, 2)
        st.qpos[:, 1] += 0.01 * np.arange(2)
    elif name == "hopper":
        st = workloads.hopper_dmain(m, 2, sigma=0.01)
    else:
        st = m.reset_state(2)
        if name == "humanoid":
            st.qpos[:, 2] = 1.4
            st.qvel[:, 0] = 0.1 * np.arange(2)
        else:
            st.qpos[:] = 0.05 * (1 + np.arange(m.nq)) + 0.01 * np.arange(2)[:, None]
    st.ctrl[:] += 0.05 * np.arange(2)[:, None]
    return st


class Setup:
    """a model, its two states and forces, and solvers of one configuration"""

    def __init__(self, ia, name, variant=None):
        self.ia, self.name, self.variant = ia, name, variant
        self.m = af.model(ia, name)
        self.N = HORIZON[name]
        self.st = _states(ia, self.m, name)
        self.qf, self.xf = _cpu_forces(name)
        self.rows = cs.make_schedule(af.cost(ia, name), self.m, self.N) if variant == "sched" else None

    def solver(self, H=None):
        ia = self.ia
        g = af.solver(ia, self.m, self.name, self.st, self.qf, self.xf, H=H or self.N)
        v = self.variant
        if v == "f32":
            g.set_fd_precision("f32")
        if v == "sched":
            g.set_cost_schedule(self.rows)
        if v in ("corrected", "std", "reg"):
            g.set_layout("corrected")
        if v in ("std", "reg"):
            g.set_recursion("standard")
            g.set_mu(0.0)
        if v == "reg":
            g.set_regularization(REG)
        if v == "limits":
            g.set_ctrl_limits("model")
        return g

    def warmed(self):
        """a solver after two iterate(): non-trivial gains and records"""
        g = self.solver()
        g.iterate()
        g.iterate()
        g.synchronize()
        return g

    def tick_rows(self, n):
        """(the n new rows of a tick, the schedule after it)"""
        new = cs.make_schedule(af.cost(self.ia, self.name), self.m, self.N, seed=77)[:n]
        return new, np.concatenate([new, self.rows[:self.N + 1 - n]])

    def shift(self, g, n):
        """the tick: the schedule first, then the horizon"""
        if self.variant == "sched":
            g.shift_cost_schedule(self.tick_rows(n)[0], n)
        g.shift_horizon(n)

    def twin(self, want, n):
        """a solver with the same history, loaded from the host with the shifted arrays"""
        t = self.warmed()
        if self.variant == "sched":
            t.set_cost_schedule(self.tick_rows(n)[1])
        t.set_traj(sr.as_state(self.ia, want))
        t.set_gains(want["K"], want["k"])
        return t


def _ns(N):
    return sorted({1, N // 2 + 1, N})


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_longer_passive_rollout(ia, name):
    """init at horizon N then shift_horizon(n) is points 0 .. N of init at horizon N + n"""
    su = Setup(ia, name)
    N = su.N
    for n in sorted({1, 2, N // 2 + 1, N}):
        g, g2 = su.solver(), su.solver(N + n)
        g.shift_horizon(n)
        a, b = sr.solver_arrays(g), sr.solver_arrays(g2)
        for f in sr.FIELDS:
            exact(a[f], b[f][:, :N + 1], f"{name} n={n} {f}")
        assert not np.any(a["K"]) and not np.any(a["k"])
    assert np.any(a["qpos"][0] != a["qpos"][1])


def _check_against_restatement(ia, ora, su, n):
    """test 2 and 3 for one n: returns nothing, asserts everything"""
    name, N = su.name, su.N
    g = su.warmed()
    h = sr.solver_arrays(g)
    assert np.any(h["K"] != 0) and np.any(h["k"] != 0) and np.any(h["deriv"] != 0)
    before = g.reg_state() if su.variant == "reg" else None
    trace_len = len(g.reg_trace()) if su.variant == "reg" else None
    su.shift(g, n)
    got = sr.solver_arrays(g)
    # trajectory and gains: the restatement with the oracle's step and with Model.step
    m, om = af.oracle_model(ia, ora, name, su.m)
    for how, step in (("oracle", sr.oracle_step(om, su.qf, su.xf)), ("Model.step", sr.device_step(ia, su.m, su.qf, su.xf))):
        want = sr.shift(h, n, step)
        exact_arrays(got, want, f"{name}/{su.variant} n={n} vs {how}", sr.FIELDS + ("K", "k"))
    assert not np.any(got["K"][:, :n]) and not np.any(got["k"][:, :n])
    assert not np.any(np.signbit(got["K"][:, :n])) and not np.any(np.signbit(got["k"][:, :n]))
    # records: the old bits at and above n, a twin's sweep of the shifted trajectory below
    exact(got["deriv"][:, n:], h["deriv"][:, :N + 1 - n], f"{name}/{su.variant} n={n} moved records")
    twin = su.twin(want, n)
    twin.fd_sweep()
    twin.synchronize()
    exact(got["deriv"][:, :n], twin.deriv()[:, :n], f"{name}/{su.variant} n={n} tail records")
    assert np.all(np.isfinite(got["deriv"][:, :n])) and np.any(got["deriv"][:, :n] != 0)
    # state that is stale by construction
    if su.variant == "reg":
        after = g.reg_state()
        assert not np.any(after["valid"]) and np.all(before["valid"] == 1)
        for f in ("mu", "dmu", "status", "retries"):
            exact(np.asarray(after[f], dtype=np.float64), np.asarray(before[f], dtype=np.float64), f"reg {f}")
        assert len(g.reg_trace()) == trace_len
    if su.variant == "limits":
        mask, info = g.clamped()
        assert not np.any(mask) and not np.any(info)
    # ready to run: the recursion over the resident records, then iterate() from the shifted dinit
    twin.set_deriv(got["deriv"])
    g.riccati_pass()
    twin.riccati_pass()
    for f, (x, y) in dict(gains=(g.gains(), twin.gains()), value=(g.value(), twin.value())).items():
        exact(x[0], y[0], f"{name}/{su.variant} n={n} backward {f}[0]")
        exact(x[1], y[1], f"{name}/{su.variant} n={n} backward {f}[1]")
    assert np.any(g.gains()[0][:, 1:] != 0)
    twin.set_dinit(sr.dinit_state(ia, want))
    fields = af.FIELDS + (("dV", "first_bad") if su.variant in ("std", "reg") else ()) + (
        ("clamp_mask", "clamp_info") if su.variant == "limits" else ())
    for x in (None, su.st):
        if x is not None:
            g.set_dinit(x)
            twin.set_dinit(x)
        g.iterate()
        twin.iterate()
        ra, rb = af.results(g), af.results(twin)
        for f in fields:
            exact(ra[f], rb[f], f"{name}/{su.variant} n={n} iterate {'set_dinit ' if x is not None else ''}{f}")
    if su.variant == "reg":
        a, b = g.reg_state(), twin.reg_state()
        for f in a:
            exact(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64), f"reg state {f} after iterate")


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_against_restatement(ia, ora, name):
    """trajectory, gains and records after a shift; then the solver is ready to run"""
    su = Setup(ia, name)
    for n in _ns(su.N):
        _check_against_restatement(ia, ora, su, n)


@gpu
@pytest.mark.parametrize("variant", ("f32", "sched", "corrected", "std", "reg", "limits"))
def test_against_restatement_hopper_variants(ia, ora, variant):
    """the same with fp32 FD, a cost schedule (shift_cost_schedule first), the
    corrected layout, STANDARD, STANDARD + regularisation, and control limits"""
    su = Setup(ia, "hopper", variant)
    for n in _ns(su.N):
        _check_against_restatement(ia, ora, su, n)


@gpu
@pytest.mark.parametrize("name", ("hopper", "humanoid"))
def test_shifts_compose_without_sync(ia, name):
    """shift(1); shift(1); shift(2) enqueued back to back is one shift(4)"""
    su = Setup(ia, name)
    a, b = su.warmed(), su.warmed()
    for n in (1, 1, 2):
        a.shift_horizon(n)
    b.shift_horizon(4)
    exact_arrays(sr.solver_arrays(a), sr.solver_arrays(b), f"{name} 1+1+2 vs 4")


@gpu
@pytest.mark.parametrize("name", ("inverted_pendulum", "hopper"))
def test_ticks_without_host_sync(ia, name):
    """three ticks of shift_horizon(1); iterate() with no host sync between the
    calls equal the same ticks with synchronize() after every call"""
    su = Setup(ia, name)
    a, b = su.warmed(), su.warmed()
    for _ in range(3):
        a.shift_horizon(1)
        a.iterate()
    for _ in range(3):
        b.shift_horizon(1)
        b.synchronize()
        b.iterate()
        b.synchronize()
    ra, rb = af.results(a), af.results(b)
    for f in af.FIELDS:
        exact(ra[f], rb[f], f"{name} ticks {f}")


@gpu
def test_pointers_unchanged(ia):
    su = Setup(ia, "hopper")
    g = su.warmed()
    before = [g.device_traj_ptr(f) for f in sr.FIELDS] + list(g.device_deriv()) + [g.device_costs_ptr()]
    for n in (1, su.N):
        g.shift_horizon(n)
        g.synchronize()
        assert [g.device_traj_ptr(f) for f in sr.FIELDS] + list(g.device_deriv()) + [g.device_costs_ptr()] == before
    assert all(before)


@gpu
def test_seed_groups(ia):
    """hopper, set_groups(2): iterate(); shift_horizon(1); iterate() is the ungrouped solver's"""
    su = Setup(ia, "hopper")
    a, b = su.solver(), su.solver()
    a.set_groups(2)
    assert a.groups == 2
    for g in (a, b):
        g.iterate()
        g.shift_horizon(1)
        g.iterate()
    ra, rb = af.results(a), af.results(b)
    for f in af.FIELDS:
        exact(ra[f], rb[f], f"groups {f}")


@gpu
def test_arguments(ia):
    su = Setup(ia, "inverted_pendulum")
    g, fresh = su.solver(), su.solver()
    L = ia.lib()
    for n, tail in ((0, 0), (-1, 0), (su.N + 1, 0), (1, 1), (1, -1)):
        assert L.ilqg_solver_shift_horizon(g._h, n, tail) == ERR_ARG, (n, tail)
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_horizon(0)
    with pytest.raises(ia.IlqgError):
        g.shift_horizon(1, tail="zero")
    # a solver that was created but never initialised
    m = su.m
    alphas = np.ones(1)
    o = ia._Opts(horizon=su.N, nseed=2, nalpha=1, alphas=ia._ptr(alphas), select_mode=0, mu=1000.0, device=0)
    c = ia.PENDULUM_COST.struct(m.nq, m.nv, m.nu)
    h = ctypes.c_void_p()
    assert L.ilqg_solver_create(m._h, ctypes.byref(o), ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        assert L.ilqg_solver_shift_horizon(h, 1, 0) == ERR_ARG
    finally:
        L.ilqg_solver_free(h)
    # the refused calls changed nothing
    g.iterate()
    fresh.iterate()
    ra, rb = af.results(g), af.results(fresh)
    for f in af.FIELDS:
        exact(ra[f], rb[f], f"after refused calls {f}")
    # and the largest shift is accepted
    g.shift_horizon(su.N)
    g.synchronize()

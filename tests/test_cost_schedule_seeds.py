"""Per-seed cost schedules (ilqg_solver_set_cost_schedule_seeds): every seed of
a solver tracks a reference of its own.

The reference for seed s is a one-seed solver given seed s's state and seed s's
rows through the shared call (sched_seeds.against_singles), and the CPU oracle
composed piecewise with seed s's rows (cost_sched_ref.SchedRef).  Rows come from
cost_sched_ref.make_schedule with another seed per solver seed.  Every
comparison is bit for bit (tobytes() equality).
"""
import ctypes
import fnmatch
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import applied_forces as af
import cost_sched_ref as cs
import sched_seeds as ss
from sched_seeds import ALPHAS, S3, exact

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ilqg_solver_set_cost_schedule_seeds", "ilqg_solver_get_cost_schedule_seeds",
         "ilqg_solver_shift_cost_schedule_seeds")
ERR_ARG = 1


# ---------------------------------------------------------------- CPU ----
def test_header_exports_and_library(ia):
    """fails without the feature: the declarations, the export map, the binding's list, the library's symbols"""
    with open(os.path.join(ROOT, "include", "ilqg_amd.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "ilqg-mujoco_amd", "csrc", "exports.map")) as f:
        emap = f.read()
    exported = re.findall(r"([\w*?]+)\s*;", emap.split("local:")[0].split("global:")[1])
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert any(fnmatch.fnmatchcase(n, pat) for pat in exported), (n, exported)
        assert n in ia.EXPORTS
        assert hasattr(ia.lib(), n)


def test_python_methods(ia):
    for n in ("set_cost_schedule_seeds", "cost_schedule_seeds", "shift_cost_schedule_seeds"):
        assert callable(getattr(ia.ILQR, n, None)), n


def test_null_solver(ia):
    """ILQG_ERR_ARG for a null solver, before any device call"""
    L = ia.lib()
    x = np.zeros(4)
    assert L.ilqg_solver_set_cost_schedule_seeds(None, ia._ptr(x)) == ERR_ARG
    assert L.ilqg_solver_set_cost_schedule_seeds(None, None) == ERR_ARG
    assert L.ilqg_solver_get_cost_schedule_seeds(None, None, None) == ERR_ARG
    assert L.ilqg_solver_shift_cost_schedule_seeds(None, 1, ia._ptr(x)) == ERR_ARG


def test_rows_differ_by_seed(ia):
    """the rows the GPU tests hand out: another table per seed, at every point but
    make_schedule's two fixed rows (1 all zero, 2 linear terms only); weight_rows'
    weights differ wherever they are not zero"""
    m = ia.Model.load(os.path.join(ROOT, "ilqg-mujoco_amd", "models", "hopper.xml"))
    H = ss.HORIZON["hopper"]
    rows = ss.seed_rows(ia.HOPPER_COST, m, H)
    assert rows.shape == (S3, H + 1, cs.row_size(m))
    for a in range(S3):
        for b in range(a + 1, S3):
            differ = np.any(rows[a] != rows[b], axis=1)
            assert differ[0] and differ[3:].all() and not differ[1:3].any(), (a, b, differ)
    w, sl = ss.weight_rows(ia.HOPPER_COST, m, H), cs.row_slices(m)
    for x in "qvu":
        a, b = w[1][:, sl["w" + x]], w[2][:, sl["w" + x]]
        assert np.all((a != b) | ((a == 0) & (b == 0))) and np.any(a != b)


# ---------------------------------------------------------------- GPU ----
def _make(ia, m, c, H, alphas=ALPHAS, prepare=None):
    def make(st):
        g = ia.ILQR(m, st, H, c, alphas=alphas, select="min_cost" if len(alphas) > 1 else "reference")
        if prepare:
            prepare(g)
        return g
    return make


def _steps_script(rows, iters=2):
    """forward, fd_sweep, backward as three calls, then `iters` iterate()s: a snapshot after each"""
    def script(g, b):
        b.set(rows)
        g.forward_pass()
        g.fd_sweep()
        g.riccati_pass()
        out = [ss.snapshot(g)]
        for _ in range(iters):
            g.iterate()
            out.append(ss.snapshot(g))
        return out
    return script


def _iter_script(rows, iters=2):
    def script(g, b):
        b.set(rows)
        out = []
        for _ in range(iters):
            g.iterate()
            out.append(ss.snapshot(g))
        return out
    return script


_equal_runs = {}


def _equal_run(ia, name, layout):
    """test 2's runs of one model, once per session: (m, H, rows, one state, the
    S-seed solver's snapshots, the one-seed solvers' snapshots)"""
    key = (name, layout)
    if key not in _equal_runs:
        m = ss.model(ia, name)
        c, H = ss.cost(ia, name, m), ss.HORIZON[name]
        st = ss.same_state(ia, ss.states(ia, m, name))
        rows = ss.seed_rows(c, m, H)
        make = _make(ia, m, c, H, prepare=lambda g: g.set_layout(layout))
        got, singles = ss.against_singles(ia, st, make, _steps_script(rows), f"{name} {layout}")
        _equal_runs[key] = (m, H, rows, st, got, singles)
    return _equal_runs[key]


@gpu
def test_inputs_bind(ia):
    """1 (a condition): from one state, the three one-seed references differ
    pairwise in the selected cost, in cost-gradient entries of the FD records and
    in K -- a kernel that read seed 0's rows for every seed could not pass test 2"""
    m, H, rows, st, got, singles = _equal_run(ia, "hopper", "reference")
    G = 2 * m.nv * m.nv + m.nv * m.nu
    for i in range(len(got)):
        for a in range(S3):
            for b in range(a + 1, S3):
                x, y = singles[a][i], singles[b][i]
                assert x["costs"][0, x["sel"][0]] != y["costs"][0, y["sel"][0]], (i, a, b, "selected cost")
                assert np.any(x["deriv"][0, :, G:] != y["deriv"][0, :, G:]), (i, a, b, "cost gradients")
                assert np.any(x["K"][0] != y["K"][0]), (i, a, b, "K")
    # the first sweep is over one trajectory (K = k = 0): its Jacobian blocks agree, the rows alone differ
    for b in range(1, S3):
        exact(singles[0][0]["deriv"][..., :G], singles[b][0]["deriv"][..., :G], "Jacobian blocks of the first sweep")


@gpu
@pytest.mark.parametrize("name,layout", [("hopper", "reference"), ("hopper", "corrected"),
                                         ("inverted_pendulum", "reference"), ("chain", "reference"),
                                         ("ballarm", "reference")])
def test_equals_single_solvers(ia, ora, name, layout):
    """2: one state, S tables.  forward, fd_sweep, backward, then two iterate()s:
    trajectory, candidate costs, selection, FD records, K, k, V, v of seed s are
    the one-seed solver's under rows[s], and (reference layout) the composed
    oracle's: static fused sweep (hopper, pendulum), generic kernels (chain),
    ball joints (ballarm: nq != nv in the row packing)"""
    m, H, rows, st, got, singles = _equal_run(ia, name, layout)
    assert np.any(got[-1]["K"] != 0)
    if layout != "reference":
        return
    om = ora.OModel(m.blob())
    ora_iters = len(got) if name in ("hopper", "inverted_pendulum") else 2
    for s in range(S3):
        ref = cs.SchedRef(ora, m, om, af.state_dict(st, s), H, rows[s], ALPHAS)
        for i in range(ora_iters):
            c, sel = ref.iterate()
            snap, rt, ra = got[i], ref.traj(), ref.arrays()
            exact(snap["costs"][s], c, f"{name} oracle step {i} seed {s} costs")
            assert snap["sel"][s] == sel
            for f in cs.FIELDS:
                exact(snap[f][s].reshape(rt[f].shape), rt[f], f"{name} oracle step {i} seed {s} traj.{f}")
            for f in ("deriv", "K", "k", "V", "v"):
                exact(snap[f][s].reshape(ra[f].shape), ra[f], f"{name} oracle step {i} seed {s} {f}")


@gpu
def test_same_rows_equal_shared(ia):
    """3: the same table for every seed is the shared schedule, from differing seed states"""
    name = "hopper"
    m = ss.model(ia, name)
    c, H = ss.cost(ia, name, m), ss.HORIZON[name]
    st = ss.states(ia, m, name)
    rows = cs.make_schedule(c, m, H)
    a, b = _make(ia, m, c, H)(st), _make(ia, m, c, H)(st)
    a.set_cost_schedule(rows)
    b.set_cost_schedule_seeds(np.stack([rows] * S3))
    assert b.cost_schedule_seeds()[1] and not a.cost_schedule_seeds()[1]
    exact(a.cost_schedule_seeds()[0], b.cost_schedule_seeds()[0], "get: the shared rows once per seed")
    for it in range(2):
        a.iterate()
        b.iterate()
        x, y = ss.snapshot(a), ss.snapshot(b)
        for f in ss.KEYS:
            exact(x[f], y[f], f"it{it} {f}")
    assert np.any(x["K"][0] != x["K"][1])


def _differing(ia, name, rows_fn=ss.seed_rows):
    m = ss.model(ia, name)
    c, H = ss.cost(ia, name, m), ss.HORIZON[name]
    return m, c, H, ss.states(ia, m, name), rows_fn(c, m, H)


@gpu
def test_sweep_range(ia):
    """4a: ilqg_fd_sweep_range over a middle range writes the whole sweep's
    records of those points, each seed's under its own rows, and no others"""
    m, c, H, st, rows = _differing(ia, "hopper")

    def script(g, b):
        b.set(rows)
        g.forward_pass()
        g.fd_sweep()
        full = ss.snapshot(g)
        g.set_deriv(np.full_like(full["deriv"], np.nan))
        g.fd_sweep_range(3, 5)
        g.synchronize()
        D = g.deriv()
        exact(D[:, 3:8], full["deriv"][:, 3:8], "the range against the whole sweep")
        assert np.isnan(D[:, :3]).all() and np.isnan(D[:, 8:]).all()
        return [full, dict(deriv=D[:, 3:8])]
    ss.against_singles(ia, st, _make(ia, m, c, H), script, "sweep range")


@gpu
def test_fp32_sweep(ia):
    """4b: the fp32 FD sweep (test_cost_schedule.py compares it bit for bit too)"""
    m, c, H, st, rows = _differing(ia, "hopper")
    make = _make(ia, m, c, H, prepare=lambda g: g.set_fd_precision("f32"))
    got, _ = ss.against_singles(ia, st, make, _iter_script(rows), "fp32 FD")
    assert np.all(np.isfinite(got[-1]["deriv"]))


@gpu
def test_humanoid_fp32_mfma(ia):
    """4c: the humanoid at N = 6, fp32 FD and the MFMA engine (228-double rows,
    the 27-dof instances): each seed is the one-seed solver of the same settings,
    the same kernels on the same inputs, so bit for bit"""
    m, c, H, st, rows = _differing(ia, "humanoid")

    def prep(g):
        g.set_fd_precision("f32")
        g.set_riccati("mfma")
    got, _ = ss.against_singles(ia, st, _make(ia, m, c, H, alphas=(1.0,), prepare=prep), _iter_script(rows),
                                "humanoid fp32 + mfma")
    assert np.any(got[-1]["K"] != 0) and np.all(np.isfinite(got[-1]["K"]))


@gpu
def test_forward_sharded(ia, monkeypatch):
    """4d: both ranks of ilqg_forward_sharded(rank, 2) hold the full table: the
    points a rank owns carry the unsharded sweep's records, the others are untouched"""
    monkeypatch.setenv("ILQG_PIPE_CHUNK", "3")
    monkeypatch.setenv("ILQG_FUSED", "0")
    m, c, H, st, rows = _differing(ia, "hopper")
    mk = _make(ia, m, c, H, alphas=(1.0,))
    g = mk(st)
    g.set_cost_schedule_seeds(rows)
    g.forward_pass()
    g.fd_sweep()
    full = ss.snapshot(g)
    world = 2
    owner = g.point_owners(world)
    assert set(owner) == set(range(world))
    gathered = np.full_like(full["deriv"], np.nan)
    for r in range(world):
        h = mk(st)
        h.set_cost_schedule_seeds(rows)
        h.set_deriv(np.full_like(full["deriv"], np.nan))
        h.forward_sharded(r, world)
        snap, mine = ss.snapshot(h), owner == r
        exact(snap["deriv"][:, mine], full["deriv"][:, mine], f"rank {r}'s points")
        assert np.isnan(snap["deriv"][:, ~mine]).all()
        for f in ("costs", "sel") + cs.FIELDS:
            exact(snap[f], full[f], f"rank {r} {f}")
        gathered[:, mine] = snap["deriv"][:, mine]
    exact(gathered, full["deriv"], "the ranks' records together")
    # and the unsharded records are the one-seed solvers'
    for s in range(S3):
        one = mk(af.sub(ia, st, s))
        one.set_cost_schedule(rows[s])
        one.forward_pass()
        one.fd_sweep()
        exact(ss.snapshot(one)["deriv"][0], full["deriv"][s], f"seed {s} against its one-seed solver")


@gpu
def test_seed_groups(ia):
    """5: two uneven seed groups (2 + 1 seeds), each reading its own seeds' rows:
    two iterate()s equal the ungrouped per-seed run and the one-seed solvers"""
    m, c, H, st, rows = _differing(ia, "hopper")

    def grouped(g):
        if g.S > 1:
            g.set_groups(2)
            assert g.groups == 2
    got, _ = ss.against_singles(ia, st, _make(ia, m, c, H, prepare=grouped), _iter_script(rows), "seed groups")
    plain = _make(ia, m, c, H)(st)
    want = _iter_script(rows)(plain, ss.Bound(plain))
    for i, (a, b) in enumerate(zip(got, want)):
        for f in ss.KEYS:
            exact(a[f], b[f], f"grouped against ungrouped: it{i} {f}")


def _reg_prepare(g):
    g.set_layout("corrected")
    g.set_recursion("standard")
    g.set_regularization(True, trace_len=8)


def _reg_snapshot(g):
    out = ss.snapshot(g)
    dV, bad = g.expected()
    out.update(dV=dV, first_bad=bad, **{"reg_" + k: v for k, v in g.reg_state().items()})
    out["trace"] = np.ascontiguousarray(np.swapaxes(g.reg_trace(), 0, 1))  # seed-major
    return out


@gpu
def test_standard_recursion_and_regularization(ia):
    """6: rows whose weights differ per seed (lxx, luu of k_backward_std_reg read
    seed s's row), 4 iterate()s enqueued back to back: get_expected, reg_state
    and the trace columns of seed s are the one-seed solver's; the nominal cost
    reads invalid right after set_..._seeds and after shift_..._seeds"""
    m, c, H, st, rows = _differing(ia, "hopper", ss.weight_rows)
    new = ss.weight_rows(c, m, H)[:, 3:5] * 1.25

    def script(g, b):
        b.set(rows)
        for _ in range(4):
            g.iterate()
        out = [_reg_snapshot(g)]
        assert out[0]["reg_valid"].all()
        b.set(rows)
        assert not g.reg_state()["valid"].any(), "set: the nominal cost must read invalid"
        g.iterate()
        assert g.reg_state()["valid"].all()
        b.shift(2, new)
        assert not g.reg_state()["valid"].any(), "shift: the nominal cost must read invalid"
        g.iterate()
        out.append(_reg_snapshot(g))
        return out
    got, singles = ss.against_singles(ia, st, _make(ia, m, c, H, prepare=_reg_prepare), script, "standard + reg")
    assert got[0]["trace"].shape[1] == 4 and np.all(got[0]["dV"][:, 0] != 0)
    # the plain standard recursion (k_backward_std), without the mode
    def std(g):
        g.set_layout("corrected")
        g.set_recursion("standard")

    def script2(g, b):
        b.set(rows)
        out = []
        for _ in range(2):
            g.iterate()
            snap = ss.snapshot(g)
            snap["dV"], snap["first_bad"] = g.expected()
            out.append(snap)
        return out
    got2, _ = ss.against_singles(ia, st, _make(ia, m, c, H, prepare=std), script2, "standard")
    assert np.all(got2[-1]["dV"][:, 0] != 0)


@gpu
def test_ctrl_limits(ia):
    """7: the reference recursion with the model's control limits on the hopper:
    boxed gains, get_clamped and the clamped trajectory of seed s are the one-seed
    solver's.  Every seed starts from the same seeded gains, large enough for the
    rollout to run into the limits (test_ctrl_limits.py's)"""
    m, c, H, st, rows = _differing(ia, "hopper")
    lo, hi = m.ctrlrange()
    rng = np.random.default_rng(20261020)
    K0 = rng.standard_normal((1, H + 1, m.nu * 2 * m.nv)) * 5.0
    k0 = rng.standard_normal((1, H + 1, m.nu)) * 3.0

    def script(g, b):
        b.set(rows)
        g.set_gains(np.repeat(K0, g.S, 0), np.repeat(k0, g.S, 0))
        out = []
        for _ in range(2):
            g.iterate()
            snap = ss.snapshot(g)
            snap["mask"], snap["info"] = g.clamped()
            out.append(snap)
        return out
    got, _ = ss.against_singles(ia, st, _make(ia, m, c, H, prepare=lambda g: g.set_ctrl_limits("model")), script,
                                "control limits")
    for snap in got:
        assert np.all(snap["ctrl"] >= lo) and np.all(snap["ctrl"] <= hi)
    ctrl = got[0]["ctrl"]
    assert all(np.any(ctrl[s] == lo) or np.any(ctrl[s] == hi) for s in range(S3)), "the limits must bind in the rollout"
    assert any(snap["mask"].any() for snap in got), "a backward step must clamp a control"


@gpu
def test_shift_rows(ia):
    """8: shift_..._seeds(n) for n = 1 and n = N + 1 is a numpy shift of every
    seed's table; the shared shift on a per-seed table broadcasts its rows"""
    name = "inverted_pendulum"
    m = ss.model(ia, name)
    c, H = ss.cost(ia, name, m), ss.HORIZON[name]
    g = _make(ia, m, c, H)(ss.states(ia, m, name))
    rows = ss.seed_rows(c, m, H)
    new = np.stack([cs.make_schedule(c, m, H, seed=900 + s) for s in range(S3)])
    g.set_cost_schedule_seeds(rows)
    got, per = g.cost_schedule_seeds()
    assert per and g.cost_schedule_seeds()[1]
    exact(got, rows, "get")
    g.shift_cost_schedule_seeds(1, new[:, 4:5])
    want = np.concatenate([new[:, 4:5], rows[:, :-1]], axis=1)
    exact(g.cost_schedule_seeds()[0], want, "shift 1")
    g.shift_cost_schedule(new[0, 1:3], 2)
    want = np.concatenate([np.stack([new[0, 1:3]] * S3), want[:, :-2]], axis=1)
    got, per = g.cost_schedule_seeds()
    assert per
    exact(got, want, "the shared shift: the same rows to every seed")
    g.shift_cost_schedule_seeds(H + 1, new)
    exact(g.cost_schedule_seeds()[0], new, "shift by the whole window")
    # the shared call takes over, and hands back
    g.set_cost_schedule(rows[1])
    got, per = g.cost_schedule_seeds()
    assert not per
    exact(got, np.stack([rows[1]] * S3), "shared: each block reads as the shared rows")
    exact(g.cost_schedule(), rows[1], "shared get")
    g.set_cost_schedule_seeds(rows)
    assert g.cost_schedule_seeds()[1]
    g.set_cost_schedule(None)
    got, per = g.cost_schedule_seeds()
    assert not per and g.cost_schedule() is None
    exact(got, np.tile(cs.constant_schedule(c, m, H), (S3, 1, 1)), "off: each block reads as the creation cost")


@gpu
@pytest.mark.parametrize("name", ["hopper", "chain"])
def test_shift_whole_tick(ia, name):
    """9: shift_..._seeds(2), shift_horizon(2, hold), iterate(): the tail records
    are taken under each seed's rows in force, and all equals the one-seed
    solvers doing the shared tick"""
    m, c, H, st, rows = _differing(ia, name)
    new = np.stack([cs.make_schedule(c, m, H, seed=700 + s) for s in range(S3)])[:, 3:5]

    def script(g, b):
        b.set(rows)
        g.iterate()
        g.iterate()
        b.shift(2, new)
        g.shift_horizon(2, "hold")
        out = [ss.snapshot(g)]
        g.iterate()
        out.append(ss.snapshot(g))
        return out
    got, _ = ss.against_singles(ia, st, _make(ia, m, c, H), script, f"{name} tick",
                                keys=cs.FIELDS + ("deriv", "K", "k"))
    assert np.all(np.isfinite(got[0]["deriv"])) and np.any(got[0]["deriv"][:, :2] != 0)


def _results(g):
    g.synchronize()
    t = g.traj()
    return (t.qpos, t.qvel, t.ctrl, t.warm, *g.gains(), *g.value(), g.costs()[0])


@gpu
@pytest.mark.parametrize("off", ["seeds", "shared"])
def test_off_path(ia, off):
    """10: set_..._seeds(rows) then set_..._seeds(None) (or set_cost_schedule(None)):
    two iterate()s equal a fresh solver's, through the fused launch (timing index 5
    counts, index 4 does not)"""
    m, c, H, st, rows = _differing(ia, "hopper")
    g, fresh = _make(ia, m, c, H)(st), _make(ia, m, c, H)(st)
    g.set_cost_schedule_seeds(rows)
    if off == "seeds":
        g.set_cost_schedule_seeds(None)
    else:
        g.set_cost_schedule(None)
    assert g.cost_schedule() is None and not g.cost_schedule_seeds()[1]
    g.set_timing(True)
    res = []
    for s in (g, fresh):
        s.iterate()
        s.iterate()
        res.append(_results(s))
    for a, b in zip(*res):
        exact(a, b, "schedule switched off against a fresh solver")
    tm = g.timing()
    assert tm["fd_backward"][1] == 2 and tm["backward"][1] == 0, tm


@gpu
def test_arguments(ia):
    """11: refused arguments (ILQG_ERR_ARG = 1); a refused call changes nothing"""
    name = "inverted_pendulum"
    m = ss.model(ia, name)
    c, H = ss.cost(ia, name, m), ss.HORIZON[name]
    g = _make(ia, m, c, H)(ss.states(ia, m, name))
    rows = ss.seed_rows(c, m, H)
    C = rows.shape[2]
    L = ia.lib()
    ip = ctypes.POINTER(ctypes.c_int)
    per = np.zeros(1, dtype=np.int32)
    assert L.ilqg_solver_get_cost_schedule_seeds(g._h, None, None) == 0
    # shift_..._seeds while off and while shared
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule_seeds(1, rows[:, :1])
    g.set_cost_schedule(rows[0])
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule_seeds(1, rows[:, :1])
    exact(g.cost_schedule(), rows[0], "refused shift")
    g.set_cost_schedule(None)
    # non-finite rows, in the last seed's table
    for bad in (np.nan, np.inf, -np.inf):
        r = rows.copy()
        r[S3 - 1, H, C - 1] = bad
        with pytest.raises(ia.IlqgError, match="code 1"):
            g.set_cost_schedule_seeds(r)
        assert not g.cost_schedule_seeds()[1] and g.cost_schedule() is None
    g.set_cost_schedule_seeds(rows)
    # the shared getter: enabled, but no single table
    assert L.ilqg_solver_get_cost_schedule(g._h, None, per.ctypes.data_as(ip)) == 0 and per[0] == 1
    one = np.zeros((H + 1, C))
    assert L.ilqg_solver_get_cost_schedule(g._h, ia._ptr(one), per.ctypes.data_as(ip)) == ERR_ARG
    assert L.ilqg_solver_get_cost_schedule_seeds(g._h, None, per.ctypes.data_as(ip)) == 0 and per[0] == 1
    # the shift's arguments
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule_seeds(0, rows[:, :1])
    assert L.ilqg_solver_shift_cost_schedule_seeds(g._h, -1, ia._ptr(rows)) == ERR_ARG
    big = np.ascontiguousarray(np.concatenate([rows, rows[:, :1]], axis=1))
    assert L.ilqg_solver_shift_cost_schedule_seeds(g._h, H + 2, ia._ptr(big)) == ERR_ARG
    assert L.ilqg_solver_shift_cost_schedule_seeds(g._h, 1, None) == ERR_ARG
    r = np.ascontiguousarray(rows[:, :2])
    r[S3 - 1, 1, 0] = np.nan
    with pytest.raises(ia.IlqgError, match="code 1"):
        g.shift_cost_schedule_seeds(2, r)
    with pytest.raises(ia.IlqgError):
        g.set_cost_schedule_seeds(rows[:2])       # a table short
    with pytest.raises(ia.IlqgError):
        g.shift_cost_schedule_seeds(2, rows[:, :1])  # n rows per seed
    got, on = g.cost_schedule_seeds()
    assert on
    exact(got, rows, "refused calls change nothing")


@gpu
def test_arguments_dual0(ia, tmp_path):
    """11, last item: under ILQG_DUAL=0 (read once per process: a child) iterate()
    refuses a per-seed schedule with the shared schedule's ILQG_ERR_UNSUPPORTED"""
    out = str(tmp_path / "dual0.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_seeds.py"), out],
                       env=dict(os.environ, ILQG_DUAL="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        shared, seeds = f.read().splitlines()
    assert "code 4" in shared and "ILQG_DUAL=0" in shared, shared
    assert seeds == shared

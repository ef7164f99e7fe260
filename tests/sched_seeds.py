"""TEST INFRASTRUCTURE of tests/test_cost_schedule_seeds.py: models, states and
per-seed rows, a seed-major snapshot, and the one comparison every test there
makes -- a solver of S seeds under a per-seed schedule against S one-seed
solvers, each given seed s's state and seed s's rows through the shared call
(ilqg_solver_set_cost_schedule, the path test_cost_schedule.py holds to the
oracle).

Run as a program (python sched_seeds.py OUT.txt) it is the child process of
test_arguments_dual0: the rollout kernel set (ILQG_DUAL) is chosen once per
process, at the first rollout launch.
"""
import os
import sys

import numpy as np

import applied_forces as af
import cost_sched_ref as cs
from ball_models import ball_model

S3 = 3                      # odd: two seed groups are uneven (2 + 1)
ALPHAS = (1.0, 0.5, 0.25)
ROW_SEED = 20261021         # seed s's rows: make_schedule(seed=ROW_SEED + 17 s)
HORIZON = {"inverted_pendulum": 8, "hopper": 12, "chain": 6, "ballarm": 6, "humanoid": 6}
KEYS = ("costs", "sel", "time", "qpos", "qvel", "warm", "ctrl", "deriv", "K", "k", "V", "v")


def exact(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a != b)
        first = bad[0].tolist() if len(bad) else "a sign or a NaN payload"
        raise AssertionError(f"{what}: not bit for bit, {len(bad)} entries differ, first {first}")


def model(ia, name):
    return ball_model(ia, name) if name == "ballarm" else af.model(ia, name)


def cost(ia, name, m):
    if name == "ballarm":   # test_ball_joints.py's: every quaternion component weighted
        return ia.Cost(wq=0.5 + 0.25 * np.arange(m.nq), tq=0.1 * np.cos(np.arange(m.nq)),
                       lq=0.2 * np.sin(1 + np.arange(m.nq)) + 0.3, wv=[0.05] * m.nv, wu=[0.01] * m.nu)
    return af.cost(ia, name)


def states(ia, m, name, S=S3):
    """S different states, built with the device's own physics"""
    if name == "ballarm":
        st = m.reset_state(S)
        rng = np.random.default_rng(20261021)
        for a in (0, 5):    # the shoulder's and the wrist's quaternions
            q = rng.normal(size=(S, 4)) + np.array([2.0, 0, 0, 0])
            st.qpos[:, a:a + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
        st.qpos[:, 4] = 0.3 + 0.1 * np.arange(S)
        st.qvel[:] = rng.normal(0, 1.0, st.qvel.shape)
        m.step(st, 5)
        return st
    if name in ("inverted_pendulum", "hopper"):
        import workloads
        if name == "hopper":
            return workloads.hopper_dmain(m, S, sigma=0.01)
        st = workloads.pendulum_dmain(m, S)
        st.qpos[:, 1] += 0.01 * np.arange(S)
        return st
    st = m.reset_state(S)
    if name == "humanoid":
        st.qpos[:, 2] = 1.4
        st.qpos[:, 7:] += 0.02 * np.arange(S)[:, None]
        m.step(st, 5)
    else:
        st.qpos[:] = 0.05 * (1 + np.arange(m.nq)) + 0.01 * np.arange(S)[:, None]
    return st


def same_state(ia, st, S=S3):
    """seed 0's state S times: only the rows then differ between the seeds"""
    return af.sub(ia, st, [0] * S)


def seed_rows(c, m, H, S=S3):
    """(S, H + 1, C): a schedule of its own per seed"""
    return np.stack([cs.make_schedule(c, m, H, seed=ROW_SEED + 17 * s) for s in range(S)])


def weight_rows(c, m, H, S=S3):
    """seed_rows with seed s's weights scaled by 1 + s / 2 on top: the cost
    Hessians lxx, luu differ by seed at every point, the zero weights stay zero"""
    rows, sl = seed_rows(c, m, H, S), cs.row_slices(m)
    for s in range(S):
        for x in "qvu":
            rows[s][:, sl["w" + x]] *= 1.0 + 0.5 * s
    return rows


def snapshot(g):
    """every result of the solver, seed-major"""
    g.synchronize()
    S, P = g.S, g.P
    t, (K, k), (V, v), (c, sel) = g.traj(), g.gains(), g.value(), g.costs()
    out = {f: getattr(t, f).reshape(S, P, -1).copy() for f in cs.FIELDS}
    out.update(costs=c, sel=sel, deriv=g.deriv(), K=K, k=k, V=V, v=v)
    return out


class Bound:
    """the schedule calls of one solver: the S-seed solver takes the whole table
    through the _seeds calls (s is None), a one-seed solver seed s's part of the
    same arguments through the shared calls"""

    def __init__(self, g, s=None):
        self.g, self.s = g, s

    def set(self, rows):
        if self.s is None:
            self.g.set_cost_schedule_seeds(rows)
        else:
            self.g.set_cost_schedule(rows[self.s])

    def shift(self, n, new):
        if self.s is None:
            self.g.shift_cost_schedule_seeds(n, new)
        else:
            self.g.shift_cost_schedule(new[self.s], n)


def against_singles(ia, st, make, script, what, keys=None):
    """script(g, Bound) -> a list of seed-major dicts, run on make(st) and on
    make(seed s's state) for every seed: entry s of the former is entry 0 of the
    latter, bit for bit.  -> (the S-seed solver's list, [the one-seed lists])"""
    S = st.qpos.shape[0]
    g = make(st)
    got = script(g, Bound(g))
    singles = []
    for s in range(S):
        h = make(af.sub(ia, st, s))
        want = script(h, Bound(h, s))
        assert len(want) == len(got)
        for i, (a, b) in enumerate(zip(got, want)):
            for f in keys or b:
                exact(a[f][s], b[f][0], f"{what}: step {i}, seed {s}, {f}")
        singles.append(want)
    return got, singles


# ------------------------------------------------------------------ the child process
def _main(path):
    """what iterate() answers under a shared and under a per-seed schedule, one line each"""
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import conftest  # noqa: F401  (the package's and the oracle's directories)
    import ilqg_amd as ia
    name = "inverted_pendulum"
    m = model(ia, name)
    c, H = cost(ia, name, m), HORIZON[name]
    rows = seed_rows(c, m, H)
    lines = []
    for per_seed in (False, True):
        g = ia.ILQR(m, states(ia, m, name), H, c, alphas=ALPHAS, select="min_cost")
        if per_seed:
            g.set_cost_schedule_seeds(rows)
        else:
            g.set_cost_schedule(rows[0])
        try:
            g.iterate()
            g.synchronize()
            lines.append("ran")
        except ia.IlqgError as e:
            lines.append(str(e).replace("\n", " "))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    _main(sys.argv[1])

"""Reference of the cost schedule (ilqg_solver_set_cost_schedule): iterate()
with one cost row per trajectory point, composed piecewise from the oracle
(nothing under oracle/ changes):

  rollout   the oracle's forward_candidates loop restated per candidate -- the
            oracle's state difference, the control law in sequential doubles,
            an optional clamp, the oracle's mj_step -- each point n charged with
            ora_cost_eval_desc(row n) on the recorded state, summed in a Python
            float in n = N..0 order from 0.0;
  records   per point p: ora_set_cost_desc(row p), then ora_ilqr_fd_point(s, p);
  recursion OILQR.backward_from_records.

With every row equal to one cost this is OILQR.iterate_ls bit for bit
(test_cost_schedule.py::test_reference_is_iterate_ls), which pins the
composition itself.  Also the deterministic schedule the tests run.
"""
import ctypes

import numpy as np

_dp = ctypes.POINTER(ctypes.c_double)
FIELDS = ("time", "qpos", "qvel", "warm", "ctrl")


def row_size(m):
    return 3 * (m.nq + m.nv + m.nu)


def row_slices(m):
    """the nine arrays of a packed row: name -> slice, in Cost.packed's order"""
    out, o = {}, 0
    for x, n in (("q", m.nq), ("v", m.nv), ("u", m.nu)):
        for a in ("w", "t", "l"):
            out[a + x] = slice(o, o + n)
            o += n
    return out


def desc_from_row(ora, m, row):
    c = ora.CostDesc()
    c.nq, c.nv, c.nu = m.nq, m.nv, m.nu
    for name, sl in row_slices(m).items():
        arr = getattr(c, name)
        for i, x in enumerate(row[sl]):
            arr[i] = float(x)
    return c


def constant_schedule(cost, m, N):
    return np.tile(cost.row(m.nq, m.nv, m.nu), (N + 1, 1))


def make_schedule(cost, m, N, seed=20261020):
    """(N+1, C) rows around `cost`: weights >= 0 with exact zeros scattered in,
    targets that move with the point, sparse linear terms of both signs; row 1
    all zero, row 2 linear terms only, row 0 (the terminal cost) ten times
    heavier.  Deterministic: workloads.normals."""
    import workloads
    P, C, sl = N + 1, row_size(m), row_slices(m)
    base = cost.row(m.nq, m.nv, m.nu)
    z = workloads.normals(seed, 5 * P * C).reshape(5, P, C)
    rows = np.zeros((P, C))
    for p in range(P):
        for x in "qvu":
            w, t, l = sl["w" + x], sl["t" + x], sl["l" + x]
            wt = (base[w] + 0.2) * (0.5 + np.abs(z[0, p, w]))
            wt[z[1, p, w] < -0.7] = 0.0
            rows[p, w] = wt
            rows[p, t] = base[t] + 0.1 * np.sin(0.7 * p + np.arange(t.stop - t.start)) + 0.01 * z[2, p, t]
            rows[p, l] = np.where(z[3, p, l] > 0.8, 0.05 * z[4, p, l], 0.0)
    for x in "qvu":
        rows[0, sl["w" + x]] *= 10.0
    if P > 2:
        rows[1] = 0.0
    if P > 3:
        for x in "qvu":
            rows[2, sl["w" + x]] = 0.0
            rows[2, sl["t" + x]] = 0.0
            n = sl["l" + x].stop - sl["l" + x].start
            rows[2, sl["l" + x]] = 0.05 * (1 + np.arange(n)) * np.where(np.arange(n) % 2, -1.0, 1.0)
    assert np.all(np.isfinite(rows))
    return rows


class SchedRef:
    """the composed reference solver of one seed"""

    def __init__(self, ora, m, om, dstate, N, rows, alphas=(1.0,), select="min_cost", lo=None, hi=None):
        self.ora, self.m, self.om, self.N = ora, m, om, N
        self.rows = np.array(rows, dtype=np.float64)
        assert self.rows.shape == (N + 1, row_size(m))
        self.alphas, self.select = tuple(float(a) for a in alphas), select
        self.lo, self.hi = lo, hi
        L = om.lib.L
        L.ora_cost_eval_desc.restype = ctypes.c_double
        L.ora_cost_eval_desc.argtypes = [ctypes.POINTER(ora.CostDesc), _dp, _dp, _dp]
        self.desc = [desc_from_row(ora, m, r) for r in self.rows]
        L.ora_set_cost_desc(self.desc[0])
        d = om.make_data()
        d.set_state(**dstate)
        self.il = ora.OILQR(om, d, N, cost_fn="ora_cost_desc_fn")
        self.il.set_dinit(d)
        self.costs, self.sel, self.clamped = None, None, 0

    def _dinit(self):
        class S(ctypes.Structure):
            _fields_ = [("m", ctypes.c_void_p), ("N", ctypes.c_int), ("nv", ctypes.c_int), ("nu", ctypes.c_int),
                        ("nx", ctypes.c_int), ("D", ctypes.c_int), ("d", ctypes.c_void_p)]
        return ctypes.cast(self.il.s, ctypes.POINTER(S)).contents.d

    def point_cost(self, n, qpos, qvel, ctrl):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (qpos, qvel, ctrl)]
        return float(self.om.lib.L.ora_cost_eval_desc(self.desc[n], *(x.ctypes.data_as(_dp) for x in a)))

    def rollout(self, alpha):
        """one candidate: (records per point, cost, controls the clamp changed)"""
        m, om, il, N = self.m, self.om, self.il, self.N
        nu, nx = m.nu, 2 * m.nv
        nom = il.traj()
        oa = il.arrays()
        K, k = oa["K"], oa["k"]
        d = om.make_data()
        om.lib.L.ora_cpMjData(om.m, d.d, self._dinit())
        rec = {f: [None] * (N + 1) for f in FIELDS + ("qacc",)}
        c, hit = 0.0, 0
        for n in range(N, -1, -1):
            dx = self.ora.state_diff(om, d.arr("qpos"), d.arr("qvel"), nom["qpos"][n], nom["qvel"][n])
            u = np.zeros(nu)
            for i in range(nu):
                t = 0.0
                for j in range(nx):
                    t += float(K[n, i + j * nu]) * float(dx[j])
                cv = (t + alpha * float(k[n, i])) + float(nom["ctrl"][n, i])
                if self.lo is not None:
                    lo, hi = float(self.lo[i]), float(self.hi[i])
                    hit += bool(cv < lo or cv > hi)
                    cv = lo if cv < lo else (hi if cv > hi else cv)
                u[i] = cv
            d.arr("ctrl")[:] = u
            s = d.state()
            for f in FIELDS:
                rec[f][n] = s[f]
            rec["qacc"][n] = d.arr("qacc").copy()
            c += self.point_cost(n, s["qpos"], s["qvel"], s["ctrl"])
            d.step()
        return rec, c, hit

    def forward(self):
        """every candidate, selection, the selected records into dArray, setDInit(dArray[N])"""
        cands = [self.rollout(a) for a in self.alphas]
        costs = np.array([c for _, c, _ in cands])
        best = 0
        if self.select == "min_cost":
            bc = costs[0]
            for a in range(1, len(costs)):
                if costs[a] < bc or (bc != bc and costs[a] == costs[a]):
                    bc, best = costs[a], a
        rec = cands[best][0]
        for n in range(self.N + 1):
            pt = self.il.point(n)
            pt.set_state(time=rec["time"][n], qpos=rec["qpos"][n], qvel=rec["qvel"][n], warm=rec["warm"][n],
                         ctrl=rec["ctrl"][n])
            pt.arr("qacc")[:] = rec["qacc"][n]
        self.il.set_dinit(self.il.point(self.N))
        self.costs, self.sel, self.clamped = costs, best, cands[best][2]
        self.cand_ctrl = [np.array(r["ctrl"]) for r, _, _ in cands]
        return costs, best

    def sweep(self):
        """the FD record of every point under its own row"""
        L = self.om.lib.L
        for p in range(self.N + 1):
            L.ora_set_cost_desc(self.desc[p])
            L.ora_ilqr_fd_point(self.il.s, p)
        L.ora_set_cost_desc(self.desc[0])
        return self.il.arrays()["deriv"]

    def backward(self, V0=None, v0=None):
        self.il.backward_from_records(self.sweep(), V0, v0)

    def iterate(self):
        out = self.forward()
        self.backward()
        return out

    def traj(self):
        return self.il.traj()

    def arrays(self):
        return self.il.arrays()

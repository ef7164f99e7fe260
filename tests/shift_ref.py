"""Reference of the horizon shift (ilqg_solver_shift_horizon): a numpy
restatement of its four steps on host arrays, and the step functions that
drive its tail.  Not collected.

A solver's arrays are seed-major, h[f] of shape (S, P, ...): the trajectory's
five fields (time (S, P); qpos, qvel, warm, ctrl), K (S, P, nu * 2nv), k
(S, P, nu) and deriv (S, P, D).  Point N = P - 1 is now, point 0 terminal.

  shift(h, n, step, sweep)
    1. move     every array's point p takes point p - n, p = N .. n
    2. tail     points n-1 .. 0: from new point n, one step(s, state) with the
                stored ctrl[n] per point, the state after it stored with
                ctrl[n] held; K = 0 and k = 0 below n
    3. records  deriv of points < n from sweep(s, p, state), or NaN without one
    4. dinit    out["dinit"][f] = new point N

step(s, state) -> state is one mj_step of seed s (its applied forces) from a
state dict (time, qpos, qvel, warm, ctrl): oracle_step (the oracle's mj_step)
or device_step (Model.step, i.e. ilqg_step_batch).
"""
import numpy as np

FIELDS = ("time", "qpos", "qvel", "warm", "ctrl")
ARRAYS = FIELDS + ("K", "k", "deriv")


def bits_equal(a, b):
    """same shape and the same 64-bit patterns (NaN payloads and signed zeros count)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def shift(h, n, step, sweep=None):
    S, P = h["qpos"].shape[:2]
    N = P - 1
    assert 1 <= n <= N
    names = [f for f in ARRAYS if f in h]
    out = {f: np.array(h[f], dtype=np.float64, copy=True) for f in names}
    for f in names:
        for p in range(N, n - 1, -1):
            out[f][:, p] = h[f][:, p - n]
    for s in range(S):
        st = {f: np.copy(out[f][s, n]) for f in FIELDS}
        for p in range(n - 1, -1, -1):
            u = np.copy(st["ctrl"])
            st = dict(step(s, st))
            st["ctrl"] = u
            for f in FIELDS:
                out[f][s, p] = st[f]
            if "deriv" in out:
                out["deriv"][s, p] = sweep(s, p, st) if sweep else np.nan
    for f in ("K", "k"):
        if f in out:
            out[f][:, :n] = 0.0
    out["dinit"] = {f: np.copy(out[f][:, N]) for f in FIELDS}
    return out


def oracle_step(om, qf, xf):
    """step(s, state) with the oracle's mj_step; qf (S, nv), xf (S, nbody, 6) or None"""
    data = {}

    def step(s, st):
        if s not in data:
            d = om.make_data()
            d.arr("qfrc_applied")[:] = 0.0 if qf is None else qf[s]
            d.xfrc()[:] = 0.0 if xf is None else np.ravel(xf[s])
            data[s] = d
        d = data[s]
        d.set_state(**{f: st[f] for f in FIELDS})
        d.step()
        return d.state()
    return step


def device_step(ia, m, qf, xf):
    """step(s, state) with Model.step (ilqg_step_batch), one state per call"""
    def step(s, st):
        b = ia.State(np.array([st["time"]]), st["qpos"][None], st["qvel"][None], st["warm"][None], st["ctrl"][None])
        m.step(b, 1, qfrc_applied=None if qf is None else qf[s:s + 1], xfrc_applied=None if xf is None else xf[s:s + 1])
        return dict(time=b.time[0], qpos=b.qpos[0], qvel=b.qvel[0], warm=b.warm[0], ctrl=b.ctrl[0])
    return step


def oracle_sweep(ora, om, qf, xf, cost_fn="ora_cost_desc_fn"):
    """sweep(s, p, state): the oracle's calcMJDerivatives at the state under the installed cost"""
    def sweep(s, p, st):
        d = om.make_data()
        d.set_state(**{f: st[f] for f in FIELDS})
        d.arr("qfrc_applied")[:] = 0.0 if qf is None else qf[s]
        d.xfrc()[:] = 0.0 if xf is None else np.ravel(xf[s])
        return ora.calc_derivatives(om, d, cost_fn=cost_fn, nthread=1)
    return sweep


def solver_arrays(g):
    """a synchronised solver's arrays in shift()'s layout"""
    g.synchronize()
    S, P = g.S, g.P
    t = g.traj()
    K, k = g.gains()
    return dict(time=t.time.reshape(S, P), qpos=t.qpos.reshape(S, P, -1), qvel=t.qvel.reshape(S, P, -1),
                warm=t.warm.reshape(S, P, -1), ctrl=t.ctrl.reshape(S, P, -1), K=K, k=k, deriv=g.deriv())


def as_state(ia, h):
    """the trajectory of shift()'s layout as the State that set_traj takes"""
    S, P = h["qpos"].shape[:2]
    return ia.State(h["time"].reshape(S * P), h["qpos"].reshape(S * P, -1), h["qvel"].reshape(S * P, -1),
                    h["warm"].reshape(S * P, -1), h["ctrl"].reshape(S * P, -1))


def dinit_state(ia, h):
    """point N of every seed as the State that set_dinit takes"""
    return ia.State(h["time"][:, -1], h["qpos"][:, -1], h["qvel"][:, -1], h["warm"][:, -1], h["ctrl"][:, -1])

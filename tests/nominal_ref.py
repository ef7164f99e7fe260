"""Reference of the nominal refresh (ilqg_solver_refresh_nominal): the cost of a
stored trajectory under one cost row per point, in plain Python floats and in
the order the rollout charges a candidate.  A helper: not collected.

    c = 0
    for n = N .. 0:                       (point N first, the terminal point last)
        s = 0
        for x in (qpos_n, qvel_n, ctrl_n), index ascending, with the row's w, t, l:
            w_i != 0:  dx = x_i - t_i;  s += (w_i dx) dx
            l_i != 0:  s += l_i x_i
        c += s

A point's subtotal is formed from 0 before it is added: the sum is not
associative and the device forms it the same way.
"""
import numpy as np


def point_cost(row, qpos, qvel, ctrl):
    """one point under one packed row (wq tq lq wv tv lv wu tu lu)"""
    s, o = 0.0, 0
    for x in (qpos, qvel, ctrl):
        k = len(x)
        w, t, l = row[o:o + k], row[o + k:o + 2 * k], row[o + 2 * k:o + 3 * k]
        o += 3 * k
        for i in range(k):
            xi = float(x[i])
            if w[i] != 0:
                dx = xi - float(t[i])
                s += (float(w[i]) * dx) * dx
            if l[i] != 0:
                s += float(l[i]) * xi
    assert o == len(row)
    return s


def traj_cost(rows, qpos, qvel, ctrl):
    """rows: (N+1, C), one creation-cost row repeated or a schedule; qpos, qvel,
    ctrl: (N+1, nq / nv / nu), point 0 the terminal one"""
    rows, qpos, qvel, ctrl = (np.asarray(a, dtype=np.float64) for a in (rows, qpos, qvel, ctrl))
    P = qpos.shape[0]
    assert rows.shape[0] == P and qvel.shape[0] == P and ctrl.shape[0] == P
    c = 0.0
    for n in range(P - 1, -1, -1):
        c += point_cost(rows[n], qpos[n], qvel[n], ctrl[n])
    return c

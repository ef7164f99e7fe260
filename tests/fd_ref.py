"""TEST INFRASTRUCTURE: independent finite-difference derivative records on top of
tests/rigid_ref.py, in the dtype the Ref was made with (np.longdouble for the
reference, float64 to measure the reference's own rounding).  It calls neither
the oracle nor the product.

A state is a dict with q, v, ctrl, qf (or None), xf (or None) and contact (bool).
The record is calcMJDerivatives' (mjderivative.cpp:43-209), D = nv (2 nv + nu) + 2 nv + nu:

  deriv[c + r nv]                    d qacc_r / d qpos_c   central, tangent space
  deriv[nv nv + c + r nv]            d qacc_r / d qvel_c   central
  deriv[2 nv nv + a + r nu]          d qacc_r / d ctrl_a   central
  deriv[nv (2 nv + nu) + ...]        cost columns: qpos (nv), qvel (nv), ctrl (nu), forward

A qpos column steps in the tangent space: a slide, a hinge and a free joint's
position by a plain add, a ball or free rotation dof by quat (x) exp(+-eps e_k),
the rotation vector in the body frame (Ref.integrate_pos).  frame="world" and
drop_xf=True are deliberately wrong variants; only the sensitivity test of
tests/test_fd_reference.py uses them.
"""
import numpy as np

import mjcf_indep as mi

BLOCKS = ("dq", "dv", "du", "cost")


def block_slices(nv, nu):
    a, b, c = nv * nv, 2 * nv * nv, nv * (2 * nv + nu)
    return dict(dq=slice(0, a), dv=slice(a, b), du=slice(b, c), cost=slice(c, c + 2 * nv + nu))


def qacc(R, s, q=None, v=None, ctrl=None, drop_xf=False):
    """the acceleration at the state, any of q, v, ctrl replaced: the unconstrained one of
    an airborne state, the minimiser of the constraint problem of a contact state"""
    q = s["q"] if q is None else q
    v = s["v"] if v is None else v
    ctrl = s["ctrl"] if ctrl is None else ctrl
    xf = None if drop_xf else s.get("xf")
    if not s["contact"]:
        return R.forward(q, v, ctrl, s.get("qf"), xf).qacc_smooth
    return R.minimise(R.problem(q, v, ctrl, s.get("qf"), xf))


def _unit(R, n, i):
    e = np.zeros(n, dtype=R.dt)
    e[i] = 1
    return e


def step_q(R, q, i, h, frame="body"):
    """q moved by h along dof i of the tangent space"""
    if frame == "body":
        return R.integrate_pos(q, _unit(R, R.nv, i), R.dt(h))
    # the wrong convention: the rotation vector in the parent's (a free joint: the world's) frame
    assert frame == "world"
    q = R.T(q).copy()
    for ji, j in enumerate(R.C.joints):
        qa, da = R.jq[ji], R.jd[ji]
        if j["type"] == "free":
            qa, da = qa + 3, da + 3
        if j["type"] in ("free", "ball") and da <= i < da + 3:
            quat = q[qa:qa + 4] / np.sqrt(q[qa:qa + 4] @ q[qa:qa + 4])
            half = R.dt(h) / 2
            ex = np.concatenate([[np.cos(half)], np.sin(half) * _unit(R, 3, i - da)]).astype(R.dt)
            q[qa:qa + 4] = mi.qmul(ex, quat)
            return q
    return R.integrate_pos(q, _unit(R, R.nv, i), R.dt(h))


def dyn_blocks(R, s, eps, frame="body", drop_xf=False):
    """(dq, dv, du) flattened in the record's layout, by central differences of qacc"""
    nv, nu, h = R.nv, len(R.C.act), R.dt(eps)
    dq, dv = np.zeros((nv, nv), dtype=R.dt), np.zeros((nv, nv), dtype=R.dt)
    du = np.zeros((nv, nu), dtype=R.dt)
    v0, u0 = R.T(s["v"]), R.T(s["ctrl"])
    for i in range(nv):
        dq[:, i] = (qacc(R, s, q=step_q(R, s["q"], i, h, frame), drop_xf=drop_xf)
                    - qacc(R, s, q=step_q(R, s["q"], i, -h, frame), drop_xf=drop_xf)) / (2 * h)
        e = _unit(R, nv, i)
        dv[:, i] = (qacc(R, s, v=v0 + h * e, drop_xf=drop_xf) - qacc(R, s, v=v0 - h * e, drop_xf=drop_xf)) / (2 * h)
    for a in range(nu):
        e = _unit(R, nu, a)
        du[:, a] = (qacc(R, s, ctrl=u0 + h * e, drop_xf=drop_xf)
                    - qacc(R, s, ctrl=u0 - h * e, drop_xf=drop_xf)) / (2 * h)
    return dq.ravel(), dv.ravel(), du.ravel()     # row-major: entry (r, c) at c + r ncol


def split_cost_row(R, cost_row):
    """a cost row (wq tq lq wv tv lv wu tu lu, ilqg_amd.Cost.row) as ((w, t, l) of qpos, of qvel, of ctrl)"""
    nq, nv, nu = R.nq, R.nv, len(R.C.act)
    row = R.T(cost_row)
    assert row.shape == (3 * (nq + nv + nu),)
    out, at = [], 0
    for n in (nq, nv, nu):
        out.append((row[at:at + n], row[at + n:at + 2 * n], row[at + 2 * n:at + 3 * n]))
        at += 3 * n
    return out


def step_cost(R, cost_row, q, v, ctrl):
    """sum w (x - t)^2 + l x over qpos, qvel and ctrl (the raw control, not the clipped one)"""
    c = R.dt(0)
    for (w, t, l), x in zip(split_cost_row(R, cost_row), (R.T(q), R.T(v), R.T(ctrl))):
        c = c + w @ ((x - t) ** 2) + l @ x
    return c


def cost_columns(R, cost_row, s, eps, frame="body"):
    """(c(x (+) eps e_i) - c(x)) / eps in the record's order: qpos (nv), qvel (nv), ctrl (nu)"""
    nv, nu, h = R.nv, len(R.C.act), R.dt(eps)
    q0, v0, u0 = R.T(s["q"]), R.T(s["v"]), R.T(s["ctrl"])
    c0 = step_cost(R, cost_row, q0, v0, u0)
    out = np.zeros(2 * nv + nu, dtype=R.dt)
    for i in range(nv):
        out[i] = (step_cost(R, cost_row, step_q(R, q0, i, h, frame), v0, u0) - c0) / h
        out[nv + i] = (step_cost(R, cost_row, q0, v0 + h * _unit(R, nv, i), u0) - c0) / h
    for a in range(nu):
        out[2 * nv + a] = (step_cost(R, cost_row, q0, v0, u0 + h * _unit(R, nu, a)) - c0) / h
    return out


def record(R, cost_row, s, eps, frame="body", drop_xf=False):
    """the full record, D = nv (2 nv + nu) + 2 nv + nu"""
    return np.concatenate(dyn_blocks(R, s, eps, frame, drop_xf) + (cost_columns(R, cost_row, s, eps, frame),))


def rows(R, q):
    """the constraint rows at q: (kind, where, sign of dist) of the limit rows, then of
    the contacts in pair order, as Ref.problem lists them"""
    out = [("limit", (ji, side), bool(dist > 0)) for ji, side, dist in R.limit_rows(q)]
    out += [(c["kind"], (c["g1"], c["g2"]), bool(c["dist"] > 0)) for c in R.contacts(q)[0]]
    return out


def same_active_set(R, s, eps):
    """a condition on the reference alone: at every +-eps step of a qpos dof the list of
    constraint rows (kinds, geom pairs, limit joints and sides, in order) is the centre's and
    no row's dist changes sign.  qvel and ctrl steps move no geometry, so their rows are the
    centre's by construction."""
    centre = rows(R, s["q"])
    for i in range(R.nv):
        for sg in (1, -1):
            if rows(R, step_q(R, s["q"], i, sg * eps)) != centre:
                return False
    return True

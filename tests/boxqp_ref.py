"""Box-constrained Riccati step in np.longdouble: the reference of
tests/test_ctrl_limits.py.  A helper: not collected.

The boxed step minimises  1/2 k'H k + g'k  over  bl <= k <= bh  with H = -Mm
(Mm = -2 B'VsB - 2 r r', what the device's stage 3 builds) and g = B'w + r.
solve() ENUMERATES all 3^nu active sets (every control free, at lo or at hi),
solves the free block of each by Gaussian elimination and keeps the one that
satisfies the KKT conditions -- no projected Newton, no line search, so it
shares nothing with the device's iteration (or with newton() below, the plain
restatement of Tassa, Mansard & Todorov 2014 it is checked against).

recursion() is ora_riccati_step's loops (tests/riccati_cases.py step_inputs
and the closed-loop value update, oracle/ilqr_ora.c) in longdouble with this
solve in place of the LDLT solve; with infinite bounds it is the unconstrained
recursion, which measures the exact engine's own rounding (E0)."""
from itertools import product

import numpy as np

LD = np.longdouble


def gauss_solve(M, R):
    """M X = R by Gaussian elimination with partial pivoting (numpy.linalg has no longdouble)"""
    M = np.array(M, dtype=LD)
    R = np.array(R, dtype=LD)
    vec = R.ndim == 1
    if vec:
        R = R[:, None]
    n = M.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            R[[k, p]] = R[[p, k]]
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:] -= f[:, None] * M[k]
        R[k + 1:] -= f[:, None] * R[k]
    X = np.zeros_like(R)
    for k in range(n - 1, -1, -1):
        X[k] = (R[k] - M[k, k + 1:] @ X[k + 1:]) / M[k, k]
    return X[:, 0] if vec else X


def _active_solve(H, g, bl, bh, st):
    """the stationary point of active set st (0 free, 1 at lo, 2 at hi), or None when a bound it uses is infinite"""
    n = len(g)
    k = np.zeros(n, dtype=LD)
    for a in range(n):
        if st[a]:
            k[a] = bl[a] if st[a] == 1 else bh[a]
            if not np.isfinite(k[a]):
                return None
    fr = [a for a in range(n) if not st[a]]
    if fr:
        cl = [a for a in range(n) if st[a]]
        rhs = -g[fr] - (H[np.ix_(fr, cl)] @ k[cl] if cl else 0)
        k[fr] = gauss_solve(H[np.ix_(fr, fr)], rhs)
    return k


def solve(H, g, bl, bh):
    """-> k, state (nu ints: 0 free, 1 at lo, 2 at hi), margin.  margin is the
    smallest of: each clamped control's multiplier (the gradient's component
    pointing out of the box) and each free control's distance to either bound --
    positive exactly for the KKT point, and a measure of how far the step is
    from a degenerate one.  Every active set is visited; the one with the
    largest margin wins (H positive definite: at most one is positive)."""
    H, g, bl, bh = (np.asarray(x, dtype=LD) for x in (H, g, bl, bh))
    n = len(g)
    best = None
    for st in product(range(3), repeat=n):
        k = _active_solve(H, g, bl, bh, st)
        if k is None:
            continue
        grad = H @ k + g
        mg = LD(np.inf)
        for a in range(n):
            if st[a] == 1:
                mg = min(mg, grad[a])
            elif st[a] == 2:
                mg = min(mg, -grad[a])
            else:
                mg = min(mg, k[a] - bl[a], bh[a] - k[a])
        if best is None or mg > best[2]:
            best = (k, np.array(st), mg)
    return best


def newton(H, g, bl, bh, maxit=100):
    """projected Newton (Tassa, Mansard & Todorov 2014, plainly): from the
    clamped unconstrained minimiser; the clamped set is the controls at a bound
    whose gradient points outward; a Newton step on the free block; Armijo
    backtracking with projection.  -> k, state, iterations"""
    H, g, bl, bh = (np.asarray(x, dtype=LD) for x in (H, g, bl, bh))
    n = len(g)
    f = lambda x: x @ (H @ x) / 2 + g @ x
    x = np.clip(gauss_solve(H, -g), bl, bh)
    prev = None
    for it in range(maxit):
        grad = H @ x + g
        lo = (x == bl) & (grad > 0)
        hi = (x == bh) & (grad < 0)
        cl = lo | hi
        st = np.where(lo, 1, np.where(hi, 2, 0))
        if cl.all() or (prev is not None and np.array_equal(st, prev[0]) and prev[1]):
            return x, st, it
        fr = ~cl
        xt = x.copy()
        xt[fr] = gauss_solve(H[np.ix_(fr, fr)], -g[fr] - H[np.ix_(fr, cl)] @ x[cl])
        step, f0 = LD(1), f(x)
        while True:
            xc = np.clip(xt if step == 1 else x + step * (xt - x), bl, bh)
            if f(xc) - f0 <= LD(0.1) * (grad @ (xc - x)):
                break
            step *= LD(0.6)
            assert step > 1e-12, "line search"
        prev = (st, bool(step == 1 and np.array_equal(xc, xt)))
        x = xc
    raise AssertionError("projected Newton did not converge")


def kkt_residual(H, g, bl, bh, k, st):
    """largest violation of stationarity on the free controls, of the bounds, and of the multipliers' signs"""
    H, g, bl, bh, k = (np.asarray(x, dtype=LD) for x in (H, g, bl, bh, k))
    grad = H @ k + g
    r = LD(0)
    for a in range(len(g)):
        if st[a] == 0:
            r = max(r, abs(grad[a]), bl[a] - k[a], k[a] - bh[a])
        elif st[a] == 1:
            r = max(r, abs(k[a] - bl[a]), -grad[a])
        else:
            r = max(r, abs(k[a] - bh[a]), grad[a])
    return r


def assemble_AB(rec, nv, nu, dt, layout):
    """Differentiator::updateDerivatives in the reference (0) or corrected (1) layout (ilqg_amd.assemble_AB)"""
    rec = np.asarray(rec, dtype=LD)
    order = "C" if layout else "F"
    nx, nn = 2 * nv, nv * nv
    A = np.zeros((nx, nx), dtype=LD)
    A[:nv, :nv] = np.eye(nv)
    A[:nv, nv:] = np.eye(nv) * LD(dt)
    A[nv:, :nv] = rec[:nn].reshape(nv, nv, order=order) * LD(dt)
    A[nv:, nv:] = np.eye(nv) + rec[nn:2 * nn].reshape(nv, nv, order=order) * LD(dt)
    B = np.zeros((nx, nu), dtype=LD)
    B[nv:] = rec[2 * nn:2 * nn + nv * nu].reshape(nv, nu, order=order) * LD(dt)
    return A, B


def step(rec, nv, nu, dt, mu, V, v, c, ustar, lo, hi, layout=0):
    """one backward step -> dict(K (nu, nx), k, V, v, state, margin, scale, kunc, and the QP's H, g)"""
    nx = 2 * nv
    A, B = assemble_AB(rec, nv, nu, dt, layout)
    rec = np.asarray(rec, dtype=LD)
    o = 2 * nv * nv + nv * nu
    q, r = rec[o:o + nx], rec[o + nx:o + nx + nu]
    V, v, c = (np.asarray(x, dtype=LD) for x in (V, v, c))
    Vs = (V + V.T) / 2 + LD(mu) * np.eye(nx, dtype=LD)
    T1 = B.T @ Vs
    R = np.outer(r, r)
    Mm = -2 * (T1 @ B) - 2 * R
    T3 = T1 @ A
    w = v + 2 * (Vs @ c)
    g = B.T @ w + r
    H = -Mm
    bl = np.asarray(lo, dtype=LD) - np.asarray(ustar, dtype=LD)
    bh = np.asarray(hi, dtype=LD) - np.asarray(ustar, dtype=LD)
    kunc = gauss_solve(H, -g)
    k, st, mg = solve(H, g, bl, bh)
    fr = [a for a in range(nu) if not st[a]]
    K = np.zeros((nu, nx), dtype=LD)
    if fr:
        K[fr] = gauss_solve(Mm[np.ix_(fr, fr)], 2 * T3[fr])
    ABK = A + B @ K
    T6 = K.T @ R
    y = B @ k + c
    kR = k @ R
    Vn = (ABK.T @ Vs) @ ABK + np.outer(q, q) + T6 @ K
    z = (2 * y) @ Vn
    vn = z @ ABK + v @ ABK + q + (2 * kR) @ K
    # the step's scale for the non-degeneracy condition: the size of the controls in play
    fin = np.concatenate([np.abs(kunc), np.abs(bl[np.isfinite(bl)]), np.abs(bh[np.isfinite(bh)])])
    return dict(K=K, k=k, V=Vn, v=vn, state=st, margin=mg, scale=fin.max(), kunc=kunc, H=H, g=g)


def recursion(recs, qpos, qvel, ctrl, nv, nu, dt, mu, lo, hi, layout=0, V0=None, v0=None):
    """initV (v = q_0, V = v v', or V0 / v0) and steps n = 1 .. P-1 over one
    seed's records (P, D) and nominal trajectory (nq == nv).  -> dict of
    K (P, nu nx: column-major like the device's), k (P, nu), V (nx nx
    column-major), v, mask (P,), margin / scale / kunc / H / g per step"""
    P, nx = len(recs), 2 * nv
    o = 2 * nv * nv + nv * nu
    if V0 is None:
        v = np.asarray(recs[0][o:o + nx], dtype=LD)
        V = np.outer(v, v)
    else:
        V, v = np.asarray(V0, dtype=LD), np.asarray(v0, dtype=LD)
    x = np.concatenate([np.asarray(qpos, dtype=LD), np.asarray(qvel, dtype=LD)], axis=1)
    out = dict(K=np.zeros((P, nu * nx), dtype=LD), k=np.zeros((P, nu), dtype=LD), mask=np.zeros(P, dtype=np.uint32),
               margin=np.full(P, np.inf), scale=np.ones(P), kunc=np.zeros((P, nu)), state=np.zeros((P, nu), dtype=int), H=[None] * P, g=[None] * P)
    for n in range(1, P):
        s = step(recs[n], nv, nu, dt, mu, V, v, x[n - 1] - x[n], ctrl[n], lo, hi, layout)
        V, v = s["V"], s["v"]
        out["K"][n] = s["K"].ravel(order="F")
        out["k"][n] = s["k"]
        out["state"][n] = s["state"]
        out["mask"][n] = sum(1 << a for a in range(nu) if s["state"][a])
        out["margin"][n] = float(s["margin"])
        out["scale"][n] = float(s["scale"])
        out["kunc"][n] = s["kunc"].astype(np.float64)
        out["H"][n], out["g"][n] = s["H"], s["g"]
    out["V"], out["v"] = V.ravel(order="F"), v
    return out

"""Reference of the standard recursion (ilqg_solver_set_recursion, STANDARD):
the textbook iLQR backward step in deviation coordinates.  A helper: not
collected.

For step n = 1..N, with A, B assembled from record n (either layout),
q = dgdx, r = dgdu of record n, lxx = 2 diag(wq, wv), luu = 2 diag(wu) of the
cost row of point n:

    Qx  = q + A'v            Qu  = r + B'v
    Qxx = lxx + A'VA         Qux = B'VA            Quu = luu + B'VB
    Quu_r = luu + B'(V + mu I)B                    Qux_r = B'(V + mu I)A
    k = -Quu_r^-1 Qu         K = -Quu_r^-1 Qux_r
    dV1 += k'Qu              dV2 += 1/2 k'Quu k
    v <- Qx + K'Quu k + K'Qu + Qux'k
    V <- Qxx + K'Quu K + K'Qux + Qux'K ;  V <- (V + V')/2

from v = dgdx of record 0, V = lxx of row 0 (or V0, v0).  A step whose Quu_r
has a pivot <= 0 or NaN under a diagonally pivoted LDLT (or whose gains come
out non-finite) takes K = 0, k = 0, adds nothing to dV, and is flagged.

The recursion is written twice: recursion_ld in np.longdouble (numpy products,
Gaussian elimination as boxqp_ref.gauss_solve) and recursion_f64 in Python
floats with sequential loops, every sum in ascending index.  e64() is the
largest deviation between the two on the same records: the reference's own
rounding, which sets the tests' tolerance.

StdRef composes a one-seed solver from the oracle in the manner of
cost_sched_ref.SchedRef: the rollout through OILQR.forward_candidates, the
records through ora_ilqr_fd_point (under ora_set_cost_desc(row p) when
scheduled), this recursion, and the gains handed back with OILQR.set_gains.
"""
import math

import numpy as np

import boxqp_ref as bq
import cost_sched_ref as csr

LD = np.longdouble
ARRAYS = ("K", "k", "V", "v", "dV")


def assemble_AB(rec, nv, nu, dt, layout):
    """A, B of one record in fp64 (Differentiator::updateDerivatives): 'reference'
    reads the row-major blocks column-major (quirk Q1), 'corrected' as they are"""
    nx = 2 * nv
    order = "F" if layout == "reference" else "C"
    A = np.zeros((nx, nx))
    A[:nv, :nv] = np.eye(nv)
    A[:nv, nv:] = np.eye(nv) * dt
    A[nv:, :nv] = rec[: nv * nv].reshape(nv, nv, order=order) * dt
    A[nv:, nv:] = np.eye(nv) + rec[nv * nv: 2 * nv * nv].reshape(nv, nv, order=order) * dt
    B = np.zeros((nx, nu))
    B[nv:, :] = rec[2 * nv * nv: 2 * nv * nv + nv * nu].reshape(nv, nu, order=order) * dt
    return A, B


def hessians(rows, nq, nv, nu):
    """(lxx (P, 2 nv), luu (P, nu)): the diagonals 2 (wq, wv), 2 wu of packed cost rows (P, C)"""
    assert nq == nv
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    wq = rows[:, 0:nq]
    wv = rows[:, 3 * nq:3 * nq + nv]
    wu = rows[:, 3 * nq + 3 * nv:3 * nq + 3 * nv + nu]
    return 2 * np.concatenate([wq, wv], axis=1), 2 * wu


def _split(rec, nv, nu):
    o = 2 * nv * nv + nv * nu
    return rec[o:o + 2 * nv], rec[o + 2 * nv:o + 2 * nv + nu]


def _pivots(M, zero):
    """the D of a diagonally pivoted LDLT of the symmetric M (largest |diagonal|
    first), in M's own number type; NaN where the elimination cannot go on"""
    n = len(M)
    M = [list(r) for r in M]
    out = []
    for k in range(n):
        p = k
        for i in range(k + 1, n):
            if abs(M[i][i]) > abs(M[p][p]):
                p = i
        if p != k:
            M[k], M[p] = M[p], M[k]
            for r in M:
                r[k], r[p] = r[p], r[k]
        d = M[k][k]
        out.append(d)
        if not (abs(d) > zero):
            out += [d] * (n - k - 1)
            return out
        for i in range(k + 1, n):
            f = M[i][k] / d
            for j in range(k + 1, n):
                M[i][j] = M[i][j] - f * M[k][j]
    return out


def recursion_ld(rec, nv, nu, dt, mu, layout, lxx, luu, V0=None, v0=None):
    """the recursion in np.longdouble over records rec (P, D); lxx (P, nx),
    luu (P, nu) the Hessian diagonals per point.  -> dict K (P, nu nx
    column-major), k (P, nu), V (nx nx column-major), v, dV (2), first_bad"""
    rec = np.asarray(rec, dtype=np.float64)
    P, nx = rec.shape[0], 2 * nv
    K, k = np.zeros((P, nu * nx), dtype=LD), np.zeros((P, nu), dtype=LD)
    v = np.array(_split(rec[0], nv, nu)[0] if v0 is None else v0, dtype=LD)
    V = np.diag(np.asarray(lxx[0], dtype=LD)) if V0 is None else np.array(V0, dtype=LD).reshape(nx, nx, order="F")
    V = (V + V.T) / 2
    dV1, dV2, first_bad = LD(0), LD(0), -1
    I = np.eye(nx, dtype=LD)
    for n in range(1, P):
        A, B = (x.astype(LD) for x in assemble_AB(rec[n], nv, nu, dt, layout))
        q, r = (x.astype(LD) for x in _split(rec[n], nv, nu))
        Lx, Lu = np.diag(np.asarray(lxx[n], dtype=LD)), np.diag(np.asarray(luu[n], dtype=LD))
        Qx, Qu = q + A.T @ v, r + B.T @ v
        Qxx, Qux, Quu = Lx + A.T @ V @ A, B.T @ V @ A, Lu + B.T @ V @ B
        Vr = V + LD(mu) * I
        Quur, Quxr = Lu + B.T @ Vr @ B, B.T @ Vr @ A
        piv = _pivots(Quur.tolist(), LD(0))
        bad = not all(d > 0 for d in piv)
        Kn, kn = np.zeros((nu, nx), dtype=LD), np.zeros(nu, dtype=LD)
        if not bad:
            with np.errstate(all="ignore"):
                kn = -bq.gauss_solve(Quur, Qu)
                Kn = -bq.gauss_solve(Quur, Quxr)
            if not (np.all(np.isfinite(kn)) and np.all(np.isfinite(Kn))):
                bad = True
                Kn, kn = np.zeros((nu, nx), dtype=LD), np.zeros(nu, dtype=LD)
        if bad:
            first_bad = n if first_bad < 0 else first_bad
        else:
            dV1 += kn @ Qu
            dV2 += (kn @ Quu @ kn) / 2
        v = Qx + Kn.T @ Quu @ kn + Kn.T @ Qu + Qux.T @ kn
        V = Qxx + Kn.T @ Quu @ Kn + Kn.T @ Qux + Qux.T @ Kn
        V = (V + V.T) / 2
        K[n], k[n] = Kn.ravel(order="F"), kn
    return dict(K=K, k=k, V=V.ravel(order="F"), v=v, dV=np.array([dV1, dV2], dtype=LD), first_bad=first_bad)


# ---- fp64, sequential loops (Python floats are IEEE doubles; ascending sums from 0.0)
def _mm(A, B):
    n, m, p = len(A), len(B), len(B[0])
    out = [[0.0] * p for _ in range(n)]
    for i in range(n):
        Ai = A[i]
        for j in range(p):
            s = 0.0
            for t in range(m):
                s += Ai[t] * B[t][j]
            out[i][j] = s
    return out


def _tr(A):
    return [list(c) for c in zip(*A)]


def _mv(A, x):
    out = []
    for row in A:
        s = 0.0
        for a, b in zip(row, x):
            s += a * b
        out.append(s)
    return out


def _add(A, B):
    return [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def _diag(d):
    n = len(d)
    return [[float(d[i]) if i == j else 0.0 for j in range(n)] for i in range(n)]


def _ldlt_solve(M, R):
    """M X = R (columns of R) through an unpivoted-after-permutation LDL' of the
    symmetric positive definite M, diagonal pivoting; sequential doubles"""
    n = len(M)
    M = [list(r) for r in M]
    perm = list(range(n))
    for k in range(n):  # the pivot order: the diagonal of the Schur complement, largest first
        p = k
        for i in range(k + 1, n):
            if abs(M[i][i]) > abs(M[p][p]):
                p = i
        if p != k:
            M[k], M[p] = M[p], M[k]
            for r in M:
                r[k], r[p] = r[p], r[k]
            perm[k], perm[p] = perm[p], perm[k]
        d = M[k][k]
        for i in range(k + 1, n):
            f = M[i][k] / d
            M[i][k] = f
            for j in range(k + 1, n):
                M[i][j] = M[i][j] - f * M[k][j]
    X = []
    for col in _tr(R):
        y = [col[perm[i]] for i in range(n)]
        for i in range(n):
            for j in range(i):
                y[i] -= M[i][j] * y[j]
        for i in range(n):
            y[i] /= M[i][i]
        for i in range(n - 1, -1, -1):
            for j in range(i + 1, n):
                y[i] -= M[j][i] * y[j]
        x = [0.0] * n
        for i in range(n):
            x[perm[i]] = y[i]
        X.append(x)
    return _tr(X)


def recursion_f64(rec, nv, nu, dt, mu, layout, lxx, luu, V0=None, v0=None):
    """recursion_ld's formulas in fp64 with sequential loops; the same dict (float64 arrays)"""
    rec = np.asarray(rec, dtype=np.float64)
    P, nx = rec.shape[0], 2 * nv
    mu = float(mu)
    K, k = np.zeros((P, nu * nx)), np.zeros((P, nu))
    v = [float(x) for x in (_split(rec[0], nv, nu)[0] if v0 is None else v0)]
    V = _diag(lxx[0]) if V0 is None else np.asarray(V0, dtype=np.float64).reshape(nx, nx, order="F").tolist()
    V = [[(V[i][j] + V[j][i]) / 2 for j in range(nx)] for i in range(nx)]
    dV1, dV2, first_bad = 0.0, 0.0, -1
    for n in range(1, P):
        A, B = (x.tolist() for x in assemble_AB(rec[n], nv, nu, dt, layout))
        q, r = (x.tolist() for x in _split(rec[n], nv, nu))
        At, Bt = _tr(A), _tr(B)
        Lx, Lu = _diag(lxx[n]), _diag(luu[n])
        Qx = [a + b for a, b in zip(q, _mv(At, v))]
        Qu = [a + b for a, b in zip(r, _mv(Bt, v))]
        BtV, AtV = _mm(Bt, V), _mm(At, V)
        Qxx, Qux, Quu = _add(Lx, _mm(AtV, A)), _mm(BtV, A), _add(Lu, _mm(BtV, B))
        Vr = [[V[i][j] + mu if i == j else V[i][j] for j in range(nx)] for i in range(nx)]
        BtVr = _mm(Bt, Vr)
        Quur, Quxr = _add(Lu, _mm(BtVr, B)), _mm(BtVr, A)
        piv = _pivots(Quur, 0.0)
        bad = not all(d > 0 for d in piv)
        Kn, kn = [[0.0] * nx for _ in range(nu)], [0.0] * nu
        if not bad:
            try:
                X = _ldlt_solve(Quur, [[-Quxr[a][j] for j in range(nx)] + [-Qu[a]] for a in range(nu)])
                ok = all(math.isfinite(x) for row in X for x in row)
            except (ZeroDivisionError, OverflowError):
                ok = False
            if ok:
                Kn, kn = [row[:nx] for row in X], [row[nx] for row in X]
            else:
                bad = True
        if bad:
            first_bad = n if first_bad < 0 else first_bad
        else:
            d1 = 0.0
            for a in range(nu):
                d1 += kn[a] * Qu[a]
            d2 = 0.0
            for a, s in enumerate(_mv(Quu, kn)):
                d2 += kn[a] * s
            dV1 += d1
            dV2 += d2 / 2
        Kt, Quxt = _tr(Kn), _tr(Qux)
        t1, t2, t3 = _mv(Kt, _mv(Quu, kn)), _mv(Kt, Qu), _mv(Quxt, kn)
        v = [((a + b) + c) + d for a, b, c, d in zip(Qx, t1, t2, t3)]
        M1, M2, M3 = _mm(_mm(Kt, Quu), Kn), _mm(Kt, Qux), _mm(Quxt, Kn)
        V = [[((Qxx[i][j] + M1[i][j]) + M2[i][j]) + M3[i][j] for j in range(nx)] for i in range(nx)]
        V = [[(V[i][j] + V[j][i]) / 2 for j in range(nx)] for i in range(nx)]
        K[n], k[n] = np.array(Kn).ravel(order="F"), kn
    return dict(K=K, k=k, V=np.array(V).ravel(order="F"), v=np.array(v), dV=np.array([dV1, dV2]),
                first_bad=first_bad)


def rel(a, b):
    """max |a - b| relative to max |b|, in longdouble"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


def e64(ld, f64):
    """the largest deviation of the fp64 evaluation from the longdouble one, over K, k, V, v, dV"""
    return max(rel(f64[n], ld[n]) for n in ARRAYS)


def tol(E64):
    return max(1e-12, 10 * E64)


def both(rec, nv, nu, dt, mu, layout, lxx, luu, V0=None, v0=None):
    """(longdouble reference, E64) on one seed's records"""
    ld = recursion_ld(rec, nv, nu, dt, mu, layout, lxx, luu, V0, v0)
    f = recursion_f64(rec, nv, nu, dt, mu, layout, lxx, luu, V0, v0)
    assert f["first_bad"] == ld["first_bad"], (f["first_bad"], ld["first_bad"])
    return ld, e64(ld, f)


class StdRef:
    """the composed reference solver of one seed: oracle rollout and records, the
    fp64 recursion above (or the longdouble one: precise=True)"""

    def __init__(self, ora, m, om, dstate, N, rows, alphas=(1.0,), select="min_cost", layout="corrected", mu=0.0,
                 scheduled=False, precise=False):
        self.ora, self.m, self.om, self.N = ora, m, om, N
        self.rows = np.array(rows, dtype=np.float64)
        assert self.rows.shape == (N + 1, csr.row_size(m))
        self.alphas, self.select, self.layout, self.mu = tuple(float(a) for a in alphas), select, layout, float(mu)
        self.scheduled, self.precise = scheduled, precise
        self.lxx, self.luu = hessians(self.rows, m.nq, m.nv, m.nu)
        self.desc = [csr.desc_from_row(ora, m, r) for r in (self.rows if scheduled else self.rows[:1])]
        om.lib.L.ora_set_cost_desc(self.desc[0])
        d = om.make_data()
        d.set_state(**dstate)
        self.il = ora.OILQR(om, d, N, cost_fn="ora_cost_desc_fn")
        self.il.set_dinit(d)
        self.out = None

    def forward(self):
        return self.il.forward_candidates(self.alphas, self.select)

    def sweep(self):
        L = self.om.lib.L
        for p in range(self.N + 1):
            if self.scheduled:
                L.ora_set_cost_desc(self.desc[p])
            L.ora_ilqr_fd_point(self.il.s, p)
        L.ora_set_cost_desc(self.desc[0])
        return self.il.arrays()["deriv"]

    def backward(self, rec=None, V0=None, v0=None):
        rec = self.sweep() if rec is None else rec
        f = recursion_ld if self.precise else recursion_f64
        self.out = f(rec, self.m.nv, self.m.nu, self.m.timestep, self.mu, self.layout, self.lxx, self.luu, V0, v0)
        self.il.set_gains(np.asarray(self.out["K"], dtype=np.float64), np.asarray(self.out["k"], dtype=np.float64))
        return self.out

    def iterate(self):
        costs, sel = self.forward()
        self.backward()
        return costs, sel

    def traj(self):
        return self.il.traj()

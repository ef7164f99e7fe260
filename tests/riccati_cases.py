"""Crafted FD records for the Riccati backward pass, and plain-numpy
restatements of the oracle's step-1 inputs and of its pivoted LDLT
(oracle/ilqr_ora.c: ora_assemble_AB, ora_riccati_step_c, ora_ldlt_factor,
ora_ldlt_solve).  A helper for tests/test_riccati_cases.py: not collected.

A record is D = nv (2 nv + nu) + 2 nv + nu doubles: fq, fv (nv x nv each) and fu
(nv x nu), each read by the reference layout as deriv[r + c nv], then q (2 nv)
and r (nu).  The matrix the step factors is Mm = -2 B'(Vs)B - 2 r r' with
B = [0; dt fu], Vs = sym(V) + mu I.

Family T ("single-term"): fq = fv = 0, every column a of fu has one non-zero
b_a > 0 in a row p(a) of its own, and V0 = 0 (q_0 = 0 in the point-0 record).
Then Mm = -2 mu dt^2 diag(b^2) - 2 r r' and every inner product that feeds Mm,
T3 and B'w has at most one non-zero term: any summation order gives the same
bits.  (b_a, |r_a|) come from a few pairs, so the |diagonal| keys of the pivot
scan tie; the T-ties assignments are redrawn until the scan's swaps carry a
row behind its equals, so that Eigen's order is not the index-stable one.
Family S ("sign-mixed ties"): fu as in T with one b, r = 0, and a V0 whose
diagonal at the p(a) positions is -mu +- s, plus symmetric off-diagonal
entries: |diagonal| ties between entries of opposite sign, with coupling.
Family D ("dense"): standard-normal records.

Every case is three records (horizon 2): point 0 (q_0 = 0 for family T),
point 1 the crafted record, point 2 a dense one, so a second, general step runs
on top of the degenerate gains.  Everything is seeded and deterministic."""
from dataclasses import dataclass, field
from itertools import product
from typing import Optional

import numpy as np

DBL_MIN = 2.2250738585072014e-308
MU = 1000.0
H = 2
DENORM_B = 1e-156
# (b, |r|) pairs of family T, keys 2 mu dt^2 b^2 + 2 r^2 ascending: lo ... hi
PAIRS = ((0.7, 0.17), (0.9, 0.23), (1.3, 0.31), (2.1, 0.45))
S_VALUES = (8.0, 16.0, 24.0, 32.0)
S_B = 1.25


def record_size(nv, nu):
    return nv * (2 * nv + nu) + 2 * nv + nu


@dataclass
class Case:
    name: str
    family: str            # "T", "S", "D"
    kind: str              # "ties", "zero", "alltie", "allzero", "rank1", "denorm", "nan", "enum", "S", "D"
    rec: np.ndarray        # (3, D)
    V0: Optional[np.ndarray] = None   # (nx, nx), symmetric
    v0: Optional[np.ndarray] = None   # (nx,)
    special: tuple = ()    # the controls that are structurally zero / denormal / NaN
    meta: dict = field(default_factory=dict)

    @property
    def finite(self):
        return self.kind != "nan"

    @property
    def tie_case(self):
        """counted by the tie-order conditions (T-ties, T-zero, the enumeration)"""
        return self.kind in ("ties", "zero", "enum")


def pack(nv, nu, fu=None, q=None, r=None):
    """a record with fq = fv = 0; fu is (nv, nu) in the reference's reading, fu[r, c] = deriv[2 nv^2 + r + c nv]"""
    rec = np.zeros(record_size(nv, nu))
    o = 2 * nv * nv
    if fu is not None:
        rec[o:o + nv * nu] = np.asarray(fu, dtype=np.float64).ravel(order="F")
    o += nv * nu
    if q is not None:
        rec[o:o + 2 * nv] = q
    o += 2 * nv
    if r is not None:
        rec[o:o + nu] = r
    return rec


def unpack(rec, nv, nu):
    """fq, fv (nv, nv), fu (nv, nu) in the reference's reading, q, r"""
    o = 0
    fq = rec[o:o + nv * nv].reshape(nv, nv, order="F"); o += nv * nv
    fv = rec[o:o + nv * nv].reshape(nv, nv, order="F"); o += nv * nv
    fu = rec[o:o + nv * nu].reshape(nv, nu, order="F"); o += nv * nu
    q = rec[o:o + 2 * nv]; o += 2 * nv
    return fq, fv, fu, q, rec[o:o + nu]


def _single_term_fu(nv, nu, rows, b):
    fu = np.zeros((nv, nu))
    fu[rows, np.arange(nu)] = b
    return fu


def _counts(nu):
    if nu >= 21:
        return dict(ties=16, zero=8, S=4, noff=36)
    if nu >= 7:
        return dict(ties=8, zero=4, S=3, noff=12)
    return dict(ties=0, zero=0, S=2 if nu > 1 else 1, noff=4 if nu > 1 else 1)


def make_cases(nv, nu, dt, mu=MU, seed=20261019):
    """the named cases of one model size, in a fixed order"""
    assert nu <= nv
    rng = np.random.default_rng([seed, nv, nu])
    D, nx = record_size(nv, nu), 2 * nv
    keys = [2 * mu * dt * dt * b * b + 2 * r * r for b, r in PAIRS]
    assert all(a < b for a, b in zip(keys, keys[1:])), keys  # distinct, ascending
    out = []

    def dense():
        return rng.standard_normal(D)

    def add_T(name, kind, b, r, special=(), **meta):
        rows = rng.permutation(nv)[:nu]
        q1 = rng.standard_normal(nx)
        rec = np.stack([np.zeros(D), pack(nv, nu, _single_term_fu(nv, nu, rows, b), q1, r), dense()])
        out.append(Case(name, "T", kind, rec, special=tuple(int(i) for i in special),
                        meta=dict(rows=rows, b=np.asarray(b, float), r=np.asarray(r, float), **meta)))

    def draw(npairs, displaced=False):
        # displaced: redrawn until the scan's swaps reorder a tie group (the
        # keys order like the pair indices)
        pick = rng.integers(0, npairs, nu)
        while displaced and eigen_order(pick) == stable_order(pick):
            pick = rng.integers(0, npairs, nu)
        b = np.array([PAIRS[i][0] for i in pick])
        r = np.array([PAIRS[i][1] for i in pick]) * rng.choice([-1.0, 1.0], nu)
        return b, r

    cnt = _counts(nu)
    if nu == 1:
        add_T("T-zero", "enum1", [0.0], [0.0], special=[0])
        add_T("T-denorm", "denorm", [DENORM_B], [0.0], special=[0])
        add_T("T-normal", "enum1", [PAIRS[1][0]], [-PAIRS[1][1]])
        add_T("T-rank1", "rank1", [0.0], [0.3])
        add_T("T-nan", "nan", [PAIRS[1][0]], [np.nan], special=[0])
    else:
        if nu == 3:  # exhaustive: every assignment of {zero, lo, hi} to the three controls
            lvl = ((0.0, 0.0), PAIRS[0], PAIRS[3])
            for pat in product(range(3), repeat=3):
                b = np.array([lvl[i][0] for i in pat])
                r = np.array([lvl[i][1] for i in pat]) * rng.choice([-1.0, 1.0], 3)
                add_T("T-enum-" + "".join("zlh"[i] for i in pat), "enum", b, r,
                      special=[a for a in range(3) if pat[a] == 0])
        for i in range(cnt["ties"]):
            b, r = draw(3 + i % 2, displaced=True)
            add_T(f"T-ties-{i}", "ties", b, r)
        for i in range(cnt["zero"]):
            b, r = draw(3 + i % 2)
            z = rng.permutation(nu)[:1 + i % 3]
            b[z] = 0.0
            r[z] = 0.0
            add_T(f"T-zero-{i}", "zero", b, r, special=z)
        b = np.full(nu, PAIRS[2][0])
        add_T("T-alltie", "alltie", b, PAIRS[2][1] * rng.choice([-1.0, 1.0], nu))
        add_T("T-allzero", "allzero", np.zeros(nu), np.zeros(nu), special=range(nu))
        add_T("T-rank1", "rank1", np.zeros(nu), 0.3 * rng.choice([-1.0, 1.0], nu))
        b, r = draw(3)
        z = rng.permutation(nu)[:min(3, max(1, nu // 2))]
        b[z] = DENORM_B
        r[z] = 0.0
        add_T("T-denorm", "denorm", b, r, special=z)
        b, r = draw(4)
        z = rng.permutation(nu)[:1]
        r[z] = np.nan
        add_T("T-nan", "nan", b, r, special=z)

    for i in range(cnt["S"]):
        rows = rng.permutation(nv)[:nu]
        fu = _single_term_fu(nv, nu, rows, S_B)
        V0 = np.zeros((nx, nx))
        pos = nv + rows
        sgn, sv = rng.choice([-1.0, 1.0], nu), rng.choice(S_VALUES, nu)
        V0[pos, pos] = -mu + sgn * sv
        for e in range(cnt["noff"]):
            if nu > 1 and e % 2 == 0:  # coupling inside Mm
                a, c = rng.choice(pos, 2, replace=False)
            else:
                a, c = rng.choice(nx, 2, replace=False)
            V0[a, c] = V0[c, a] = rng.choice([0.5, 1.0, 2.0])
        rec = np.stack([dense(), pack(nv, nu, fu, rng.standard_normal(nx), None), dense()])
        out.append(Case(f"S-{i}", "S", "S", rec, V0=V0, v0=rng.standard_normal(nx),
                        meta=dict(rows=rows, sign=sgn, s=sv)))
    for i in range(2):
        out.append(Case(f"D-{i}", "D", "D", np.stack([dense(), dense(), dense()])))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- numpy restatements of the oracle (its loop order; products rounded before they are added)
def assemble_AB(rec, nv, nu, dt):
    fq, fv, fu, _, _ = unpack(rec, nv, nu)
    nx = 2 * nv
    A = np.zeros((nx, nx))
    A[:nv, :nv] = np.eye(nv)
    A[:nv, nv:] = np.eye(nv) * dt
    A[nv:, :nv] = fq * dt
    A[nv:, nv:] = np.eye(nv) + fv * dt
    B = np.zeros((nx, nu))
    B[nv:] = fu * dt
    return A, B


def seq_dot(X, Y, reverse=False):
    """out[i, j] = sum_k X[i, k] Y[k, j], added one term at a time from +0 in ascending (or descending) k"""
    n = X.shape[1]
    s = np.zeros((X.shape[0], Y.shape[1]))
    with np.errstate(all="ignore"):
        for k in (range(n - 1, -1, -1) if reverse else range(n)):
            s = s + np.outer(X[:, k], Y[k, :])
    return s


def step_inputs(rec, nv, nu, dt, mu, V, v, c, reverse=False):
    """Mm, T3 and the feed-forward right-hand side B'w + r of one step (ora_riccati_step_c)"""
    A, B = assemble_AB(rec, nv, nu, dt)
    r = unpack(rec, nv, nu)[4]
    Vs = (V + V.T) / 2
    Vs[np.diag_indices_from(Vs)] += mu
    T1 = seq_dot(B.T, Vs, reverse)
    with np.errstate(all="ignore"):
        Mm = -2 * seq_dot(T1, B, reverse) - 2 * np.outer(r, r)
        T3 = seq_dot(T1, A, reverse)
        w = v + 2 * seq_dot(Vs, c[:, None], reverse)[:, 0]
        rhs = seq_dot(B.T, w[:, None], reverse)[:, 0] + r
    return Mm, T3, rhs


def same_bits(a, b):
    """equal bit for bit where neither is NaN, and NaN in the same places"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na],
                                                                            b.view(np.int64)[~nb])


def eigen_order(keys):
    """the rows (original indices) in the order Eigen's scan picks them: at
    step k the first position i >= k of largest key (strict >), then positions
    k and i swap"""
    ids = list(range(len(keys)))
    ky = [float(x) for x in keys]
    for k in range(len(ky)):
        big = k
        for i in range(k + 1, len(ky)):
            if ky[i] > ky[big]:
                big = i
        ky[k], ky[big] = ky[big], ky[k]
        ids[k], ids[big] = ids[big], ids[k]
    return ids


def stable_order(keys):
    """the rows by key descending, equal keys by index ascending"""
    return sorted(range(len(keys)), key=lambda i: (-float(keys[i]), i))


def ldlt_factor(M, rule="eigen"):
    """ora_ldlt_factor on a copy of M (n x n): returns (factor, transp).
    rule "stable" replaces the scan's first-hit rule among equal keys by the
    smallest original index (the pivot order stable_order gives)"""
    mat = np.array(M, dtype=np.float64)
    n = mat.shape[0]
    transp = [0] * n
    ids = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            big, bigv = k, abs(mat[k, k])
            for i in range(k + 1, n):
                a = abs(mat[i, i])
                if a > bigv or (rule == "stable" and a == bigv and ids[i] < ids[big]):
                    big, bigv = i, a
            transp[k] = big
            if k != big:
                ids[k], ids[big] = ids[big], ids[k]
                for j in range(k):
                    mat[k, j], mat[big, j] = mat[big, j], mat[k, j]
                for i in range(big + 1, n):
                    mat[i, k], mat[i, big] = mat[i, big], mat[i, k]
                mat[k, k], mat[big, big] = mat[big, big], mat[k, k]
                for i in range(k + 1, big):
                    mat[i, k], mat[big, i] = mat[big, i], mat[i, k]
            if k > 0:
                temp = [mat[j, j] * mat[k, j] for j in range(k)]
                for i in range(k, n):
                    s = 0.0
                    for j in range(k):
                        s += mat[i, j] * temp[j]
                    mat[i, k] -= s
            if k == 0 and not abs(mat[0, 0]) > 0:
                return mat, list(range(n))
            if n - k - 1 > 0 and abs(mat[k, k]) > 0:
                for i in range(k + 1, n):
                    mat[i, k] /= mat[k, k]
    return mat, transp


def ldlt_solve(L, transp, x):
    """ora_ldlt_solve on a copy of x"""
    x = [float(t) for t in x]
    n = len(x)
    with np.errstate(all="ignore"):
        for k in range(n):
            x[k], x[transp[k]] = x[transp[k]], x[k]
        for i in range(n):
            for j in range(i):
                x[i] -= L[i, j] * x[j]
        for i in range(n):
            x[i] = x[i] / L[i, i] if abs(L[i, i]) > DBL_MIN else 0.0
        for i in range(n - 1, -1, -1):
            for j in range(i + 1, n):
                x[i] -= L[j, i] * x[j]
        for k in range(n - 1, -1, -1):
            x[k], x[transp[k]] = x[transp[k]], x[k]
    return np.array(x)

"""numpy statement of hak_find_fundamental (include/hipakaze.h): RANSAC fundamental matrix over a match list, bit for bit.

The checker only -- the product never calls it.  Vectorised over hypotheses: float64 for the seven-point solve (Hartley
normalisation, a 7 x 9 elimination with row pivoting, the cubic det(a A + B) = 0 solved by bisection with + - * / sqrt only),
float32 for the Sampson scoring.  numpy forms no FMA, and every expression below is written in the evaluation order of
kernels_fundamental.hip.
"""
import numpy as np

import homography_ref as hr
from homography_ref import _mul3, records

FUNDAMENTAL_DTYPE = np.dtype([("F", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("root", "<i4"), ("n", "<i4")])
assert FUNDAMENTAL_DTYPE.itemsize == 52        # 9 floats + 4 ints

DRAWS = 32


def sample_indices(seed, h, n):
    """(len(h), 7) int64 indices (-1 where not drawn) and a validity flag per hypothesis"""
    return hr.sample_indices(seed, h, n, 7, DRAWS)


def _normalise(x, y):
    """Hartley normalisation of seven points (lists of (H,) float64): (X, Y, cx, cy, s, ok)"""
    sx, sy = np.zeros_like(x[0]), np.zeros_like(x[0])
    for k in range(7):
        sx = sx + x[k]
        sy = sy + y[k]
    cx, cy = sx / 7.0, sy / 7.0
    q = np.zeros_like(cx)
    dx, dy = [], []
    for k in range(7):
        dx.append(x[k] - cx)
        dy.append(y[k] - cy)
        q = q + (dx[k] * dx[k] + dy[k] * dy[k])
    s = np.sqrt(14.0 / q)
    ok = (q != 0.0) & np.isfinite(s)
    return [s * d for d in dx], [s * d for d in dy], cx, cy, s, ok


def null_space(M):
    """M: 7 rows of 9 (H,) float64 arrays.  Gaussian elimination with partial pivoting over rows, pivot columns 0..6 in order;
    -> (A, B, ok): the null vectors with (f7, f8) = (1, 0) and (0, 1) as lists of nine (H,) arrays"""
    M = np.stack([np.stack(row, axis=-1) for row in M], axis=-2)        # (H, 7, 9)
    nh = M.shape[0]
    rows = np.arange(nh)
    ok = np.ones(nh, bool)
    for c in range(7):
        piv = np.full(nh, c)
        best = np.abs(M[:, c, c])
        for r in range(c + 1, 7):
            v = np.abs(M[:, r, c])
            gt = v > best
            best = np.where(gt, v, best)
            piv = np.where(gt, r, piv)
        ok &= (best > 0.0) & np.isfinite(best)
        top, other = M[rows, c].copy(), M[rows, piv].copy()
        M[rows, piv] = top
        M[rows, c] = other
        for r in range(c + 1, 7):
            f = M[:, r, c] / M[:, c, c]
            for q in range(c + 1, 9):
                M[:, r, q] = M[:, r, q] - f * M[:, c, q]
    out = []
    for free in (7, 8):
        f = [None] * 9
        f[7] = np.full(nh, 1.0 if free == 7 else 0.0)
        f[8] = np.full(nh, 1.0 if free == 8 else 0.0)
        for i in range(6, -1, -1):
            acc = -M[:, i, free]
            for j in range(i + 1, 7):
                acc = acc - M[:, i, j] * f[j]
            f[i] = acc / M[:, i, i]
        out.append(f)
    return out[0], out[1], ok


def _det(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def _with_row(P, Q, i):
    """P with row i taken from Q"""
    return [Q[k] if k // 3 == i else P[k] for k in range(9)]


def cubic(A, B):
    """(c3, c2, c1, c0) of det(a A + B)"""
    c3, c0 = _det(A), _det(B)
    c2 = (_det(_with_row(A, B, 0)) + _det(_with_row(A, B, 1))) + _det(_with_row(A, B, 2))
    c1 = (_det(_with_row(B, A, 0)) + _det(_with_row(B, A, 1))) + _det(_with_row(B, A, 2))
    return c3, c2, c1, c0


def real_roots(c3, c2, c1, c0):
    """the real roots of c3 a^3 + c2 a^2 + c1 a + c0 by bracketing and 64 bisections: (roots (H, 3), count (H,), ok (H,));
    roots beyond the count are NaN"""
    with np.errstate(all="ignore"):
        c3, c2, c1, c0 = (np.asarray(v, np.float64) for v in (c3, c2, c1, c0))
        ok = (c3 != 0.0) & np.isfinite(c3) & np.isfinite(c2) & np.isfinite(c1) & np.isfinite(c0)
        b2, b1, b0 = c2 / c3, c1 / c3, c0 / c3

        def q(a):
            return ((a + b2) * a + b1) * a + b0

        m = np.abs(b2)
        m = np.where(np.abs(b1) > m, np.abs(b1), m)
        m = np.where(np.abs(b0) > m, np.abs(b0), m)
        bound = 1.0 + m
        ok &= np.isfinite(b2) & np.isfinite(b1) & np.isfinite(b0) & np.isfinite(bound)
        D = b2 * b2 - 3.0 * b1
        three = D > 0.0
        s = np.sqrt(np.where(three, D, 0.0))
        t1, t2 = (-b2 - s) / 3.0, (-b2 + s) / 3.0
        brackets = ((-bound, np.where(three, t1, bound), np.ones_like(three)), (t1, t2, three), (t2, bound, three))
        roots = np.full(c3.shape + (3,), np.nan)
        count = np.zeros(c3.shape, np.int64)
        rows = np.arange(len(c3))
        for lo, hi, use in brackets:
            lo, hi = lo.copy(), hi.copy()
            neg = q(lo) < 0.0
            has = ok & use & (neg != (q(hi) < 0.0))
            for _ in range(64):
                mid = 0.5 * (lo + hi)
                left = (q(mid) < 0.0) == neg
                lo = np.where(left, mid, lo)
                hi = np.where(left, hi, mid)
            r = 0.5 * (lo + hi)
            roots[rows[has], count[has]] = r[has]
            count = count + has
        return roots, count, ok


def models(rec, seed, h):
    """the float32 models of hypotheses h: (F (len(h), 3, 9) float32, valid (len(h), 3) bool)"""
    n = len(rec)
    h = np.asarray(h, np.int64)
    F = np.zeros((len(h), 3, 9), np.float32)
    valid = np.zeros((len(h), 3), bool)
    if n < 7 or len(h) == 0:
        return F, valid
    idx, ok = sample_indices(seed, h, n)
    p = rec[np.where(idx < 0, 0, idx)].astype(np.float64)               # (H, 7, 4)
    with np.errstate(all="ignore"):
        x, y, cx1, cy1, s1, ok1 = _normalise([p[:, k, 0] for k in range(7)], [p[:, k, 1] for k in range(7)])
        u, v, cx2, cy2, s2, ok2 = _normalise([p[:, k, 2] for k in range(7)], [p[:, k, 3] for k in range(7)])
        ok = ok & ok1 & ok2
        one = np.ones_like(s1)
        M = [[u[k] * x[k], u[k] * y[k], u[k], v[k] * x[k], v[k] * y[k], v[k], x[k], y[k], one] for k in range(7)]
        A, B, okn = null_space(M)
        roots, count, okc = real_roots(*cubic(A, B))
        ok = ok & okn & okc
        zero = np.zeros_like(s1)
        T1 = [s1, zero, -(s1 * cx1), zero, s1, -(s1 * cy1), zero, zero, one]
        T2t = [s2, zero, zero, zero, s2, zero, -(s2 * cx2), -(s2 * cy2), one]
        for r in range(3):
            a = roots[:, r]
            G = _mul3(T2t, _mul3([a * A[k] + B[k] for k in range(9)], T1))
            d = G[0]
            for k in range(1, 9):
                d = np.where(np.abs(G[k]) > np.abs(d), G[k], d)
            Fr = np.stack([(G[k] / d).astype(np.float32) for k in range(9)], axis=-1)
            good = ok & (r < count) & (d != 0.0) & np.isfinite(d) & np.isfinite(Fr).all(axis=-1)
            F[:, r] = np.where(good[:, None], Fr, np.float32(0.0))
            valid[:, r] = good
    return F, valid


def inlier_mask(F, rec, t2):
    """bool (len(F), n) for float32 F (k, 9), records (n, 4) float32, t2 float32: Sampson distance below the threshold"""
    F = np.asarray(F, np.float32).reshape(-1, 9)
    x1, y1, x2, y2 = (rec[None, :, c] for c in range(4))
    f = [F[:, k:k + 1] for k in range(9)]
    with np.errstate(all="ignore"):
        a = (f[0] * x1 + f[1] * y1) + f[2]
        b = (f[3] * x1 + f[4] * y1) + f[5]
        c = (f[6] * x1 + f[7] * y1) + f[8]
        e = (a * x2 + b * y2) + c
        p = (f[0] * x2 + f[3] * y2) + f[6]
        q = (f[1] * x2 + f[4] * y2) + f[7]
        den = (a * a + b * b) + (p * p + q * q)
        return e * e < t2 * den


def find_fundamental(matches, iterations=1024, threshold=1.0, seed=0, block=256):
    """-> (record of FUNDAMENTAL_DTYPE, mask uint8 (n,))"""
    rec = records(matches)
    n = len(rec)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), FUNDAMENTAL_DTYPE)
    out["hypothesis"], out["n"] = -1, n
    best = hr.best_model(iterations, block, lambda hs: models(rec, seed, hs),               # inliers, h, root, F
                         lambda F: inlier_mask(F, rec, t2).sum(axis=1))
    mask = np.zeros(n, np.uint8)
    if best[1] < 0:
        return out, mask
    out["F"], out["inliers"], out["hypothesis"], out["root"] = best[3], best[0], best[1], best[2]
    mask[:] = inlier_mask(best[3], rec, t2)[0]
    return out, mask


def sampson(F, rec):
    """float64 Sampson distance in pixels of (n, 4) records under F (for geometric checks, not part of the contract)"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    r = np.asarray(rec, np.float64)
    p1 = np.concatenate([r[:, :2], np.ones((len(r), 1))], axis=1)
    p2 = np.concatenate([r[:, 2:], np.ones((len(r), 1))], axis=1)
    l2, l1 = p1 @ F.T, p2 @ F
    e = (p2 * l2).sum(axis=1)
    return np.abs(e) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)

"""numpy statement of hak_refine_fundamental (include/hipakaze.h): rank-2 least-squares refit of a fundamental matrix over its
inliers, iterated, bit for bit.

The checker only -- the product never calls it.  float64 without FMA for the sums (in the device order of homography_ref._lanes:
lane l of a wave takes the matches i = l mod 64 in ascending i, then an xor butterfly), the cyclic Jacobi eigen-solves, the rank-2
projection and the denormalisation; float32 Sampson scoring by fundamental_ref.inlier_mask.  Every expression below is written in
the evaluation order of kernels_fundrefit.hip.
"""
import numpy as np

from fundamental_ref import FUNDAMENTAL_DTYPE, inlier_mask, records
from homography_ref import _lanes, _mul3

SWEEPS9, SWEEPS3 = 8, 6
MIN_INLIERS = 8
REFINED_ROOT = 3


def jacobi(A, n, sweeps):
    """cyclic Jacobi on the symmetric n x n float64 matrix A (not modified): -> (the eigenvector of the smallest diagonal entry
    after `sweeps` sweeps, ties to the smallest index; A after the sweeps; V)"""
    A = np.array(A, np.float64).reshape(n, n).copy()
    V = np.eye(n, dtype=np.float64)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if apq == 0.0:
                        continue
                    th = (A[q, q] - A[p, p]) / (2.0 * apq)
                    sg = one if th >= 0.0 else -one
                    t = sg / (np.abs(th) + np.sqrt(th * th + one))
                    c = one / np.sqrt(t * t + one)
                    sn = t * c
                    x, y = A[:, p].copy(), A[:, q].copy()
                    app, aqq = A[p, p] - t * apq, A[q, q] + t * apq
                    A[:, p] = A[p, :] = c * x - sn * y
                    A[:, q] = A[q, :] = sn * x + c * y
                    A[p, p], A[q, q] = app, aqq
                    A[p, q] = A[q, p] = 0.0
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p] = c * vp - sn * vq
                    V[:, q] = sn * vp + c * vq
    j = 0
    for k in range(1, n):
        if A[k, k] < A[j, j]:
            j = k
    return V[:, j].copy(), A, V


def normal_matrix(rec, mask):
    """steps 1-4 on the masked records: (N (9, 9) float64, (s1, c1x, c1y, s2, c2x, c2y)) or None when the round fails"""
    m = int(mask.sum())
    if m < MIN_INLIERS:
        return None
    mm = float(m)
    r = rec.astype(np.float64)
    with np.errstate(all="ignore"):
        s = _lanes(r, mask)
        c1x, c1y, c2x, c2y = s[0] / mm, s[1] / mm, s[2] / mm, s[3] / mm
        dx1, dy1, dx2, dy2 = r[:, 0] - c1x, r[:, 1] - c1y, r[:, 2] - c2x, r[:, 3] - c2y
        q = _lanes(np.stack([dx1 * dx1 + dy1 * dy1, dx2 * dx2 + dy2 * dy2], axis=1), mask)
        s1, s2 = np.sqrt((2.0 * mm) / q[0]), np.sqrt((2.0 * mm) / q[1])
        if not (q[0] > 0.0 and q[1] > 0.0 and np.isfinite(s1) and np.isfinite(s2)):
            return None
        x, y, u, v = s1 * dx1, s1 * dy1, s2 * dx2, s2 * dy2
        w = [u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)]
        sums = _lanes(np.stack([w[p] * w[q_] for p in range(9) for q_ in range(p, 9)], axis=1), mask)
    N = np.zeros((9, 9), np.float64)
    k = 0
    for p in range(9):
        for q_ in range(p, 9):
            N[p, q_] = N[q_, p] = sums[k]
            k += 1
    return N, (s1, c1x, c1y, s2, c2x, c2y)


def rank2(f):
    """step 6: Fn (9,) float64 -> Fn' with its smallest singular triplet subtracted, as a list of nine float64"""
    Fn = [np.float64(v) for v in f]
    with np.errstate(all="ignore"):
        G = np.array([[(Fn[i] * Fn[j] + Fn[3 + i] * Fn[3 + j]) + Fn[6 + i] * Fn[6 + j] for j in range(3)] for i in range(3)])
        v = jacobi(G, 3, SWEEPS3)[0]
        g = [(Fn[3 * i] * v[0] + Fn[3 * i + 1] * v[1]) + Fn[3 * i + 2] * v[2] for i in range(3)]
        return [Fn[3 * i + j] - g[i] * v[j] for i in range(3) for j in range(3)]


def denormalise(Fn, norm):
    """step 7: T2^T (Fn T1) over its entry of largest magnitude, rounded to float32: (F (9,) float32, ok)"""
    s1, c1x, c1y, s2, c2x, c2y = norm
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(all="ignore"):
        T1 = [s1, zero, -(s1 * c1x), zero, s1, -(s1 * c1y), zero, zero, one]
        T2t = [s2, zero, zero, zero, s2, zero, -(s2 * c2x), -(s2 * c2y), one]
        G = _mul3(T2t, _mul3(Fn, T1))
        d = G[0]
        for k in range(1, 9):
            if np.abs(G[k]) > np.abs(d):
                d = G[k]
        F = np.array([np.float32(G[k] / d) for k in range(9)], np.float32)
    return F, bool(d != 0.0 and np.isfinite(d) and np.isfinite(F).all())


def refit_round(rec, F, t2):
    """one round (steps 1-7 up to the scoring) from the model F: (F' float32 (9,), ok)"""
    nm = normal_matrix(rec, inlier_mask(F, rec, t2)[0])
    if nm is None:
        return None, False
    f = jacobi(nm[0], 9, SWEEPS9)[0]
    if not np.isfinite(f).all():
        return None, False
    return denormalise(rank2(f), nm[1])


def refine_fundamental(matches, record, threshold=1.0, rounds=3):
    """-> (record of FUNDAMENTAL_DTYPE, mask uint8 (n,))"""
    assert 1 <= rounds <= 8
    rec = records(matches)
    n = len(rec)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), FUNDAMENTAL_DTYPE)
    out["hypothesis"], out["n"] = -1, n
    mask = np.zeros(n, np.uint8)
    cur = np.array(record["F"], np.float32).reshape(9)
    if int(record["hypothesis"]) < 0 or not np.isfinite(cur).all():
        return out, mask
    cnt = int(inlier_mask(cur, rec, t2)[0].sum())
    root = int(record["root"])
    for _ in range(rounds):
        F, ok = refit_round(rec, cur, t2)
        if not ok:
            break
        c = int(inlier_mask(F, rec, t2)[0].sum())
        if c < cnt:
            break
        cur, cnt, root = F, c, REFINED_ROOT
    out["F"], out["inliers"], out["hypothesis"], out["root"] = cur, cnt, int(record["hypothesis"]), root
    mask[:] = inlier_mask(cur, rec, t2)[0]
    return out, mask

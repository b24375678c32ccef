"""numpy statement of hak_solve_pnp (include/hipakaze.h): RANSAC absolute pose from 3-D to 2-D correspondences by Grunert's
three-point solve, bit for bit.

The checker only -- the product never calls it.  Vectorised over hypotheses: float64 for the sample and its solve (+ - * / sqrt
only; the quartic's critical points by the cubic routine of fundamental_ref, its roots by bracketing and 64 bisections), float32
for the scoring.  numpy forms no FMA, and every expression below is written in the evaluation order of kernels_pnp.hip.
"""
import numpy as np

import homography_ref as hr
from fundamental_ref import real_roots
from pose_ref import _cross, _dot, intrinsics

CORR3D_DTYPE = np.dtype([("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("u", "<f4"), ("v", "<f4"), ("src3d", "<i4"), ("src2d", "<i4"),
                         ("pad", "<i4")])
ABS_POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("solution", "<i4"),
                           ("n", "<i4")])
assert CORR3D_DTYPE.itemsize == 32 and ABS_POSE_DTYPE.itemsize == 64

DRAWS = 16


def records(corr):
    """(n, 5) float32 {X, Y, Z, u, v} from a CORR3D structured array or an (n, 5) array; a row with a non-finite field gets
    X = NaN, as the kernels load it"""
    if corr.dtype.names:
        r = np.stack([corr[f] for f in ("X", "Y", "Z", "u", "v")], axis=1).astype(np.float32)
    else:
        r = np.array(corr, np.float32).reshape(-1, 5)
    r = r.copy()
    r[~np.isfinite(r).all(axis=1), 0] = np.float32(np.nan)
    return r


def sample_indices(seed, h, n):
    """step 1: (len(h), 3) int64 indices (-1 where not drawn) and a validity flag per hypothesis"""
    return hr.sample_indices(seed, h, n, 3, DRAWS)


def _sub(a, b):
    return [a[i] - b[i] for i in range(3)]


def _triad(P1, P2, P3):
    """step 5's orthonormal triad of three points: (e1, e2, e3, ok)"""
    d1, d2 = _sub(P2, P1), _sub(P3, P1)
    l1 = np.sqrt(_dot(d1, d1))
    e1 = [v / l1 for v in d1]
    nv = _cross(d1, d2)
    ln = np.sqrt(_dot(nv, nv))
    e3 = [v / ln for v in nv]
    e2 = _cross(e3, e1)
    return e1, e2, e3, np.isfinite(l1) & (l1 > 0.0) & np.isfinite(ln) & (ln > 0.0)


def quartic(a2, b2, c2, ca, cb, cg):
    """step 3: (A4, A3, A2, A1, A0, p)"""
    p, q = (a2 - c2) / b2, (a2 + c2) / b2
    rab, rcb, rbc, rba = a2 / b2, c2 / b2, (b2 - c2) / b2, (b2 - a2) / b2
    ca2, cb2, cg2 = ca * ca, cb * cb, cg * cg
    pm, pp, pq = p - 1.0, p * p, 1.0 + p
    A4 = pm * pm - 4.0 * (rcb * ca2)
    A3 = 4.0 * (((p * (1.0 - p)) * cb - ((1.0 - q) * ca) * cg) + 2.0 * ((rcb * ca2) * cb))
    A2 = 2.0 * (((((pp - 1.0) + 2.0 * (pp * cb2)) + 2.0 * (rbc * ca2)) - 4.0 * (((q * ca) * cb) * cg)) + 2.0 * (rba * cg2))
    A1 = 4.0 * (((-(p * pq)) * cb + 2.0 * ((rab * cg2) * cb)) - ((1.0 - q) * ca) * cg)
    A0 = pq * pq - 4.0 * (rab * cg2)
    return A4, A3, A2, A1, A0, p


def positive_roots(A4, A3, A2, A1, A0):
    """step 4: (roots (H, 4), count (H,), ok (H,)); roots beyond the count are NaN"""
    nh = len(A4)
    rows = np.arange(nh)
    ok = (A4 != 0.0) & np.isfinite(A4) & np.isfinite(A3) & np.isfinite(A2) & np.isfinite(A1) & np.isfinite(A0)
    b3, b2, b1, b0 = A3 / A4, A2 / A4, A1 / A4, A0 / A4

    def q(v):
        return (((v + b3) * v + b2) * v + b1) * v + b0

    m = np.abs(b3)
    for b in (b2, b1, b0):
        m = np.where(np.abs(b) > m, np.abs(b), m)
    bound = 1.0 + m
    ok &= np.isfinite(b3) & np.isfinite(b2) & np.isfinite(b1) & np.isfinite(b0) & np.isfinite(bound)
    crit, ccount, okc = real_roots(np.ones(nh), 0.75 * b3, 0.5 * b2, 0.25 * b1)
    ok &= okc
    pts = np.zeros((nh, 5))
    cnt = np.ones(nh, np.int64)                                         # pts[:, 0] = 0
    for r in range(3):
        c = crit[:, r]
        keep = (r < ccount) & (c > 0.0) & (c < bound)
        pts[rows[keep], cnt[keep]] = c[keep]
        cnt = cnt + keep
    pts[rows, cnt] = bound
    roots = np.full((nh, 4), np.nan)
    count = np.zeros(nh, np.int64)
    for j in range(4):
        lo, hi = pts[:, j].copy(), pts[:, min(j + 1, 4)].copy()
        neg = q(lo) < 0.0
        has = ok & (j < cnt) & (neg != (q(hi) < 0.0))
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            left = (q(mid) < 0.0) == neg
            lo = np.where(left, mid, lo)
            hi = np.where(left, hi, mid)
        r = 0.5 * (lo + hi)
        roots[rows[has], count[has]] = r[has]
        count = count + has
    return roots, count, ok


def models(rec, K, seed, h):
    """steps 1-5 for hypotheses h: (M (len(h), 4, 12) float32 {R row-major, t}, valid (len(h), 4) bool)"""
    n = len(rec)
    h = np.asarray(h, np.int64)
    M = np.zeros((len(h), 4, 12), np.float32)
    valid = np.zeros((len(h), 4), bool)
    if n < 3 or len(h) == 0:
        return M, valid
    idx, ok = sample_indices(seed, h, n)
    pt = rec[np.where(idx < 0, 0, idx)].astype(np.float64)              # (H, 3, 5)
    fx, fy, cx, cy = (np.float64(K[f]) for f in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        X, b = [], []
        for k in range(3):
            X.append([pt[:, k, 0], pt[:, k, 1], pt[:, k, 2]])
            x, y = (pt[:, k, 3] - cx) / fx, (pt[:, k, 4] - cy) / fy
            nrm = np.sqrt((x * x + y * y) + 1.0)
            b.append([x / nrm, y / nrm, 1.0 / nrm])
        da, db, dc = _sub(X[1], X[2]), _sub(X[0], X[2]), _sub(X[0], X[1])
        a2, b2, c2 = _dot(da, da), _dot(db, db), _dot(dc, dc)
        ca, cb, cg = _dot(b[1], b[2]), _dot(b[0], b[2]), _dot(b[0], b[1])
        ok = ok & (b2 != 0.0)
        for v in (a2, b2, c2, ca, cb, cg):
            ok = ok & np.isfinite(v)
        A4, A3, A2, A1, A0, p = quartic(a2, b2, c2, ca, cb, cg)
        roots, count, okr = positive_roots(A4, A3, A2, A1, A0)
        ok = ok & okr
        f1, f2, f3, okf = _triad(X[0], X[1], X[2])
        ok = ok & okf
        pm, pq = p - 1.0, 1.0 + p
        for s in range(4):
            v = roots[:, s]
            vv = v * v
            den = 2.0 * (cg - v * ca)
            w = (1.0 + vv) - (2.0 * v) * cb
            u = ((pm * vv - ((2.0 * p) * cb) * v) + pq) / den
            s1 = np.sqrt(b2 / w)
            s2, s3 = u * s1, v * s1
            good = ok & (s < count) & (den != 0.0) & (w > 0.0)
            for sc in (s1, s2, s3):
                good = good & np.isfinite(sc) & (sc > 0.0)
            P = [[sc * c for c in b[k]] for k, sc in enumerate((s1, s2, s3))]
            e1, e2, e3, oke = _triad(P[0], P[1], P[2])
            good = good & oke
            R = [(e1[i] * f1[j] + e2[i] * f2[j]) + e3[i] * f3[j] for i in range(3) for j in range(3)]
            t = [P[0][i] - _dot(R[3 * i:3 * i + 3], X[0]) for i in range(3)]
            Ms = np.stack([v_.astype(np.float32) for v_ in R + t], axis=-1)
            good = good & np.isfinite(Ms).all(axis=-1)
            M[:, s] = np.where(good[:, None], Ms, np.float32(0.0))
            valid[:, s] = good
    return M, valid


def inlier_mask(M, rec, K, t2):
    """step 6: bool (len(M), n) for float32 models (k, 12), records (n, 5) float32, K of INTRINSICS_DTYPE, t2 float32"""
    M = np.asarray(M, np.float32).reshape(-1, 12)
    X, Y, Z, u, v = (rec[None, :, c] for c in range(5))
    m = [M[:, k:k + 1] for k in range(12)]
    fx, fy, cx, cy = (np.float32(K[f]) for f in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        xc = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[9]
        yc = ((m[3] * X + m[4] * Y) + m[5] * Z) + m[10]
        zc = ((m[6] * X + m[7] * Y) + m[8] * Z) + m[11]
        ex = (fx * xc + cx * zc) - u * zc
        ey = (fy * yc + cy * zc) - v * zc
        return (zc > 0) & (ex * ex + ey * ey < t2 * (zc * zc))


def solve_pnp(corr, K, iterations=1024, threshold=1.0, seed=0, block=256):
    """-> (record of ABS_POSE_DTYPE, mask uint8 (n,))"""
    rec = records(corr)
    n = len(rec)
    K = intrinsics(K)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), ABS_POSE_DTYPE)
    out["R"], out["hypothesis"], out["n"] = np.eye(3, dtype=np.float32).reshape(9), -1, n
    best = hr.best_model(iterations, block, lambda hs: models(rec, K, seed, hs),              # inliers, h, solution, model
                         lambda M: inlier_mask(M, rec, K, t2).sum(axis=1))
    mask = np.zeros(n, np.uint8)
    if best[1] < 0:
        return out, mask
    out["R"], out["t"] = best[3][:9], best[3][9:]
    out["inliers"], out["hypothesis"], out["solution"] = best[0], best[1], best[2]
    mask[:] = inlier_mask(best[3], rec, K, t2)[0]
    return out, mask

"""numpy statement of hak_refine_pnp (include/hipakaze.h): Gauss-Newton refit of an absolute pose over its inliers, iterated, bit
for bit.

The checker only -- the product never calls it.  float64 without FMA, + - * / only: the residuals and Jacobian rows per inlier,
the 27 sums in the device order of homography_ref._lanes (lane l of a wave takes the correspondences i = l mod 64 in ascending i,
then an xor butterfly), the 6 x 7 elimination with partial pivoting of hak_find_homography's refit, the Cayley update; float32
reprojection scoring by pnp_ref.inlier_mask.  Every expression below is written in the evaluation order of kernels_pnprefit.hip.
"""
import numpy as np

from homography_ref import _lanes
from pnp_ref import ABS_POSE_DTYPE, inlier_mask, records
from pose_ref import intrinsics

MIN_INLIERS = 4
REFINED_SOLUTION = 4
# where a call stops (`trace` of refine_pnp): the record has no model; step 1 finds fewer than four inliers; a pivot of step 4 is 0
# or non-finite; the solution or the updated pose is non-finite; the candidate scores below the current pose; every round was used
NO_MODEL, FEW, SINGULAR, NON_FINITE, REJECTED, ROUNDS = "no model", "m < 4", "singular", "non-finite", "rejected", "rounds"


def normal_equations(rec, K, cur, mask):
    """steps 2 and 3 for the pose cur (12 float32: R row-major, t) over the masked records: the 6 x 7 float64 system [N | g]"""
    M = [np.float64(v) for v in np.asarray(cur, np.float32).reshape(12)]
    fx, fy, cx, cy = (np.float64(K[f]) for f in ("fx", "fy", "cx", "cy"))
    r = rec.astype(np.float64)
    X, Y, Z, u, v = (r[:, c] for c in range(5))
    with np.errstate(all="ignore"):
        xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[9]
        yc = ((M[3] * X + M[4] * Y) + M[5] * Z) + M[10]
        zc = ((M[6] * X + M[7] * Y) + M[8] * Z) + M[11]
        iz = 1.0 / zc
        a, b = xc * iz, yc * iz
        rx, ry = (fx * a + cx) - u, (fy * b + cy) - v
        px, py = fx * iz, fy * iz
        zero = np.zeros_like(px)
        jx = [-((px * a) * yc), px * zc + (px * a) * xc, -(px * yc), px, zero, -(px * a)]
        jy = [(-(py * zc)) - (py * b) * yc, (py * b) * xc, py * xc, zero, py, -(py * b)]
        cols = [jx[p] * jx[q] + jy[p] * jy[q] for p in range(6) for q in range(p, 6)]
        cols += [-(jx[p] * rx + jy[p] * ry) for p in range(6)]
        sums = _lanes(np.stack(cols, axis=1), mask)
    S = np.zeros((6, 7), np.float64)
    k = 0
    for p in range(6):
        for q in range(p, 6):
            S[p, q] = S[q, p] = sums[k]
            k += 1
    S[:, 6] = sums[21:]
    return S


def solve(S):
    """step 4: Gaussian elimination with partial pivoting of the 6 x 7 system, as hak_find_homography's refit solves its 8 x 9:
    (d (6,) float64, None) or (None, SINGULAR / NON_FINITE)"""
    M = np.array(S, np.float64).reshape(6, 7).copy()
    with np.errstate(all="ignore"):
        for c in range(6):
            piv, best = c, abs(M[c, c])
            for r_ in range(c + 1, 6):
                if abs(M[r_, c]) > best:
                    best, piv = abs(M[r_, c]), r_
            if not (best > 0.0) or not np.isfinite(best):
                return None, SINGULAR
            if piv != c:
                M[[c, piv], c:] = M[[piv, c], c:]
            for r_ in range(c + 1, 6):
                f = M[r_, c] / M[c, c]
                for q_ in range(c + 1, 7):
                    M[r_, q_] = M[r_, q_] - f * M[c, q_]
        d = np.zeros(6, np.float64)
        for i in range(5, -1, -1):
            acc = M[i, 6]
            for j in range(i + 1, 6):
                acc = acc - M[i, j] * d[j]
            d[i] = acc / M[i, i]
    if not np.isfinite(d).all():
        return None, NON_FINITE
    return d, None


def cayley_update(cur, d):
    """step 5 up to the scoring: (the candidate pose as 12 float32, ok)"""
    M = [np.float64(v) for v in np.asarray(cur, np.float32).reshape(12)]
    d = [np.float64(v) for v in d]
    with np.errstate(all="ignore"):
        w0, w1, w2 = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
        ww = (w0 * w0 + w1 * w1) + w2 * w2
        k, den = 1.0 - ww, 1.0 + ww
        Cm = [k + 2.0 * (w0 * w0), 2.0 * (w0 * w1 - w2), 2.0 * (w0 * w2 + w1),
              2.0 * (w0 * w1 + w2), k + 2.0 * (w1 * w1), 2.0 * (w1 * w2 - w0),
              2.0 * (w0 * w2 - w1), 2.0 * (w1 * w2 + w0), k + 2.0 * (w2 * w2)]
        Cm = [c / den for c in Cm]
        R = [(Cm[3 * i] * M[j] + Cm[3 * i + 1] * M[3 + j]) + Cm[3 * i + 2] * M[6 + j] for i in range(3) for j in range(3)]
        t = [((Cm[3 * i] * M[9] + Cm[3 * i + 1] * M[10]) + Cm[3 * i + 2] * M[11]) + d[3 + i] for i in range(3)]
        out = np.array([np.float32(v) for v in R + t], np.float32)
    return out, bool(np.isfinite(out).all())


def refit_round(rec, K, cur, t2):
    """steps 1-5 up to the scoring, from the pose cur: (the candidate (12,) float32 or None, None or why the round failed)"""
    mask = inlier_mask(cur, rec, K, t2)[0]
    if int(mask.sum()) < MIN_INLIERS:
        return None, FEW
    d, why = solve(normal_equations(rec, K, cur, mask))
    if d is None:
        return None, why
    cand, ok = cayley_update(cur, d)
    return (cand, None) if ok else (None, NON_FINITE)


def refine_pnp(corr, K, record, threshold=2.0, rounds=3, trace=None):
    """-> (record of ABS_POSE_DTYPE, mask uint8 (n,)); `trace`, a list, receives (accepted rounds, where the call stopped)"""
    assert 1 <= rounds <= 8
    rec = records(corr)
    n = len(rec)
    K = intrinsics(K)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), ABS_POSE_DTYPE)
    out["R"], out["hypothesis"], out["n"] = np.eye(3, dtype=np.float32).reshape(9), -1, n
    mask = np.zeros(n, np.uint8)
    cur = np.concatenate([np.array(record["R"], np.float32).reshape(9), np.array(record["t"], np.float32).reshape(3)])
    if int(record["hypothesis"]) < 0 or not np.isfinite(cur).all():
        if trace is not None:
            trace.append((0, NO_MODEL))
        return out, mask
    cnt = int(inlier_mask(cur, rec, K, t2)[0].sum())
    solution = int(record["solution"])
    accepted, why = 0, ROUNDS
    for _ in range(rounds):
        cand, why = refit_round(rec, K, cur, t2)
        if cand is None:
            break
        c = int(inlier_mask(cand, rec, K, t2)[0].sum())
        if c < cnt:
            why = REJECTED
            break
        cur, cnt, solution, accepted, why = cand, c, REFINED_SOLUTION, accepted + 1, ROUNDS
    if trace is not None:
        trace.append((accepted, why))
    out["R"], out["t"], out["inliers"], out["hypothesis"], out["solution"] = cur[:9], cur[9:], cnt, int(record["hypothesis"]), solution
    mask[:] = inlier_mask(cur, rec, K, t2)[0]
    return out, mask

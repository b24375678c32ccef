"""numpy statement of hak_refine_pose (include/hipakaze.h): calibrated Gauss-Newton refit of a relative pose over the matches that
count under it, iterated, bit for bit.

The checker only -- the product never calls it.  float64 without FMA, + - * / sqrt only: the float32 F of a pose, the matches that
count under it (float32 Sampson inliers of that F by fundamental_ref.inlier_mask, in front by pose_ref.front_mask), per round the
residuals and Jacobian rows, the 20 sums in the device order of homography_ref._lanes (lane l of a wave takes the matches
i = l mod 64 in ascending i, then an xor butterfly), the 5 x 6 elimination with partial pivoting of hak_find_homography's refit,
the Cayley update of R and the renormalised tangent step of t.  Every expression below is written in the evaluation order of
kernels_poserefit.hip.
"""
import numpy as np

from fundamental_ref import inlier_mask, records
from homography_ref import _lanes
from pose_ref import POSE_DTYPE, _cross, _dot, depths, front_mask, intrinsics

MIN_COUNT = 5
REFINED_CANDIDATE = 4
# where a call stops (`trace` of refine_pose): the record has no model; fewer than five matches count; a pivot is 0 or non-finite;
# the solution, the updated pose or its F is non-finite; the candidate scores below the current pose; every round was used
NO_MODEL, FEW, SINGULAR, NON_FINITE, REJECTED, ROUNDS = "no model", "m < 5", "singular", "non-finite", "rejected", "rounds"


def _k(K):
    return tuple(np.float64(K[f]) for f in ("fx", "fy", "cx", "cy"))


def pose_F(R, t, K1, K2):
    """step 2: (the float32 F (9,) of the pose (R, t as float32), ok)"""
    R = [np.float64(v) for v in np.asarray(R, np.float32).reshape(9)]
    t = [np.float64(v) for v in np.asarray(t, np.float32).reshape(3)]
    fx1, fy1, cx1, cy1 = _k(K1)
    fx2, fy2, cx2, cy2 = _k(K2)
    F = [None] * 9
    with np.errstate(all="ignore"):
        for j in range(3):
            F[j] = t[1] * R[6 + j] - t[2] * R[3 + j]
            F[3 + j] = t[2] * R[j] - t[0] * R[6 + j]
            F[6 + j] = t[0] * R[3 + j] - t[1] * R[j]
        for i in range(3):
            g0, g1 = F[3 * i] / fx1, F[3 * i + 1] / fy1
            F[3 * i + 2] = (F[3 * i + 2] - g0 * cx1) - g1 * cy1
            F[3 * i], F[3 * i + 1] = g0, g1
        for j in range(3):
            f0, f1 = F[j] / fx2, F[3 + j] / fy2
            F[6 + j] = (F[6 + j] - f0 * cx2) - f1 * cy2
            F[j], F[3 + j] = f0, f1
        d = F[0]
        for k in range(1, 9):
            if np.abs(F[k]) > np.abs(d):
                d = F[k]
        out = np.array([np.float32(F[k] / d) for k in range(9)], np.float32)
    return out, bool(d != 0.0 and np.isfinite(d))


def counting(rec, K1, K2, cur, t2, md):
    """the matches that count under the model cur (21 float32: R, t, F): (inliers of F (n,) bool, of those in front (n,) bool)"""
    inl = inlier_mask(cur[12:], rec, t2)[0]
    R = [np.float64(v) for v in cur[:9]]
    t = [np.float64(v) for v in cur[9:12]]
    return inl, inl & front_mask(rec, K1, K2, R, t, md)


def tangent_basis(t):
    """(b1, b2) of t (three float64)"""
    a = [np.abs(v) for v in t]
    k = (2 if a[2] < a[1] else 1) if a[1] < a[0] else (2 if a[2] < a[0] else 0)
    zero = np.float64(0.0)
    nv = [[zero, t[2], -t[1]], [-t[2], zero, t[0]], [t[1], -t[0], zero]][k]
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(nv, nv))
        b1 = [nv[i] / ln for i in range(3)]
        return b1, _cross(t, b1)


def normal_equations(rec, K1, K2, cur, mask):
    """step 3 for the model cur over the masked records: the 5 x 6 float64 system [N | g]"""
    R = [np.float64(v) for v in cur[:9]]
    t = [np.float64(v) for v in cur[9:12]]
    fx1, fy1, cx1, cy1 = _k(K1)
    fx2, fy2, cx2, cy2 = _k(K2)
    r = rec.astype(np.float64)
    with np.errstate(all="ignore"):
        b1, b2 = tangent_basis(t)
        x, y = (r[:, 0] - cx1) / fx1, (r[:, 1] - cy1) / fy1
        b = [(r[:, 2] - cx2) / fx2, (r[:, 3] - cy2) / fy2, np.ones(len(r))]
        q = [(R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] for k in range(3)]
        c = _cross(t, q)
        e = _dot(b, c)
        v = _cross(b, t)
        u0 = (R[0] * v[0] + R[3] * v[1]) + R[6] * v[2]
        u1 = (R[1] * v[0] + R[4] * v[1]) + R[7] * v[2]
        p0, p1, p2, p3 = c[0] / fx2, c[1] / fy2, u0 / fx1, u1 / fy1
        s = np.sqrt((p0 * p0 + p1 * p1) + (p2 * p2 + p3 * p3))
        res = e / s
        jw = _cross(q, v)
        h = _cross(q, b)
        w = [jw[0] / s, jw[1] / s, jw[2] / s, _dot(h, b1) / s, _dot(h, b2) / s]
        cols = [w[p] * w[q_] for p in range(5) for q_ in range(p, 5)]
        cols += [-(w[p] * res) for p in range(5)]
        sums = _lanes(np.stack([np.broadcast_to(col, (len(r),)) for col in cols], axis=1), mask)
    S = np.zeros((5, 6), np.float64)
    k = 0
    for p in range(5):
        for q_ in range(p, 5):
            S[p, q_] = S[q_, p] = sums[k]
            k += 1
    S[:, 5] = sums[15:]
    return S


def solve(S):
    """Gaussian elimination with partial pivoting of the 5 x 6 system, as hak_find_homography's refit solves its 8 x 9:
    (d (5,) float64, None) or (None, SINGULAR / NON_FINITE)"""
    M = np.array(S, np.float64).reshape(5, 6).copy()
    with np.errstate(all="ignore"):
        for c in range(5):
            piv, best = c, abs(M[c, c])
            for r_ in range(c + 1, 5):
                if abs(M[r_, c]) > best:
                    best, piv = abs(M[r_, c]), r_
            if not (best > 0.0) or not np.isfinite(best):
                return None, SINGULAR
            if piv != c:
                M[[c, piv], c:] = M[[piv, c], c:]
            for r_ in range(c + 1, 5):
                f = M[r_, c] / M[c, c]
                for q_ in range(c + 1, 6):
                    M[r_, q_] = M[r_, q_] - f * M[c, q_]
        d = np.zeros(5, np.float64)
        for i in range(4, -1, -1):
            acc = M[i, 5]
            for j in range(i + 1, 5):
                acc = acc - M[i, j] * d[j]
            d[i] = acc / M[i, i]
    if not np.isfinite(d).all():
        return None, NON_FINITE
    return d, None


def update(cur, d, K1, K2):
    """the update of step 3: (the candidate model (21,) float32, ok)"""
    R = [np.float64(v) for v in cur[:9]]
    t = [np.float64(v) for v in cur[9:12]]
    d = [np.float64(v) for v in d]
    with np.errstate(all="ignore"):
        b1, b2 = tangent_basis(t)
        w0, w1, w2 = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
        ww = (w0 * w0 + w1 * w1) + w2 * w2
        k, den = 1.0 - ww, 1.0 + ww
        Cm = [k + 2.0 * (w0 * w0), 2.0 * (w0 * w1 - w2), 2.0 * (w0 * w2 + w1),
              2.0 * (w0 * w1 + w2), k + 2.0 * (w1 * w1), 2.0 * (w1 * w2 - w0),
              2.0 * (w0 * w2 - w1), 2.0 * (w1 * w2 + w0), k + 2.0 * (w2 * w2)]
        Cm = [c / den for c in Cm]
        Rn = [(Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
        tn = [(t[i] + d[3] * b1[i]) + d[4] * b2[i] for i in range(3)]
        ln = np.sqrt(_dot(tn, tn))
        pose = np.array([np.float32(v) for v in Rn] + [np.float32(tn[i] / ln) for i in range(3)], np.float32)
    ok = bool(np.isfinite(ln) and np.isfinite(pose).all())
    F, okf = pose_F(pose[:9], pose[9:], K1, K2)
    return np.concatenate([pose, F]), ok and okf


def refit_round(rec, K1, K2, cur, t2, md):
    """one round from the model cur: (the candidate (21,) float32 or None, None or why the round failed)"""
    mask = counting(rec, K1, K2, cur, t2, md)[1]
    if int(mask.sum()) < MIN_COUNT:
        return None, FEW
    d, why = solve(normal_equations(rec, K1, K2, cur, mask))
    if d is None:
        return None, why
    cand, ok = update(cur, d, K1, K2)
    return (cand, None) if ok else (None, NON_FINITE)


def count_under(matches, record, K1, K2=None, threshold=1.0, max_depth=np.inf):
    """step 2 alone: how many matches count under the record's pose at this threshold (0 without a model)"""
    rec = records(matches)
    K1 = intrinsics(K1)
    K2 = K1 if K2 is None else intrinsics(K2)
    pose = np.concatenate([np.array(record["R"], np.float32).reshape(9), np.array(record["t"], np.float32).reshape(3)])
    if int(record["candidate"]) < 0 or not np.isfinite(pose).all():
        return 0
    F, ok = pose_F(pose[:9], pose[9:], K1, K2)
    if not ok:
        return 0
    t2 = np.float32(threshold) * np.float32(threshold)
    return int(counting(rec, K1, K2, np.concatenate([pose, F]), t2, max_depth)[1].sum())


def refine_pose(matches, K1, record, K2=None, threshold=1.0, max_depth=np.inf, rounds=3, trace=None):
    """-> (record of POSE_DTYPE, mask uint8 (n,), xyz float32 (n, 3)); `trace`, a list, receives (accepted rounds, where the call
    stopped)"""
    assert 1 <= rounds <= 8
    rec = records(matches)
    n = len(rec)
    K1 = intrinsics(K1)
    K2 = K1 if K2 is None else intrinsics(K2)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), POSE_DTYPE)
    out["R"], out["candidate"], out["n"] = np.eye(3, dtype=np.float32).reshape(9), -1, n
    mask, xyz = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    pose = np.concatenate([np.array(record["R"], np.float32).reshape(9), np.array(record["t"], np.float32).reshape(3)])
    F, ok = pose_F(pose[:9], pose[9:], K1, K2)
    if int(record["candidate"]) < 0 or not np.isfinite(pose).all() or not ok:
        if trace is not None:
            trace.append((0, NO_MODEL))
        return out, mask, xyz
    cur = np.concatenate([pose, F])
    cnt = int(counting(rec, K1, K2, cur, t2, max_depth)[1].sum())
    candidate = int(record["candidate"])
    accepted, why = 0, ROUNDS
    for _ in range(rounds):
        cand, why = refit_round(rec, K1, K2, cur, t2, max_depth)
        if cand is None:
            break
        c = int(counting(rec, K1, K2, cand, t2, max_depth)[1].sum())
        if c < cnt:
            why = REJECTED
            break
        cur, cnt, candidate, accepted, why = cand, c, REFINED_CANDIDATE, accepted + 1, ROUNDS
    if trace is not None:
        trace.append((accepted, why))
    inl, front = counting(rec, K1, K2, cur, t2, max_depth)
    out["R"], out["t"], out["inliers"], out["in_front"], out["candidate"] = cur[:9], cur[9:12], int(inl.sum()), cnt, candidate
    mask[:] = front
    R = [np.float64(v) for v in cur[:9]]
    t = [np.float64(v) for v in cur[9:12]]
    _, z1, _, x, y = depths(rec, K1, K2, R, t)
    with np.errstate(all="ignore"):
        pts = np.stack([z1 * x, z1 * y, z1], axis=1).astype(np.float32)
    xyz[front] = pts[front]
    return out, mask, xyz

"""numpy statement of hak_recover_pose (include/hipakaze.h): relative pose, front mask and first 3-D points of a match list from
its fundamental matrix and the two cameras' intrinsics, bit for bit.

The checker only -- the product never calls it.  float64 without FMA, + - * / sqrt only; float32 Sampson inliers by
fundamental_ref.inlier_mask; the 3 x 3 eigen-solve is fundamental_refit_ref.jacobi.  Every expression below is written in the
evaluation order of kernels_pose.hip.  The counts are integers, so no summation order is part of the rule.
"""
import numpy as np

from fundamental_ref import inlier_mask, records
from fundamental_refit_ref import SWEEPS3, jacobi
from homography_ref import _mul3

INTRINSICS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("in_front", "<i4"), ("candidate", "<i4"),
                       ("n", "<i4")])
assert INTRINSICS_DTYPE.itemsize == 16 and POSE_DTYPE.itemsize == 64


def intrinsics(K):
    """an INTRINSICS_DTYPE record from (fx, fy, cx, cy), a 3 x 3 matrix or a record"""
    if isinstance(K, np.ndarray) and K.dtype == INTRINSICS_DTYPE:
        return K.reshape(()).copy()
    K = np.asarray(K, np.float64)
    v = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(4))
    return np.array(v, INTRINSICS_DTYPE)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _matvec(E, v):
    return [(E[3 * i] * v[0] + E[3 * i + 1] * v[1]) + E[3 * i + 2] * v[2] for i in range(3)]


def essential(F, K1, K2):
    """step 2: (E as nine float64, ok)"""
    one, zero = np.float64(1.0), np.float64(0.0)
    Fd = [np.float64(v) for v in np.asarray(F, np.float32).reshape(9)]
    k1, k2 = ({f: np.float64(K[f]) for f in ("fx", "fy", "cx", "cy")} for K in (K1, K2))
    Km = [k1["fx"], zero, k1["cx"], zero, k1["fy"], k1["cy"], zero, zero, one]
    K2t = [k2["fx"], zero, zero, zero, k2["fy"], zero, k2["cx"], k2["cy"], one]
    with np.errstate(all="ignore"):
        E = _mul3(K2t, _mul3(Fd, Km))
        d = E[0]
        for k in range(1, 9):
            if np.abs(E[k]) > np.abs(d):
                d = E[k]
        if not (d != 0.0 and np.isfinite(d)):
            return None, False
        return [E[k] / d for k in range(9)], True


def decompose(E):
    """steps 3 and 4: (Ra, Rb as nine float64 each, u3 as three float64, ok)"""
    with np.errstate(all="ignore"):
        G = np.array([[(E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j] for j in range(3)] for i in range(3)])
        _, A, V = jacobi(G, 3, SWEEPS3)
        j3 = 0
        for k in range(1, 3):
            if A[k, k] < A[j3, j3]:
                j3 = k
        ja, jb = [j for j in range(3) if j != j3]
        v1, v2 = [V[i, ja] for i in range(3)], [V[i, jb] for i in range(3)]
        v3 = _cross(v1, v2)
        x = _matvec(E, v1)
        l1 = np.sqrt(_dot(x, x))
        u1 = [x[i] / l1 for i in range(3)]
        y = _matvec(E, v2)
        d = _dot(u1, y)
        wv = [y[i] - d * u1[i] for i in range(3)]
        l2 = np.sqrt(_dot(wv, wv))
        u2 = [wv[i] / l2 for i in range(3)]
        u3 = _cross(u1, u2)
        if not (np.isfinite(l1) and l1 > 0.0 and np.isfinite(l2) and l2 > 0.0):
            return None, None, None, False
        Ra = [(u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j] for i in range(3) for j in range(3)]
        Rb = [(u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j] for i in range(3) for j in range(3)]
    return Ra, Rb, u3, True


def depths(rec, K1, K2, R, t):
    """step 5 for every record: (det, z1, z2, x1n (x, y)) as float64 arrays"""
    r = rec.astype(np.float64)
    k1, k2 = ({f: np.float64(K[f]) for f in ("fx", "fy", "cx", "cy")} for K in (K1, K2))
    with np.errstate(all="ignore"):
        x, y = (r[:, 0] - k1["cx"]) / k1["fx"], (r[:, 1] - k1["cy"]) / k1["fy"]
        b = [(r[:, 2] - k2["cx"]) / k2["fx"], (r[:, 3] - k2["cy"]) / k2["fy"], np.ones(len(r))]
        a = [(R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] for i in range(3)]
        aa, bb, ab = _dot(a, a), _dot(b, b), _dot(a, b)
        at, bt = _dot(a, t), _dot(b, t)
        det = aa * bb - ab * ab
        z1 = (ab * bt - bb * at) / det
        z2 = (aa * bt - ab * at) / det
    return det, z1, z2, x, y


def front_mask(rec, K1, K2, R, t, max_depth):
    md = np.float64(np.float32(max_depth))
    det, z1, z2, _, _ = depths(rec, K1, K2, R, t)
    with np.errstate(all="ignore"):
        return (det > 0.0) & (z1 > 0.0) & (z1 < md) & (z2 > 0.0) & (z2 < md)


def candidates(F, K1, K2):
    """the four (R, t) of step 4 as float64 lists, or None when steps 2-3 give no pose"""
    E, ok = essential(F, K1, K2)
    if not ok:
        return None
    Ra, Rb, u3, ok = decompose(E)
    if not ok:
        return None
    neg = [-v for v in u3]
    return [(Ra, u3), (Ra, neg), (Rb, u3), (Rb, neg)]


def recover_pose(matches, F, K1, K2=None, threshold=1.0, max_depth=np.inf):
    """F: nine float32 or a FUNDAMENTAL_DTYPE record -> (record of POSE_DTYPE, mask uint8 (n,), xyz float32 (n, 3))"""
    rec = records(matches)
    n = len(rec)
    K1 = intrinsics(K1)
    K2 = K1 if K2 is None else intrinsics(K2)
    out = np.zeros((), POSE_DTYPE)
    out["R"], out["candidate"], out["n"] = np.eye(3, dtype=np.float32).reshape(9), -1, n
    mask, xyz = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    hyp = 0
    if getattr(F, "dtype", None) is not None and F.dtype.names:       # a record (0-d array or numpy.void)
        hyp, F = int(F["hypothesis"]), F["F"]
    F = np.asarray(F, np.float32).reshape(9)
    if hyp < 0 or not np.isfinite(F).all():
        return out, mask, xyz
    cands = candidates(F, K1, K2)
    if cands is None:
        return out, mask, xyz
    t2 = np.float32(threshold) * np.float32(threshold)
    inl = inlier_mask(F, rec, t2)[0]
    fronts = [inl & front_mask(rec, K1, K2, R, t, max_depth) for R, t in cands]
    best = 0
    for c in range(1, 4):
        if fronts[c].sum() > fronts[best].sum():
            best = c
    R, t = cands[best]
    out["R"], out["t"] = np.array(R, np.float64).astype(np.float32), np.array(t, np.float64).astype(np.float32)
    out["inliers"], out["in_front"], out["candidate"] = int(inl.sum()), int(fronts[best].sum()), best
    mask[:] = fronts[best]
    _, z1, _, x, y = depths(rec, K1, K2, R, t)
    with np.errstate(all="ignore"):
        pts = np.stack([z1 * x, z1 * y, z1], axis=1).astype(np.float32)
    xyz[fronts[best]] = pts[fronts[best]]
    return out, mask, xyz

"""numpy statement of hak_triangulate (include/hipakaze.h): 3-D points of a match list under two known views, bit for bit.

The checker only -- the product never calls it.  float64 without FMA, + - * / only, for the two-ray solve; the float32
reprojection test is pnp_ref.inlier_mask, unchanged.  Every expression below is written in the evaluation order of
kernels_triangulate.hip; float32 inputs are widened before the first operation and the point is rounded by one astype.  The
counts are integers, so no summation order is part of the rule.
"""
import numpy as np

from homography_ref import records
from pnp_ref import ABS_POSE_DTYPE, inlier_mask
from pose_ref import POSE_DTYPE, _dot, intrinsics

TRIANGULATION_DTYPE = np.dtype([("n", "<i4"), ("kept", "<i4"), ("rejected", "<i4", (3,)), ("model", "<i4"), ("pad", "<i4", (2,))])
assert TRIANGULATION_DTYPE.itemsize == 32
VIEW_IDENTITY, VIEW_RELATIVE, VIEW_ABSOLUTE = 0, 1, 2


def view(v):
    """step 1 for one view: (M: twelve float32 {R row-major, t}, model).  v: None (identity), twelve numbers, or a POSE_DTYPE /
    ABS_POSE_DTYPE record (0-d array or numpy.void)"""
    if v is None:
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), True
    model = True
    if getattr(v, "dtype", None) is not None and v.dtype.names:
        model = int(v["candidate"] if "candidate" in v.dtype.names else v["hypothesis"]) >= 0
        v = np.concatenate([np.asarray(v["R"], np.float32).reshape(9), np.asarray(v["t"], np.float32).reshape(3)])
    M = np.asarray(v, np.float32).reshape(12).copy()
    return M, bool(model and np.isfinite(M).all())


def centre(M):
    """step 2: (R as nine float64, the centre as three float64)"""
    R = [np.float64(v) for v in M[:9]]
    t = [np.float64(v) for v in M[9:]]
    return R, [-((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]) for j in range(3)]


def _ray(R, x, y):
    return [(R[j] * x + R[3 + j] * y) + R[6 + j] for j in range(3)]


def solve(rec, MA, MB, KA, KB):
    """steps 2 and 3 for every record: (det, z1, z2, aa bb, cA, cB, a, b), float64"""
    r = rec.astype(np.float64)
    ka, kb = ({f: np.float64(K[f]) for f in ("fx", "fy", "cx", "cy")} for K in (KA, KB))
    RA, cA = centre(MA)
    RB, cB = centre(MB)
    w = [cA[j] - cB[j] for j in range(3)]
    with np.errstate(all="ignore"):
        a = _ray(RA, (r[:, 0] - ka["cx"]) / ka["fx"], (r[:, 1] - ka["cy"]) / ka["fy"])
        b = _ray(RB, (r[:, 2] - kb["cx"]) / kb["fx"], (r[:, 3] - kb["cy"]) / kb["fy"])
        aa, bb, ab, aw, bw = _dot(a, a), _dot(b, b), _dot(a, b), _dot(a, w), _dot(b, w)
        det = aa * bb - ab * ab
        z1 = (ab * bw - bb * aw) / det
        z2 = (aa * bw - ab * aw) / det
        return det, z1, z2, aa * bb, cA, cB, a, b


def gates(matches, viewA, viewB, KA, KB=None, threshold=2.0, max_depth=np.inf, min_sin=0.0):
    """-> (model, first failed gate per match int (n,): 0, 1, 2 or 3 = none, P float32 (n, 3) for every match)"""
    rec = records(matches)
    n = len(rec)
    KA = intrinsics(KA)
    KB = KA if KB is None else intrinsics(KB)
    (MA, okA), (MB, okB) = view(viewA), view(viewB)
    if not (okA and okB):
        return False, np.zeros(n, np.int64), np.zeros((n, 3), np.float32)
    md = np.float64(np.float32(max_depth))
    s2 = np.float64(np.float32(min_sin)) * np.float64(np.float32(min_sin))
    t2 = np.float32(threshold) * np.float32(threshold)
    det, z1, z2, aabb, cA, cB, a, b = solve(rec, MA, MB, KA, KB)
    with np.errstate(all="ignore"):
        g0 = (det > 0.0) & (det >= s2 * aabb)
        g1 = (z1 > 0.0) & (z1 < md) & (z2 > 0.0) & (z2 < md)
        P = np.stack([0.5 * ((cA[j] + z1 * a[j]) + (cB[j] + z2 * b[j])) for j in range(3)], axis=1).astype(np.float32)
        g2 = inlier_mask(MA, np.concatenate([P, rec[:, 0:2]], axis=1), KA, t2)[0] & \
            inlier_mask(MB, np.concatenate([P, rec[:, 2:4]], axis=1), KB, t2)[0]
    return True, np.where(~g0, 0, np.where(~g1, 1, np.where(~g2, 2, 3))), P


def triangulate(matches, viewA, viewB, KA, KB=None, threshold=2.0, max_depth=np.inf, min_sin=0.0):
    """-> (record of TRIANGULATION_DTYPE, mask uint8 (n,), xyz float32 (n, 3))"""
    model, gate, P = gates(matches, viewA, viewB, KA, KB, threshold, max_depth, min_sin)
    n = len(gate)
    out = np.zeros((), TRIANGULATION_DTYPE)
    out["n"] = n
    mask, xyz = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    if not model:
        return out, mask, xyz
    keep = gate == 3
    out["kept"], out["model"] = int(keep.sum()), 1
    out["rejected"] = [int((gate == g).sum()) for g in range(3)]
    mask[:] = keep
    xyz[keep] = P[keep]
    return out, mask, xyz

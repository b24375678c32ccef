"""The numpy statement of projection-guided matching (include/hipakaze.h, hak_match_projected): float32 operations in the stated
order, no FMA (numpy rounds every array operation to float32), the accept rule in Python integers.  The checker of
tests/test_gpu_projected_match.py; tests/test_projected_match_cpu.py checks it against a plain double loop.

The checker only -- the product never calls it."""
import numpy as np

from guided_match_ref import decide, hamming, keys
from pnp_ref import CORR3D_DTYPE
from pose_ref import intrinsics
from triangulate_ref import view


def eligible(A, mask, n_desc):
    """step 1: bool (nA,)"""
    e = A["train"].astype(np.int64)
    ok = (e >= 0) & (e < n_desc)
    if mask is not None:
        ok &= np.asarray(mask).reshape(len(A)) != 0
    return ok


def project(xyz, M, K):
    """step 2: px, py, zc of every landmark: xc, yc, zc as step 6 of hak_solve_pnp, px = (fx (xc / zc)) + cx, py = (fy (yc / zc)) + cy"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    m = [np.float32(v) for v in view(M)[0]]                             # (M in any form view() takes; the model flag is search()'s business)
    K = intrinsics(K)
    fx, fy, cx, cy = (np.float32(K[f]) for f in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        xc = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[9]
        yc = ((m[3] * X + m[4] * Y) + m[5] * Z) + m[10]
        zc = ((m[6] * X + m[7] * Y) + m[8] * Z) + m[11]
        return (fx * (xc / zc)) + cx, (fy * (yc / zc)) + cy, zc


def gate(A, mask, xyz, n_desc, T, M, K, radius):
    """step 3: (nA, n2) bool: eligible, zc > 0 and (dx dx) + (dy dy) < r2; any NaN makes a comparison false"""
    px, py, zc = project(xyz, M, K)
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(all="ignore"):
        dx = T["x"].astype(np.float32)[None, :] - px[:, None]
        dy = T["y"].astype(np.float32)[None, :] - py[:, None]
        return (eligible(A, mask, n_desc) & (zc > 0))[:, None] & ((dx * dx) + (dy * dy) < r2)


def distances(A, mask, D, T):
    """step 4: (nA, n2) int32, d(m, j) for the eligible landmarks (0 elsewhere: such a row is in no gate)"""
    dist = np.zeros((len(A), len(T)), np.int32)
    el = eligible(A, mask, len(D))
    if el.any() and len(T):
        dist[el] = hamming(D[A["train"][el]], T)
    return dist


def search(A, mask, xyz, D, T, v, K, radius, dist=None):
    """steps 1-5 up to the accept rule, which alone depends on ratio, cross_check and max_dist: (k1, k2, rev) -- per landmark the
    smallest and the second smallest key d << 20 | j over J_m, per train point the smallest key d << 20 | m over the landmarks that
    gate it, NONE where there is none -- or None when nothing can be accepted (an empty side, a view without a model).
    dist: distances(A, mask, D, T) when the caller has it."""
    nA, n2 = len(A), len(T)
    M, model = view(v)
    if not (nA and n2 and model):
        return None
    g = gate(A, mask, np.asarray(xyz, np.float32).reshape(nA, 3), len(D), T, M, K, radius)
    return keys(g, distances(A, mask, D, T) if dist is None else dist)


def accept(found, xyz, T, ratio=(4, 5), cross_check=True, max_dist=0):
    """the accept rule and the output of step 6 from search()'s result -> (corr, why) as match_projected returns them"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    why, acc = decide(found, len(xyz), ratio, cross_check, max_dist)
    out = np.zeros(len(acc), CORR3D_DTYPE)
    if acc:
        ms, js = np.array(acc, np.int64).T[:2]
        for k, f in enumerate(("X", "Y", "Z")):                         # the words, copied
            out[f].view(np.uint32)[:] = xyz[ms, k].view(np.uint32)
        out["u"], out["v"] = T["x"][js], T["y"][js]
        out["src3d"], out["src2d"] = ms, js
    return out, why


def match_projected(A, mask, xyz, D, T, v, K, radius, ratio=(4, 5), cross_check=True, max_dist=0, dist=None):
    """A: MATCH_PAIR records (only `train` is read); mask: nA bytes or None; xyz: (nA, 3) float32; D, T: point records; v: a view
    in the forms triangulate_ref.view takes (None, twelve numbers, a POSE_DTYPE or ABS_POSE_DTYPE record).
    -> (corr: CORR3D array of the accepted landmarks in ascending m, why (nA,): 0 accepted, 1 J_m empty (not eligible, no model,
    zc <= 0 or nothing in the gate), 2 d1 >= max_dist, 3 ratio test, 4 cross-check alone)"""
    return accept(search(A, mask, xyz, D, T, v, K, radius, dist), xyz, T, ratio, cross_check, max_dist)

"""The numpy statement of epipolar guided matching (include/hipakaze.h, hak_match_epipolar): float32 operations in the stated order,
no FMA (numpy rounds every array operation to float32), the accept rule in Python integers.  The distance, the packed keys, the
record layout and everything else behind the gate are those of tests/guided_match_ref.py (match_gated); only the gate differs.
The checker of tests/test_gpu_epipolar_match.py; tests/test_epipolar_match_cpu.py checks it against a plain double loop."""
import numpy as np

from guided_match_ref import MATCH_PAIR_DTYPE, NONE, hamming, match_gated  # noqa: F401  (re-exported)

L = np.float32(16384.0)
DEN_MIN = np.float32(2.0 ** -100)


def line(pts1, F):
    """a, b, c, den of every query: a = (F0 x + F1 y) + F2, b = (F3 x + F4 y) + F5, c = (F6 x + F7 y) + F8, den = a a + b b"""
    f = np.asarray(F, np.float32).reshape(9)
    x, y = pts1["x"].astype(np.float32), pts1["y"].astype(np.float32)
    with np.errstate(all="ignore"):
        a = (f[0] * x + f[1] * y) + f[2]
        b = (f[3] * x + f[4] * y) + f[5]
        c = (f[6] * x + f[7] * y) + f[8]
        return a, b, c, a * a + b * b


def gate(pts1, pts2, F, radius):
    """(n1, n2) bool: both points in the domain and e e < r2 den; any NaN makes a comparison false"""
    a, b, c, den = line(pts1, F)
    r2 = np.float32(radius) * np.float32(radius)
    x1, y1 = pts1["x"].astype(np.float32), pts1["y"].astype(np.float32)
    x2, y2 = pts2["x"].astype(np.float32), pts2["y"].astype(np.float32)
    with np.errstate(all="ignore"):
        qdom = (np.abs(x1) <= L) & (np.abs(y1) <= L) & (den >= DEN_MIN) & (den < np.float32(np.inf))
        tdom = (np.abs(x2) <= L) & (np.abs(y2) <= L)
        e = (a[:, None] * x2[None, :] + b[:, None] * y2[None, :]) + c[:, None]
        return qdom[:, None] & tdom[None, :] & ((e * e) < (r2 * den)[:, None])


def match_epipolar(pts1, pts2, F, radius, ratio=(4, 5), cross_check=True, max_dist=0, dist=None, model=True):
    """returns (out, pairs, why): out = a copy of pts1 with match / distance / match_x / match_y as the call writes them, pairs = the
    accepted matches in ascending query order, why[i] = 0 accepted, 1 J_i empty, 2 d1 >= max_dist, 3 ratio test, 4 cross-check alone.
    dist: hamming(pts1, pts2) when the caller has it.  model = False: a batch pair without a model (every query rejected)."""
    return match_gated(pts1, pts2, lambda: gate(pts1, pts2, F, radius), ratio, cross_check, max_dist, dist, model)

"""The numpy statement of epipolar guided matching (include/hipakaze.h, hak_match_epipolar): float32 operations in the stated order,
no FMA (numpy rounds every array operation to float32), the accept rule in Python integers.  The distance, the packed keys and the
record layout are those of tests/guided_match_ref.py; only the gate differs.  The checker of tests/test_gpu_epipolar_match.py;
tests/test_epipolar_match_cpu.py checks it against a plain double loop."""
import numpy as np

from guided_match_ref import MATCH_PAIR_DTYPE, NONE, hamming

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
    n1, n2 = len(pts1), len(pts2)
    max_dist = 96 if max_dist <= 0 else int(max_dist)
    num, den = int(ratio[0]), int(ratio[1])
    out = pts1.copy()
    out["match"], out["distance"], out["match_x"], out["match_y"] = -1, -1, -1.0, -1.0
    why = np.ones(n1, np.int32)
    pairs = []
    if n1 and n2 and model:
        g = gate(pts1, pts2, F, radius)
        d = (hamming(pts1, pts2) if dist is None else dist).astype(np.int64)
        fkey = np.where(g, (d << 20) | np.arange(n2, dtype=np.int64)[None, :], NONE)
        rkey = np.where(g, (d << 20) | np.arange(n1, dtype=np.int64)[:, None], NONE)
        k1 = fkey.min(axis=1)
        j1 = (k1 & 0xFFFFF).astype(np.int64)
        rest = fkey.copy()
        rest[np.arange(n1), j1] = NONE                                   # J_i \ {j1}
        k2 = rest.min(axis=1)
        rev = rkey.min(axis=0)
        for i in range(n1):
            if k1[i] == NONE:
                continue
            d1 = int(k1[i] >> 20)
            d2 = 512 if k2[i] == NONE else int(k2[i] >> 20)
            j = int(j1[i])
            if not d1 < max_dist:
                why[i] = 2
            elif not d1 * den < d2 * num:
                why[i] = 3
            elif cross_check and int(rev[j] & 0xFFFFF) != i:
                why[i] = 4
            else:
                why[i] = 0
                out["match"][i], out["distance"][i] = j, d1
                out["match_x"][i], out["match_y"][i] = pts2["x"][j], pts2["y"][j]
                pairs.append((i, j, d1, d2, pts1["x"][i], pts1["y"][i], pts2["x"][j], pts2["y"][j]))
    return out, np.array(pairs, MATCH_PAIR_DTYPE), why

"""The numpy statement of guided matching (include/hipakaze.h, hak_match_guided): float32 operations in the stated order, no FMA
(numpy rounds every array operation to float32), the accept rule in Python integers.  The checker of tests/test_gpu_guided_match.py;
tests/test_guided_match_cpu.py checks it against a plain double loop."""
import numpy as np

MATCH_PAIR_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                             ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
NONE = 1 << 40                                    # key of "no candidate"


def hamming(pts1, pts2):
    """(n1, n2) int32 Hamming distances over the 61 descriptor bytes: |a ^ b| = |a| + |b| - 2 a.b on the unpacked bits (exact in
    float32: every value is an integer below 2^24)"""
    a = np.unpackbits(np.ascontiguousarray(pts1["features"]), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(pts2["features"]), axis=1).astype(np.float32)
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def project(pts1, H):
    """px, py, wz of every query: wz = (h6 x + h7 y) + h8, u = (h0 x + h1 y) + h2, v = (h3 x + h4 y) + h5, px = u / wz, py = v / wz"""
    h = np.asarray(H, np.float32).reshape(9)
    x, y = pts1["x"].astype(np.float32), pts1["y"].astype(np.float32)
    with np.errstate(all="ignore"):
        wz = (h[6] * x + h[7] * y) + h[8]
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        return u / wz, v / wz, wz


def gate(pts1, pts2, H, radius):
    """(n1, n2) bool: wz > 0 and (dx dx) + (dy dy) < r2; any NaN makes a comparison false"""
    px, py, wz = project(pts1, H)
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(all="ignore"):
        dx = pts2["x"].astype(np.float32)[None, :] - px[:, None]
        dy = pts2["y"].astype(np.float32)[None, :] - py[:, None]
        return (wz > 0)[:, None] & ((dx * dx) + (dy * dy) < r2)


def keys(g, d):
    """the packed keys of a gate matrix g (nq, n2) bool and a distance matrix d (nq, n2): forward keys d << 20 | j and reverse keys
    d << 20 | i where g holds, NONE elsewhere -> (k1, k2, rev): per query the smallest and the second smallest forward key over J_i,
    per train point the smallest reverse key over the queries that gate it"""
    nq, n2 = g.shape
    d = np.asarray(d).astype(np.int64) << 20
    fkey = np.where(g, d | np.arange(n2, dtype=np.int64)[None, :], NONE)
    rev = np.where(g, d | np.arange(nq, dtype=np.int64)[:, None], NONE).min(axis=0)
    k1 = fkey.min(axis=1)
    fkey[np.arange(nq), k1 & 0xFFFFF] = NONE                             # J_i \ {j1}
    return k1, fkey.min(axis=1), rev


def decide(found, nq, ratio=(4, 5), cross_check=True, max_dist=0):
    """the accept decision from keys()'s result (None: nothing can be accepted) -> (why, acc): why[i] = 0 accepted, 1 J_i empty,
    2 d1 >= max_dist, 3 ratio test, 4 cross-check alone; acc = the accepted (i, j1, d1, d2) in ascending i"""
    max_dist = 96 if max_dist <= 0 else int(max_dist)
    num, den = int(ratio[0]), int(ratio[1])
    why = np.ones(nq, np.int32)
    acc = []
    if found is not None:
        k1, k2, rev = found
        for i in np.nonzero(k1 != NONE)[0]:
            d1 = int(k1[i] >> 20)
            d2 = 512 if k2[i] == NONE else int(k2[i] >> 20)
            j = int(k1[i] & 0xFFFFF)
            if not d1 < max_dist:
                why[i] = 2
            elif not d1 * den < d2 * num:
                why[i] = 3
            elif cross_check and int(rev[j] & 0xFFFFF) != i:
                why[i] = 4
            else:
                why[i] = 0
                acc.append((int(i), j, d1, d2))
    return why, acc


def match_gated(pts1, pts2, gate_of, ratio, cross_check, max_dist, dist, model):
    """match_guided / match_epipolar behind their gates: gate_of() gives the (n1, n2) gate matrix"""
    n1, n2 = len(pts1), len(pts2)
    out = pts1.copy()
    out["match"], out["distance"], out["match_x"], out["match_y"] = -1, -1, -1.0, -1.0
    found = keys(gate_of(), hamming(pts1, pts2) if dist is None else dist) if n1 and n2 and model else None
    why, acc = decide(found, n1, ratio, cross_check, max_dist)
    pairs = []
    for i, j, d1, d2 in acc:
        out["match"][i], out["distance"][i] = j, d1
        out["match_x"][i], out["match_y"][i] = pts2["x"][j], pts2["y"][j]
        pairs.append((i, j, d1, d2, pts1["x"][i], pts1["y"][i], pts2["x"][j], pts2["y"][j]))
    return out, np.array(pairs, MATCH_PAIR_DTYPE), why


def match_guided(pts1, pts2, H, radius, ratio=(4, 5), cross_check=True, max_dist=0, dist=None, model=True):
    """returns (out, pairs, why): out = a copy of pts1 with match / distance / match_x / match_y as the call writes them, pairs = the
    accepted matches in ascending query order, why[i] = 0 accepted, 1 J_i empty, 2 d1 >= max_dist, 3 ratio test, 4 cross-check alone.
    dist: hamming(pts1, pts2) when the caller has it.  model = False: a batch pair without a model (every query rejected)."""
    return match_gated(pts1, pts2, lambda: gate(pts1, pts2, H, radius), ratio, cross_check, max_dist, dist, model)

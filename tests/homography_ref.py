"""numpy statement of hak_find_homography (include/hipakaze.h): RANSAC homography over a match list, bit for bit.

The checker only -- the product never calls it.  Vectorised over hypotheses x matches: float64 for the sample and its solve,
float32 for the scoring, and the refit's sums in the device order (lane l of a wave takes matches i = l mod 64 in ascending i,
then an xor butterfly over 32, 16, 8, 4, 2, 1).  numpy forms no FMA, and every expression below is written in the evaluation
order of kernels_homography.hip.
"""
import numpy as np

HOMOGRAPHY_DTYPE = np.dtype([("H", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4"), ("n", "<i4")])
assert HOMOGRAPHY_DTYPE.itemsize == 52         # 9 floats + 4 ints

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
_TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def records(matches):
    """(n, 4) float32 {x1, y1, x2, y2} from a MATCH_PAIR structured array or an (n, 4) array; a row with a non-finite coordinate
    gets x1 = NaN, as the kernels load it"""
    if matches.dtype.names:
        r = np.stack([matches[f] for f in ("x1", "y1", "x2", "y2")], axis=1).astype(np.float32)
    else:
        r = np.array(matches, np.float32).reshape(-1, 4)
    r = r.copy()
    r[~np.isfinite(r).all(axis=1), 0] = np.float32(np.nan)
    return r


def sample_indices(seed, h, n, k=4, draws=16):
    """the sample generator of all three estimators (the homography's k and draws by default): (len(h), k) int64 indices (-1 where
    not drawn) and a validity flag per hypothesis"""
    h = np.asarray(h, np.uint64)
    idx = np.full((len(h), k), -1, np.int64)
    got = np.zeros(len(h), np.int64)
    rows = np.arange(len(h))
    with np.errstate(over="ignore"):
        for d in range(draws):
            r = mix64(np.uint64(seed) + (np.uint64(draws) * h + np.uint64(d + 1)) * _GOLD)
            j = (((r >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
            take = (got < k) & (j[:, None] != idx).all(axis=1)
            idx[rows[take], got[take]] = j[take]
            got = got + take
    return idx, got == k


def best_model(iterations, block, models, count):
    """the RANSAC loop of all three estimators: (inliers, hypothesis, r, model) of the winner, (-1, -1, -1, None) if there is none.
    models(hs) -> (M (len(hs), NM, NW) float32, valid (len(hs), NM) bool); count(M (k, NW)) -> (k,) inlier counts.  The largest
    count wins, ties go to the smallest hypothesis and then its smallest r, whatever the block size"""
    best = (-1, -1, -1, None)
    for h0 in range(0, iterations, block):
        hs = np.arange(h0, min(iterations, h0 + block))
        M, valid = models(hs)
        if not valid.any():
            continue
        hh, rr = np.nonzero(valid)                                      # ascending (h, r)
        cnt = count(M[hh, rr])
        j = int(np.argmax(cnt))                                         # first maximum: the smallest (h, r) of this block
        if cnt[j] > best[0]:
            best = (int(cnt[j]), int(hs[hh[j]]), int(rr[j]), M[hh[j], rr[j]].copy())
    return best


def _square_to_quad(x, y):
    dx1, dx2, dx3 = x[1] - x[2], x[3] - x[2], ((x[0] - x[1]) + x[2]) - x[3]
    dy1, dy2, dy3 = y[1] - y[2], y[3] - y[2], ((y[0] - y[1]) + y[2]) - y[3]
    den = dx1 * dy2 - dx2 * dy1
    g = (dx3 * dy2 - dx2 * dy3) / den
    h = (dx1 * dy3 - dx3 * dy1) / den
    one = np.ones_like(x[0])
    return [(x[1] - x[0]) + g * x[1], (x[3] - x[0]) + h * x[3], x[0],
            (y[1] - y[0]) + g * y[1], (y[3] - y[0]) + h * y[3], y[0], g, h, one]


def _mul3(A, B):
    return [(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _to_float(F):
    """(H float32 (..., 9), ok)"""
    d = F[8]
    ok = (d != 0.0) & np.isfinite(d)
    with np.errstate(all="ignore"):
        H = np.stack([(F[k] / d).astype(np.float32) for k in range(8)] + [np.ones_like(d, np.float32)], axis=-1)
    return H, ok & np.isfinite(H).all(axis=-1)


def hypotheses(rec, seed, h):
    """H (len(h), 9) float32 and validity of hypotheses h over the records rec"""
    n = len(rec)
    h = np.asarray(h, np.int64)
    if n < 4:
        return np.zeros((len(h), 9), np.float32), np.zeros(len(h), bool)
    idx, ok = sample_indices(seed, h, n)
    p = rec[np.where(idx < 0, 0, idx)].astype(np.float64)            # (H, 4, 4)
    ax, ay, bx, by = ([p[:, q, c] for q in range(4)] for c in range(4))
    with np.errstate(all="ignore"):
        for a, b, c in _TRIPLES:
            c1 = (ax[b] - ax[a]) * (ay[c] - ay[a]) - (ay[b] - ay[a]) * (ax[c] - ax[a])
            c2 = (bx[b] - bx[a]) * (by[c] - by[a]) - (by[b] - by[a]) * (bx[c] - bx[a])
            ok &= (np.abs(c1) > 1.0) & (np.abs(c2) > 1.0) & ((c1 > 0.0) == (c2 > 0.0))
        S1, S2 = _square_to_quad(ax, ay), _square_to_quad(bx, by)
        A = [S1[4] * S1[8] - S1[5] * S1[7], S1[2] * S1[7] - S1[1] * S1[8], S1[1] * S1[5] - S1[2] * S1[4],
             S1[5] * S1[6] - S1[3] * S1[8], S1[0] * S1[8] - S1[2] * S1[6], S1[2] * S1[3] - S1[0] * S1[5],
             S1[3] * S1[7] - S1[4] * S1[6], S1[1] * S1[6] - S1[0] * S1[7], S1[0] * S1[4] - S1[1] * S1[3]]
        H, fok = _to_float(_mul3(S2, A))
    return H, ok & fok


def inlier_mask(H, rec, t2):
    """bool (len(H), n) for float32 H (k, 9), records (n, 4) float32, t2 float32"""
    H = np.asarray(H, np.float32).reshape(-1, 9)
    x1, y1, x2, y2 = (rec[None, :, c] for c in range(4))
    h = [H[:, k:k + 1] for k in range(9)]
    with np.errstate(all="ignore"):
        wz = (h[6] * x1 + h[7] * y1) + np.float32(1.0)
        u = (h[0] * x1 + h[1] * y1) + h[2]
        v = (h[3] * x1 + h[4] * y1) + h[5]
        ex = u - x2 * wz
        ey = v - y2 * wz
        return (wz > np.float32(0.0)) & (ex * ex + ey * ey < t2 * (wz * wz))


def _lanes(terms, mask):
    """device order of a sum over the masked rows: per lane l the rows i = l (mod 64) ascending, then the xor butterfly.
    terms: (n, k) float64; returns (k,) float64"""
    n, k = terms.shape
    acc = np.zeros((64, k), np.float64)
    rounds = (n + 63) // 64
    pad = rounds * 64 - n
    t = np.concatenate([terms, np.zeros((pad, k))]).reshape(rounds, 64, k)
    mk = np.concatenate([mask, np.zeros(pad, bool)]).reshape(rounds, 64)
    for r in range(rounds):
        acc = np.where(mk[r][:, None], acc + t[r], acc)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return acc[0]


def refit(rec, mask):
    """the least-squares refit of the masked records: (H float32 (9,), ok)"""
    m = float(int(mask.sum()))
    r = rec.astype(np.float64)
    with np.errstate(all="ignore"):
        s = _lanes(r, mask)
        c1x, c1y, c2x, c2y = s[0] / m, s[1] / m, s[2] / m, s[3] / m
        dx1, dy1, dx2, dy2 = r[:, 0] - c1x, r[:, 1] - c1y, r[:, 2] - c2x, r[:, 3] - c2y
        q = _lanes(np.stack([dx1 * dx1 + dy1 * dy1, dx2 * dx2 + dy2 * dy2], axis=1), mask)
        s1, s2 = np.sqrt((2.0 * m) / q[0]), np.sqrt((2.0 * m) / q[1])
        X, Y = s1 * (r[:, 0] - c1x), s1 * (r[:, 1] - c1y)
        U, V = s2 * (r[:, 2] - c2x), s2 * (r[:, 3] - c2y)
        one, zero = np.ones_like(X), np.zeros_like(X)
        a = [X, Y, one, zero, zero, zero, -(X * U), -(Y * U)]
        b = [zero, zero, zero, X, Y, one, -(X * V), -(Y * V)]
        cols = [a[p] * a[q] + b[p] * b[q] for p in range(8) for q in range(p, 8)]
        cols += [a[p] * U + b[p] * V for p in range(8)]
        sums = _lanes(np.stack(cols, axis=1), mask)
    M = np.zeros((8, 9), np.float64)
    k = 0
    for p in range(8):
        for q in range(p, 8):
            M[p, q] = M[q, p] = sums[k]
            k += 1
    M[:, 8] = sums[36:]
    with np.errstate(all="ignore"):
        for c in range(8):
            piv, best = c, abs(M[c, c])
            for r_ in range(c + 1, 8):
                if abs(M[r_, c]) > best:
                    best, piv = abs(M[r_, c]), r_
            if not (best > 0.0) or not np.isfinite(best):
                return _IDENT.copy(), False
            if piv != c:
                M[[c, piv], c:] = M[[piv, c], c:]
            for r_ in range(c + 1, 8):
                f = M[r_, c] / M[c, c]
                for q_ in range(c + 1, 9):
                    M[r_, q_] = M[r_, q_] - f * M[c, q_]
        hn = np.zeros(9, np.float64)
        for i in range(7, -1, -1):
            acc = M[i, 8]
            for j in range(i + 1, 8):
                acc = acc - M[i, j] * hn[j]
            hn[i] = acc / M[i, i]
        hn[8] = 1.0
        is2 = 1.0 / s2
        T1 = [s1, 0.0, -(s1 * c1x), 0.0, s1, -(s1 * c1y), 0.0, 0.0, 1.0]
        T2i = [is2, 0.0, c2x, 0.0, is2, c2y, 0.0, 0.0, 1.0]
        F = _mul3(T2i, _mul3([np.float64(v) for v in hn], [np.float64(v) for v in T1]))
        H, ok = _to_float([np.float64(v) for v in F])
    return H, bool(ok)


def find_homography(matches, iterations=1024, threshold=3.0, seed=0, refine=True, block=256):
    """-> (record of HOMOGRAPHY_DTYPE, mask uint8 (n,))"""
    rec = records(matches)
    n = len(rec)
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), HOMOGRAPHY_DTYPE)
    out["H"], out["hypothesis"], out["n"] = _IDENT, -1, n
    inl, best_h, _, H = best_model(iterations, block, lambda hs: tuple(v[:, None] for v in hypotheses(rec, seed, hs)),
                                   lambda M: inlier_mask(M, rec, t2).sum(axis=1))
    mask = np.zeros(n, np.uint8)
    if best_h < 0:
        return out, mask
    refined = 0
    if refine and inl >= 4:
        R, ok = refit(rec, inlier_mask(H, rec, t2)[0])
        if ok:
            c = int(inlier_mask(R, rec, t2)[0].sum())
            if c >= inl:
                H, inl, refined = R, c, 1
    out["H"], out["inliers"], out["hypothesis"], out["refined"] = H, inl, best_h, refined
    mask[:] = inlier_mask(H, rec, t2)[0]
    return out, mask


def apply(H, xy):
    """map (k, 2) points through H in float64 (for geometric checks, not part of the contract)"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.concatenate([np.asarray(xy, np.float64), np.ones((len(xy), 1))], axis=1) @ H.T
    return p[:, :2] / p[:, 2:]

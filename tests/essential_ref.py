"""numpy statement of hak_find_essential (include/hipakaze.h): five-point RANSAC essential matrix over a match list, bit for bit.

The checker only -- the product never calls it.  Vectorised over hypotheses: float64 for the five-point solve (bearings, a 5 x 9
elimination with complete pivoting, the mixed null-space basis, the ten cubic constraints, a 10 x 10 Gauss-Jordan, the degree-10
polynomial and its real roots by a derivative chain of bisections: + - * / only), float32 for the Sampson scoring, which is
fundamental_ref's.  numpy forms no FMA, and every expression below is written in the evaluation order of kernels_essential.hip.
"""
import numpy as np

import fundamental_ref as fr
import homography_ref as hr
import pose_ref as pr
from homography_ref import _mul3, records

FUNDAMENTAL_DTYPE = fr.FUNDAMENTAL_DTYPE
DRAWS = 32
POLISH = 3                                      # Newton steps per root
ROOT_BASE = 16                                  # record.root = ROOT_BASE + r
MIX = (1.125, -0.625, 0.875)                    # X' = X - a1 W, Y' = Y - a2 W, Z' = Z - a3 W

# monomials over the variables v = (x, y, z, 1): degree 2 as the pairs i <= j, degree 3 as the triples i <= j <= k, both in
# lexicographic order; NISTER[c] = the lexicographic index of column c of the constraint matrix
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]
TRIPLES = [(i, j, k) for i in range(4) for j in range(i, 4) for k in range(j, 4)]
M2 = {p: n for n, p in enumerate(PAIRS)}
M3 = {t: n for n, t in enumerate(TRIPLES)}
NISTER = [0, 10, 1, 4, 2, 3, 11, 12, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19]
# x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
BINOM = [[1 if k == 0 else 0 for k in range(11)] for _ in range(11)]
for _n in range(1, 11):
    for _k in range(1, _n + 1):
        BINOM[_n][_k] = BINOM[_n - 1][_k - 1] + BINOM[_n - 1][_k]


def sample_indices(seed, h, n):
    return hr.sample_indices(seed, h, n, 5, DRAWS)


def null_space(M):
    """M (H, 5, 9) float64.  Gaussian elimination with complete pivoting -> (N (H, 4, 9): X', Y', Z', W after the mix, ok)"""
    M = M.copy()
    nh = M.shape[0]
    rows = np.arange(nh)
    ok = np.ones(nh, bool)
    perm = np.tile(np.arange(9), (nh, 1))
    for c in range(5):
        best = np.abs(M[:, c, c])
        pr_, pc = np.full(nh, c), np.full(nh, c)
        for r in range(c, 5):
            for q in range(c, 9):
                if r == c and q == c:
                    continue
                v = np.abs(M[:, r, q])
                gt = v > best
                best = np.where(gt, v, best)
                pr_ = np.where(gt, r, pr_)
                pc = np.where(gt, q, pc)
        ok &= (best > 0.0) & np.isfinite(best)
        top, other = M[rows, c].copy(), M[rows, pr_].copy()
        M[rows, pr_] = top
        M[rows, c] = other
        left, right = M[rows, :, c].copy(), M[rows, :, pc].copy()
        M[rows, :, pc] = left
        M[rows, :, c] = right
        a, b = perm[rows, c].copy(), perm[rows, pc].copy()
        perm[rows, pc] = a
        perm[rows, c] = b
        for r in range(c + 1, 5):
            f = M[:, r, c] / M[:, c, c]
            for q in range(c + 1, 9):
                M[:, r, q] = M[:, r, q] - f * M[:, c, q]
    N = np.zeros((nh, 4, 9))
    for k in range(4):
        f = [None] * 9
        for j in range(4):
            f[5 + j] = np.full(nh, 1.0 if j == k else 0.0)
        for i in range(4, -1, -1):
            acc = -M[:, i, 5 + k]
            for j in range(i + 1, 5):
                acc = acc - M[:, i, j] * f[j]
            f[i] = acc / M[:, i, i]
        for p in range(9):
            N[rows, k, perm[:, p]] = f[p]
    for k in range(3):
        N[:, k] = N[:, k] - MIX[k] * N[:, 3]
    return N, ok


def _pmul11(out, a, b):
    """out (.., 10) += a (.., 4) * b (.., 4), ascending (i, j)"""
    for i in range(4):
        for j in range(4):
            m = M2[(min(i, j), max(i, j))]
            out[..., m] = out[..., m] + a[..., i] * b[..., j]
    return out


def _pmul21(out, A, b):
    """out (.., 20) += A (.., 10) * b (.., 4), ascending (a, k)"""
    for a in range(10):
        for k in range(4):
            m = M3[tuple(sorted(PAIRS[a] + (k,)))]
            out[..., m] = out[..., m] + A[..., a] * b[..., k]
    return out


def constraints(N):
    """the ten cubic constraints of E = x X' + y Y' + z Z' + W: (H, 10, 20) in Nister's column order.  Row 0 is det E, row
    1 + 3 i + j entry (i, j) of 2 E E^T E - tr(E E^T) E"""
    nh = N.shape[0]
    E = np.ascontiguousarray(N.transpose(0, 2, 1)).reshape(nh, 3, 3, 4)          # E[i][j] as a polynomial over (x, y, z, 1)
    z2 = lambda: np.zeros((nh, 10))
    C = np.zeros((nh, 10, 20))
    c0 = _pmul11(z2(), E[:, 1, 1], E[:, 2, 2]) - _pmul11(z2(), E[:, 1, 2], E[:, 2, 1])
    c1 = _pmul11(z2(), E[:, 1, 2], E[:, 2, 0]) - _pmul11(z2(), E[:, 1, 0], E[:, 2, 2])
    c2 = _pmul11(z2(), E[:, 1, 0], E[:, 2, 1]) - _pmul11(z2(), E[:, 1, 1], E[:, 2, 0])
    row = np.zeros((nh, 20))
    _pmul21(row, c0, E[:, 0, 0])
    _pmul21(row, c1, E[:, 0, 1])
    _pmul21(row, c2, E[:, 0, 2])
    C[:, 0] = row
    L = np.zeros((nh, 3, 3, 10))                                                 # L[i][k] = sum_l E[i][l] E[k][l]
    for l in range(3):
        _pmul11(L, E[:, :, None, l, :], E[:, None, :, l, :])
    t = (L[:, 0, 0] + L[:, 1, 1]) + L[:, 2, 2]
    A = 2.0 * L
    for i in range(3):
        A[:, i, i] = A[:, i, i] - t
    R = np.zeros((nh, 3, 3, 20))
    for k in range(3):
        _pmul21(R, A[:, :, None, k, :], E[:, None, k, :, :])
    C[:, 1:] = R.reshape(nh, 9, 20)
    return C[:, :, NISTER]


def gauss_jordan(C):
    """Gauss-Jordan on the left 10 x 10 block without row exchanges: the pivot of column c is the largest |entry| among the rows
    that hold no pivot yet, ties to the smallest row.  -> (T (H, 6, 10): the right halves of the rows with the pivots of columns
    4..9, ok)"""
    C = C.copy()
    nh = C.shape[0]
    rows = np.arange(nh)
    used = np.zeros((nh, 10), bool)
    ok = np.ones(nh, bool)
    owner = np.zeros((nh, 10), np.int64)
    for c in range(10):
        best, piv = np.full(nh, -1.0), np.zeros(nh, np.int64)
        for r in range(10):
            v = np.abs(C[:, r, c])
            gt = ~used[:, r] & (v > best)
            best = np.where(gt, v, best)
            piv = np.where(gt, r, piv)
        ok &= (best > 0.0) & np.isfinite(best)
        used[rows, piv] = True
        owner[:, c] = piv
        p = C[rows, piv, c]
        v = [C[rows, piv, q] / p for q in range(c + 1, 20)]
        for r in range(10):
            mine = piv == r
            f = C[:, r, c].copy()
            for n, q in enumerate(range(c + 1, 20)):
                C[:, r, q] = np.where(mine, v[n], C[:, r, q] - f * v[n])
    T = np.stack([C[rows, owner[:, c], 10:] for c in range(4, 10)], axis=1)
    return T, ok


def _conv(a, b):
    """polynomial product, coefficients ascending: out[i + j] += a[i] * b[j] in ascending (i, j)"""
    out = [np.zeros_like(a[0]) for _ in range(len(a) + len(b) - 1)]
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] + a[i] * b[j]
    return out


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def b_matrix(T):
    """rows k = e - z f, l = g - z h, m = i - z j of B(z): [row][column x, y, 1] -> coefficient list, ascending powers of z"""
    B = []
    for s in range(3):
        e, f = T[:, 2 * s], T[:, 2 * s + 1]
        row = []
        for o in (0, 3):                                                # x: columns xz^2 xz x; y: yz^2 yz y
            row.append([e[:, o + 2], e[:, o + 1] - f[:, o + 2], e[:, o] - f[:, o + 1], -f[:, o]])
        row.append([e[:, 9], e[:, 8] - f[:, 9], e[:, 7] - f[:, 8], e[:, 6] - f[:, 7], -f[:, 6]])
        B.append(row)
    return B


def poly10(B):
    """det B(z): eleven coefficient arrays, ascending"""
    (kx, ky, k1), (lx, ly, l1), (mx, my, m1) = B
    c0 = _sub(_conv(ly, m1), _conv(l1, my))
    c1 = _sub(_conv(l1, mx), _conv(lx, m1))
    c2 = _sub(_conv(lx, my), _conv(ly, mx))
    t0, t1, t2 = _conv(kx, c0), _conv(ky, c1), _conv(k1, c2)
    return [(t0[k] + t1[k]) + t2[k] for k in range(11)]


def _horner(a, z):
    """a: coefficient arrays ascending (.., deg + 1) as a list; fixed form ((a_d z + a_(d-1)) z + ..) + a_0"""
    acc = a[-1] * np.ones_like(z)
    for k in range(len(a) - 2, -1, -1):
        acc = acc * z + a[k]
    return acc


def real_roots(c):
    """the real roots of sum c[k] z^k (k = 0..10) by the derivative chain: (points (H, 10), has (H, 10), ok (H,)); bracket q of
    the last level holds a root iff has[:, q]"""
    with np.errstate(all="ignore"):
        c10 = c[10]
        ok = (c10 != 0.0)
        for k in range(11):
            ok &= np.isfinite(c[k])
        b = [c[k] / c10 for k in range(10)] + [np.ones_like(c10)]
        m = np.abs(b[0])
        for k in range(1, 10):
            m = np.where(np.abs(b[k]) > m, np.abs(b[k]), m)
        bound = 1.0 + m
        for k in range(10):
            ok &= np.isfinite(b[k])
        ok &= np.isfinite(bound)
        nh = len(c10)
        pts = np.zeros((nh, 0))
        has = None
        for d in range(1, 11):
            s = 10 - d
            a = [(float(BINOM[j + s][s]) * b[j + s])[:, None] for j in range(d + 1)]
            ends = np.concatenate([-bound[:, None], pts, bound[:, None]], axis=1)
            lo, hi = ends[:, :d].copy(), ends[:, 1:].copy()
            top = hi.copy()
            neg = _horner(a, lo) < 0.0
            has = neg != (_horner(a, hi) < 0.0)
            for _ in range(64):
                mid = 0.5 * (lo + hi)
                left = (_horner(a, mid) < 0.0) == neg
                lo = np.where(left, mid, lo)
                hi = np.where(left, hi, mid)
            pts = np.where(has, 0.5 * (lo + hi), top)
        return pts, has, ok


def polish(B, dB, x, y, z):
    """POLISH Newton steps on the three equations B(z) (x, y, 1)^T = 0 in (x, y, z), solved by Cramer's rule"""
    for _ in range(POLISH):
        J, r = [], []
        for i in range(3):
            a, b, c = (_horner(B[i][k], z) for k in range(3))
            da, db, dc = (_horner(dB[i][k], z) for k in range(3))
            r.append((a * x + b * y) + c)
            J += [a, b, (da * x + db * y) + dc]
        det = fr._det(J)
        dx = fr._det([r[0], J[1], J[2], r[1], J[4], J[5], r[2], J[7], J[8]]) / det
        dy = fr._det([J[0], r[0], J[2], J[3], r[1], J[5], J[6], r[2], J[8]]) / det
        dz = fr._det([J[0], J[1], r[0], J[3], J[4], r[1], J[6], J[7], r[2]]) / det
        x, y, z = x - dx, y - dy, z - dz
    return x, y, z


def _solve(p, k1, k2):
    """p (H, 5, 4) float64 sample records -> (F (H, 10, 9) float32, valid (H, 10) bool, nroots (H,))"""
    nh = p.shape[0]
    F = np.zeros((nh, 10, 9), np.float32)
    valid = np.zeros((nh, 10), bool)
    with np.errstate(all="ignore"):
        x, y = (p[:, :, 0] - k1["cx"]) / k1["fx"], (p[:, :, 1] - k1["cy"]) / k1["fy"]
        u, v = (p[:, :, 2] - k2["cx"]) / k2["fx"], (p[:, :, 3] - k2["cy"]) / k2["fy"]
        ok = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1) & np.isfinite(u).all(axis=1) & np.isfinite(v).all(axis=1)
        M = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=-1)
        N, okn = null_space(M)
        T, okg = gauss_jordan(constraints(N))
        B = b_matrix(T)
        dB = [[[float(k) * poly[k] for k in range(1, len(poly))] for poly in row] for row in B]
        pts, has, okr = real_roots(poly10(B))
        ok = ok & okn & okg & okr
        slot = np.cumsum(has, axis=1) - has                             # roots are numbered in ascending bracket order
        one, zero = np.ones(nh), np.zeros(nh)
        K1i = [1.0 / k1["fx"] * one, zero, -(k1["cx"] / k1["fx"]) * one, zero, 1.0 / k1["fy"] * one, -(k1["cy"] / k1["fy"]) * one,
               zero, zero, one]
        K2it = [1.0 / k2["fx"] * one, zero, zero, zero, 1.0 / k2["fy"] * one, zero, -(k2["cx"] / k2["fx"]) * one,
                -(k2["cy"] / k2["fy"]) * one, one]
        rows = np.arange(nh)
        for q in range(10):
            z = pts[:, q]
            Bz = [[_horner(poly, z) for poly in row] for row in B]
            best, ca, cb = None, None, None
            for a_, b_ in ((0, 1), (0, 2), (1, 2)):
                ra, rb = Bz[a_], Bz[b_]
                w = ra[0] * rb[1] - ra[1] * rb[0]
                cx, cy = ra[1] * rb[2] - ra[2] * rb[1], ra[2] * rb[0] - ra[0] * rb[2]
                if best is None:
                    best, ca, cb = w, cx, cy
                else:
                    gt = np.abs(w) > np.abs(best)
                    best, ca, cb = np.where(gt, w, best), np.where(gt, cx, ca), np.where(gt, cy, cb)
            xs, ys = ca / best, cb / best
            good = ok & has[:, q] & (best != 0.0) & np.isfinite(best)
            xs, ys, z = polish(B, dB, xs, ys, z)
            E = [((xs * N[:, 0, k] + ys * N[:, 1, k]) + z * N[:, 2, k]) + N[:, 3, k] for k in range(9)]
            G = _mul3(K2it, _mul3(E, K1i))
            d = G[0]
            for k in range(1, 9):
                d = np.where(np.abs(G[k]) > np.abs(d), G[k], d)
            Fr = np.stack([(G[k] / d).astype(np.float32) for k in range(9)], axis=-1)
            good &= (d != 0.0) & np.isfinite(d) & np.isfinite(Fr).all(axis=-1)
            F[rows[good], slot[good, q]] = Fr[good]
            valid[rows[good], slot[good, q]] = True
    return F, valid, np.where(ok, has.sum(axis=1), -1)


def _k64(K):
    K = pr.intrinsics(K)
    return {f: np.float64(K[f]) for f in ("fx", "fy", "cx", "cy")}


def models(rec, K1, K2, seed, hs, roots=False):
    """the float32 models of hypotheses hs: (M (len, 10, 9) float32, valid (len, 10) bool); roots=True adds the number of real
    roots per hypothesis (-1 = degenerate)"""
    n = len(rec)
    hs = np.asarray(hs, np.int64)
    F = np.zeros((len(hs), 10, 9), np.float32)
    valid = np.zeros((len(hs), 10), bool)
    nroots = np.full(len(hs), -1)
    if n >= 5 and len(hs):
        idx, ok = sample_indices(seed, hs, n)
        p = rec[np.where(idx < 0, 0, idx)].astype(np.float64)
        Fs, vs, ns = _solve(p, _k64(K1), _k64(K2))
        F[ok], valid[ok], nroots[ok] = Fs[ok], vs[ok], ns[ok]
    return (F, valid, nroots) if roots else (F, valid)


def solve_five(points, K1=(1.0, 1.0, 0.0, 0.0), K2=None):
    """the five-point solver on samples given directly: points (H, 5, 4) float64 -> (F (H, 10, 9) float32, valid (H, 10))"""
    F, valid, _ = _solve(np.asarray(points, np.float64), _k64(K1), _k64(K1 if K2 is None else K2))
    return F, valid


def find_essential(matches, K1, K2=None, iterations=1024, threshold=1.0, seed=0, block=1024):
    """-> (record of FUNDAMENTAL_DTYPE with root = 16 + r, mask uint8 (n,))"""
    rec = records(matches)
    n = len(rec)
    K2 = K1 if K2 is None else K2
    t2 = np.float32(threshold) * np.float32(threshold)
    out = np.zeros((), FUNDAMENTAL_DTYPE)
    out["hypothesis"], out["n"] = -1, n
    best = hr.best_model(iterations, block, lambda hs: models(rec, K1, K2, seed, hs),
                         lambda F: fr.inlier_mask(F, rec, t2).sum(axis=1))
    mask = np.zeros(n, np.uint8)
    if best[1] < 0:
        return out, mask
    out["F"], out["inliers"], out["hypothesis"], out["root"] = best[3], best[0], best[1], ROOT_BASE + best[2]
    mask[:] = fr.inlier_mask(best[3], rec, t2)[0]
    return out, mask

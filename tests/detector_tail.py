"""Planes, seeded maps and the oracle walk of the stage-parity tests of the detector tail: the extrema rule as its five kernels apply it
(k_extrema<float|int>, k_hessian_stream, k_hessian_fused, k_level_tile), the key map and the candidate list, k_nms_cand, k_row_scan,
k_emit and k_refine (csrc/kernels_detect.hip, kernels_hessian*.hip; gCalcExtremaMap / gNmsRNaive / gRefine, akazed.cu:1334-1662 and
3476-3646).

Test infrastructure, numpy only, seeded; nothing here touches a device.  tests/test_detector_tail_cpu.py asserts that the inputs reach
the narrow places they are made for and ties the walk to the pipeline oracle; tests/test_gpu_detector_tail.py drives the same inputs
through hak_op_tail_* / hak_op_fast_tail_* and reads the extrema stage by itself with hak_debug_tail_maps.  Every comparison is bit
equality (NaN against NaN where a refined position is a NaN, value_domain.same_bits).

Why not images.  Float determinants of natural content never tie and hold at most ~50 extrema per strip and 16 rows, so the
mid-segment flush of k_hessian_stream's staging buffer (more than 128 candidates of one wave), the `>` against `>=` of the strict
maximum, the cross-level tie order of the key, the NMS tie clause and its lagging read cursor, and a maximum that lies exactly on a
strip, lane-quad, row-segment or domain limit are all places an image test passes by.

Contexts (the smallest at which the path exists):
  A  328 x 248, default parameters: two octaves; w % 4 == 0, so the streaming Hessian takes it (two strips: 240 + 88 owned columns at
     dilations 2 and 3, 232 + 96 at dilation 4; 16-row segments at both octaves); octave 1 sublevel 3 keeps a domain
  B  265 x 245: odd width, the tile kernels only
  C  328 x 248, one octave, derivative_factor 2.5: dilations 4, 5, 6, 7 -- one fused level and three on the k_extrema fallback; NMS radii
     4 .. 7, so both branches of k_nms_cand and waves that mix them
  D  4160 x 80, one octave: 65 bitmap words per row, so k_emit's word loop and its row_base carry run a second time; only sublevel 0 has a
     domain (rows 29 .. 50); 18 strips of 240 columns, four segments of 20 rows
  E1 328 x 600, E2 328 x 300: k_row_scan with per = 3 and 2 (A: 1, h < 256); the seeded NMS only

A `case` is {level: (kind, dense plane)} with kind "L" (an L-plane: Hessian + extrema through the fused kernel the context picks, or,
on the oracle side, okz.hessian at the level's dilation) or "det" (a determinant plane, the stand-alone extrema kernel).  `walk` applies
okz.extrema_map to fresh maps level by level (the per-level candidate sets) and to one set of maps in level order (the merged response
and layer maps); okz.nms and okz.refine_point give the records.
"""
import ctypes as C
import functools

import numpy as np

import fast_domain as fd
import value_domain as vd

f32 = np.float32
MS = 4
SEED = 23
EMPTY_F = f32(-0.0926474631)            # akaze.cpp:252-258 (D1): what the reference's maps hold where nothing was written
EMPTY_I = -1061109568                   # 0xC0C0C0C0, the FAST maps
MAX_PTS = 60000                         # of the contexts: above every survivor count of this module
FAST_THRESHOLDS = (65, 0)               # the FAST launch sequence's own, and the smallest that keeps responses positive


def align_up(a, b):
    return (a + b - 1) // b * b


def accepted(border, n, start):
    """first and last coordinate of an extent n the border rule accepts (akazed.cu:1345-1352; the loops start at (int)borders[sublevel
    0]), or None when it accepts none"""
    b, out = f32(border), []
    for i in range(start, n):
        lo = int(f32(f32(i) - b) + f32(0.5)) - 1
        hi = int(f32(f32(i) + b) + f32(0.5)) + 1
        if lo >= 0 and hi < n:
            out.append(i)
    if not out:
        return None
    assert out == list(range(out[0], out[-1] + 1))
    return out[0], out[-1]


class Context:
    """a size and the parameters that differ from the defaults; the same keywords go to okz.default_params and to Akazer.init"""

    def __init__(self, name, w, h, layer_weights=None, **kw):
        self.name, self.w, self.h, self.kw, self.layer_weights = name, w, h, kw, layer_weights
        self._sched = None

    def params(self, okz, **more):
        return okz.default_params(**dict(self.kw, **more))

    def create(self, ah, max_pts=MAX_PTS, **more):
        det = ah.Akazer()
        det.init((self.w, self.h, ah.iAlignUp(self.w, 128)), max_pts=max_pts, **dict(self.kw, **more))
        return det

    def sched(self, okz):
        if self._sched is None:
            self._sched = Sched(okz, self)
        return self._sched


class Sched:
    """geometry and per-level constants as the pipeline oracle forms them (okz_layout + okz_schedule)"""

    def __init__(self, okz, ctx):
        prm = ctx.params(okz)
        owhps, osizes, offsets = np.zeros(24, np.int32), np.zeros(8, np.int32), np.zeros(9, np.int32)
        ip = C.POINTER(C.c_int)
        self.noct = okz.lib().okz_layout(ctx.w, ctx.h, align_up(ctx.w, 128), prm.noctaves, MS, owhps.ctypes.data_as(ip),
                                         osizes.ctypes.data_as(ip), offsets.ctypes.data_as(ip))
        self.whp = [tuple(int(v) for v in owhps[3 * o:3 * o + 3]) for o in range(self.noct)]
        self.sizes, self.sigma_size, self.borders, self.psz = okz.schedule(prm, self.noct)
        self.nlev = self.noct * MS

    def domain(self, l):
        """(x0, x1, y0, y1) of level l in level coordinates, or None"""
        o = l // MS
        w, h, _ = self.whp[o]
        start = int(self.borders[o * MS])
        ax, ay = accepted(self.borders[l], w, start), accepted(self.borders[l], h, start)
        return None if ax is None or ay is None else ax + ay

    def levels(self):
        return [l for l in range(self.nlev) if self.domain(l) is not None]

    def matches(self, det):
        """the context `det` agrees on extents and level constants (pitches are each side's own)"""
        s = det.schedule()
        return (s["noct"] == self.noct and [t[:2] for t in det.geometry()] == [t[:2] for t in self.whp]
                and s["sizes"].tobytes() == self.sizes.tobytes() and s["borders"].tobytes() == self.borders.tobytes()
                and s["sigma_size"].tobytes() == self.sigma_size.tobytes())


A = Context("A", 328, 248)
B = Context("B", 265, 245)
CC = Context("C", 328, 248, layer_weights=(0.4, 0.2, 0.2, 0.2), noctaves=1, derivative_factor=2.5)
D = Context("D", 4096 + 64, 80, noctaves=1)
E1 = Context("E1", 328, 600)
E2 = Context("E2", 328, 300)
CONTEXTS = {c.name: c for c in (A, B, CC, D, E1, E2)}


# ------------------------------------------------------------------------------------------------ plane families (float path)
def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def noise(sched, l, seed=0):
    w, h, _ = sched.whp[l // MS]
    return _rng(1, l, seed).random((h, w), dtype=np.float32)


FOLD = 16


def quantised(sched, l, seed=0):
    """noise in steps of 1/8, folded: a FOLD x FOLD block mirrored to and fro along both axes.  The steps alone make no determinant
    tie (0 of 18836 maxima on A: the derivative factors 0.09375001 and 0.31250003 are not dyadic, so the products round); the plane's
    mirror symmetry about every fold does -- Lxx and Lyy are even and Lxy is odd under a reflection, operation by operation, so the two
    pixels on either side of a fold hold bit-equal determinants, and four around a crossing of folds"""
    w, h, _ = sched.whp[l // MS]
    blk = np.floor(_rng(1, l, seed).random((FOLD, FOLD), dtype=np.float32) * f32(8)) / f32(8)
    tx, ty = np.arange(w) % (2 * FOLD), np.arange(h) % (2 * FOLD)
    tx, ty = np.where(tx < FOLD, tx, 2 * FOLD - 1 - tx), np.where(ty < FOLD, ty, 2 * FOLD - 1 - ty)
    return np.ascontiguousarray(blk[np.ix_(ty, tx)])


def _refine_offsets(d):
    """gRefine's Newton step (akazed.cu:1636-1645) of 3 x 3 patches d[..., 3, 3], float64: only to choose patches, never to check"""
    v2 = 2 * d[..., 1, 1]
    dx, dy = 0.5 * (d[..., 1, 2] - d[..., 1, 0]), 0.5 * (d[..., 2, 1] - d[..., 0, 1])
    dxx, dyy = d[..., 1, 2] + d[..., 1, 0] - v2, d[..., 2, 1] + d[..., 0, 1] - v2
    dxy = 0.25 * (d[..., 2, 2] + d[..., 0, 0] - d[..., 0, 2] - d[..., 2, 0])
    dd = dxx * dyy - dxy * dxy
    with np.errstate(divide="ignore", invalid="ignore"):
        idd = np.where(dd != 0, 1.0 / dd, 0.0)
    return idd * (dxy * dy - dyy * dx), idd * (dxy * dx - dxx * dy)


def painted_levels(sched):
    """the levels painted_patches can paint: dilation >= 3"""
    return [l for l in sched.levels() if int(sched.sigma_size[l]) >= 3]


def painted_patches(sched, l, seed=0):
    """an L-plane whose determinant holds chosen 3 x 3 patches: at a dilation S >= 3 the taps of Lxx, Lyy and Lxy lie at offsets 0, +-S
    and +-2S, so inside a 3 x 3 cluster of L pixels on a zero plane every pixel sees its own value alone: Lxy = 0 and Lxx, Lyy are that
    value times one constant, the determinant its square times another.  Noise leaves gRefine's weak branch (an offset beyond one pixel,
    akazed.cu:1646) to one keypoint in 3000; here every other cluster is the square root of a patch whose Newton step is weak, the
    others of one whose step stays inside.  Clusters lie 4 S + 5 pixels apart"""
    S = int(sched.sigma_size[l])
    assert S >= 3
    w, h, _ = sched.whp[l // MS]
    x0, x1, y0, y1 = sched.domain(l)
    rng = _rng(7, l, seed)
    d = rng.random((400000, 3, 3)) * 0.999
    d[:, 1, 1] = 1.0
    o0, o1 = _refine_offsets(d)
    weak = (np.abs(o0) > 1.25) | (np.abs(o1) > 1.25)
    firm = (np.abs(o0) < 0.8) & (np.abs(o1) < 0.8)
    pools = [d[weak], d[firm]]
    a = np.zeros((h, w), np.float32)
    k = 0
    for y in range(y0 + 1, y1, 4 * S + 5):
        for x in range(x0 + 1, x1, 4 * S + 5):
            pool = pools[k % 2]
            a[y - 1:y + 2, x - 1:x + 2] = np.sqrt(pool[(k // 2) % len(pool)]).astype(np.float32)
            k += 1
    return a


def case_of(sched, family, kind="L", levels=None, seed=0):
    return {l: (kind, family(sched, l, seed)) for l in (sched.levels() if levels is None else levels)}


def lattice(sched, seed=0):
    """determinant planes with a strict maximum on every (even, even) pixel: the densest a level can be (cand_cap is sized for it)"""
    case = {}
    for l in sched.levels():
        w, h, _ = sched.whp[l // MS]
        det = np.zeros((h, w), np.float32)
        det[0::2, 0::2] = f32(1) + _rng(2, l, seed).random(((h + 1) // 2, (w + 1) // 2), dtype=np.float32)
        case[l] = ("det", det)
    return case


# The launch geometry of the kernels that apply the extrema rule, restated for the tests that aim at its seams (and nowhere used to
# form an expectation).  k_hessian_stream (kernels_hessian_stream.hip, HsGeo without the fused low-pass, as hak_op_tail_level runs it):
# a wave OWNS XV = 256 - 2 M columns of its 256, M = 4 / 8 / 8 / 12 at dilation 1 / 2 / 3 / 4, so strips are cut at multiples of 248,
# 240, 240, 232 -- not of 256; rows are cut by hak_stream_rows (hak_internal.h) into a multiple of four equal segments, halved while
# the launch has fewer than 2048 waves and a segment keeps 16 rows.  k_hessian_fused (kernels_hessian.hip): tiles of 64 columns and 32
# rows, 28 at dilation 4.  k_extrema: blocks of 64 columns x 16 rows.
STREAM_MARGIN = {1: 4, 2: 8, 3: 8, 4: 12}


def stream_geometry(sched, l):
    """(owned columns per strip, rows per segment) of k_hessian_stream on level l for a single image, or None where it does not apply
    (hak_hessian_stream_covers: w % 4 == 0 and a dilation of at most 4)"""
    S = int(sched.sigma_size[l])
    w, h, _ = sched.whp[l // MS]
    if S not in STREAM_MARGIN or w % 4:
        return None
    xv = 256 - 2 * STREAM_MARGIN[S]
    strips, nseg = (w + xv - 1) // xv, 4 * max((h + 512) // 1024, 1)
    while strips * nseg < 2048 and (h + 2 * nseg - 1) // (2 * nseg) >= 16:
        nseg *= 2
    return xv, max((h + nseg - 1) // nseg, 16)


def tile_geometry(sched, l):
    """(columns, rows) of a tile of k_hessian_fused on level l, or None above dilation 4"""
    S = int(sched.sigma_size[l])
    return (64, 28 if S == 4 else 32) if S <= 4 else None


def seam_columns(sched, l):
    """the last column of one strip / tile / block and the first of the next, inside the level's domain -> {x: tag}"""
    x0, x1, _, _ = sched.domain(l)
    out = {}
    for geo, tag in ((stream_geometry(sched, l), "strip"), (tile_geometry(sched, l), "tile"), ((64, 16), "tile")):
        if geo:
            for x in range(geo[0], x1 + 1, geo[0]):
                for c in (x - 1, x):
                    if x0 <= c <= x1:
                        out.setdefault(c, tag)
    return out


def seam_rows(sched, l):
    """the last row of one row segment / tile / block and the first of the next, inside the level's domain -> {y: tag}"""
    _, _, y0, y1 = sched.domain(l)
    out = {}
    for geo, tag in ((stream_geometry(sched, l), "segment"), (tile_geometry(sched, l), "tilerow"), ((64, 16), "tilerow")):
        if geo:
            for y in range(geo[1], y1 + 1, geo[1]):
                for r in (y - 1, y):
                    if y0 <= r <= y1:
                        out.setdefault(r, tag)
    return out


def seam_sites(sched, l):
    """level pixels a maximum is planted on: (x, y, tag).  Both sides of every limit of the domain, its corners, the last and first owned
    column of every strip of the streaming kernel and of every 64-column tile, lane-quad edges (x % 4 == 3 | 0), and the last and first
    row of every row segment of the streaming kernel, of every tile of the tile kernel and of every 16-row block of k_extrema"""
    d = sched.domain(l)
    if d is None:
        return []
    x0, x1, y0, y1 = d
    w, h, _ = sched.whp[l // MS]
    rng = _rng(3, l)
    xs_in = lambda: int(rng.integers(x0, x1 + 1))
    ys_in = lambda: int(rng.integers(y0, y1 + 1))
    out = [(x, y, "corner") for x in (x0, x1) for y in (y0, y1)]
    out += [(x, y, "outside") for x, y in ((x0 - 1, y0), (x1 + 1, y1), (x0, y0 - 1), (x1, y1 + 1), (x0 - 1, y0 - 1), (x1 + 1, y1 + 1))]
    for _ in range(2):
        out += [(x0, ys_in(), "col"), (x1, ys_in(), "col"), (xs_in(), y0, "row"), (xs_in(), y1, "row")]
        out += [(x0 - 1, ys_in(), "outside"), (x1 + 1, ys_in(), "outside"), (xs_in(), y0 - 1, "outside"), (xs_in(), y1 + 1, "outside")]
    cols, rows = seam_columns(sched, l), seam_rows(sched, l)
    strip_cols = [x for x, t in cols.items() if t == "strip"] or list(cols)
    for x, tag in cols.items():
        out += [(x, ys_in(), tag)]
    q = x0 + (3 - x0) % 4
    out += [(x, ys_in(), "quad") for x in (q, q + 1, q + 4 * ((x1 - q) // 8) , q + 4 * ((x1 - q) // 8) + 1) if x0 <= x <= x1]
    for k, (y, tag) in enumerate(sorted(rows.items())):
        # alternately anywhere on the row and on a strip edge: a maximum on a segment seam and a strip seam at once
        out += [(xs_in() if k % 2 or not strip_cols else strip_cols[(k // 2) % len(strip_cols)], y, tag)]
    return [(x, y, t) for x, y, t in out if 0 < x < w - 1 and 0 < y < h - 1]


def planted_seams(sched, kind):
    """-> list of cases.  kind "det": single determinant pixels of 1.0 on a zero plane, one case.  kind "L": single L pixels of 1.0 on a
    zero plane -- the determinant of an impulse has its strict maximum at the impulse itself (Lxx = Lyy < 0 and Lxy = 0 there, and with a
    dilation >= 2 its eight neighbours hold -Lxy^2 <= 0); impulses of one plane lie at least 4 * dilation + 3 pixels apart, so no
    response of one reaches the 3 x 3 neighbourhood of another, and the sites of a level are spread over as many planes as that takes"""
    per_level = {}
    for l in sched.levels():
        w, h, _ = sched.whp[l // MS]
        gap = 2 if kind == "det" else 4 * int(sched.sigma_size[l]) + 3
        planes = []
        for x, y, _ in seam_sites(sched, l):
            for pl in planes:
                if all(max(abs(x - u), abs(y - v)) >= gap for u, v in pl):
                    pl.append((x, y))
                    break
            else:
                planes.append([(x, y)])
        per_level[l] = planes
    cases = []
    for k in range(max(len(p) for p in per_level.values())):
        case = {}
        for l, planes in per_level.items():
            if k < len(planes):
                w, h, _ = sched.whp[l // MS]
                a = np.zeros((h, w), np.float32)
                for x, y in planes[k]:
                    a[y, x] = f32(1)
                case[l] = (kind, a)
        cases.append(case)
    return cases


def equal_levels(sched):
    """determinant planes of two sublevels (1, 2) and of two octaves (0, 4; 5, 3) that hit the same full-resolution pixels: per pair three
    sites where the later level holds the bit-equal response, one ulp more and one ulp less -> (case, [(la, lb, x, y, relation)])"""
    planes, sites = {}, []
    pairs = [(1, 2)] + ([(0, 4), (3, 5)] if sched.noct > 1 else [(0, 3)])
    for k, (la, lb) in enumerate(pairs):
        da, db = sched.domain(la), sched.domain(lb)
        oa, ob = la // MS, lb // MS
        # full-resolution pixels inside both domains, even coordinates (octave 1 scatters to those)
        fx0, fx1 = max(da[0] << oa, db[0] << ob), min(da[1] << oa, db[1] << ob)
        fy0, fy1 = max(da[2] << oa, db[2] << ob), min(da[3] << oa, db[3] << ob)
        assert fx1 - fx0 >= 12 and fy1 - fy0 >= 10, (la, lb)
        v = f32(0.75) + f32(0.125) * f32(k)
        for j, rel in enumerate((0, 1, -1)):
            x, y = (fx0 + 1) // 2 * 2 + 4 * j, (fy0 + 1) // 2 * 2 + 4 * k
            for l, o, val in ((la, oa, v), (lb, ob, v if rel == 0 else np.nextafter(v, f32(2 * rel)))):
                w, h, _ = sched.whp[o]
                planes.setdefault(l, np.zeros((h, w), np.float32))[y >> o, x >> o] = val
            sites.append((la, lb, x, y, rel))
    return {l: ("det", a) for l, a in planes.items()}, sites


def value_domain_case(sched, name, seed=5):
    """one tests/value_domain.py plane per level (tiers B and C: inf and NaN determinants), as L-planes"""
    return {l: ("L", vd.GENERATORS[name](sched.whp[l // MS][0], sched.whp[l // MS][1], seed + l)) for l in sched.levels()}


VALUE_DOMAIN = tuple(vd.TIERS["B"] + vd.TIERS["C"])


# ------------------------------------------------------------------------------------------------ plane families (FAST path)
def small_range(w, h, seed):
    """values 0 .. 96: determinants of a few hundred at the most, on both sides of the threshold 65, that tie with a neighbour at more
    than 100 maxima of A under either threshold.  (Measured on the oracle: a range of 0 .. 384 leaves 12 such ties, 0 .. 2048 and
    anything above, 3 * 2^16 included, none: the derivatives keep too many distinct values.)"""
    return _rng(4, seed).integers(0, 97, (h, w)).astype(np.int32)


FAST_FAMILIES = {"u8_range": fd.u8_range, "signed": fd.signed, "full_range": fd.full_range, "small_range": small_range}


def fast_case(sched, name, kind="L", seed=5):
    """an int32 L-plane per level; kind "det": the oracle's determinant of it, for the stand-alone kernel"""
    return {l: (kind, FAST_FAMILIES[name](sched.whp[l // MS][0], sched.whp[l // MS][1], seed + l)) for l in sched.levels()}


# ------------------------------------------------------------------------------------------------ the oracle walk
class Expected:
    pass


def _pitched(a, p):
    out = np.zeros((a.shape[0], p), a.dtype)
    out[:, :a.shape[1]] = a
    return out


def fresh_maps(sched, fast=False):
    _, h, p = sched.whp[0]
    return (np.full((h, p), EMPTY_I if fast else EMPTY_F, np.int32 if fast else np.float32), np.full((h, p), EMPTY_F, np.float32),
            np.full((h, p), -1, np.int32))


def det_planes(okz, sched, case, fast=False):
    """{level: pitched determinant plane} of a case.  A FAST "det" case hands the stand-alone kernel the oracle's determinant of the
    L-plane, so both kinds share the planes"""
    out = {}
    for l, (kind, a) in case.items():
        w, h, p = sched.whp[l // MS]
        assert a.shape == (h, w) and a.dtype == (np.int32 if fast else np.float32)
        if kind == "L" or fast:
            out[l] = (okz.fast_hessian if fast else okz.hessian)(_pitched(a, p), w, int(sched.sigma_size[l]))[2]
        else:
            out[l] = _pitched(a, p)
    return out


def apply_levels(okz, sched, dets, levels, maps, threshold, fast=False):
    """okz.extrema_map of the given levels, octave by octave and sublevels ascending; a level that is not given is a zero plane (flat:
    it holds no strict maximum)"""
    for o in range(sched.noct):
        w, h, p = sched.whp[o]
        ls = [l for l in levels if l // MS == o]
        if not ls:
            continue
        stack = np.zeros((MS, h, p), np.int32 if fast else np.float32)
        for l in ls:
            stack[l % MS] = dets[l]
        prm = np.concatenate([sched.borders[o * MS:(o + 1) * MS], sched.sizes[o * MS:(o + 1) * MS]]).astype(np.float32)
        okz.extrema_map(stack, w, prm, o, threshold, maps, sched.whp[0][2], fast=fast)


def words_of(resp, layer, w):
    """dense (h, w) response words as the key map holds them: the response's bits where a level wrote, 0 elsewhere"""
    return np.where(layer[:, :w] >= 0, np.ascontiguousarray(resp[:, :w]).view(np.uint32), np.uint32(0))


def cand_words(layer_id, ys, xs):
    return (np.uint64(layer_id) << np.uint64(32)) | (ys.astype(np.uint64) << np.uint64(16)) | xs.astype(np.uint64)


def walk(okz, sched, case, threshold, fast=False):
    """-> Expected: .dets, .maps (merged response, size, layer), .words / .layer (dense), .cand (sorted candidate words of all levels),
    .per_level {l: count}"""
    e = Expected()
    w = sched.whp[0][0]
    e.dets = det_planes(okz, sched, case, fast)
    e.maps = fresh_maps(sched, fast)
    apply_levels(okz, sched, e.dets, sorted(case), e.maps, threshold, fast)
    e.words, e.layer = words_of(e.maps[0], e.maps[2], w), np.ascontiguousarray(e.maps[2][:, :w])
    cands, e.per_level = [], {}
    for l in sorted(case):
        m = fresh_maps(sched, fast)
        apply_levels(okz, sched, e.dets, [l], m, threshold, fast)
        ys, xs = np.nonzero(m[2][:, :w] >= 0)
        assert (m[2][ys, xs] == l).all()
        cands.append(cand_words(l, ys, xs))
        e.per_level[l] = len(ys)
    e.cand = np.sort(np.concatenate(cands)) if cands else np.zeros(0, np.uint64)
    return e


def records(okz, sched, maps, dets=None, max_pts=MAX_PTS, fast=False):
    """okz.nms on full-resolution maps (+ okz.refine_point on the winning level's determinant when `dets` is given) -> (points, total)"""
    w = sched.whp[0][0]
    pts, total = okz.nms(maps[0], maps[1], maps[2], w, sched.psz, max_pts, fast=fast)
    if dets is not None:
        for i in range(len(pts)):
            l = int(pts[i]["octave"])
            pts[i] = okz.refine_point(pts[i], dets[l], l // MS, fast=fast)
    return pts, total


def weak_census(okz, sched, maps, dets):
    """(refined, weak) counts of the float records of `maps`"""
    pts, _ = records(okz, sched, maps)
    ref, _ = records(okz, sched, maps, dets)
    moved = (pts["x"].view(np.uint32) != ref["x"].view(np.uint32)) | (pts["y"].view(np.uint32) != ref["y"].view(np.uint32))
    return int(moved.sum()), int((~moved).sum())


# ------------------------------------------------------------------------------------------------ seeded NMS maps
POPULATIONS = ("distinct", "four", "ulp")
DENSITIES = (1.0, 0.25, 1.0 / 64)


def seeded_maps(sched, ctx, population, density, seed=0):
    """hand-made full-resolution maps for hak_op_tail_seed -> (response words (h, w) uint32, all below 2^31 and above 0: positive floats
    and positive ints alike; layer (h, w) int32, -1 = empty).  Random layers over all levels of the context; candidates on the frame
    x == psz, x + psz == w - 1 (same in y) and its four corners whatever the density"""
    w, h, _ = sched.whp[0]
    rng = _rng(5, POPULATIONS.index(population), int(1 / density), seed, w, h)
    pw = np.asarray(ctx.layer_weights or [1.0] * MS, np.float64)
    pw = np.tile(pw / pw.sum(), sched.noct) / sched.noct
    layer = rng.choice(sched.nlev, size=(h, w), p=pw).astype(np.int32)
    keep = rng.random((h, w)) < density
    psz = sched.psz
    for x in (psz, w - 1 - psz):
        keep[psz:h - psz:3, x] = True
    for y in (psz, h - 1 - psz):
        keep[y, psz:w - psz:3] = True
    for x in (psz, w - 1 - psz):
        for y in (psz, h - 1 - psz):
            keep[y, x] = True
    if w > 4096:
        keep[psz:h - psz, 4090:4102] |= rng.random((h - 2 * psz, 12)) < 0.5      # both sides of bitmap word 64
    layer[~keep] = -1
    if population == "distinct":
        words = np.uint32(0x3F000000) + rng.permutation(w * h).astype(np.uint32).reshape(h, w) * np.uint32(5)
    elif population == "four":
        words = np.asarray([0.5, 1.0, 1.5, 2.0], np.float32).view(np.uint32)[rng.integers(0, 4, (h, w))]
    else:
        words = np.uint32(0x3F800000) + rng.integers(0, 3, (h, w)).astype(np.uint32)
    if density < 0.1:
        # row pairs on a 16-px grid: a stronger right-hand neighbour at the largest distance d with d * d < sqsz.  The clean disc
        # reads it; the reference's lagging cursor reads column x + d at j = d + 1, under (d + 1)^2 < sqsz, or not at all (Q1)
        hi = {"distinct": None, "four": np.float32(2.0).view(np.uint32), "ulp": np.uint32(0x3F800002)}[population]
        lo = {"distinct": None, "four": np.float32(0.5).view(np.uint32), "ulp": np.uint32(0x3F800000)}[population]
        for y in range(psz + 8, h - psz - 8, 16):
            for x in range(psz + 8, w - psz - 8, 16):
                l = int(rng.choice(sched.nlev, p=pw))
                fsz = f32(sched.sizes[l])
                sqsz = int(f32(fsz * fsz))
                d = max(k for k in range(1, 9) if k * k < sqsz)
                layer[y - 7:y + 8, x - 7:x + 8] = -1
                layer[y, x] = layer[y, x + d] = l
                if lo is not None:
                    words[y, x], words[y, x + d] = lo, hi
                else:
                    words[y, x + d] = words[y, x] + np.uint32(3)
    words = np.where(layer >= 0, words, np.uint32(0)).astype(np.uint32)
    assert (words[layer >= 0] > 0).all() and (words < 2 ** 31).all()
    return words, layer


def oracle_maps(sched, words, layer, fast=False):
    """the reference's three maps (pitched) of seeded words and layers"""
    w, h, p = sched.whp[0]
    resp, size, lay = fresh_maps(sched, fast)
    on = layer >= 0
    rv = resp[:, :w]
    rv[on] = words.view(np.int32 if fast else np.float32)[on]
    sv = size[:, :w]
    sv[on] = sched.sizes[layer[on]]
    lay[:, :w] = layer
    return resp, size, lay


def nms_census(sched, words, layer, lag=True):
    """numpy restatement of gNmsRNaive (akazed.cu:1554-1613) on seeded maps, for the census of the CPU module only (the expected records
    come from okz.nms, and the CPU module checks that the two agree) -> dict of (h, w) bool arrays: `centre` (a candidate inside the psz
    frame), `larger` (a neighbour of the disc holds a larger response), `tie` (an equal one with i <= 0 and j <= 0), `wide` (isz > 4).
    lag=False: the clean disc, without the cursor lag of the centre row"""
    w, h, _ = sched.whp[0]
    psz = sched.psz
    wd = words.astype(np.int64)
    pad = 8
    big = np.zeros((h + 2 * pad, w + 2 * pad), np.int64)
    big[pad:pad + h, pad:pad + w] = wd
    centre = np.zeros((h, w), bool)
    centre[psz:h - psz, psz:w - psz] = layer[psz:h - psz, psz:w - psz] >= 0
    larger, tie, wide = np.zeros((h, w), bool), np.zeros((h, w), bool), np.zeros((h, w), bool)
    for l in range(sched.nlev):
        fsz = f32(sched.sizes[l])
        isz, sqsz = int(f32(fsz + f32(0.5))), int(f32(fsz * fsz))
        assert isz < pad
        mine = centre & (layer == l)
        if not mine.any():
            continue
        wide |= mine & (isz > 4)
        for i in range(-isz, isz + 1):
            for j in range(-isz, isz + 1):
                if (i == 0 and j == 0) or i * i + j * j >= sqsz:
                    continue
                col = j - 1 if (lag and i == 0 and j > 0) else j
                rn = big[pad + i:pad + i + h, pad + col:pad + col + w]
                on = mine & (rn > 0)                                 # (an empty pixel holds -0.0926 in the reference: never larger or equal)
                larger |= on & (rn > wd)
                tie |= on & (rn == wd) & (i <= 0 and j <= 0)
    return dict(centre=centre, larger=larger, tie=tie, wide=wide)


# ------------------------------------------------------------------------------------------------ whole images
def white_noise_image(w, h, k):
    """uniform white noise in [0, 1): the densest content the whole pipeline can be given"""
    return _rng(6, k, w, h).random((h, w), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def ordinary_u8(w, h):
    """an ordinary scene of the context's size: run after the dense cases, it shows that they left nothing behind"""
    return np.ascontiguousarray(vd._mg().case_scene(max(w, 134), h, 41)[:, :w])


def to_float(u8, p):
    out = np.zeros((u8.shape[0], p), np.float32)
    out[:, :u8.shape[1]] = u8.astype(np.float32) / f32(255)
    return out

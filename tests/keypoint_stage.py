"""Planted keypoints, planes and the oracle walk of the stage-parity tests of the keypoint kernels (csrc/kernels_describe.hip:
k_orient, k_describe_runs, k_describe, k_desc_perm; gRefine / gCalcOrient / gDescribe2, akazed.cu:1615-2001 and 3600-3850).

Test infrastructure, numpy only, seeded; nothing here touches a device.  Every case is a pure function of (SEED, case name):
tests/test_keypoint_stage_cpu.py pins the bytes, ties the walk to the pipeline oracle and asserts the census of the edges the cases
reach; tests/test_gpu_keypoint_stage.py drives the same records and planes through hak_op_orient_describe and
hak_op_fast_orient_describe.  Every comparison is bit equality (NaN against NaN for an angle, as value_domain.same_bits states it).

Why planted keypoints.  The border rule of gCalcExtremaMap (akazed.cu:1334; oracle/akaze_oracle.c okz_extrema_map) accepts column ix
of a level when (int)(ix - border + 0.5f) - 1 >= 0, with border = 10 * sqrt(2) * sigma_size.  At dilation 2 the first accepted column is
29, and the farthest sample of a pattern-10 window turned by 45 degrees lies 2 * (10 + 10) / sqrt(2) = 28.28 px away: 0.72 px of
slack (0.57, 0.07 ... at the other dilations; `accepted` computes the domain from the schedule, nothing is restated here).  A wrong
rounding, sign or clamp in the sample position shows only for a keypoint ON the last accepted row or column that is turned close to a
diagonal, which images rarely produce.  So the records here sit on all four limits and corners of every level, one inside them, and
at random interior positions; float-path records also carry the sub-pixel offsets gRefine can leave (up to one level pixel, fractions
on both sides of .5), FAST records both parities of the full-resolution coordinate at octave 1 (the detector itself only emits even
ones there; `>> o` must not care).  Level (0, 0) also holds the 49 centres of a 7 x 7 grid of 26-px cells: the orientation disc of
such a keypoint (radius 6 * 2) stays inside its cell, which lets a plane family give every keypoint a field of its own.

Geometry: 265 x 245 (odd extents at octave 0; pitch 384 in the oracle, 320 in the library), two octaves of four sublevels; octave 1 is
132 x 122 (pitch 256 / 192) and its
sublevel 3 (border 56.57) accepts columns 58..73 and rows 58..63: the smallest size at which all eight levels have a domain.

Plane families.  Float path: every generator of tests/value_domain.py (tiers A, B and C; Lt, Lx and Ly drawn independently, so a
NaN or an inf can sit in any of the three) and five orientation fields:
  rotating    level (0, 0): cell c holds a checkerboard of the directions of bins c % 42 and (c % 42 + 6) % 42, so window c % 42 is the
              only one that holds both -- every window start wins somewhere, the wrapping ones (>= 36) included; elsewhere a field whose
              direction turns slowly across the plane
  lobes       level (0, 0): two single samples per cell, mirror images about the keypoint with opposite vectors -- two windows of
              exactly equal weight and different angle: the first strict maximum from 0 decides; elsewhere Lx = +-1 in a checkerboard
              with Ly = +0: bins 21 and 41, the latter by the clamp a > 41 (atan2(+0, -1) = pi)
  magnitudes  one direction per level, magnitudes 2^-20 .. 2^20 per pixel: a bin's float sum depends on the order of its samples
  zero        no gradient at all: angle 0 by the 0 / 0 rule
  frame       everything zero but the two outermost rows and columns of each plane (Lt included): only clamped and limit samples count
FAST path: an int32 Lt plane per level from the tests/fast_domain.py generators (the full-range ones included) and `ramp_x` (Lt falls
linearly along x: Ly = 0 and Lx < 0 everywhere, the clamp a > 41 on the integer path); Lx, Ly and the determinant are the oracle's
fast_hessian of that plane at the level's dilation, so the determinant fkz_refine reads is the one hak_det_at re-evaluates.  Such
derivatives are 16-bit numbers (the `>> 16` of gDerivate), so their rotation can never leave the int range: `raw_full_range` draws Lt, Lx
and Ly independently from fast_domain.full_range instead, with the determinant formed from those derivatives (`fast_det`) -- there the
rotated derivatives saturate.  `unit_step` plants, at the first accepted corner of every level, the determinants 4 1 0 along x and
1 2 1 along y (Lx a function of x alone, Ly of y alone: the determinant is the product of their derivatives): the refinement step is
exactly +1.0 in x, the largest the rule `> 1.f` accepts.  No family is left out.
"""
import ctypes as C
import functools
import hashlib

import numpy as np

import fast_domain as fd
import value_domain as vd

W, H = 265, 245
NOCT, MS = 2, 4
SEED = 11
PATTERNS = (10, 12, 6, 8)               # planned kernel; tail loop and live clamps; a small planned one; an unplanned one without tail
MAX_PTS = 5000                          # of the contexts: the launch-shape case holds more than 4096 records
CELLS, CELL = 7, 26                     # level (0, 0): 7 x 7 cells of 26 px from the first accepted row / column
ORIENT_FAMILIES = ("rotating", "lobes", "magnitudes", "zero", "frame")
FLOAT_FAMILIES = tuple(vd.GENERATORS) + ORIENT_FAMILIES
FAST_FAMILIES = tuple(fd.GENERATORS) + ("ramp_x", "raw_full_range", "unit_step")
f32 = np.float32


def align_up(a, b):
    return (a + b - 1) // b * b


class Sched:
    """geometry and per-level constants: whp[o] = (w, h, pitch), sizes / sigma_size / borders per level o * MS + s"""

    def __init__(self, whp, sizes, sigma_size, borders):
        self.whp = [tuple(int(v) for v in t) for t in whp]
        self.sizes, self.borders = np.asarray(sizes, np.float32).copy(), np.asarray(borders, np.float32).copy()
        self.sigma_size = np.asarray(sigma_size, np.int32).copy()
        assert len(self.whp) == NOCT and len(self.sizes) == NOCT * MS

    def same(self, other):
        """extents and level constants agree (the pitches are each side's own: the library pads rows to 64 elements, the oracle to 128;
        both differ from the width at both octaves)"""
        return ([t[:2] for t in self.whp] == [t[:2] for t in other.whp] and all(t[2] != t[0] for t in self.whp + other.whp) and self.sizes.tobytes() == other.sizes.tobytes() and self.borders.tobytes() == other.borders.tobytes()
                and self.sigma_size.tobytes() == other.sigma_size.tobytes())


def params(okz, patsize=10, upright=False):
    return okz.default_params(noctaves=NOCT, max_scale=MS, descriptor_pattern_size=patsize, upright=int(upright))


def oracle_sched(okz):
    """the schedule as the pipeline oracles form it (okz_layout + okz_schedule): what the CPU twin works from"""
    owhps, osizes, offsets = np.zeros(24, np.int32), np.zeros(8, np.int32), np.zeros(9, np.int32)
    ip = C.POINTER(C.c_int)
    noct = okz.lib().okz_layout(W, H, align_up(W, 128), NOCT, MS, owhps.ctypes.data_as(ip), osizes.ctypes.data_as(ip), offsets.ctypes.data_as(ip))
    assert noct == NOCT
    sizes, sig, borders, _ = okz.schedule(params(okz), noct)
    return Sched([owhps[3 * o:3 * o + 3] for o in range(noct)], sizes, sig, borders)


def det_sched(det):
    """the same from a context (Akazer.schedule / geometry): what the GPU tests work from"""
    s = det.schedule()
    assert s["noct"] == NOCT
    return Sched(det.geometry(), s["sizes"], s["sigma_size"], s["borders"])


def accepted(border, n, start):
    """the coordinates of an extent n the border rule accepts (akazed.cu:1345-1352; the loops start at (int)borders[sublevel 0])"""
    b, out = f32(border), []
    for i in range(start, n):
        lo = int(f32(f32(i) - b) + f32(0.5)) - 1
        hi = int(f32(f32(i) + b) + f32(0.5)) + 1
        if lo >= 0 and hi < n:
            out.append(i)
    assert out and out == list(range(out[0], out[-1] + 1))
    return out[0], out[-1]


def domain(sched, l):
    o = l // MS
    w, h, _ = sched.whp[o]
    start = int(sched.borders[o * MS])
    return accepted(sched.borders[l], w, start) + accepted(sched.borders[l], h, start)


# ------------------------------------------------------------------------------------------------ positions and records
def positions(sched, seed=SEED):
    """-> list of (level, x, y, tag) in level coordinates; tags: corner, limit, inside (one inside a limit), interior, cell"""
    out = []
    for l in range(NOCT * MS):
        rng = np.random.default_rng([seed, 4201, l])
        x0, x1, y0, y1 = domain(sched, l)
        rx = lambda: int(rng.integers(x0 + 1, x1))
        ry = lambda: int(rng.integers(y0 + 1, y1))
        out += [(l, x, y, "corner") for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        for _ in range(2):
            out += [(l, x0, ry(), "limit"), (l, x1, ry(), "limit"), (l, rx(), y0, "limit"), (l, rx(), y1, "limit")]
        out += [(l, x0 + 1, y0 + 1, "inside"), (l, x1 - 1, y1 - 1, "inside"), (l, x0 + 1, ry(), "inside"), (l, x1 - 1, ry(), "inside"),
                (l, rx(), y0 + 1, "inside"), (l, rx(), y1 - 1, "inside")]
        out += [(l, rx(), ry(), "interior") for _ in range(6)]
        if l == 0:
            assert x0 + CELLS * CELL - 1 <= x1 and y0 + CELLS * CELL - 1 <= y1
            out += [(0,) + cell_centre(sched, c) + ("cell",) for c in range(CELLS * CELLS)]
    return out


def cell_centre(sched, c):
    x0, _, y0, _ = domain(sched, 0)
    return x0 + CELL * (c % CELLS) + CELL // 2, y0 + CELL * (c // CELLS) + CELL // 2


def _below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _above(v):
    return np.nextafter(f32(v), f32(np.inf))


# sub-pixel offsets in level pixels as gRefine can leave them (|offset| <= 1) and a nudge of the resulting full-resolution coordinate by
# whole float32 steps: (int)(x + 0.5f) of the orientation and of the MLDB sample sees fractions just below, at and just above .5
OFFSETS = [(0, 0), (-1, 0), (1, 0), (0.5, 0), (0.5, -1), (0.5, 1), (-0.5, 0), (-0.5, -1), (-0.5, 1), (0.25, 0), (0.25, -1), (0.25, 1),
           (-0.75, 0), (-0.75, 1), (1, -1), (-1, 1), (0.75, -1), (-0.25, 1)]


def _nudged(v, n):
    v = f32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, f32(np.inf if n > 0 else -np.inf))
    return v


def angle_sweep(seed=SEED):
    """0, the float32 values just below, at and above k pi / 4 (k = 1..7), the value just below 2 pi, and random angles"""
    rng = np.random.default_rng([seed, 4202])
    a = [f32(0)]
    for k in range(1, 8):
        v = f32(k * np.pi / 4)
        a += [_below(v), v, _above(v)]
    a.append(_below(f32(2 * np.pi)))
    return a + [f32(v) for v in rng.uniform(0.0, 2 * np.pi, 17)]


def records(okz, sched, kind, seed=SEED):
    """-> (POINT_DTYPE array, tags).  kind: "float" (sub-pixel coordinates), "fast" (integer full-resolution coordinates, both
    parities at octave 1).  Every field the kernels must not touch holds a value of its own; `angle` holds the planted angle of the
    MLDB-alone mode (corners: the four diagonals in turn)."""
    pos = positions(sched, seed)
    rng = np.random.default_rng([seed, 4203, 0 if kind == "float" else 1])
    rec = np.zeros(len(pos), okz.POINT_DTYPE)
    sweep = angle_sweep(seed)
    for i, (l, x, y, tag) in enumerate(pos):
        o, ratio = l // MS, 1 << (l // MS)
        if kind == "fast":
            px, py = f32((x << o) + (i & o)), f32((y << o) + ((i >> 1) & o))
        elif tag == "cell":
            px, py = f32(x), f32(y)
        else:
            dx = OFFSETS[i % len(OFFSETS)] if tag != "interior" else (rng.uniform(-1, 1), 0)
            dy = OFFSETS[(i * 7 + 3) % len(OFFSETS)] if tag != "interior" else (rng.uniform(-1, 1), 0)
            px = _nudged(f32(ratio * f32(f32(x) + f32(dx[0]))), dx[1])                    # akazed.cu:1659-1660
            py = _nudged(f32(ratio * f32(f32(y) + f32(dy[0]))), dy[1])
        rec[i]["x"], rec[i]["y"], rec[i]["octave"], rec[i]["size"] = px, py, l, sched.sizes[l]
        rec[i]["angle"] = f32((2 * ((l + i) % 4) + 1) * np.pi / 4) if tag == "corner" else sweep[(i * 5 + l) % len(sweep)]
        rec[i]["response"] = f32(1000.5 + i)
        rec[i]["features"], rec[i]["_pad"] = 0xAB, (0xC1, 0xC2, 0xC3)
        rec[i]["match"], rec[i]["distance"], rec[i]["match_x"], rec[i]["match_y"] = 70000 + i, -3 - i, f32(0.25 + i), f32(-0.75 - i)
    return rec, [p[3] for p in pos]


def many_records(okz, sched, kind, n=4400, seed=SEED):
    """the launch-shape case: the same records repeated in mixed level order until both grids (1024 and 4096 blocks) loop"""
    rec, _ = records(okz, sched, kind, seed)
    rng = np.random.default_rng([seed, 4204])
    out = rec[rng.integers(0, len(rec), n)].copy()
    out["response"] = np.arange(n, dtype=np.float32) + f32(0.5)
    out["match"] = np.arange(n) + 70000
    assert n > 4096 and n <= MAX_PTS and len(set(out["octave"][:64])) == NOCT * MS
    return out


# ------------------------------------------------------------------------------------------------ planes
def _pitched(a, p):
    out = np.zeros((a.shape[0], p), a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _bin_dir(b):
    """a direction in the middle of orientation bin b.  a = (int)(angle * 21 / pi) + 21 truncates toward zero (akazed.cu:1702): bin 21 is
    two units wide, bins 1..20 end at a multiple of pi / 21 and bins 22..41 start at one; bin 0 holds the angle -pi alone (`_unit`)"""
    b = np.asarray(b)
    return np.where(b < 21, b - 21.5, np.where(b == 21, 0.0, b - 20.5)) * np.pi / 21


def _unit(b):
    """(x, y) of a unit vector in bin b; bin 0 = (-1, -1e-20): the statement's atan2 is -pi (as a float, just below it) only for a
    negative y that vanishes against x -- atan2(-0, -1) is +pi, bin 41 by the clamp"""
    th = _bin_dir(b)
    return np.where(b == 0, -1.0, np.cos(th)), np.where(b == 0, -1e-20, np.sin(th))


def _checker(sched, l, xx, yy):
    """a checkerboard of the level's sample step (int)(size + 0.5f): neighbouring SAMPLES of any keypoint differ"""
    step = int(sched.sizes[l] + f32(0.5))
    return (xx // step + yy // step) % 2 == 0


def _orient_planes(name, sched, l, seed):
    o = l // MS
    w, h, _ = sched.whp[o]
    rng = np.random.default_rng([seed, 4205, l, ORIENT_FAMILIES.index(name)])
    yy, xx = np.mgrid[0:h, 0:w]
    lt = vd.GENERATORS["hdr"](w, h, seed + l)
    if name == "zero":
        return lt, np.zeros((h, w), f32), np.zeros((h, w), f32)
    if name == "frame":
        edge = (xx < 2) | (xx > w - 3) | (yy < 2) | (yy > h - 3)
        r = lambda: np.where(edge, rng.uniform(-1, 1, (h, w)), 0.0).astype(f32)
        return r(), r(), r()
    if name == "magnitudes":
        mag = np.ldexp(rng.uniform(1.0, 2.0, (h, w)), rng.integers(-20, 21, (h, w)))
        th = 0.3 + 0.77 * l
        return lt, (mag * np.cos(th)).astype(f32), (mag * np.sin(th)).astype(f32)
    if name == "rotating":
        th = 0.02 * xx + 0.013 * yy + l
        amp = rng.uniform(0.5, 1.5, (h, w))
        ux, uy = np.cos(th), np.sin(th)
        if l == 0:
            x0, _, y0, _ = domain(sched, 0)
            cx, cy = (xx - x0) // CELL, (yy - y0) // CELL
            incell = (cx >= 0) & (cx < CELLS) & (cy >= 0) & (cy < CELLS)
            b = (cy * CELLS + cx) % 42
            cxu, cyu = _unit(np.where(_checker(sched, 0, xx, yy), b, (b + 6) % 42))
            ux, uy = np.where(incell, cxu, ux), np.where(incell, cyu, uy)
        return lt, (amp * ux).astype(f32), (amp * uy).astype(f32)
    assert name == "lobes"
    if l != 0:
        return lt, np.where(_checker(sched, l, xx, yy), f32(1), f32(-1)).astype(f32), np.zeros((h, w), f32)
    lx, ly = np.zeros((h, w), f32), np.zeros((h, w), f32)
    step = int(sched.sizes[0] + f32(0.5))
    disc = [(i, j) for j in range(-6, 7) for i in range(-6, 10) if i * i + j * j < 36 and (i, j) != (0, 0)]
    for c in range(CELLS * CELLS):
        x, y = cell_centre(sched, c)
        i, j = disc[int(rng.integers(0, len(disc)))]
        vx, vy = f32(rng.uniform(-1, 1)), f32(rng.uniform(-1, 1))
        lx[y + step * j, x + step * i], ly[y + step * j, x + step * i] = vx, vy
        lx[y - step * j, x - step * i], ly[y - step * j, x - step * i] = -vx, -vy
    return lt, lx, ly


@functools.lru_cache(maxsize=2)
def float_planes(okz, family, seed=SEED):
    """-> per level dict(lt, lx, ly): pitched float32 planes (the dense part is what hak_debug_set_plane gets)"""
    sched = oracle_sched(okz)
    out = []
    for l in range(NOCT * MS):
        w, h, p = sched.whp[l // MS]
        if family in ORIENT_FAMILIES:
            lt, lx, ly = _orient_planes(family, sched, l, seed)
        else:
            g = vd.GENERATORS[family]
            lt, lx, ly = g(w, h, seed + 3 * l), g(w, h, seed + 3 * l + 1), g(w, h, seed + 3 * l + 2)
        out.append(dict(lt=_pitched(lt, p), lx=_pitched(lx, p), ly=_pitched(ly, p)))
    return out


def fast_det(okz, lx, ly, w, step):
    """the determinant plane of given derivative planes: the second half of gHessianDeterminant (akazed.cu:3371-3403) in the wrapping
    int64 arithmetic of tests/fast_domain.py -- what hak_det_at<int> re-evaluates on the device.  The CPU twin checks it against
    fkz_hessian on every family whose derivatives come from there."""
    A = fd.Arith(True)
    fac1, fac2 = okz.fast_deriv_factors()
    p = lx.shape[1]

    def d(q, S):
        ul, uc, ur = fd.shifted(q, -S, -S), fd.shifted(q, -S, 0), fd.shifted(q, -S, S)
        cl, cr = fd.shifted(q, 0, -S), fd.shifted(q, 0, S)
        ll, lc, lr = fd.shifted(q, S, -S), fd.shifted(q, S, 0), fd.shifted(q, S, S)
        gx = A.add(A.mul(fac1, A.sub(A.sub(A.add(ur, lr), ul), ll)), A.mul(fac2, A.sub(cr, cl))) >> 16
        gy = A.add(A.mul(fac1, A.sub(A.sub(A.add(lr, ll), ur), ul)), A.mul(fac2, A.sub(lc, uc))) >> 16
        return gx, gy
    dxx, dxy = d(np.asarray(lx[:, :w], np.int64), step)
    _, dyy = d(np.asarray(ly[:, :w], np.int64), step)
    det = A.sub(A.mul(dxx, dyy), A.mul(dxy, dxy))
    return _pitched(det.astype(np.int32), p)


def _integrate(F, n, step):
    """f with (f(t + step) - f(t - step)) >> 1 == F.get(t, 0): a derivative plane whose own derivative at dilation `step` is F (the
    weights of gDerivate add up to 32768 along the axis, akazed.cu:3339-3368)"""
    f = np.zeros(n + step, np.int64)
    for t in range(step, n):
        f[t + step] = f[t - step] + 2 * F.get(t, 0)
    return f[:n].astype(np.int32)


@functools.lru_cache(maxsize=2)
def fast_planes(okz, family, seed=SEED):
    """-> per level dict(lt, lx, ly, det): pitched int32 planes; Lx, Ly, det = the oracle's fast_hessian of Lt at the level's dilation"""
    sched = oracle_sched(okz)
    out = []
    for l in range(NOCT * MS):
        w, h, p = sched.whp[l // MS]
        if family == "raw_full_range":
            lt, lx, ly = (_pitched(fd.full_range(w, h, seed + 3 * l + k), p) for k in range(3))
            out.append(dict(lt=lt, lx=lx, ly=ly, det=fast_det(okz, lx, ly, w, int(sched.sigma_size[l]))))
            continue
        if family == "unit_step":
            x0, _, y0, _ = domain(sched, l)
            step = int(sched.sigma_size[l])
            lt = _pitched(fd.u8_range(w, h, seed + l), p)
            lx = _pitched(np.ascontiguousarray(np.broadcast_to(_integrate({x0 - 1: 4, x0: 1}, w, step), (h, w))), p)
            ly = _pitched(np.ascontiguousarray(np.broadcast_to(_integrate({y0 - 1: 1, y0: 2, y0 + 1: 1}, h, step)[:, None], (h, w))), p)
            out.append(dict(lt=lt, lx=lx, ly=ly, det=fast_det(okz, lx, ly, w, step)))
            continue
        if family == "ramp_x":
            lt = np.ascontiguousarray(np.broadcast_to((200000 - 700 * np.arange(w, dtype=np.int64)).astype(np.int32), (h, w)))
        else:
            lt = fd.GENERATORS[family](w, h, seed + l)
        lt = _pitched(lt, p)
        lx, ly, det = okz.fast_hessian(lt, w, int(sched.sigma_size[l]))
        out.append(dict(lt=lt, lx=lx, ly=ly, det=det))
    return out


def digest(rec, planes):
    hsh = hashlib.sha256(rec.tobytes())
    for lv in planes:
        for k in sorted(lv):
            hsh.update(np.ascontiguousarray(lv[k]).tobytes())
    return hsh.hexdigest()


# ------------------------------------------------------------------------------------------------ the oracle walk
MODES = ("orient", "angles", "upright")     # orientation + MLDB; MLDB alone with the planted angles (float path only); upright


def oracle_walk(okz, sched, rec, planes, mode, patsize, fast, census=False):
    """the statement of one call: per record (FAST: fkz_refine ->) orientation (mode "orient") -> MLDB, by the oracle's point functions
    (okz_refine_point is not part of it: the float path refines in the detector tail).  -> records, or (records, census rows) where a
    row is (clamp[4], min_edge, bin_hi, bin_lo, bin0, bin41, maxk, refined, saturated, tie) of that record's calls."""
    assert mode in MODES and not (fast and mode == "angles")
    L = okz.lib()
    vp = C.c_void_p
    out = rec.copy()
    wtab = okz.orient_weights()
    i1, i2 = okz.compare_indices()
    ptr = {l: {k: vp(a.ctypes.data) for k, a in lv.items()} for l, lv in enumerate(planes)}
    refine, orient, describe = (L.fkz_refine, L.fkz_orient, L.fkz_describe) if fast else (None, L.okz_orient_point, L.okz_describe_point)
    rows = []
    for i in range(len(out)):
        l = int(out["octave"][i])
        o = l // MS
        w, h, p = sched.whp[o]
        pt, q = vp(out.ctypes.data + i * out.itemsize), ptr[l]
        cen = okz.census_begin() if census else None
        if fast:
            refine(pt, q["det"], C.c_int(o), C.c_int(p))
        if mode == "upright":
            out["angle"][i] = 0
        elif mode == "orient":
            orient(pt, q["lx"], q["ly"], C.c_int(o), C.c_int(w), C.c_int(h), C.c_int(p), wtab.ctypes.data_as(C.POINTER(C.c_float)))
        describe(pt, q["lt"], q["lx"], q["ly"], C.c_int(o), C.c_int(w), C.c_int(h), C.c_int(p), C.c_int(patsize),
                 i1.ctypes.data_as(C.POINTER(C.c_int)), i2.ctypes.data_as(C.POINTER(C.c_int)))
        if census:
            okz.census_end()
            rows.append((tuple(cen.clamp), cen.min_edge, cen.bin_hi, cen.bin_lo, cen.bin0, cen.bin41, cen.maxk, cen.refined, cen.saturated, cen.tie))
    return (out, rows) if census else out


def first_difference(got, want):
    """-> None, or (record index, field) of the first record that differs, at its first differing stage: x, y (refinement), angle
    (orientation), features (MLDB), then the fields no kernel may touch.  Later fields are only judged when the earlier ones agree.
    Bit equality; two NaN angles agree whatever their payload (value_domain.same_bits)."""
    assert got.dtype == want.dtype and len(got) == len(want)
    for f in ("x", "y", "angle", "features", "octave", "response", "size", "_pad", "match", "distance", "match_x", "match_y"):
        g, w = got[f], want[f]
        if g.dtype.kind == "f":
            bad = ~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = (g != w).reshape(len(got), -1).any(axis=1)
        if bad.any():
            return int(np.argmax(bad)), f
    return None

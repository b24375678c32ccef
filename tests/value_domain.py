"""Content generators for the value-domain parity tests: float32 planes beyond "uint8 scene / 255".

Test infrastructure, numpy only, seeded; no GPU.  (The base scene comes from tests/golden/make_golden.py, which imports akaze_hip and so
needs libhipakaze.so built -- as tests/fuzz_parity.py does; nothing here touches a device.)  Every generator is a function (w, h, seed) -> float32 (h, w) with the attributes
`.tier` and `.name`; GENERATORS maps name -> function in a fixed order.

  tier A  finite, every value in [0, 1]           the oracle's outputs are finite everywhere (tests/test_value_domain_cpu.py asserts it)
  tier B  finite, any range                       squares and sums may overflow: inf and NaN appear in the OUTPUTS
  tier C  non-finite pixels in the input

All classes but `ramp` and `ulp_noise` start from one base: tests/golden/make_golden.case_scene (the suite's uint8 scenes) / 255 plus a
smooth float term plus 2e-3 of uniform noise, clipped to [0, 1] in float64 and rounded once to float32 -- so the base uses the whole
24-bit significand (a 320 x 240 base has > 70 000 distinct values on a lattice of 2^24 levels per binade; uint8 / 255 content has 256).
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO64 = np.float32(2.0 ** 64)           # hak_rcp_newton (csrc/fed_common.h) is the IEEE quotient on [1, 2^64) only

_mg_mod = None


def _mg():
    global _mg_mod
    if _mg_mod is None:
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
        _mg_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_mg_mod)
    return _mg_mod


def float_term(w, h, seed):
    """the float part of the base (float64): a smooth term of amplitude 0.01 plus uniform noise of amplitude 2e-3"""
    rng = np.random.default_rng([seed, 7701])
    ph = 0.1 * (seed % 61)
    smooth = np.outer(np.cos(np.arange(h) * 0.23 - ph), 0.01 * np.sin(np.arange(w) * 0.37 + ph))
    return smooth + rng.uniform(-1.0, 1.0, (h, w)) * 2e-3


def from_u8(u8, seed):
    """the base over a given uint8 scene, float64 in [0, 1] (tests/fuzz_parity.py feeds its own scenes through this)"""
    h, w = u8.shape
    return np.clip(u8.astype(np.float64) / 255.0 + float_term(w, h, seed), 0.0, 1.0)


def base64(w, h, seed):
    u8 = _mg().case_scene(max(w, 134), h, seed % 9973)[:, :w]                  # (134: the scene generator's minimum width)
    return from_u8(u8, seed)


def _f32(a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


GENERATORS = {}


def _gen(tier):
    def deco(fn):
        fn.tier, fn.name = tier, fn.__name__
        GENERATORS[fn.__name__] = fn
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ tier A: finite, [0, 1]
@_gen("A")
def hdr(w, h, seed):
    return _f32(base64(w, h, seed))


@_gen("A")
def ramp(w, h, seed):
    """smooth gradients only, no 8-bit component: sums that are exact on quantised input are inexact on every pixel here"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.1 * (seed % 61)
    a = 0.5 + 0.22 * np.sin(xx * 0.0131 + ph) * np.cos(yy * 0.0173 - ph) + 0.2 * (xx / w - 0.5) + 0.07 * np.sin((xx + 2 * yy) * 0.11)
    return _f32(np.clip(a, 0.0, 1.0))


@_gen("A")
def ulp_noise(w, h, seed):
    rng = np.random.default_rng([seed, 7702])
    a = np.full((h, w), 0.5, np.float32)
    return np.where(rng.integers(0, 2, (h, w)) == 1, np.nextafter(np.float32(0.5), np.float32(1.0)), a).astype(np.float32)


@_gen("A")
def dark(w, h, seed):
    return _f32(base64(w, h, seed) * 1e-6)


@_gen("A")
def tiny(w, h, seed):
    return _f32(base64(w, h, seed) * 1e-30)


@_gen("A")
def denormal(w, h, seed):
    """every value is subnormal (< 2^-126 = 1.18e-38) or zero"""
    return _f32(base64(w, h, seed) * 1e-38)


@_gen("A")
def sub_squares(w, h, seed):
    """base x 1e-18: the planes themselves are normal numbers, their SQUARES and products are not.  Scharr gradients reach ~1e-19, so
    dx * dx, dx * dx + dy * dy and the determinants dxx * dyy - dxy * dxy lie on both sides of 2^-126 (1.18e-38), most of them below
    (asserted in tests/test_value_domain_cpu.py); at dthreshold 1e-39 all but one keypoint response is subnormal.  `tiny` and
    `denormal` cannot do this: their squares are exactly 0"""
    return _f32(base64(w, h, seed) * 1e-18)


@_gen("A")
def signed_zero(w, h, seed):
    a = _f32(base64(w, h, seed))
    a[h // 5: h // 5 + max(4, h // 6), w // 6: w // 6 + max(8, w // 4)] = np.float32(0.0)
    a[h // 2: h // 2 + max(4, h // 5), w // 2: w // 2 + max(8, w // 3)] = np.float32(-0.0)
    a[h - 3:, : w // 3] = np.float32(-0.0)                                      # the mirrored bottom rows
    a[:, 0:2][::2] = np.float32(0.0)                                            # and alternate rows of the first columns
    return a


# ------------------------------------------------------------------------------------------------ tier B: finite, any range
@_gen("B")
def x255(w, h, seed):
    return _f32(base64(w, h, seed) * 255.0)


@_gen("B")
def x65535(w, h, seed):
    return _f32(base64(w, h, seed) * 65535.0)


@_gen("B")
def offset(w, h, seed):
    return _f32(base64(w, h, seed) - 0.5)


@_gen("B")
def negated(w, h, seed):
    return _f32(-base64(w, h, seed))


@_gen("B")
def x1e10(w, h, seed):
    return _f32(base64(w, h, seed) * 1e10)


@_gen("B")
def x1e18(w, h, seed):
    """Scharr differences reach 16e18: their squares overflow float32 at some pixels and stay finite at others"""
    return _f32(base64(w, h, seed) * 1e18)


def spike_sites(w, h):
    """isolated pixels (x, y, amplitude): x % 32 == 8 and y % 16 == 8, at least five pixels away from the contrast maximum's 16-px
    lattice, so the contrast factor stays that of the base.  Amplitudes 1e12 .. 1e25 in turn: with the Scharr weights a spike of 1e12
    gives gradient squares of ~1e26 (conductivity denominators far beyond 2^64, finite), one of 1e19 or more squares to inf"""
    amps = np.geomspace(1e12, 1e25, 14)
    sites, k = [], 0
    for y in range(8, h - 4, 16):
        for x in range(8 + 16 * ((y // 16) % 2), w - 4, 32):
            sites.append((x, y, amps[k % len(amps)]))
            k += 1
    return sites


@_gen("B")
def spikes(w, h, seed):
    """the base with isolated pixels of 1e12 .. 1e25: around each one the PM_G2 denominators 1 + dif2 are >= 2^64 (or inf), while the
    pixels between two spikes of a row keep denominators of order 1 -- fast and slow lanes of the reciprocal inside one wave"""
    a = base64(w, h, seed)
    for x, y, amp in spike_sites(w, h):
        a[y, x] = amp
    return _f32(a)


@_gen("B")
def spikes_strip(w, h, seed):
    """the base with a band of six full-width rows of random values around 1e14: every denominator of a whole 256-pixel strip is
    >= 2^64 there (all lanes of a wave on the IEEE division).  The band lies between two lattice rows"""
    a = base64(w, h, seed)
    rng = np.random.default_rng([seed, 7703])
    y0 = 16 * max(1, h // 48) + 5                                               # rows y0 .. y0+5, influence y0-3 .. y0+8: no y % 16 == 0
    a[y0:y0 + 6, :] = 1e14 * rng.uniform(0.25, 1.75, (6, w))
    return _f32(a)


@_gen("B")
def flt_max_step(w, h, seed):
    """the base | six columns of 0 | 3e38 over the last quarter of the width: sums of two neighbours overflow to inf on the far side"""
    a = base64(w, h, seed)
    x0 = w - w // 4
    a[:, x0 - 6:x0] = 0.0
    a[:, x0:] = 3e38
    return _f32(a)


# ------------------------------------------------------------------------------------------------ tier C: non-finite pixels
@_gen("C")
def one_nan(w, h, seed):
    a = _f32(base64(w, h, seed))
    a[h // 2 - 3, w // 2 + 5] = np.nan
    return a


@_gen("C")
def one_inf(w, h, seed):
    a = _f32(base64(w, h, seed))
    a[h // 2 - 3, w // 2 + 5] = np.inf
    return a


@_gen("C")
def neg_inf_block(w, h, seed):
    a = _f32(base64(w, h, seed))
    a[h // 4: h // 4 + 4, w // 8: w // 8 + 4] = -np.inf
    return a


@_gen("C")
def nan_column(w, h, seed):
    a = _f32(base64(w, h, seed))
    a[:, w // 3] = np.nan
    return a


@_gen("C")
def nan_frame(w, h, seed):
    """NaN on the outermost image row and column, where reflect-101 and the decimation mirror read"""
    a = _f32(base64(w, h, seed))
    a[0, :] = a[h - 1, :] = np.nan
    a[:, 0] = a[:, w - 1] = np.nan
    return a


TIERS = {t: [n for n, g in GENERATORS.items() if g.tier == t] for t in "ABC"}
RANGE = {"A": (0.0, 1.0)}

# Detector thresholds for the tier-A classes whose determinants lie far below the default 1e-3 (the response scales with the square of
# the amplitude): values at which the ORACLE finds more than 50 keypoints at 320 x 240, seed 5 (118 of them) -- asserted in
# tests/test_value_domain_cpu.py.  1e-39 is itself a subnormal float32.  `ulp_noise`, `tiny` and `denormal` have no such value: their determinants underflow to zero in
# float32 (amplitude^2 <= 1e-60; the base low-pass rounds the ulp noise away), which the same module asserts.
LOW_DTHRESHOLD = {"dark": 1e-15, "sub_squares": 1e-39}


def pitched(a, pitch=None):
    """dense (h, w) -> zero-padded (h, pitch) plane"""
    h, w = a.shape
    p = pitch or (w + 63) // 64 * 64
    out = np.zeros((h, p), np.float32)
    out[:, :w] = a
    return out


def same_bits(got, want):
    """THE comparison rule: two float32 arrays agree iff at each element the uint32 words are equal or both elements are NaN (sign and
    payload of a NaN are not defined by the reference; -0 and +0 are different words and must match).
    -> (ok, number of elements that passed by the NaN clause, index of the first mismatch or None)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    eqw = got.view(np.uint32) == want.view(np.uint32)
    both_nan = np.isnan(got) & np.isnan(want)                                   # (counted whether or not the words happen to agree)
    bad = ~(eqw | both_nan)
    first = tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None
    return not bad.any(), int(both_nan.sum()), first


# ------------------------------------------------------------------------------------------------ the stage cases both test modules share
# one single narrow strip; one that crosses the streaming kernels' 240 / 256-px strip edges with w % 4 != 0; one with w % 4 == 0 that
# crosses a strip edge and has >= 4 row segments of 50 rows (geometry itself is covered by tests/test_gpu_stages.py and the sweeps)
STAGE_SHAPES = [(128, 96), (517, 130), (260, 203)]
LOWPASS = [(1.0, 2), (2.56, 4)]
TAU_LISTS = [[0.07], [0.1, 0.68, 0.08, 0.19], [5.0, 41.0, 0.3]]               # the last one is far above the stability limit 0.25
HESS_STEPS = [2, 3, 4, 6]
KC_EXTREME = [1e-30, 1e30]                                                      # ikc = 1 / (kc * kc) = inf and 0
KC_UNIT = 1.0                                                                   # ikc = 1: dif2 IS the squared gradient (subnormal on `sub_squares`)
PER = 0.7


def own_kcontrast(okz, a, w):
    """(kcontrast, hmax, hist, low-pass) of a pitched plane, as the octave-0 prologue forms them (akaze.cpp:319-326)"""
    sm = okz.lowpass(a, w, 1.0, 2)
    with np.errstate(all="ignore"):
        kc, hmax, hist = okz.kcontrast(okz.scharr_grad(sm, w), w, PER)
    return kc, hmax, hist, sm


def oracle_stage_cases(okz, a, w, ops=None):
    """every stage case of a pitched plane `a` (valid width w) -> yields (op, label, extreme, args, [(name, oracle output, valid width)]).
    `extreme`: the case uses a contrast factor of KC_EXTREME (its tier is at least B whatever the input's: ikc = inf times a zero
    gradient is NaN).  `args`: what the HIP operator of that case is called with; the GPU module drives the same list through hak_op_*."""
    h = a.shape[0]
    want = lambda op: ops is None or op in ops
    with np.errstate(all="ignore"):
        kc = None
        if want("flow") or want("smooth_flow") or want("nld_steps") or want("kcontrast"):
            kc, hmax, hist, sm = own_kcontrast(okz, a, w)
        if want("lowpass"):
            for var, R in LOWPASS:
                yield "lowpass", f"var={var},R={R}", False, dict(var=var, R=R), [("lowpass", okz.lowpass(a, w, var, R), w)]
        if want("down_smooth"):
            dw, dh = w >> 1, h >> 1
            dp = (dw + 63) // 64 * 64
            dst, dsm = okz.down_smooth(a, w, dw, dh, dp)
            yield "down_smooth", "", False, dict(dw=dw, dh=dh, dp=dp), [("down", dst, dw), ("down_smooth", dsm, dw)]
        if want("kcontrast"):
            yield "kcontrast", "", False, dict(sm=sm), [("kcontrast,hmax", np.array([[kc, hmax]], np.float32), 2), ("hist", hist, None)]
        for op in ("flow", "smooth_flow"):
            if not want(op):
                continue
            src = a if op == "flow" else sm
            for diff in (0, 1, 2, 3):
                for k, ext in [(float(kc), False), (KC_UNIT, False)] + [(v, True) for v in KC_EXTREME]:
                    outs = [("flow", okz.flow(src, w, diff, k), w)]
                    if op == "smooth_flow":
                        outs.insert(0, ("smooth", sm, w))
                    yield op, f"diff={diff},kc={k!r}", ext, dict(diff=diff, kc=k), outs
        if want("nld_steps"):
            g = okz.flow(a, w, 1, float(kc))
            for taus in TAU_LISTS:
                yield "nld_steps", f"taus={taus}", False, dict(g=g, taus=taus), [("nld", okz.nld_steps(a, g, w, taus), w)]
        if want("hessian"):
            for step in HESS_STEPS:
                lx, ly, det = okz.hessian(a, w, step)
                yield "hessian", f"step={step}", False, dict(step=step), [("Lx", lx, w), ("Ly", ly, w), ("det", det, w)]


OPS = ("lowpass", "down_smooth", "kcontrast", "flow", "smooth_flow", "nld_steps", "hessian")

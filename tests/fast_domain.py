"""Inputs, int64 restatements and the case list of the stage-parity tests of the integer FAST path (fastakaze, akazed.cu:2781-4367).

Test infrastructure, numpy only, seeded; nothing here touches a device.  tests/test_fast_domain_cpu.py checks the inputs and the oracle
(oracle/akaze_oracle_fast.c) on them, tests/test_gpu_fast_stages.py drives the same case list through the hak_op_fast_* operators.

The FAST planes are int32 in 16.16 fixed point.  A uint8 scene never leaves that range, but the launch sequence does: a long FED
cycle at a coarse level blows a plane up, and from then on 32-bit products wrap, sums of squares turn negative, the conductivity is the
sqrt of a negative number or the exp of a huge one, and a histogram index wraps below zero.  The statement defines all of that (F1 and
f2i_sat in akaze_oracle_fast.c): products wrap as v_mul_lo_u32, float -> int saturates with NaN -> 0, `>> 16` is arithmetic.  So ANY
int32 value is a valid plane element, and the generators below cover the whole domain:

  u8_range       a tests/golden/make_golden.case_scene in 0..255: the control, in which nothing wraps
  signed         the scene minus 128: negative products through `>> 16`, where floor and truncation differ by one
  ramp_blown     the scene times an amplitude that rises from 2^6 to 2^22 across every 256 columns: in one plane, and inside one
                 256-px strip, the Scharr sum of squares is exact, then wrapped negative, then wrapped positive again
  full_range     uniform random int32 with INT_MIN, INT_MAX, -1 and 0 planted on the first and last row and column and at a strip
                 edge; the 3 x 3 neighbourhoods of the contrast lattice (x % 16 == y % 16 == 0) hold a few counts of noise, so that the
                 lattice maximum stays small and grad * hfactor wraps below zero for the other pixels' gradients
  int_min_block  `signed` with a 4 x 4 block of INT_MIN and one of INT_MAX
  u8_checker, u8_flat255   (uint8 operators only) a 0 / 255 checkerboard and all-255: the largest row sums

The integer contrast factor is covered for 0 .. 46340 (okz.FAST_KC_MAX).  0 is what a flat image yields: ikc = 1 / (0 * 0) = inf and
dif2 = 0 * inf can be NaN.  From 46341 on, kcontrast * kcontrast is a signed overflow in the reference (akazed.cu:4215) and in
fkz_flow alike: outside the statement and not tested.
"""
import numpy as np

import value_domain as vd

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SEED = 5
PER = vd.PER
# the smallest shapes that still vary the kernel selection: 128 = half a strip; 517 = three strips, a ragged last one, w % 4 != 0;
# 260 = a 4-px tail strip; 83 = one step per launch (w % 4 != 0) and no streaming Hessian.  Odd and even extents both occur
SHAPES = vd.STAGE_SHAPES + [(83, 81)]
HEAD_SOURCES = SHAPES + [(520, 406)]                       # (520, 406) -> a 260 x 203 head: even source, a strip edge in the result
LOWPASS = [(1.0, 2), (2.56, 4), (1.3, 3), (3.2, 5)]        # (var, R) of tests/test_gpu_stages.py
BASE_UNFUSED = (0.3, 1)                                    # the radius hak_launch_base_level does not cover: the three-launch fallback
# tau = 41: stepfac = 1 343 488, stepfac * step wraps (F1).  The 7-step list makes two launches of 4 + 3 steps under the FAST group rule
# (at most 4 per launch): the ping-pong through d_tmp, and the k_fed_sf launch that writes its conductivity plane for the second one
TAU_LISTS = vd.TAU_LISTS + [[0.1, 0.3, 0.07, 0.5, 0.12, 0.25, 2.0]]
# 37 steps, level_tile only: k_level_tile takes at most 36 per launch, so the cycle is 19 + 18 and the second launch is the continuation
# form (low-pass re-read from d_smooth, d_tmp in use); one step far above the stability limit sits in the second launch
LONG_TAUS = [0.05 + 0.01 * (i % 7) for i in range(30)] + [41.0] + [0.08, 0.11, 0.06, 0.2, 0.09, 0.13]
HESS_STEPS = [1, 2, 3, 4, 5, 6]
KC_FIXED = [0, 1, 46340]                                   # + the plane's own fkz_kcontrast
PM_G1, PM_G2, WEICKERT, CHARBONNIER = 0, 1, 2, 3           # diffusivity (hipakaze.h; `type` of fkz_flow)
BATCH = 3


def scene(w, h, seed):
    return vd._mg().case_scene(max(w, 134), h, seed % 9973)[:, :w].astype(np.int32)      # (134: the scene generator's minimum width)


GENERATORS = {}
U8_GENERATORS = {}


def _gen(table):
    def deco(fn):
        fn.name = fn.__name__
        table[fn.__name__] = fn
        return fn
    return deco


@_gen(GENERATORS)
def u8_range(w, h, seed):
    return np.ascontiguousarray(scene(w, h, seed))


@_gen(GENERATORS)
def signed(w, h, seed):
    return np.ascontiguousarray(scene(w, h, seed) - 128)


def ramp_amplitude(w):
    """amplitude per column: 2^6 over the first 15 % of every 256 columns (or of the width), then geometric up to 2^22"""
    period = min(w, 256)
    u = (np.arange(w) % period) / float(period - 1)
    return np.floor(2.0 ** (6.0 + 16.0 * np.clip((u - 0.15) / 0.85, 0.0, 1.0))).astype(np.int64)


@_gen(GENERATORS)
def ramp_blown(w, h, seed):
    return np.ascontiguousarray((scene(w, h, seed).astype(np.int64) * ramp_amplitude(w)[None, :]).astype(np.int32))   # (255 * 2^22 < 2^31)


def lattice_sites(w, h):
    return [(x, y) for y in range(0, h, 16) for x in range(0, w, 16)]


@_gen(GENERATORS)
def full_range(w, h, seed):
    rng = np.random.default_rng([seed, 8801])
    a = rng.integers(INT_MIN, INT_MAX + 1, (h, w), dtype=np.int64)
    special = [INT_MIN, INT_MAX, -1, 0]
    for k, x in enumerate(range(3, w - 1, 7)):
        a[0, x] = special[k % 4]
        a[h - 1, x] = special[(k + 1) % 4]
    for k, y in enumerate(range(3, h - 1, 7)):
        a[y, 0] = special[(k + 2) % 4]
        a[y, w - 1] = special[(k + 3) % 4]
    for xe in (239, 240, 255, 256):                         # the streaming kernels' strip edges
        if xe < w:
            a[h // 3: h // 3 + 4, xe] = special
    for x, y in lattice_sites(w, h):                        # quiet lattice neighbourhoods (module docstring)
        y0, y1, x0, x1 = max(y - 1, 0), min(y + 2, h), max(x - 1, 0), min(x + 2, w)
        a[y0:y1, x0:x1] = 1000 + rng.integers(-3, 4, (y1 - y0, x1 - x0))
    return np.ascontiguousarray(a.astype(np.int32))


@_gen(GENERATORS)
def int_min_block(w, h, seed):
    a = signed(w, h, seed)
    a[h // 4: h // 4 + 4, w // 5: w // 5 + 4] = INT_MIN
    a[h // 2: h // 2 + 4, w // 2 + 3: w // 2 + 7] = INT_MAX
    return a


@_gen(U8_GENERATORS)
def u8_scene(w, h, seed):
    """the uint8 image behind `u8_range`"""
    return np.ascontiguousarray(scene(w, h, seed).astype(np.uint8))


@_gen(U8_GENERATORS)
def u8_checker(w, h, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray((((xx + yy + seed) & 1) * 255).astype(np.uint8))


@_gen(U8_GENERATORS)
def u8_flat255(w, h, seed):
    return np.full((h, w), 255, np.uint8)


COMPLETE = ("u8_range", "ramp_blown", "full_range")       # generators whose argument lists are never shortened


def pitched(a, pitch=None):
    """dense (h, w) -> zero-padded (h, pitch) plane of the same dtype (value_domain.pitched for int32 / uint8)"""
    h, w = a.shape
    p = pitch or (w + 63) // 64 * 64
    out = np.zeros((h, p), a.dtype)
    out[:, :w] = a
    return out


# ------------------------------------------------------------------------------------------------ int64 restatements
class Arith:
    """Integer arithmetic on int64 arrays that either wraps every result to int32 (wrap=True: what the device does) or keeps the exact
    value (wrap=False).  `out_of_range` counts the results of either mode that did not fit int32, `mask` marks the pixels at which one
    did (over the operations on planes of the shape of the last one)."""

    def __init__(self, wrap):
        self.wrap, self.out_of_range, self.mask = wrap, 0, None

    def fit(self, v):
        v = np.asarray(v, np.int64)
        bad = (v < INT_MIN) | (v > INT_MAX)
        self.out_of_range += int(bad.sum())
        if bad.ndim == 2:
            self.mask = bad if self.mask is None or self.mask.shape != bad.shape else self.mask | bad
        return wrap32(v) if self.wrap else v

    def mul(self, a, b):
        return self.fit(np.asarray(a, np.int64) * np.asarray(b, np.int64))

    def add(self, a, b):
        return self.fit(np.asarray(a, np.int64) + np.asarray(b, np.int64))

    def sub(self, a, b):
        return self.fit(np.asarray(a, np.int64) - np.asarray(b, np.int64))


def wrap32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def refl(i, n):
    """reflect-101 as the reference: abs on the left / top, borderAdd on the right / bottom (akazed.cu:162-170)"""
    i = np.abs(i)
    return np.where(i < n, i, n + n - 2 - i)


def shifted(a, dy, dx):
    h, w = a.shape
    return a[refl(np.arange(h) + dy, h)][:, refl(np.arange(w) + dx, w)]


def np_conv(A, a, k, R, sums=None):
    """gConv2d: row pass (k0 c + sum k_i (l + r)) >> 16, column pass the same on the row results (akazed.cu:2922-3075).
    sums: a list that receives the two passes' sums before their `>> 16`"""
    def one(src, axis):
        ws = A.mul(int(k[0]), src)
        for i in range(1, R + 1):
            lo, hi = (shifted(src, 0, -i), shifted(src, 0, i)) if axis == 1 else (shifted(src, -i, 0), shifted(src, i, 0))
            ws = A.add(ws, A.mul(int(k[i]), A.add(lo, hi)))
        if sums is not None:
            sums.append(ws)
        return ws >> 16
    return one(one(np.asarray(a, np.int64), 1), 0)


def np_down_smooth(A, a, k, dw, dh):
    """fastakaze::gDownWithSmooth (akazed.cu:3143-3205): taps at source distance 2 and 4, mirrored on the SOURCE extents"""
    a = np.asarray(a, np.int64)
    sh, sw = a.shape
    six = 2 * np.arange(dw)
    cols = [a[:, refl(six + d, sw)] for d in (0, -2, 2, -4, 4)]
    rows = A.add(A.add(A.mul(int(k[0]), cols[0]), A.mul(int(k[1]), A.add(cols[1], cols[2]))), A.mul(int(k[2]), A.add(cols[3], cols[4]))) >> 16
    siy = 2 * np.arange(dh)
    r = [rows[refl(siy + d, sh)] for d in (0, -2, 2, -4, 4)]
    sm = A.add(A.add(A.mul(int(k[0]), r[0]), A.mul(int(k[1]), A.add(r[1], r[2]))), A.mul(int(k[2]), A.add(r[3], r[4]))) >> 16
    return a[siy][:, six], sm


def np_scharr(A, a):
    """(dx, dy, dx*dx + dy*dy) of gScharrContrastNaive / gFlowNaive (akazed.cu:3208-3232, 3406-3428)"""
    a = np.asarray(a, np.int64)
    ul, uc, ur = shifted(a, -1, -1), shifted(a, -1, 0), shifted(a, -1, 1)
    cl, cr = shifted(a, 0, -1), shifted(a, 0, 1)
    ll, lc, lr = shifted(a, 1, -1), shifted(a, 1, 0), shifted(a, 1, 1)
    dx = A.add(A.mul(10, A.sub(cr, cl)), A.mul(3, A.sub(A.sub(A.add(ur, lr), ul), ll)))
    dy = A.add(A.mul(10, A.sub(lc, uc)), A.mul(3, A.sub(A.sub(A.add(ll, lr), ul), ur)))
    return dx, dy, A.add(A.mul(dx, dx), A.mul(dy, dy))


def f2i_sat(v):
    """float -> int as v_cvt_i32_f32: toward zero, saturating, NaN -> 0 (akaze_oracle_fast.c f2i_sat)"""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int64)
    ok = ~np.isnan(v)
    hi, lo = ok & (v >= np.float32(2 ** 31)), ok & (v <= np.float32(-2 ** 31))
    mid = ok & ~hi & ~lo
    out[mid] = np.trunc(v[mid].astype(np.float64)).astype(np.int64)
    out[hi], out[lo] = INT_MAX, INT_MIN
    return out


def np_grad(sumsq):
    """(int)(sqrtf((float)sumsq) + 0.5f) (akazed.cu:3231) of the WRAPPED sum of squares"""
    with np.errstate(invalid="ignore"):
        return f2i_sat(np.sqrt(np.asarray(sumsq, np.int64).astype(np.float32)) + np.float32(0.5))


def lattice_cov(n):
    """the part of an extent that gFindMaxContrastU4's grid covers (akazed.cu:4122)"""
    return min(32 * ((n // 2 + 15) // 16), n)


def np_kcontrast(a, per, nbins=300):
    """gScharrContrastNaive + gFindMaxContrastU4 + gConstrastHistShared + hScharrContrast (akazed.cu:3208-3336, 4098-4165; D2, D3 of
    akaze_oracle_fast.c) -> (kcontrast, hmax, hist, the int64 products grad * hfactor before they are wrapped)"""
    a = np.asarray(a, np.int64)
    h, w = a.shape
    grad = np_grad(np_scharr(Arith(True), a)[2])
    hmax = max(1, int(grad[0:lattice_cov(h):16, 0:lattice_cov(w):16].max()))
    hfactor = int(np.float32(np.float32(nbins) / np.float32(hmax)) * np.float32(65536) + np.float32(0.5))      # :4133
    prod = grad * hfactor
    hi = np.clip(wrap32(prod) >> 16, 0, nbins - 1)                             # :3319-3326, a negative index counted in bin 0
    hist = np.bincount(hi.ravel(), minlength=nbins).astype(np.int64)
    hist[0] += ((w + 31) // 32 * 32 - w) * h + ((h + 15) // 16 * 16 - h) * w    # D3
    thresh = int(np.trunc(np.float32(w * h - int(hist[0])) * np.float32(per)))
    cumuv, k = 0, 1
    while k < nbins and cumuv < thresh:
        cumuv += int(hist[k])
        k += 1
    return k * hmax // nbins, hmax, hist.astype(np.int32), prod


def stepfac_of(tau):
    return int(np.float32(np.float32(np.float32(0.5) * np.float32(tau)) * np.float32(65536)) + np.float32(0.5))     # akazed.cu:4237


def np_nld_step(A, s, f, tau):
    """gNldStepNaive (akazed.cu:3448-3470) -> (L', the int64 product stepfac * step before it is wrapped)"""
    s, f = np.asarray(s, np.int64), np.asarray(f, np.int64)
    acc = None
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        t = A.mul(A.add(f, shifted(f, dy, dx)), A.sub(shifted(s, dy, dx), s))
        acc = t if acc is None else A.add(acc, t)
    step = acc >> 16
    prod = stepfac_of(tau) * step
    return A.add(A.fit(prod) >> 16, s), prod


def np_hessian(A, a, step, fac1, fac2):
    """gDerivate + gHessianDeterminant (akazed.cu:3339-3403) -> (Lx, Ly, det, the int64 products dxx * dyy and dxy * dxy)"""
    def d(p, S):
        ul, uc, ur = shifted(p, -S, -S), shifted(p, -S, 0), shifted(p, -S, S)
        cl, cr = shifted(p, 0, -S), shifted(p, 0, S)
        ll, lc, lr = shifted(p, S, -S), shifted(p, S, 0), shifted(p, S, S)
        gx = A.add(A.mul(fac1, A.sub(A.sub(A.add(ur, lr), ul), ll)), A.mul(fac2, A.sub(cr, cl))) >> 16
        gy = A.add(A.mul(fac1, A.sub(A.sub(A.add(lr, ll), ur), ul)), A.mul(fac2, A.sub(lc, uc))) >> 16
        return gx, gy
    lx, ly = d(np.asarray(a, np.int64), step)
    dxx, dxy = d(lx, step)
    _, dyy = d(ly, step)
    p1, p2 = dxx * dyy, dxy * dxy
    return lx, ly, A.sub(A.fit(p1), A.fit(p2)), p1, p2


# ------------------------------------------------------------------------------------------------ the stage cases both test modules share
OPS = ("lowpass", "down_smooth", "kcontrast", "flow", "smooth_flow", "nld_steps", "nld_steps_batch", "fed_cycle", "level_tile", "hessian")
U8_OPS = ("conv_u8", "base")


def own_kcontrast(okz, a, w):
    """the plane's own contrast factor as the octave-0 prologue forms it: fkz_kcontrast of the sigma = 1 low-pass"""
    return okz.fast_kcontrast(okz.fast_lowpass(a, w, 1.0, 2), w, PER)[0]


def fed_sf_covers(w, h, sw=None, sh=None):
    """the cases k_fed_sf takes (hak_fed_sf_covers / launch_fs_any, PM_G2): 16-byte rows, and even source extents for an octave head"""
    return w % 4 == 0 and w >= 16 and h >= 8 and (sw is None or (sw % 2 == 0 and sh % 2 == 0))


def _short(name, seq, keep):
    """the argument lists of the generators outside COMPLETE are shortened: the first `keep` entries, or the entries at indices `keep`"""
    if name in COMPLETE:
        return list(seq)
    return list(seq)[:keep] if isinstance(keep, int) else [seq[i] for i in keep]


def shapes_of(op):
    """(520, 406) is there for the octave head of fed_cycle alone"""
    return HEAD_SOURCES if op == "fed_cycle" else SHAPES


def stage_cases(okz, name, w, h, ops=None, seed=SEED):
    """every stage case of generator `name` at w x h -> yields (op, label, args, [(output name, oracle output, valid width or None)]).
    args holds the pitched input planes (numpy) and the operator's arguments; tests/test_gpu_fast_stages.py calls hak_op_fast_<op>
    with them.  One oracle evaluation per case, whoever walks the list."""
    want = lambda op: ops is None or op in ops
    gen = GENERATORS[name]
    a = pitched(gen(w, h, seed))
    kc_own = own_kcontrast(okz, a, w)
    kcs = _short(name, [kc_own] + KC_FIXED, (0, 1))
    taus_all = _short(name, TAU_LISTS, (1, 2, 3))
    if want("lowpass"):
        for var, R in _short(name, LOWPASS, 2):
            yield "lowpass", f"var={var},R={R}", dict(a=a, var=var, R=R), [("lowpass", okz.fast_lowpass(a, w, var, R), w)]
    if want("down_smooth"):
        dw, dh = w >> 1, h >> 1
        dp = (dw + 63) // 64 * 64
        dst, dsm = okz.fast_down_smooth(a, w, dw, dh, dp)
        yield "down_smooth", "", dict(a=a, dw=dw, dh=dh, dp=dp), [("down", dst, dw), ("down_smooth", dsm, dw)]
    if want("kcontrast"):
        for label, src in (("raw", a), ("lowpass", okz.fast_lowpass(a, w, 1.0, 2))):
            kc, hmax, hist = okz.fast_kcontrast(src, w, PER)
            yield "kcontrast", label, dict(a=src), [("kcontrast,hmax", np.array([kc, hmax], np.int32), None), ("hist", hist, None)]
    if want("flow") or want("smooth_flow"):
        sm = okz.fast_lowpass(a, w, 1.0, 2)
        for op in ("flow", "smooth_flow"):
            if not want(op):
                continue
            for diff in (0, 1, 2, 3):
                for kc in kcs:
                    if op == "flow":
                        outs = [("flow", okz.fast_flow(a, w, diff, kc), w)]
                    else:
                        outs = [("smooth", sm, w), ("flow", okz.fast_flow(sm, w, diff, kc), w)]
                    yield op, f"diff={diff},kc={kc}", dict(a=a, diff=diff, kc=kc), outs
    if want("nld_steps"):
        g = okz.fast_flow(a, w, 1, kc_own)
        for taus in taus_all:
            yield "nld_steps", f"taus={taus}", dict(a=a, g=g, taus=taus), [("nld", okz.fast_nld_steps(a, g, w, taus), w)]
    if want("nld_steps_batch") or want("fed_cycle") or want("level_tile"):
        planes = [a] + [pitched(gen(w, h, seed + i)) for i in range(1, BATCH)]          # distinct planes
        own = [kc_own] + [own_kcontrast(okz, q, w) for q in planes[1:]]
    if want("nld_steps_batch"):
        gs = [okz.fast_flow(q, w, 1, k) for q, k in zip(planes, own)]
        for taus in taus_all:
            outs = [(f"nld[{i}]", okz.fast_nld_steps(q, g, w, taus), w) for i, (q, g) in enumerate(zip(planes, gs))]
            yield "nld_steps_batch", f"taus={taus}", dict(a=np.stack(planes), g=np.stack(gs), taus=taus), outs
    for op in ("fed_cycle", "level_tile"):
        if not want(op):
            continue
        for head in (0, 1):
            # head: the planes are the SOURCE (Lt(o-1, 0)), the result has half their extents
            dw, dh = (w >> 1, h >> 1) if head else (w, h)
            dp = (dw + 63) // 64 * 64
            if op == "fed_cycle" and not fed_sf_covers(dw, dh, *((w, h) if head else (None, None))):
                continue
            diffs = [PM_G2] if op == "fed_cycle" else _short(name, [0, 1, 2, 3], (1, 3))
            for kcl in _short(name, [own, KC_FIXED], 1):
                for diff in diffs:
                    if head:
                        srcs, sms = zip(*[okz.fast_down_smooth(q, w, dw, dh, dp) for q in planes])
                    else:
                        srcs, sms = planes, [okz.fast_lowpass(q, w, 1.0, 2) for q in planes]
                    gs = [okz.fast_flow(s_, dw, diff, k) for s_, k in zip(sms, kcl)]
                    long_cycle = op == "level_tile" and diff == PM_G2 and kcl is own
                    for taus in taus_all + ([LONG_TAUS] if long_cycle else []):
                        outs = [(f"smooth[{i}]", s_, dw) for i, s_ in enumerate(sms)]
                        outs += [(f"L[{i}]", okz.fast_nld_steps(q, g, dw, taus), dw) for i, (q, g) in enumerate(zip(srcs, gs))]
                        yield op, f"head={head},diff={diff},kc={kcl},taus={taus}", dict(
                            a=np.stack(planes), head=head, dw=dw, dh=dh, dp=dp, diff=diff, kc=list(kcl), taus=taus, g=np.stack(gs)), outs
    if want("hessian"):
        for step in _short(name, HESS_STEPS, (1, 3, 5)):
            lx, ly, det = okz.fast_hessian(a, w, step)
            yield "hessian", f"step={step}", dict(a=a, step=step), [("Lx", lx, w), ("Ly", ly, w), ("det", det, w)]


def u8_stage_cases(okz, name, w, h, ops=None, seed=SEED):
    """the cases of the two operators that read a uint8 image (generators U8_GENERATORS), same tuple layout"""
    want = lambda op: ops is None or op in ops
    u8 = pitched(U8_GENERATORS[name](w, h, seed))
    p = u8.shape[1]
    if want("conv_u8"):
        for var, R in LOWPASS:
            yield "conv_u8", f"var={var},R={R}", dict(u8=u8, var=var, R=R), [("conv", okz.fast_conv_u8(u8, w, p, var, R), w)]
    if want("base"):
        sm = okz.fast_conv_u8(u8, w, p, 1.0, 2)
        kc, hmax, hist = okz.fast_kcontrast(sm, w, PER)
        for var, R in LOWPASS + [BASE_UNFUSED]:
            outs = [("Lt", okz.fast_conv_u8(u8, w, p, var, R), w), ("kcontrast,hmax", np.array([kc, hmax], np.int32), None), ("hist", hist, None)]
            yield "base", f"var={var},R={R}", dict(u8=u8, var=var, R=R), outs

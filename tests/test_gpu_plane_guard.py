"""GPU write contract of the scale-space kernels: a launcher's kernels write the pixels [0, h) x [0, w) of the planes they are given
and nothing else, and no result depends on what lies beside those pixels.

Every stage operator of include/hipakaze_test.h that takes caller planes runs on a guarded arena (tests/plane_guard.py: all planes
of a call in one allocation, 32 guard rows around each, the poison word in the guards, in the pad columns [w, p) of every row -- the
inputs' too -- and in the whole of every output plane).  Each call asserts, with no tolerance:
    the owned pixels equal the oracle's bit for bit (the okz calls of tests/test_gpu_stages.py and tests/fast_domain.py; the oracle is
      given dense planes, so a tap that read the poisoned padding shows as a difference);
    no owned pixel of a plane the operator produces still holds the poison;
    no word outside the owned pixels of those planes changed: pad columns, rows below, the guard in front, the other planes of the
      call (inputs, and planes the call must leave alone: `flow` and `tmp` of a one-launch cycle, the third plane of the prologue),
      the other images' slots.
The last test does the same to a context's whole arena through the real launch sequence.

Shapes come from the kernels' own constants (named beside each list): one lane group of 4 columns short of a stored strip, exactly
one strip, one group over, two strips plus a four-column edge strip; for operators that take any width also w % 4 = 1, 2, 3 (85, 86,
83); heights 21 and 37 (several row segments with a short last one, both y reflections) and each streaming kernel's cover minimum at
w = 16; pitches align4(w) (p == w when w % 4 == 0: a store past column w lands in the next row), that plus 4, and align64(w); one
image and three where a batch form exists.  Width x pitch is crossed fully at h = 21; height 37, three images and the minimum appear
once per kernel.  The kernel a case is meant for is forced as tests/test_gpu_strip_seams.py does and the reported route asserted."""
import ctypes as C

import numpy as np
import pytest

import plane_guard as pg

pytestmark = pytest.mark.gpu
_fp = C.POINTER(C.c_float)
f32, i32 = np.float32, np.int32
PM_G2 = 1
PER = 0.7

ANY_WIDTH = [85, 86, 83]                                    # w % 4 = 1, 2, 3
TILE_64 = [60, 64, 68, 132]                                 # TILE_X, SF_TX, BS_TX, HF_TX = 64 columns per block of the tile kernels
STRIP_248 = [244, 248, 252, 500]                            # fed_xv(1..4), BS_XV, k_hessian_stream at S = 1: 256 - 2 * 4 stored columns
STRIP_240 = [236, 240, 244, 484]                            # k_hessian_stream at S = 2..4, k_fed_sf at 1..4 steps (fs_hx = 8): 256 - 16
STRIP_112 = [108, 112, 116, 228]                            # fed_xv(5..8): 128 - 2 * 8
STRIP_108_104 = [100, 104, 108, 112, 212, 220]              # k_fed_sf<6 | 7>: 108 columns (halo 10) where that saves a strip (108, 212),
                                                            # else 104 (halo 12), fs_hx_for; k_fed_sf<8>: 104
LEVEL_16 = [12, 16, 20, 36]                                 # k_level_tile: tiles shrink to T = 16 while a launch has fewer than 96 blocks
H_SHORT, H_TALL = 21, 37


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def shapes(widths, batch=False, cover_min=None):
    """(w, h, p, nimg): widths x pitches at the short height and one image; the tall height (three images where a batch form exists)
    at the first and the last width; the kernel's cover minimum at w = 16"""
    out = [(w, H_SHORT, p, 1) for w in widths for p in pg.pitches(w)]
    out += [(widths[0], H_TALL, pg.pitches(widths[0])[0], 3 if batch else 1), (widths[-1], H_TALL, pg.pitches(widths[-1])[1], 3 if batch else 1)]
    if cover_min:
        out += [(16, cover_min, 16, 1), (16, cover_min, 20, 3 if batch else 1)]
    return out


# ------------------------------------------------------------------------------------------------ element types
class Float:
    name, dtype = "float", f32
    kc = [0.37, 0.05, 0.41]

    @staticmethod
    def content(seed, n, h, w):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w].astype(f32)
        return np.stack([(0.5 + 0.4 * np.sin(xx * (0.05 + 0.02 * i) + yy * 0.03) + rng.uniform(-0.1, 0.1, (h, w))).astype(f32) for i in range(n)])

    @staticmethod
    def conductivity(seed, n, h, w):
        return np.random.default_rng(seed).uniform(0.01, 1.0, (n, h, w)).astype(f32)

    def __init__(self, okz, lib):
        self.lowpass, self.down_smooth, self.flow, self.nld_steps, self.hessian = okz.lowpass, okz.down_smooth, okz.flow, okz.nld_steps, okz.hessian
        self.op = lambda name: getattr(lib, "hak_op_" + name)
        self.kc_c = lambda v: C.c_float(v)
        self.kc_array = lambda v: (C.c_float * len(v))(*v)


class Int:
    name, dtype = "int", i32
    kc = [2100, 300, 46340]

    @staticmethod
    def content(seed, n, h, w):
        """16.16 values of an 8-bit image with texture"""
        return (Float.content(seed, n, h, w).astype(np.float64) * 255 * 65536).astype(i32)

    @staticmethod
    def conductivity(seed, n, h, w):
        return np.random.default_rng(seed).integers(600, 65537, (n, h, w)).astype(i32)

    def __init__(self, okz, lib):
        self.lowpass, self.down_smooth, self.flow, self.nld_steps, self.hessian = (okz.fast_lowpass, okz.fast_down_smooth, okz.fast_flow,
                                                                                   okz.fast_nld_steps, okz.fast_hessian)
        self.op = lambda name: getattr(lib, "hak_op_fast_" + name)
        self.kc_c = lambda v: C.c_int(v)
        self.kc_array = lambda v: (C.c_int * len(v))(*v)


KINDS = {"float": Float, "int": Int}


def kind_of(name, okz, ah):
    return KINDS[name](okz, ah.lib)


def per_image(fn, *stacks):
    """an oracle stage function on every image of the stacks -> stacked result(s)"""
    outs = [fn(*(np.ascontiguousarray(s[i]) for s in stacks)) for i in range(len(stacks[0]))]
    if isinstance(outs[0], tuple):
        return tuple(np.stack([o[k] for o in outs]) for k in range(len(outs[0])))
    return np.stack(outs)


def interleaved(lx, ly):
    out = np.empty(lx.shape[:-1] + (2 * lx.shape[-1],), lx.dtype)
    out[..., 0::2], out[..., 1::2] = lx, ly
    return out


def taus_of(n):
    """n distinct step sizes, one of them far beyond the stability limit (as the long FED cycles have)"""
    t = np.array([0.07 + 0.05 * ((3 * i) % 7) for i in range(n)], f32)
    t[n // 2] = 5.0 if n > 2 else t[n // 2]
    return t


# ------------------------------------------------------------------------------------------------ one guarded call
class Run:
    """uploads the arena, hands plane addresses to `call`, downloads, and collects what the three assertions find"""

    def __init__(self, torch, ah):
        self.torch, self.ah, self.fails, self.calls = torch, ah, [], 0

    def __call__(self, what, arena, call, want, images=None):
        d = self.torch.from_numpy(arena.buffer().view(i32)).cuda()
        base = d.data_ptr()
        call(lambda name, img=0: arena.address(base, name, img))
        after = d.cpu().numpy().view(arena.dtype)
        self.calls += 1
        for name, ref in want.items():
            left = arena.unwritten(after, name, images)
            if left:
                self.fails.append(f"{what}: {len(left)} owned pixels of {name!r} never written, first (image, row, col) {left[:3]}")
            if ref is None:
                continue
            got = arena.owned(after, name).view(np.uint32)
            ref = np.ascontiguousarray(ref).reshape(got.shape).view(np.uint32)
            bad = np.argwhere(got != ref)
            if bad.size:
                first = tuple(int(v) for v in bad[0])
                self.fails.append(f"{what}: {name!r} differs from the oracle at {len(bad)} pixels, first (image, row, col) {first}: "
                                  f"{int(got[first]):#010x} != {int(ref[first]):#010x}")
        rep = arena.violations(after, list(want), images)
        if rep.count:
            self.fails.append(f"{what}: {rep}")
        return after

    def done(self, least=1):
        print(f"{self.calls} guarded calls, {len(self.fails)} findings")
        assert self.calls >= least
        assert not self.fails, "\n".join(self.fails[:16] + ([f"... {len(self.fails)} findings"] if len(self.fails) > 16 else []))


# ------------------------------------------------------------------------------------------------ the harness itself, on the device
@pytest.mark.parametrize("kind", list(KINDS))
def test_harness_reports_every_class_from_the_device(torch, kind):
    """no kernel is altered: one word of every class is changed with a torch index assignment in the uploaded buffer"""
    w, h, p = 20, 7, 24
    a = pg.Arena(KINDS[kind].dtype, [("src", w, h, p), ("dxy", w, h, p, 2), ("det", w, h, p), ("tmp", w, h, p)], nimg=3)
    a.put("src", KINDS[kind].content(1, 3, h, w))
    clean = a.buffer()
    a.owned(clean, "dxy")[:2] = 3
    a.owned(clean, "det")[:2] = 4
    d = torch.from_numpy(clean.view(i32)).cuda()
    assert a.violations(d.cpu().numpy().view(a.dtype), ["dxy", "det"], images=[0, 1]).count == 0
    s = a.stride
    plant = {pg.PAD: s + a.offset("det") + 3 * p + w, pg.BELOW: s + a.offset("det") + h * p + 1, pg.FRONT: s + a.offset("src") - 2,
             pg.OTHER_PLANE: s + a.offset("tmp") + 2 * p + 1, pg.OTHER_IMAGE: 2 * s + a.offset("det") + 5}
    where = {pg.PAD: ("det", 1, 3, w), pg.BELOW: ("det", 1, h, 1), pg.FRONT: ("src", 1, -1, p - 2), pg.OTHER_PLANE: ("tmp", 1, 2, 1),
             pg.OTHER_IMAGE: ("det", 2, 0, 5)}
    for cls, k in plant.items():
        e = d.clone()
        e[k] = 12345
        rep = a.violations(e.cpu().numpy().view(a.dtype), ["dxy", "det"], images=[0, 1])
        assert rep.count == 1 and rep.classes == {cls: 1}, (cls, str(rep))
        assert (rep[0].plane, rep[0].image, rep[0].row, rep[0].col) == where[cls] and rep[0].got == 12345, (cls, rep[0])
    e = d.clone()
    e[s + a.offset("det") + 2 * p + 4] = int(np.array([a.poison]).view(i32)[0])
    assert a.unwritten(e.cpu().numpy().view(a.dtype), "det", images=[0, 1]) == [(1, 2, 4)]
    for k in plant.values():
        d[k] = 777
    rep = a.violations(d.cpu().numpy().view(a.dtype), ["dxy", "det"], images=[0, 1])
    assert rep.count == 5 and rep.classes == {c: 1 for c in pg.CLASSES}


# ------------------------------------------------------------------------------------------------ tile kernels of any width
@pytest.mark.parametrize("kind", list(KINDS))
def test_lowpass(ah, okz, torch, kind):
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for w, h, p, _ in shapes(TILE_64 + ANY_WIDTH):                         # TILE_X = 64, TILE_Y = 16 (kernels_scalespace.hip)
        src = K.content(w + h, 1, h, w)
        for var, R in ((1.0, 2), (3.2, 5)):
            a = pg.Arena(K.dtype, [("src", w, h, p), ("dst", w, h, p)]).put("src", src)
            run(f"lowpass {kind} {w}x{h} p={p} R={R}", a, lambda at: ah.check(K.op("lowpass")(at("src"), at("dst"), w, h, p, var, R)),
                {"dst": per_image(lambda s: K.lowpass(s, w, var, R), src)})
    run.done()


def test_fast_conv_u8(ah, okz, torch):
    run = Run(torch, ah)
    for w, h, p, _ in shapes(TILE_64 + ANY_WIDTH):
        u8 = np.random.default_rng(w).integers(0, 256, (h, w)).astype(np.uint8)
        sp = pg.align4(w + 1)                                               # at least one pad column, poisoned
        d_u8 = torch.from_numpy(pg.padded_u8(u8, sp)).cuda()
        for var, R in ((1.0, 2), (2.56, 4), (3.2, 5)):
            a = pg.Arena(i32, [("dst", w, h, p)])
            run(f"conv_u8 {w}x{h} p={p} R={R}", a, lambda at: ah.check(ah.lib.hak_op_fast_conv_u8(d_u8.data_ptr(), sp, at("dst"), w, h, p, var, R)),
                {"dst": okz.fast_conv_u8(u8, w, w, var, R)})
    run.done()


@pytest.mark.parametrize("kind", list(KINDS))
def test_down_smooth(ah, okz, torch, kind):
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for dw, dh, dp, _ in shapes(TILE_64 + ANY_WIDTH):                       # TILE_X = 64 destination columns per block
        first = dp == pg.pitches(dw)[0]
        for odd in ((0, 1) if first else (0,)):                             # even source extents, and odd ones (the last column / row is dropped)
            sw, sh = 2 * dw + odd, 2 * dh + odd
            sp = pg.pitches(sw)[0 if first else -1]
            src = K.content(sw + sh, 1, sh, sw)
            a = pg.Arena(K.dtype, [("src", sw, sh, sp), ("dst", dw, dh, dp), ("smooth", dw, dh, dp)]).put("src", src)
            dst, sm = K.down_smooth(np.ascontiguousarray(src[0]), sw, dw, dh, dw)
            run(f"down_smooth {kind} {sw}x{sh} p={sp} -> {dw}x{dh} p={dp}", a,
                lambda at: ah.check(K.op("down_smooth")(at("src"), at("dst"), at("smooth"), sw, sh, sp, dw, dh, dp)), {"dst": dst, "smooth": sm})
    run.done()


@pytest.mark.parametrize("kind", list(KINDS))
def test_flow(ah, okz, torch, kind):
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for n, (w, h, p, _) in enumerate(shapes(TILE_64 + ANY_WIDTH)):
        src = K.content(w + h, 1, h, w)
        for diff in ((0, 1, 2, 3) if n == 0 else (n % 4,)):
            a = pg.Arena(K.dtype, [("src", w, h, p), ("dst", w, h, p)]).put("src", src)
            run(f"flow {kind} {w}x{h} p={p} diffusivity {diff}", a,
                lambda at: ah.check(K.op("flow")(at("src"), at("dst"), w, h, p, diff, K.kc_c(K.kc[0]))),
                {"dst": per_image(lambda s: K.flow(s, w, diff, K.kc[0]), src)})
    run.done()


@pytest.mark.parametrize("kind", list(KINDS))
def test_smooth_flow(ah, okz, torch, kind):
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for n, (w, h, p, _) in enumerate(shapes(TILE_64 + ANY_WIDTH)):         # SF_TX = 64, SF_TY = 32 (kernels_smoothflow.hip)
        src = K.content(w + h, 1, h, w)
        sm = per_image(lambda s: K.lowpass(s, w, 1.0, 2), src)
        for diff in ((0, 1, 2, 3) if n == 0 else (n % 4,)):
            a = pg.Arena(K.dtype, [("src", w, h, p), ("smooth", w, h, p), ("flow", w, h, p)]).put("src", src)
            run(f"smooth_flow {kind} {w}x{h} p={p} diffusivity {diff}", a,
                lambda at: ah.check(K.op("smooth_flow")(at("src"), at("smooth"), at("flow"), w, h, p, diff, K.kc_c(K.kc[2]))),
                {"smooth": sm, "flow": per_image(lambda s: K.flow(s, w, diff, K.kc[2]), sm)})
    run.done()


# ------------------------------------------------------------------------------------------------ FED steps
# launches of a cycle of n steps and the steps behind the launch that lands in `tmp` (0: tmp is not to be touched).  float: groups of
# at most 4 steps on 4-px lanes unless deeper groups (up to 8, 2-px lanes) need fewer launches; int: at most 4; a width that is no
# multiple of 4 takes one step per launch (hak_fed_groups, kernels_fed.hip) -- stated here as data, per case
FED_CASES = {
    #         n: (widths, launches, steps in tmp)
    "float": {1: (ANY_WIDTH + [250], 1, 0),                 # k_fed_generic: strips of 248 columns, any width
              4: (STRIP_248, 1, 0),                         # k_fed_multi<4>, 4-px lanes
              6: (STRIP_112, 1, 0), 7: (STRIP_112, 1, 0), 8: (STRIP_112, 1, 0),      # k_fed_multi<6 | 7 | 8>, 2-px lanes
              12: (STRIP_112, 2, 6)},                       # 6 + 6: the first launch lands in tmp
    "int": {1: (ANY_WIDTH + [250], 1, 0),                   # kf_nld_step: 64 x 16 tiles
            4: (STRIP_248, 1, 0),
            6: (STRIP_248, 2, 3), 7: (STRIP_248, 2, 4), 8: (STRIP_248, 2, 4),        # 3 + 3, 4 + 3, 4 + 4
            12: (STRIP_248, 3, 8)},                         # 4 + 4 + 4: dst, tmp, dst
}


@pytest.mark.parametrize("n", [1, 4, 6, 7, 8, 12])
@pytest.mark.parametrize("kind", list(KINDS))
def test_nld_steps(ah, okz, torch, kind, n):
    """hak_op_nld_steps on one image, hak_op_nld_steps_batch on three"""
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    widths, launches, in_tmp = FED_CASES[kind][n]
    tau = taus_of(n)
    tp = tau.ctypes.data_as(_fp)
    for w, h, p, nimg in shapes(widths, batch=True, cover_min=8):
        src, g = K.content(w + h, nimg, h, w), K.conductivity(w + h + 1, nimg, h, w)
        a = pg.Arena(K.dtype, [("src", w, h, p), ("flow", w, h, p), ("dst", w, h, p), ("tmp", w, h, p)], nimg).put("src", src).put("flow", g)
        want = {"dst": per_image(lambda s, f: K.nld_steps(s, f, w, tau), src, g)}
        if launches > 1:
            want["tmp"] = per_image(lambda s, f: K.nld_steps(s, f, w, tau[:in_tmp]), src, g)
        if nimg == 1:
            call = lambda at: ah.check(K.op("nld_steps")(at("src"), at("flow"), at("dst"), at("tmp"), w, h, p, tp, n))
        else:
            call = lambda at: ah.check(K.op("nld_steps_batch")(at("src"), at("flow"), at("dst"), at("tmp"), a.stride, w, h, p, nimg, tp, n))
        run(f"nld_steps {kind} n={n} {w}x{h} p={p} images {nimg}", a, call, want)
    run.done()


def test_nld_steps_one_step_per_launch(ah, okz, torch, monkeypatch):
    """HAK_FED_MAX_FUSE = 1: k_fed_multi<1> on 4-px lanes, four launches alternating between tmp and dst"""
    monkeypatch.setenv("HAK_FED_MAX_FUSE", "1")
    for kind in KINDS:
        K, run = kind_of(kind, okz, ah), Run(torch, ah)
        tau = taus_of(4)
        for w, h, p, nimg in shapes(STRIP_248[:2], batch=True):
            src, g = K.content(w + h, nimg, h, w), K.conductivity(w + h + 1, nimg, h, w)
            a = pg.Arena(K.dtype, [("src", w, h, p), ("flow", w, h, p), ("dst", w, h, p), ("tmp", w, h, p)], nimg).put("src", src).put("flow", g)
            want = {"dst": per_image(lambda s, f: K.nld_steps(s, f, w, tau), src, g),
                    "tmp": per_image(lambda s, f: K.nld_steps(s, f, w, tau[:3]), src, g)}
            run(f"nld_steps {kind} 4 x 1 step {w}x{h} p={p} images {nimg}", a,
                lambda at: ah.check(K.op("nld_steps_batch")(at("src"), at("flow"), at("dst"), at("tmp"), a.stride, w, h, p, nimg,
                                                            tau.ctypes.data_as(_fp), 4)), want)
        run.done()


# k_fed_sf: low-pass + conductivity + the first group of steps in one launch; (widths, launches, steps in tmp)
CYCLE_CASES = {
    "float": {4: (STRIP_240, 1, 0),                         # k_fed_sf<4>: 4-px lanes, x halo 8
              6: (STRIP_108_104, 1, 0), 7: (STRIP_108_104, 1, 0),
              8: ([100, 104, 108, 212], 1, 0),              # k_fed_sf<8>: 104 columns
              12: (STRIP_108_104, 2, 6)},                   # k_fed_sf<6> stores the conductivity, k_fed_multi<6> reads it
    "int": {4: (STRIP_240, 1, 0), 7: (STRIP_240, 2, 4)},    # k_fed_sf<4> + k_fed_multi<3>
}


@pytest.mark.parametrize("head", [0, 1], ids=["plain", "head"])
@pytest.mark.parametrize("kind,n", [(k, n) for k in CYCLE_CASES for n in CYCLE_CASES[k]])
def test_fed_cycle(ah, okz, torch, monkeypatch, kind, n, head):
    monkeypatch.setenv("HAK_FUSE_SF", "2")
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    widths, launches, in_tmp = CYCLE_CASES[kind][n]
    tau = taus_of(n)
    for w, h, p, nimg in shapes(widths, batch=True, cover_min=8):          # h = 8: launch_fs_any's minimum
        sw, sh = (2 * w, 2 * h) if head else (w, h)
        sp = pg.pitches(sw)[pg.pitches(w).index(p) % len(pg.pitches(sw))] if head else p
        src = K.content(w + h, nimg, sh, sw)
        if head:
            L0, sm = per_image(lambda s: K.down_smooth(s, sw, w, h, w), src)
        else:
            L0, sm = src, per_image(lambda s: K.lowpass(s, w, 1.0, 2), src)
        g = np.stack([K.flow(np.ascontiguousarray(sm[i]), w, PM_G2, K.kc[i]) for i in range(nimg)])
        a = pg.Arena(K.dtype, [("src", sw, sh, sp), ("smooth", w, h, p), ("flow", w, h, p), ("dst", w, h, p), ("tmp", w, h, p)], nimg).put("src", src)
        want = {"smooth": sm, "dst": per_image(lambda s, f: K.nld_steps(s, f, w, tau), L0, g)}
        if launches > 1:                                                    # a later launch reads the conductivity: stored then, and only then
            want["flow"] = g
            want["tmp"] = per_image(lambda s, f: K.nld_steps(s, f, w, tau[:in_tmp]), L0, g)
        run(f"fed_cycle {kind} n={n} head={head} {w}x{h} p={p} images {nimg}", a,
            lambda at: ah.check(K.op("fed_cycle")(at("src"), head, sw, sh, sp, at("smooth"), at("flow"), at("dst"), at("tmp"), a.stride, w, h, p,
                                                  nimg, K.kc_array(K.kc[:nimg]), tau.ctypes.data_as(_fp), n)), want)
    run.done()


@pytest.mark.parametrize("head", [0, 1], ids=["plain", "head"])
def test_fast_level_tile(ah, okz, torch, head):
    K, run = kind_of("int", okz, ah), Run(torch, ah)
    for n in (3, 9):
        tau = taus_of(n)
        for w, h, p, nimg in shapes(LEVEL_16 + TILE_64[:3] + ANY_WIDTH, batch=True):
            if n == 9 and p != pg.pitches(w)[0]:
                continue
            sw, sh = (2 * w, 2 * h) if head else (w, h)
            sp = pg.pitches(sw)[0] if head else p
            diff = (w + n) % 4
            src = K.content(w + h, nimg, sh, sw)
            if head:
                L0, sm = per_image(lambda s: K.down_smooth(s, sw, w, h, w), src)
            else:
                L0, sm = src, per_image(lambda s: K.lowpass(s, w, 1.0, 2), src)
            g = np.stack([K.flow(np.ascontiguousarray(sm[i]), w, diff, K.kc[i]) for i in range(nimg)])
            a = pg.Arena(i32, [("src", sw, sh, sp), ("smooth", w, h, p), ("dst", w, h, p), ("tmp", w, h, p)], nimg).put("src", src)
            nl = C.c_int()
            run(f"level_tile n={n} head={head} {w}x{h} p={p} images {nimg} diffusivity {diff}", a,
                lambda at: ah.check(ah.lib.hak_op_fast_level_tile(at("src"), head, sw, sh, sp, at("smooth"), at("dst"), at("tmp"), a.stride, w, h, p,
                                                                  nimg, diff, K.kc_array(K.kc[:nimg]), tau.ctypes.data_as(_fp), n, C.byref(nl))),
                {"smooth": sm, "dst": per_image(lambda s, f: K.nld_steps(s, f, w, tau), L0, g)})
            assert nl.value == 1                                            # one launch up to LV_MAX_STEPS = 36 steps: tmp is not to be touched
    run.done()


# ------------------------------------------------------------------------------------------------ Hessian
def hessian_case(ah, okz, torch, run, K, w, h, p, nimg, step, route_want):
    src = K.content(w + h + step, nimg, h, w)
    a = pg.Arena(K.dtype, [("dxy", w, h, p, 2), ("det", w, h, p), ("src", w, h, p)], nimg).put("src", src)
    lx, ly, det = per_image(lambda s: K.hessian(s, w, step), src)
    route = C.c_int()
    run(f"hessian_planes {K.name} S={step} {w}x{h} p={p} images {nimg}", a,
        lambda at: ah.check(K.op("hessian_planes")(at("src"), at("dxy"), at("det"), a.stride, w, h, p, nimg, step, C.byref(route))),
        {"dxy": interleaved(lx, ly), "det": det})
    assert route.value == route_want, (w, h, step, route.value)


@pytest.mark.parametrize("step", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", list(KINDS))
def test_hessian_streaming(ah, okz, torch, monkeypatch, kind, step):
    monkeypatch.setenv("HAK_HESS_STREAM", "2")
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for w, h, p, nimg in shapes(STRIP_248 if step == 1 else STRIP_240, batch=True, cover_min=2 * step + 2):    # hak_hessian_stream_covers
        hessian_case(ah, okz, torch, run, K, w, h, p, nimg, step, 1)
    run.done()


@pytest.mark.parametrize("step", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("kind", list(KINDS))
def test_hessian_tile_and_unfused(ah, okz, torch, monkeypatch, kind, step):
    """k_hessian_fused<S> (HF_TX = 64, TY = 32 or 28 rows) up to dilation 4, k_derivate + k_hessian (64 x 16) at 6"""
    monkeypatch.setenv("HAK_HESS_STREAM", "0")
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    for w, h, p, nimg in shapes(TILE_64 + ANY_WIDTH, batch=True):
        hessian_case(ah, okz, torch, run, K, w, h, p, nimg, step, 3 if step == 6 else 2)
    run.done()


@pytest.mark.parametrize("kind", list(KINDS))
def test_hessian_into_three_planes(ah, okz, torch, monkeypatch, kind):
    """hak_op_hessian / hak_op_fast_hessian and their batch forms: the caller's dense Lx, Ly and determinant planes (k_deinterleave and
    the copy out of the operator's own allocation).  The batch forms take images h * p elements apart: to the arena a batch of three is
    one plane of 3 h rows"""
    monkeypatch.setenv("HAK_HESS_STREAM", "2")
    K, run = kind_of(kind, okz, ah), Run(torch, ah)
    step = 2
    for w, h, p, nimg in shapes([252, 256, 260, 516] + ANY_WIDTH, batch=True):      # k_deinterleave: 256 columns per block
        src = K.content(w + h, nimg, h, w)
        a = pg.Arena(K.dtype, [(n, w, nimg * h, p) for n in ("src", "lx", "ly", "det")]).put("src", src.reshape(nimg * h, w))
        lx, ly, det = per_image(lambda s: K.hessian(s, w, step), src)
        route = C.c_int()
        if nimg > 1:
            call = lambda at: ah.check(K.op("hessian_batch")(at("src"), at("lx"), at("ly"), at("det"), w, h, p, nimg, step, C.byref(route)))
        elif kind == "float":
            call = lambda at: ah.check(ah.lib.hak_op_hessian(at("src"), at("lx"), at("ly"), at("det"), w, h, p, step))
        else:
            call = lambda at: ah.check(ah.lib.hak_op_fast_hessian(at("src"), at("lx"), at("ly"), at("det"), w, h, p, step, C.byref(route)))
        run(f"hessian {kind} {w}x{h} p={p} images {nimg}", a, call, {"lx": lx, "ly": ly, "det": det})
        assert (kind == "float" and nimg == 1) or route.value == (1 if w % 4 == 0 else 2), (w, route.value)
    run.done()


# ------------------------------------------------------------------------------------------------ FAST octave-0 prologue
@pytest.mark.parametrize("route", [1, 2, 3], ids=["k_base_stream", "kf_base", "unfused"])
def test_fast_base(ah, okz, torch, monkeypatch, route):
    monkeypatch.setenv("HAK_BASE_STREAM", "2" if route == 1 else "0")
    run = Run(torch, ah)
    # k_base_stream: BS_XV = 248 stored columns, w % 4 == 0, at least 16 x 16; kf_base / the three launches: BS_TX = TILE_X = 64, any width
    cases = shapes(STRIP_248, cover_min=16) if route == 1 else shapes(TILE_64 + ANY_WIDTH)
    for var, R in {1: [(2.56, 4), (1.0, 2)], 2: [(2.56, 4), (3.2, 5)], 3: [(0.3, 1)]}[route]:
        for w, h, p, _ in cases:
            u8 = np.random.default_rng(w + h).integers(0, 256, (h, w)).astype(np.uint8)
            sp = pg.align4(w + 1)
            d_u8 = torch.from_numpy(pg.padded_u8(u8, sp)).cuda()
            sm = okz.fast_conv_u8(u8, w, w, 1.0, 2)
            kc_want, hmax_want, hist_want = okz.fast_kcontrast(sm, w, PER)
            a = pg.Arena(i32, [("lt", w, h, p), ("grad", w, h, p), ("smooth", w, h, p)])
            kc, hmax, rt = C.c_int(), C.c_int(), C.c_int()
            hist = np.zeros(300, i32)
            want = {"lt": okz.fast_conv_u8(u8, w, w, var, R)}
            want.update({"smooth": sm} if route == 3 else {"grad": None})   # (the gradient magnitude has no stage function in the oracle:
            what = f"fast_base route {route} {w}x{h} p={p} R={R}"          #  every pixel written, and the histogram made of it below)
            run(what, a, lambda at: ah.check(ah.lib.hak_op_fast_base_planes(
                d_u8.data_ptr(), sp, at("lt"), at("grad"), at("smooth"), w, h, p, var, R, PER, C.byref(kc), C.byref(hmax),
                hist.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rt))), want)
            assert rt.value == route, (what, rt.value)
            # hak_op_fast_base: the same on an allocation of its own, Lt copied out to the caller's plane
            b = pg.Arena(i32, [("lt", w, h, p)])
            run(what + " (Lt copied out)", b, lambda at: ah.check(ah.lib.hak_op_fast_base(
                d_u8.data_ptr(), sp, at("lt"), w, h, p, var, R, PER, C.byref(kc), C.byref(hmax), hist.ctypes.data_as(C.POINTER(C.c_int)),
                C.byref(rt))), {"lt": want["lt"]})
            assert rt.value == route, (what, rt.value)
            if (kc.value, hmax.value) != (kc_want, hmax_want) or not np.array_equal(hist, hist_want):
                run.fails.append(f"{what}: contrast factor, maximum or histogram differ: {(kc.value, hmax.value)} != {(kc_want, hmax_want)}")
    run.done()


# ------------------------------------------------------------------------------------------------ the whole launch sequence
TILE_KNOBS = {"HAK_HESS_STREAM": "0", "HAK_FUSE_SF": "0", "HAK_BASE_STREAM": "0"}
# 640 x 336, 3 octaves: p == w at octaves 0 and 1, 160 -> pitch 192 at octave 2; 324 x 168, 2 octaves: octave 1 is 162 wide, w % 4 == 2
CONTEXTS = {"640x336": (640, 336, 3), "324x168": (324, 168, 2)}
PIPE_BATCH, PIPE_MAX_PTS = 3, 3000
_pipe_ref = {}


def pipe_images(w, h):
    from akaze_hip import synth
    return [synth.scene(w, h, 300 + i, nshapes=60) for i in range(PIPE_BATCH)]


def pipe_oracle(okz, synth, fast, w, h, noct):
    key = (fast, w, h)
    if key not in _pipe_ref:
        prm = okz.default_params(noctaves=noct)
        imgs = pipe_images(w, h)
        p = (w + 127) // 128 * 128
        _pipe_ref[key] = [okz.fast_detect_and_compute(u, prm, max_pts=PIPE_MAX_PTS).points if fast else
                          okz.detect_and_compute(synth.to_float(u, p), w, prm, max_pts=PIPE_MAX_PTS).points for u in imgs]
    return _pipe_ref[key]


def pad_mask(layout):
    """True at every pad column of every plane of one image's arena, from the layout as the library reports it"""
    m = np.zeros(layout["elements"], bool)
    for o in layout["octaves"]:
        w, h, p = o["w"], o["h"], o["p"]
        for off in o["lt"] + [o["smooth"], o["flow"], o["tmp"]]:
            m[off:off + h * p].reshape(h, p)[:, w:] = True
        for off in o["dxy"]:
            m[off:off + 2 * h * p].reshape(h, 2 * p)[:, 2 * w:] = True
    return m


@pytest.mark.parametrize("knobs", [{}, TILE_KNOBS], ids=["default", "tile"])
@pytest.mark.parametrize("fast", [False, True], ids=["float", "fast"])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_pipeline_leaves_the_padding_alone(ah, okz, torch, monkeypatch, ctx, fast, knobs):
    """detect-and-compute on a batch of three, twice (the second call replays the captured sequence), on a context whose every pad
    column is poisoned: results equal an unpoisoned twin's and the oracle's byte for byte, and no pad word has changed"""
    from akaze_hip import synth
    from conftest import assert_points_equal
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)                                            # (before hak_create: a context reads the knobs once)
    w, h, noct = CONTEXTS[ctx]
    p = ah.iAlignUp(w, 128)
    imgs = pipe_images(w, h)
    if fast:
        stack = np.zeros((PIPE_BATCH, h, p), np.uint8)
        stack[:, :, :w] = np.stack(imgs)
    else:
        stack = np.stack([synth.to_float(u, p) for u in imgs])
    d_img = torch.from_numpy(stack).cuda()
    entry = ah.lib.hak_fast_detect_and_compute_batch if fast else ah.lib.hak_detect_and_compute_batch
    word = np.uint32(pg.POISON_I32 if fast else pg.POISON_F32_BITS)

    def detect(det):
        d_pts = torch.zeros(PIPE_BATCH * PIPE_MAX_PTS * 104, dtype=torch.uint8, device="cuda")
        d_num = torch.zeros(PIPE_BATCH, dtype=torch.int32, device="cuda")
        ah.check(entry(det.ctx, d_img.data_ptr(), h * p, p, PIPE_BATCH, d_pts.data_ptr(), d_num.data_ptr(), 1))
        ah.check(ah.lib.hak_sync(det.ctx))
        nums = d_num.cpu().numpy()
        allp = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(PIPE_BATCH, PIPE_MAX_PTS)
        return [allp[i, :nums[i]].copy() for i in range(PIPE_BATCH)]

    twin, det = ah.Akazer(), ah.Akazer()
    try:
        for d in (twin, det):
            d.init((w, h, p), noctaves=noct, max_pts=PIPE_MAX_PTS, batch=PIPE_BATCH)
        layout = det.arena_layout()
        assert len(layout["octaves"]) == noct and layout["batch"] == PIPE_BATCH
        assert [(o["w"], o["p"] == o["w"]) for o in layout["octaves"]] == {"640x336": [(640, True), (320, True), (160, False)],
                                                                          "324x168": [(324, False), (162, False)]}[ctx]
        mask = pad_mask(layout)
        assert mask.any()
        for i in range(PIPE_BATCH):
            words = det.arena_read(i)
            words[mask] = word
            det.arena_write(words, i)
        plain = detect(twin)
        results = [detect(det), detect(det)]
        want = pipe_oracle(okz, synth, fast, w, h, noct)
        for i in range(PIPE_BATCH):
            assert len(want[i]) > 20
            for got in results:
                assert got[i].tobytes() == plain[i].tobytes(), f"image {i}: the poisoned context's records differ from its twin's"
                assert_points_equal(got[i], want[i])
        for i in range(PIPE_BATCH):
            words = det.arena_read(i)
            changed = np.nonzero(mask & (words != word))[0]
            assert changed.size == 0, (f"image {i}: {changed.size} pad words written, first at arena elements {changed[:4].tolist()}: "
                                       f"{[hex(int(v)) for v in words[changed[:4]]]}")
    finally:
        twin.close()
        det.close()

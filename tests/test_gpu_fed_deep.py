"""GPU parity of the deep FED groups (5..8 steps per launch on 2-px lanes, kernels_fed.hip / kernels_fedsf.hip): k_fed_multi and
k_fed_sf (sublevel and decimating octave-head form) against the CPU oracle's stage functions, bit for bit, on batches of three
different images; one run through the whole batch pipeline; and the launch count hak_query_traffic reports.

Shapes: the smallest at which these kernels can go wrong.  Widths (all % 4 == 0): one strip holding both image borders (64); the
stored width of one 2-px strip and that width + 4 -- the strip seam and an edge strip of four columns -- for each strip geometry
(k_fed_multi and k_fed_sf<5>: 128 - 2 * 8 = 112; k_fed_sf<6..8>: 128 - 2 * 12 = 104); three strips (352).  Heights: 9 (shorter
than the warm-up rows of an 8-step group), 33, and 135 (octave 3 of 1080p: a full row segment per wave).  Step counts 5..9, 16
and 23 with the FED schedule's own tau arrays: one deep group; two groups of which one is a 4-px group (9 = 5 + 4); 8 + 8;
8 + 8 + 7."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_points_equal

pytestmark = pytest.mark.gpu

WIDTHS = [64, 104, 108, 112, 116, 352]
HEIGHTS = [9, 33, 135]
STEPS = [5, 6, 7, 8, 9, 16, 23]
NIMG = 3
KCONTRAST = np.array([0.37, 0.05, 0.41], np.float32)
PM_G2 = 1           # akaze_structures.h:53-59 (the only diffusivity k_fed_sf covers)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def taus(okz):
    """tau arrays of FED cycles with exactly n steps (tau_max 0.25, reordered: the demo schedule's settings)"""
    out = {}
    for n in STEPS:
        t = okz.fed_tau(0.97 * 0.25 * (n * n + n) / 3.0, 1, 0.25, True)
        assert len(t) == n
        out[n] = t
    return out


def pitch(w):
    return (w + 63) // 64 * 64


def content(seed, w, h, p):
    """NIMG different images: noise on a smooth ramp, so that the conductivity spans its range"""
    rng = np.random.default_rng(seed)
    a = np.zeros((NIMG, h, p), np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for i in range(NIMG):
        a[i, :, :w] = (0.5 + 0.4 * np.sin(xx * (0.05 + 0.02 * i) + yy * 0.03) + rng.uniform(-0.1, 0.1, (h, w))).astype(np.float32)
    return a


_multi_ref = {}
_cycle_ref = {}


def multi_case(okz, w, h):
    """inputs of the k_fed_multi cases of one plane size, and a cache of the oracle's results per step count"""
    key = (w, h)
    if key not in _multi_ref:
        p = pitch(w)
        rng = np.random.default_rng(1000 * w + h)
        g = np.zeros((NIMG, h, p), np.float32)
        g[:, :, :w] = rng.uniform(0.01, 1.0, (NIMG, h, w)).astype(np.float32)
        _multi_ref[key] = (content(w + 3 * h, w, h, p), g, {})
    return _multi_ref[key]


def same_bits(got, want, w):
    return got[..., :w].tobytes() == np.ascontiguousarray(want[..., :w]).tobytes()


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_fed_multi_deep(ah, okz, torch, taus, w, h, n):
    a, g, cache = multi_case(okz, w, h)
    p = pitch(w)
    if n not in cache:
        cache[n] = np.stack([okz.nld_steps(a[i], g[i], w, taus[n]) for i in range(NIMG)])
    # per image: src | flow | dst | tmp
    plane = h * p
    arena = torch.zeros((NIMG, 4 * plane), dtype=torch.float32, device="cuda")
    arena[:, :plane] = torch.from_numpy(a.reshape(NIMG, plane)).cuda()
    arena[:, plane:2 * plane] = torch.from_numpy(g.reshape(NIMG, plane)).cuda()
    base, sz = arena.data_ptr(), 4
    t = np.ascontiguousarray(taus[n], np.float32)
    ah.check(ah.lib.hak_op_nld_steps_batch(base, base + sz * plane, base + sz * 2 * plane, base + sz * 3 * plane, 4 * plane, w, h, p, NIMG,
                                        t.ctypes.data_as(C.POINTER(C.c_float)), n))
    got = arena[:, 2 * plane:3 * plane].cpu().numpy().reshape(NIMG, h, p)
    assert same_bits(got, cache[n], w)


def cycle_case(okz, w, h, head):
    key = (w, h, head)
    if key not in _cycle_ref:
        if head:
            sw, sh = 2 * w, 2 * h
            src = content(7 * w + h, sw, sh, pitch(sw))
            dec_sm = [okz.down_smooth(src[i], sw, w, h, pitch(w)) for i in range(NIMG)]
            L0 = np.stack([d for d, _ in dec_sm])
            sm = np.stack([s for _, s in dec_sm])
        else:
            src = content(5 * w + h, w, h, pitch(w))
            L0 = src
            sm = np.stack([okz.lowpass(src[i], w, 1.0, 2) for i in range(NIMG)])
        g = np.stack([okz.flow(sm[i], w, PM_G2, float(KCONTRAST[i])) for i in range(NIMG)])
        _cycle_ref[key] = (src, L0, sm, g, {})
    return _cycle_ref[key]


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("head", [0, 1], ids=["sublevel", "head"])
def test_fed_sf_deep(ah, okz, torch, taus, head, w, h, n):
    """k_fed_sf + the remaining k_fed_multi groups == oracle low-pass (or decimation + low-pass), conductivity and n steps"""
    src, L0, sm, g, cache = cycle_case(okz, w, h, head)
    p = pitch(w)
    if n not in cache:
        cache[n] = np.stack([okz.nld_steps(L0[i], g[i], w, taus[n]) for i in range(NIMG)])
    sh, sp = src.shape[1], src.shape[2]
    plane, splane = h * p, sh * sp
    # per image: src | smooth | flow | dst | tmp
    stride = splane + 4 * plane
    arena = torch.zeros((NIMG, stride), dtype=torch.float32, device="cuda")
    arena[:, :splane] = torch.from_numpy(src.reshape(NIMG, splane)).cuda()
    base, sz = arena.data_ptr(), 4
    off = [splane + k * plane for k in range(4)]
    t = np.ascontiguousarray(taus[n], np.float32)
    ah.check(ah.lib.hak_op_fed_cycle(base, head, 2 * w if head else w, sh, sp, base + sz * off[0], base + sz * off[1],
                                  base + sz * off[2], base + sz * off[3], stride, w, h, p, NIMG,
                                  KCONTRAST.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)), n))
    out = arena.cpu().numpy()

    def got(k):
        return out[:, off[k]:off[k] + plane].reshape(NIMG, h, p)
    assert same_bits(got(0), sm, w), "smooth"
    assert same_bits(got(2), cache[n], w), "L after the cycle"
    if n > 8:                                               # more than one launch: the conductivity plane is stored for the later ones
        assert same_bits(got(1), g, w), "conductivity"


@pytest.mark.parametrize("w,h,noct", [(256, 192, 2), (640, 640, 4)])
def test_batch_pipeline_deep(ah, okz, torch, w, h, noct):
    """hak_detect_and_compute_batch with 4 octaves asked for: records of three different images against the oracle (the
    streaming kernels are forced for the small planes of the tests).  An octave needs 80 px (akaze.cpp:204-237), so 256 x 192 gets
    two of the four; 640 x 640 is the smallest size that gets all four, and its octave 1 (320 columns) is wide enough for the launch
    sequence to take the deep groups; the narrower planes keep the 4-px groups (hak_fed_wide_only)."""
    from akaze_hip import synth
    mp = 2000
    p = ah.iAlignUp(w, 128)
    u8 = [synth.scene(w, h, 40 + i) for i in range(NIMG)]
    imgs = np.stack([synth.to_float(u, p) for u in u8])
    det = ah.Akazer()
    det.init((w, h, p), max_pts=mp, batch=NIMG)
    sched = det.schedule()
    assert sched["noct"] == noct and (sched["nsteps"].reshape(noct, 4)[1:, 1:] > 4).all()      # (octave 1's head: 4 steps)
    d_img = torch.from_numpy(imgs).cuda()
    pts = torch.zeros(NIMG * mp * 104, dtype=torch.uint8, device="cuda")
    num = torch.zeros(NIMG, dtype=torch.int32, device="cuda")
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d_img.data_ptr(), h * p, p, NIMG, pts.data_ptr(), num.data_ptr(), 1))
    ah.check(ah.lib.hak_sync(det.ctx))
    got = pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(NIMG, mp)
    cnt = num.cpu().numpy()
    det.close()
    for i in range(NIMG):
        r = okz.detect_and_compute(imgs[i], w, max_pts=mp)
        assert len(r.points) > 20
        assert_points_equal(got[i, :cnt[i]], r.points)


def test_launch_count_1080p(ah, torch, monkeypatch):
    """hak_query_traffic's FED launch count of a 4-octave 1080p plan: octaves 0 and 3 keep groups of at most 4 steps (octave 3's
    240 columns would fill 62 % of three 128-px strips), octaves 1 and 2 take groups of at most 8 where that saves launches;
    HAK_FED_MAX_FUSE=4 gives the 4-px count"""
    w, h = 1920, 1080

    def launches():
        det = ah.Akazer()
        det.init((w, h, ah.iAlignUp(w, 128)))
        ns = det.schedule()["nsteps"].reshape(4, 4)
        n = det.traffic().fed_launches
        det.close()
        return ns, n
    ns, deep = launches()
    wide = sum(-(-int(n) // 4) for n in ns.ravel())
    want = sum(-(-int(n) // 4) for n in np.concatenate([ns[0], ns[3]])) + sum(min(-(-int(n) // 4), -(-int(n) // 8)) for n in ns[1:3].ravel())
    assert deep == want and deep < wide
    monkeypatch.setenv("HAK_FED_MAX_FUSE", "4")
    assert launches()[1] == wide

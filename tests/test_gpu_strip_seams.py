"""GPU parity on the strip seams of the streaming kernels whose strips tile the pyramid's plane widths exactly, against the oracle, bit
for bit.

k_hessian_stream at dilation 4 (kernels_hessian_stream.hip): a wave owns 240 of its 256 columns, one column short of the halo the
dilation needs on either side; the end lanes fetch that column (strip columns -1 and 256) into a ring of their own.  The planes are the
smallest that put a seam everywhere it can lie: 244 (the second strip owns four columns), 248, 488 and 728 (the column right of the
strip is column w: its tap is the reflected w - 2), 480 (the seam is the right image edge), 484 and 724 (two and three strips and an
edge strip of four columns); heights 21 and 37 cut several row segments and reach both y reflections; one image and three; pitch w (the
last image's last row ends the buffer) and w + 4 with NaN (int: a sentinel) in the padding.  Extrema: single maxima on either side of
every seam, also on the first and last row of a row segment, through the detector tail (key map, candidate list, records).

k_fed_sf<6> and <7> (kernels_fedsf.hip): an x halo of 10 on 2-px lanes, 108 stored columns, at the widths where that takes fewer strips
than the halo of 12 (fs_hx_for).  Widths 216 (two whole strips of 108 against three of 104), 316 (three against four; the last holds
100 columns) and 960 (octave 1 of 1080p, nine strips: a seam at every multiple of 108) take the narrow halo, 220 keeps the halo of 12
(three strips either way; an edge strip of four columns under a halo of 10); height 40, one launch (6 and 7 steps) and two (12 = 6 + 6,
14 = 7 + 7: the first launch stores the conductivity), and the decimating octave head at widths 216 (narrow halo) and 220."""
import ctypes as C

import numpy as np
import pytest

import detector_tail as dt
import fast_domain as fd
import value_domain as vd

pytestmark = pytest.mark.gpu
f32 = np.float32
STEP = 4
WIDTHS = [244, 248, 480, 484, 488, 724, 728]
HEIGHTS = [21, 37]
SENTINEL = np.int32(0x5A5A5A5A)
SEAM_COLUMNS = (range(236, 244), range(476, 484))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ------------------------------------------------------------------------------------------------ dilation-4 planes
def hessian_inputs(kind, w, h, nimg):
    if kind == "float":
        return np.random.default_rng([w, h, nimg]).random((nimg, h, w), dtype=np.float32)
    return np.stack([fd.full_range(w, h, 11 * w + h + i) for i in range(nimg)]).astype(np.int32)


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", ["float", "int"])
def test_dilation4_planes(ah, okz, torch, monkeypatch, kind, w, h):
    """Lx, Ly and the determinant of k_hessian_stream<V, 4> on every pixel"""
    monkeypatch.setenv("HAK_HESS_STREAM", "2")
    op = ah.lib.hak_op_hessian_batch if kind == "float" else ah.lib.hak_op_fast_hessian_batch
    ref = okz.hessian if kind == "float" else okz.fast_hessian
    dtype = np.float32 if kind == "float" else np.int32
    for nimg in (1, 3):
        a = hessian_inputs(kind, w, h, nimg)
        for p in (w, w + 4):
            src = np.full((nimg, h, p), np.nan if kind == "float" else SENTINEL, dtype)
            src[:, :, :w] = a
            want = [ref(src[i], w, STEP) for i in range(nimg)]
            d_src = torch.from_numpy(src).cuda()
            outs = [torch.zeros((nimg, h, p), dtype=d_src.dtype, device="cuda") for _ in range(3)]
            route = C.c_int(0)
            ah.check(op(d_src.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), w, h, p, nimg, STEP, C.byref(route)))
            assert route.value == 1, "not the streaming kernel"
            for k, name in enumerate(("Lx", "Ly", "det")):
                got = outs[k].cpu().numpy()
                for i in range(nimg):
                    g, r = got[i, :, :w].view(np.uint32), np.ascontiguousarray(want[i][k][:, :w]).view(np.uint32)
                    for cols in SEAM_COLUMNS:
                        cols = [c for c in cols if c < w]
                        bad = np.argwhere(g[:, cols] != r[:, cols])
                        assert bad.size == 0, (name, "seam columns", cols[0], nimg, i, p, len(bad), bad[:3].tolist())
                    bad = np.argwhere(g != r)
                    assert bad.size == 0, (name, nimg, i, p, len(bad), bad[:3].tolist())


# ------------------------------------------------------------------------------------------------ extrema on the seams
W = dt.Context("W", 728, 248)
THR = f32(0.001)
FAST_THR = 65
FAST_IMPULSE = 1 << 16                  # 1.0 in 16.16


def seam_cases(sched, one):
    """-> [(level, [planes])] for the dilation-4 levels with a domain: single pixels of `one` on zero planes at columns 239 | 240 and
    479 | 480, each on a row inside a row segment, on the last row of a segment and on the first row of the next.  Pixels of one plane
    lie 4 * 4 + 3 or more apart (detector_tail.planted_seams has the reason), so the two sides of a seam go to different planes"""
    out = []
    for l in sched.levels():
        if int(sched.sigma_size[l]) != STEP:
            continue
        w, h, _ = sched.whp[l // dt.MS]
        x0, x1, y0, y1 = sched.domain(l)
        ry = dt.stream_geometry(sched, l)[1]
        cuts = [y for y in range(ry, h, ry) if y0 <= y - 1 and y <= y1][::2]
        mid = next(y for y in range((y0 + y1) // 2, y1 + 1) if y % ry not in (0, ry - 1))
        assert cuts and 2 * ry >= 4 * STEP + 3, (l, ry, y0, y1)
        planes = []
        for side in (0, 1):
            cols = [c - 1 + side for c in (240, 480) if x0 <= c - 1 and c <= x1]
            assert cols, (l, x0, x1)
            for rows in ([y - 1 for y in cuts], cuts, [mid]):
                a = np.zeros((h, w), np.asarray(one).dtype)
                for y in rows:
                    a[y, cols] = one
                planes.append(a)
        out.append((l, planes))
    return out


def check_tail(det, okz, sched, case, fast, threshold, what, nsites):
    exp = dt.walk(okz, sched, case, threshold, fast=fast)
    assert len(exp.cand) == nsites, (what, len(exp.cand), nsites)       # (the oracle finds every planted maximum)
    det.tail_begin()
    for l in sorted(case):
        o, s = divmod(l, dt.MS)
        if fast:
            det.fast_tail_level(o, s, case[l][1], threshold)
        else:
            det.tail_level(o, s, case[l][1])
    words, layer, cand, cap, ncand = det.tail_maps()
    pts, total = det.tail_finish(max_pts=dt.MAX_PTS, refine=not fast, fast=fast)
    assert ncand == len(exp.cand) <= cap, (what, ncand, len(exp.cand))
    bad = np.argwhere(layer != exp.layer)
    assert bad.size == 0, (what, "layer", bad[:3].tolist())
    bad = np.argwhere(words != exp.words)
    assert bad.size == 0, (what, "response word", bad[:3].tolist())
    assert np.array_equal(np.sort(cand), exp.cand), (what, "candidate list")
    want, wtotal = dt.records(okz, sched, exp.maps, None if fast else exp.dets, fast=fast)
    assert total == len(pts) == len(want) == wtotal, (what, total, len(pts), len(want), wtotal)
    assert np.array_equal(pts["octave"], want["octave"]), (what, "octave")
    for f in ("x", "y", "response", "size"):
        ok, _, first = vd.same_bits(pts[f], want[f])
        assert ok, (what, f, first)


@pytest.mark.parametrize("fast", [False, True], ids=["float", "fast"])
def test_planted_maxima_on_the_seams(ah, okz, torch, monkeypatch, fast):
    monkeypatch.setenv("HAK_HESS_STREAM", "2")
    s = W.sched(okz)
    det = W.create(ah)
    assert s.matches(det)
    cases = seam_cases(s, np.int32(FAST_IMPULSE) if fast else f32(1))
    assert {s.whp[l // dt.MS][0] for l, _ in cases} == {728, 364}           # seams at 240 and 480, and at 240 alone
    for l, planes in cases:
        for k, a in enumerate(planes):
            check_tail(det, okz, s, {l: ("L", a)}, fast, FAST_THR if fast else THR, f"level {l} plane {k}", int((a != 0).sum()))
    det.close()


# ------------------------------------------------------------------------------------------------ deep FED strips
NIMG = 3
KCONTRAST = np.array([0.37, 0.05, 0.41], np.float32)
PM_G2 = 1
FED_STEPS = [6, 7, 12, 14]
_fed_ref = {}


def pitch(w):
    return (w + 63) // 64 * 64


def content(seed, w, h, p):
    rng = np.random.default_rng(seed)
    a = np.zeros((NIMG, h, p), np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for i in range(NIMG):
        a[i, :, :w] = (0.5 + 0.4 * np.sin(xx * (0.05 + 0.02 * i) + yy * 0.03) + rng.uniform(-0.1, 0.1, (h, w))).astype(np.float32)
    return a


def fed_case(okz, w, h, head):
    """source planes, the oracle's L before the steps, low-pass and conductivity; computed once per shape"""
    key = (w, h, head)
    if key not in _fed_ref:
        if head:
            src = content(7 * w + h, 2 * w, 2 * h, pitch(2 * w))
            pairs = [okz.down_smooth(src[i], 2 * w, w, h, pitch(w)) for i in range(NIMG)]
            L0, sm = np.stack([d for d, _ in pairs]), np.stack([m for _, m in pairs])
        else:
            src = content(5 * w + h, w, h, pitch(w))
            L0, sm = src, np.stack([okz.lowpass(src[i], w, 1.0, 2) for i in range(NIMG)])
        g = np.stack([okz.flow(sm[i], w, PM_G2, float(KCONTRAST[i])) for i in range(NIMG)])
        _fed_ref[key] = (src, L0, sm, g, {})
    return _fed_ref[key]


def differing_columns(got, want, w):
    g, r = got[..., :w].view(np.uint32), np.ascontiguousarray(want[..., :w]).view(np.uint32)
    return sorted(set(np.argwhere(g != r)[:, -1].tolist()))


@pytest.mark.parametrize("n", FED_STEPS)
@pytest.mark.parametrize("w,head", [(216, 0), (220, 0), (316, 0), (960, 0), (216, 1), (220, 1)],
                         ids=["216", "220", "316", "960", "head216", "head220"])
def test_fed_sf_108_column_strips(ah, okz, torch, monkeypatch, w, head, n):
    """k_fed_sf<6 | 7> (+ the second group of 12 and 14 steps) == the oracle's low-pass, conductivity and n steps, on every column: the
    widths put image columns on either side of every multiple of 108"""
    monkeypatch.setenv("HAK_FUSE_SF", "2")
    h = 40
    src, L0, sm, g, cache = fed_case(okz, w, h, head)
    tau = okz.fed_tau(0.97 * 0.25 * (n * n + n) / 3.0, 1, 0.25, True)
    assert len(tau) == n
    if n not in cache:
        cache[n] = np.stack([okz.nld_steps(L0[i], g[i], w, tau) for i in range(NIMG)])
    p, sh, sp = pitch(w), src.shape[1], src.shape[2]
    plane, splane = h * p, sh * sp
    stride = splane + 4 * plane                                 # per image: src | smooth | flow | dst | tmp
    arena = torch.zeros((NIMG, stride), dtype=torch.float32, device="cuda")
    arena[:, :splane] = torch.from_numpy(src.reshape(NIMG, splane)).cuda()
    base = arena.data_ptr()
    off = [splane + k * plane for k in range(4)]
    t = np.ascontiguousarray(tau, np.float32)
    ah.check(ah.lib.hak_op_fed_cycle(base, head, 2 * w if head else w, sh, sp, base + 4 * off[0], base + 4 * off[1], base + 4 * off[2],
                                     base + 4 * off[3], stride, w, h, p, NIMG, KCONTRAST.ctypes.data_as(C.POINTER(C.c_float)),
                                     t.ctypes.data_as(C.POINTER(C.c_float)), n))
    out = arena.cpu().numpy()

    def got(k):
        return out[:, off[k]:off[k] + plane].reshape(NIMG, h, p)
    assert differing_columns(got(0), sm, w) == [], "smooth"
    assert differing_columns(got(2), cache[n], w) == [], "L after the cycle"
    if n > 8:                                                   # two launches: the first stores the conductivity for the second
        assert differing_columns(got(1), g, w) == [], "conductivity"

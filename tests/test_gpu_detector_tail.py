"""Stage parity of the detector tail against the oracle walk of tests/detector_tail.py (its docstring describes contexts, plane families
and seeded maps; tests/test_detector_tail_cpu.py asserts what they reach).  The extrema stage is read by itself, through
hak_debug_tail_maps, before the NMS can mask a missed or an extra candidate: response words and layers of the key map, the candidate
count and the candidate list as a sorted multiset.  Then the records of hak_op_tail_finish, whole.  Everything is compared bit for bit.

Kernel selections of the fused Hessian + extrema level: the streaming kernel (HAK_HESS_STREAM=2, where it covers the level), the tile
kernel (HAK_HESS_STREAM=0) with its staging buffer at 256 entries and at 4 (HAK_HESS_CBUF: every tile overflows), and the stand-alone
k_extrema on determinant planes.  The environment is read when a context is created.  After its cases every context runs an ordinary
image through the pipeline: the dense cases left nothing behind in the key map, the bitmap or the row counts."""
import numpy as np
import pytest

import detector_tail as dt
import value_domain as vd
from conftest import assert_points_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
THR = f32(0.001)
SELECTIONS = {
    "stream": {"HAK_HESS_STREAM": "2"},
    "tile": {"HAK_HESS_STREAM": "0", "HAK_HESS_CBUF": "256"},
    "tile_cbuf4": {"HAK_HESS_STREAM": "0", "HAK_HESS_CBUF": "4"},
}
_cache = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def select(monkeypatch, selection):
    for k, v in SELECTIONS[selection].items():
        monkeypatch.setenv(k, v)


# every context with extrema levels under every selection.  (B's odd width keeps the streaming kernel out of octave 0 whatever the
# selection; its octave 1, 132 wide, streams.  E1 and E2 are sizes of the seeded NMS alone.)
CONTEXTS = (dt.A, dt.B, dt.CC, dt.D)


def create(ah, okz, ctx, **more):
    det = ctx.create(ah, **more)
    assert ctx.sched(okz).matches(det)
    return det


def run_levels(det, sched, case, exp, fast=False, threshold=None, order=None):
    """begin + the case's levels (ascending, or in `order`) -> hak_debug_tail_maps.  hak_op_tail_finish has to follow"""
    det.tail_begin()
    for l in (sorted(case) if order is None else order):
        kind, a = case[l]
        o, s = divmod(l, dt.MS)
        if fast and kind == "L":
            det.fast_tail_level(o, s, a, threshold)
        elif fast:
            det.fast_tail_det_level(o, s, exp.dets[l][:, :a.shape[1]], threshold)
        elif kind == "L":
            det.tail_level(o, s, a)
        else:
            det.tail_det_level(o, s, a)
    return det.tail_maps()


def check_maps(got, exp, what):
    words, layer, cand, cap, ncand = got
    assert ncand == len(exp.cand) <= cap, (what, ncand, len(exp.cand), cap)
    bad = np.argwhere(layer != exp.layer)
    assert bad.size == 0, (what, "layer", len(bad), bad[:3].tolist())
    bad = np.argwhere(words != exp.words)
    assert bad.size == 0, (what, "response word", len(bad), bad[:3].tolist())
    assert np.array_equal(np.sort(cand), exp.cand), (what, "candidate list")


def check_records(got, count, want, wtotal, what, total=None):
    """count: what hak_op_tail_finish reports (the survivors, clamped to max_pts); total: hak_debug_tail_total (before the clamp)"""
    assert count == len(got) == len(want) <= wtotal and total in (None, wtotal), (what, count, total, wtotal, len(got), len(want))
    assert np.array_equal(got["octave"], want["octave"]), (what, "octave")
    for f in ("x", "y", "response", "size"):
        ok, _, first = vd.same_bits(got[f], want[f])                 # (NaN only where the oracle has a NaN)
        assert ok, (what, f, first)
    assert not got["angle"].any() and not got["features"].any() and (got["match"] == -1).all(), what


def run_case(det, okz, sched, case, exp, what, refine, fast=False, threshold=None, order=None, max_pts=dt.MAX_PTS):
    got = run_levels(det, sched, case, exp, fast, threshold, order)
    pts, total = det.tail_finish(max_pts=max_pts, refine=refine, fast=fast)
    assert det.tail_total() == total
    check_maps(got, exp, what)
    want, wtotal = cached(("rec", what, refine), lambda: dt.records(okz, sched, exp.maps, exp.dets if refine else None, fast=fast))
    check_records(pts, total, want, wtotal, what)
    return total


def ordinary_image(ah, okz, torch, det, ctx, **more):
    """an ordinary scene through the same context equals the pipeline oracle (more: the parameters the context was created with)"""
    w, h = ctx.w, ctx.h
    p = ah.iAlignUp(w, 128)
    img = dt.to_float(dt.ordinary_u8(w, h), p)
    want = cached(("ordinary", ctx.name, tuple(sorted(more.items()))),
                  lambda: okz.detect_and_compute(img, w, ctx.params(okz, **more), max_pts=8000).points)
    data = ah.AkazeData()
    ah.initAkazeData(data, 8000, True, True)
    try:
        d_img = torch.from_numpy(img).cuda()
        det.detectAndCompute(d_img.data_ptr(), data, (w, h, p), True)
        assert data.num_pts == len(want) > (0 if ctx is dt.D else 20)
        assert_points_equal(data.h_data[:data.num_pts], want)
    finally:
        ah.freeAkazeData(data)


def float_walk(okz, ctx, name, case, thr=THR):
    return cached(("walk", ctx.name, name, float(thr)), lambda: dt.walk(okz, ctx.sched(okz), case, thr))


# ------------------------------------------------------------------------------------------------ extrema stage + records, float path
@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_dense_and_tied_planes(ah, okz, torch, monkeypatch, selection):
    """noise: several hundred extrema per strip and segment, so k_hessian_stream's staging buffer flushes mid-segment and the tile
    kernel's overflows; quantised: determinants that tie across every fold.  C's levels 1 .. 3 (dilations 5, 6, 7) take the k_extrema
    fallback inside hak_op_tail_level.  Records with the refinement"""
    select(monkeypatch, selection)
    for ctx in CONTEXTS:
        s = ctx.sched(okz)
        det = create(ah, okz, ctx)
        for fam in (dt.noise, dt.quantised):
            what = f"{ctx.name} {fam.__name__}"
            case = dt.case_of(s, fam)
            exp = float_walk(okz, ctx, fam.__name__, case)
            for _ in range(2):                                       # twice: the sequence leaves the maps clean behind it
                assert run_case(det, okz, s, case, exp, what, refine=True) > 100
        ordinary_image(ah, okz, torch, det, ctx)
        det.close()


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_painted_patches_reach_both_branches_of_the_refinement(ah, okz, torch, monkeypatch, selection):
    """determinant patches chosen through 3 x 3 clusters of L pixels, half of them with a Newton step beyond one pixel.  (D has no level
    of dilation >= 3 with a domain: nothing to paint there, the ordinary image still runs)"""
    select(monkeypatch, selection)
    for ctx in CONTEXTS:
        s = ctx.sched(okz)
        det = create(ah, okz, ctx)
        for l in dt.painted_levels(s):
            case = {l: ("L", dt.painted_patches(s, l))}
            what = f"{ctx.name} painted {l}"
            run_case(det, okz, s, case, float_walk(okz, ctx, what, case), what, refine=True)
        ordinary_image(ah, okz, torch, det, ctx)
        det.close()


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_planted_seams(ah, okz, torch, monkeypatch, selection):
    """single maxima on both sides of every domain limit of every level, on its corners, on lane-quad edges, and on either side of every
    seam of the launch geometry (detector_tail.seam_columns / seam_rows): the last and first column a strip of the streaming kernel owns
    (multiples of 240, of 232 at dilation 4), the 64-column tile edges, the row segments of the streaming kernel (16 rows; 20 on D), the
    32- and 28-row tiles of the tile kernel and the 16-row blocks of k_extrema"""
    select(monkeypatch, selection)
    for ctx in CONTEXTS:
        s = ctx.sched(okz)
        det = create(ah, okz, ctx)
        for k, case in enumerate(cached(("seams", ctx.name), lambda: dt.planted_seams(s, "L"))):
            what = f"{ctx.name} seams {k}"
            run_case(det, okz, s, case, float_walk(okz, ctx, what, case), what, refine=True)
        ordinary_image(ah, okz, torch, det, ctx)
        det.close()


@pytest.mark.parametrize("name", [c.name for c in CONTEXTS])
@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_value_domain_planes(ah, okz, torch, monkeypatch, selection, name):
    """inf and NaN determinants in front of the extrema rule of the fused kernels (the ordered compares: a NaN neighbour, a NaN centre,
    an inf maximum) and of the refinement"""
    select(monkeypatch, selection)
    ctx = dt.CONTEXTS[name]
    s = ctx.sched(okz)
    det = create(ah, okz, ctx)
    for gen in dt.VALUE_DOMAIN:
        case = cached(("vdcase", name, gen), lambda: dt.value_domain_case(s, gen))
        what = f"{name} {gen}"
        run_case(det, okz, s, case, float_walk(okz, ctx, gen, case), what, refine=True)
    ordinary_image(ah, okz, torch, det, ctx)
    det.close()


def test_standalone_extrema_kernel(ah, okz, torch):
    """k_extrema<float> on determinant planes: the densest lattice (the list stays inside its capacity), noise and quantised determinants,
    the planted seams, and two levels on one full-resolution pixel with bit-equal responses and one ulp either way -- fed in ascending
    and in descending level order: the key decides, not the arrival"""
    for ctx in CONTEXTS:
        s = ctx.sched(okz)
        det = create(ah, okz, ctx)
        cases = [("lattice", dt.lattice(s))]
        for fam in (dt.noise, dt.quantised):
            dets = float_walk(okz, ctx, fam.__name__, dt.case_of(s, fam)).dets
            cases.append((fam.__name__ + " det", {l: ("det", np.ascontiguousarray(d[:, :s.whp[l // dt.MS][0]])) for l, d in dets.items()}))
        cases += [(f"seams det {k}", c) for k, c in enumerate(dt.planted_seams(s, "det"))]
        for name, case in cases:
            what = f"{ctx.name} {name}"
            run_case(det, okz, s, case, float_walk(okz, ctx, name, case), what, refine=False)
        if ctx is dt.A:
            case, sites = dt.equal_levels(s)
            exp = float_walk(okz, ctx, "equal_levels", case)
            for order in (sorted(case), sorted(case, reverse=True)):
                run_case(det, okz, s, case, exp, "A equal_levels", refine=False, order=order)
        ordinary_image(ah, okz, torch, det, ctx)
        det.close()


# ------------------------------------------------------------------------------------------------ extrema stage + records, FAST path
@pytest.mark.parametrize("selection", list(SELECTIONS) + ["k_extrema"])
def test_fast_extrema(ah, okz, torch, monkeypatch, selection):
    """the `int` twins: integer responses tie; thresholds 65 (the FAST sequence's own) and 0.  A negative threshold is refused, for the
    reason hak_create refuses a negative dthreshold (the key orders positive responses only)"""
    kind = "det" if selection == "k_extrema" else "L"
    if kind == "L":
        select(monkeypatch, selection)
    for ctx in CONTEXTS:
        s = ctx.sched(okz)
        det = create(ah, okz, ctx)
        for name in dt.FAST_FAMILIES:
            case = dt.fast_case(s, name, kind)
            for thr in dt.FAST_THRESHOLDS:
                what = f"{ctx.name} fast {name} {thr}"
                exp = cached(("fwalk", ctx.name, name, thr), lambda: dt.walk(okz, s, case, thr, fast=True))
                run_case(det, okz, s, case, exp, what, refine=False, fast=True, threshold=thr)
        plane = next(iter(case.values()))[1]
        for op in (det.fast_tail_level, det.fast_tail_det_level):
            with pytest.raises(ah.HakError, match="threshold"):
                op(s.levels()[0] // dt.MS, s.levels()[0] % dt.MS, plane, -1)
        ordinary_image(ah, okz, torch, det, ctx)
        det.close()


# ------------------------------------------------------------------------------------------------ NMS on seeded maps
@pytest.mark.parametrize("name", ["A", "C", "D", "E1", "E2"])
def test_seeded_nms(ah, okz, torch, name):
    """k_nms_cand (both radius branches and, on C, waves that mix them; ties; the lagging cursor), k_row_scan (h below 256, not a
    multiple of it, per 1, 2 and 3) and k_emit (D: a second pass of the word loop) on hand-made maps: survivors, order, count, total"""
    ctx = dt.CONTEXTS[name]
    s = ctx.sched(okz)
    det = create(ah, okz, ctx)
    w = s.whp[0][0]
    for pop in dt.POPULATIONS:
        for dens in dt.DENSITIES:
            words, layer = dt.seeded_maps(s, ctx, pop, dens)
            for fast in (False, True):
                what = f"{name} {pop} {dens:.3f} {'fast' if fast else 'float'}"
                want, wtotal = cached(("seeded", what), lambda: dt.records(okz, s, dt.oracle_maps(s, words, layer, fast), fast=fast))
                assert wtotal == len(want) > 10
                # the clamp: below, at and above the survivor count (once per population; above it everywhere)
                for max_pts in ((wtotal - 1, wtotal, wtotal + 1) if dens == dt.DENSITIES[1] else (dt.MAX_PTS,)):
                    det.tail_begin()
                    det.tail_seed(words.view(np.int32) if fast else words.view(np.float32), layer)
                    gw, gl, cand, cap, ncand = det.tail_maps()
                    pts, total = det.tail_finish(max_pts=max_pts, refine=False, fast=fast)
                    assert np.array_equal(gw, words) and np.array_equal(gl, layer) and ncand == int((layer >= 0).sum()) <= cap, what
                    ys, xs = np.nonzero(layer >= 0)
                    assert np.array_equal(np.sort(cand), np.sort(dt.cand_words(0, ys, xs) | (layer[ys, xs].astype(np.uint64) << np.uint64(32)))), what
                    check_records(pts, total, want[:max_pts], wtotal, (what, max_pts), det.tail_total())
    ordinary_image(ah, okz, torch, det, ctx)
    det.close()


# ------------------------------------------------------------------------------------------------ threshold
def test_zero_threshold_matches_and_negative_is_refused(ah, okz, torch):
    """dthreshold = 0 keeps every response positive: the key's order (the bits of a positive float) is the reference's.  Below zero it is
    not -- a negative maximum would enter the key map above every positive one, where the reference compares floats against maps that
    start at -0.0926 -- so hak_create refuses it, and a NaN (hipakaze.h)"""
    ctx = dt.A
    s = ctx.sched(okz)
    det = create(ah, okz, ctx, dthreshold=0.0)
    case = dt.case_of(s, dt.noise)
    exp = float_walk(okz, ctx, "noise", case, f32(0))
    assert len(exp.cand) > len(float_walk(okz, ctx, "noise", case).cand)
    run_case(det, okz, s, case, exp, "A noise threshold 0", refine=True)
    ordinary_image(ah, okz, torch, det, ctx, dthreshold=0.0)
    det.close()
    for bad in (-1.0, -1e-30, float("nan")):
        with pytest.raises(ah.HakError, match="dthreshold"):
            ctx.create(ah, dthreshold=bad)


# ------------------------------------------------------------------------------------------------ whole pipeline
@pytest.mark.parametrize("selection", ["default", "level_tile", "hess_tile"])
def test_whole_pipeline_on_white_noise(ah, okz, torch, monkeypatch, selection):
    """nine white-noise images of 328 x 248, each alone and in batches of 2 and 8: k_level_tile's own extrema pass and the NMS grid of
    nimg >= 8 on dense content"""
    if selection == "level_tile":
        monkeypatch.setenv("HAK_LEVEL_TILE", "2")
    elif selection == "hess_tile":
        monkeypatch.setenv("HAK_HESS_STREAM", "0")
    ctx = dt.A
    w, h, mp = ctx.w, ctx.h, 4000
    p = ah.iAlignUp(w, 128)
    imgs = [dt._pitched(dt.white_noise_image(w, h, k), p) for k in range(9)]
    want = cached("white noise", lambda: [okz.detect_and_compute(a, w, ctx.params(okz), max_pts=mp).points for a in imgs])
    assert all(300 < len(o) < mp for o in want)
    stack = torch.from_numpy(np.stack(imgs)).cuda()
    det = ctx.create(ah, max_pts=mp, batch=8)
    data = ah.AkazeData()
    ah.initAkazeData(data, mp, True, True)
    for k in range(9):
        det.detectAndCompute(stack[k].data_ptr(), data, (w, h, p), True)
        assert_points_equal(data.h_data[:data.num_pts], want[k])
    ah.freeAkazeData(data)
    d_pts = torch.zeros(8 * mp * ah.POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_num = torch.zeros(8, dtype=torch.int32, device="cuda")
    for first, B in ((7, 2), (0, 8), (1, 8)):
        ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, stack[first].data_ptr(), h * p, p, B, d_pts.data_ptr(), d_num.data_ptr(), 1))
        ah.check(ah.lib.hak_sync(det.ctx))
        nums = d_num.cpu().numpy()
        allp = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(8, mp)
        for i in range(B):
            assert nums[i] == len(want[first + i])
            assert_points_equal(allp[i, :nums[i]], want[first + i])
    ordinary_image(ah, okz, torch, det, ctx)
    det.close()

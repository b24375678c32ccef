"""Oracle-only twin of tests/test_gpu_detector_tail.py: the inputs of tests/detector_tail.py reach the places they claim to reach, so
that a pass on the GPU means something, and the walk the GPU module compares against is the pipeline oracle's own."""
import numpy as np
import pytest

import detector_tail as dt

f32 = np.float32
THR = f32(0.001)


@pytest.fixture(scope="module")
def walks(okz):
    """the oracle walk of (context, family), computed once"""
    cache = {}

    def get(ctx, family):
        key = (ctx.name, family.__name__)
        if key not in cache:
            s = ctx.sched(okz)
            cache[key] = dt.walk(okz, s, dt.case_of(s, family), THR)
        return cache[key]
    return get


def test_contexts_are_what_the_module_says(okz):
    a, b, c, d = (x.sched(okz) for x in (dt.A, dt.B, dt.CC, dt.D))
    assert a.noct == 2 and a.levels() == list(range(8)) and a.whp[1][:2] == (164, 124)
    assert a.domain(7)[2:] == (58, 65)                               # octave 1 sublevel 3 keeps rows 58 .. 65
    assert b.noct == 2 and b.levels() == list(range(8)) and b.whp[0][0] % 4 != 0
    assert c.noct == 1 and list(c.sigma_size) == [4, 5, 6, 7] and c.levels() == [0, 1, 2, 3]
    assert [int(f32(v) + f32(0.5)) for v in c.sizes] == [4, 5, 6, 7]              # NMS radii: one narrow class, three wide ones
    assert d.noct == 1 and d.levels() == [0] and d.domain(0)[2:] == (29, 50) and (d.whp[0][0] + 63) // 64 == 65
    assert all(int(f32(v) + f32(0.5)) <= 4 for v in a.sizes)         # A and B: the narrow branch only
    for e, per in ((dt.E1, 3), (dt.E2, 2), (dt.A, 1)):
        assert (e.h + 255) // 256 == per and e.h % 256 != 0


def test_noise_fills_the_streaming_kernels_staging_buffer(okz, walks):
    """k_hessian_stream flushes mid-segment when one wave has staged more than 128 candidates: every level of A but the last holds a
    block of one wave -- the columns its strip owns (240, or 232 at dilation 4) x one 16-row segment, detector_tail.stream_geometry --
    with at least 129 extrema.  Level 7 cannot: its domain is 48 x 8 pixels, 96 strict maxima at the most (it holds 37)"""
    s = dt.A.sched(okz)
    e = walks(dt.A, dt.noise)
    for l in s.levels():
        o = l // dt.MS
        mine = e.cand[(e.cand >> np.uint64(32)) == l]
        xs, ys = (mine & np.uint64(0xFFFF)).astype(np.int64) >> o, ((mine >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64) >> o
        xv, ry = dt.stream_geometry(s, l)
        assert (xv, ry) == ((232 if l % 4 == 3 else 240), 16)
        best = np.bincount((ys // ry) * 8 + xs // xv).max()
        x0, x1, y0, y1 = s.domain(l)
        if l == 7:
            assert ((x1 - x0 + 2) // 2) * ((y1 - y0 + 2) // 2) < 129 and best >= 25
            continue
        assert best >= 129, (l, best)
        if l < 3:
            assert best >= 300, (l, best)                            # (the flush fires more than once per segment)


def test_planted_seams_reach_every_limit(okz):
    for ctx in (dt.A, dt.B, dt.CC, dt.D):
        s = ctx.sched(okz)
        for kind in ("L", "det"):
            rows, cols = {l: set() for l in s.levels()}, {l: set() for l in s.levels()}
            got = set()
            cases = dt.planted_seams(s, kind)
            assert 1 <= len(cases) <= 40
            for case in cases:
                e = dt.walk(okz, s, case, THR)
                for c in e.cand:
                    l = int(c >> np.uint64(32))
                    x, y = (int(c) & 0xFFFF) >> (l // dt.MS), ((int(c) >> 16) & 0xFFFF) >> (l // dt.MS)
                    rows[l].add(y); cols[l].add(x); got.add((l, x, y))
            for l in s.levels():
                x0, x1, y0, y1 = s.domain(l)
                assert {y0, y1} <= rows[l] and {x0, x1} <= cols[l], (ctx.name, kind, l)
                assert min(rows[l]) == y0 and max(rows[l]) == y1 and min(cols[l]) == x0 and max(cols[l]) == x1   # none outside
                for x, y, tag in dt.seam_sites(s, l):
                    assert ((l, x, y) in got) == (tag != "outside"), (ctx.name, kind, l, x, y, tag)
                tags = {t for _, _, t in dt.seam_sites(s, l)}
                assert {"corner", "col", "row", "outside"} <= tags
                # every seam of every kernel's launch geometry that crosses the domain carries a maximum on either side
                assert set(dt.seam_columns(s, l)) <= cols[l] and set(dt.seam_rows(s, l)) <= rows[l], (ctx.name, kind, l)
            if ctx is dt.A:
                # the streaming kernel's strips: 240 owned columns at dilations 2 and 3, 232 at dilation 4; tiles of 64 columns
                assert {239, 240, 255, 256} <= cols[0] and {239, 240} <= cols[1] and {231, 232} <= cols[3]
                assert dt.seam_columns(s, 0)[239] == dt.seam_columns(s, 3)[231] == "strip" and 239 not in dt.seam_columns(s, 3)
                assert any(x % 4 == 3 for x in cols[0]) and any(x % 4 == 0 for x in cols[0])
                assert {y % 16 for y in rows[0]} >= {0, 15} and {y % 32 for y in rows[0]} >= {0, 31}
                assert {83, 84, 111, 112} <= rows[3]                 # the 28-row tiles of dilation 4
            if ctx is dt.D:
                assert {39, 40} <= rows[0] and {31, 32} <= rows[0]   # four segments of 20 rows; 32-row tiles
                assert {239, 240, 3839, 3840, 4079, 4080} <= cols[0]


def test_quantised_planes_tie(okz, walks):
    """at least 100 pixels per context fail the strict maximum by an equal neighbour alone: above the threshold, >= all eight
    neighbours, inside the level's domain, and not a candidate"""
    for ctx in (dt.A, dt.B):
        s = ctx.sched(okz)
        e = walks(ctx, dt.quantised)
        n = 0
        for l in s.levels():
            t, m = _fails_by_a_tie_alone(e.dets[l][:, :s.whp[l // dt.MS][0]], s.domain(l), THR)
            assert m == e.per_level[l]
            n += t
        assert n >= 100, (ctx.name, n)


def test_lattice_is_the_densest_case(okz):
    s = dt.A.sched(okz)
    e = dt.walk(okz, s, dt.lattice(s), THR)
    for l in s.levels():
        x0, x1, y0, y1 = s.domain(l)
        assert e.per_level[l] == len(range(x0 + x0 % 2, x1 + 1, 2)) * len(range(y0 + y0 % 2, y1 + 1, 2))
    cap = sum(dt.MS * ((w + 1) // 2) * ((h + 1) // 2) for w, h, _ in s.whp)      # hak_create's cand_cap
    assert 10000 < len(e.cand) <= cap


def test_equal_levels_reach_both_tie_orders(okz):
    s = dt.A.sched(okz)
    case, sites = dt.equal_levels(s)
    e = dt.walk(okz, s, case, THR)
    seen = set()
    for la, lb, x, y, rel in sites:
        assert e.layer[y, x] == (lb if rel > 0 else la), (la, lb, rel)             # equal: the earlier level stays (akazed.cu:1368)
        seen.add((lb // dt.MS - la // dt.MS, rel))
    assert seen == {(d, r) for d in (0, 1) for r in (0, 1, -1)}
    assert len(e.cand) == 2 * len(sites)


@pytest.mark.parametrize("name", ["A", "C", "D", "E1", "E2"])
def test_seeded_maps_census(okz, name):
    """the numpy census agrees with okz.nms on every seeded map, and the four-valued maps are decided by ties and by the cursor lag"""
    ctx = dt.CONTEXTS[name]
    s = ctx.sched(okz)
    w, h, _ = s.whp[0]
    for pop in dt.POPULATIONS:
        for dens in dt.DENSITIES:
            words, layer = dt.seeded_maps(s, ctx, pop, dens)
            cs = dt.nms_census(s, words, layer)
            keep = cs["centre"] & ~cs["larger"] & ~cs["tie"]
            for fast in (False, True):
                pts, total = dt.records(okz, s, dt.oracle_maps(s, words, layer, fast), fast=fast)
                assert total == len(pts) == int(keep.sum())
                ys, xs = np.nonzero(keep)
                assert np.array_equal(pts["x"], xs.astype(f32)) and np.array_equal(pts["y"], ys.astype(f32))
            psz = s.psz
            on = layer >= 0
            assert on[psz, psz] and on[psz, w - 1 - psz] and on[h - 1 - psz, psz] and on[h - 1 - psz, w - 1 - psz]
            if pop == "four" and dens == 1.0:
                assert int((cs["centre"] & ~cs["larger"] & cs["tie"]).sum()) >= 100          # suppressed by the tie clause alone
            if pop == "four" and dens < 0.1:                         # (the map with the planted row pairs)
                # the clean-disc cursor is the oracle's own alternative reading (okz_reading_variant & 1); the numpy census with
                # lag=False restates it: same survivors, position by position
                okz.lib().okz_set_reading_variant(1)
                try:
                    cpts, ctotal = dt.records(okz, s, dt.oracle_maps(s, words, layer))
                finally:
                    okz.lib().okz_set_reading_variant(0)
                ckeep = np.zeros((h, w), bool)
                ckeep[cpts["y"].astype(np.int64), cpts["x"].astype(np.int64)] = True
                clean = dt.nms_census(s, words, layer, lag=False)
                assert ctotal == len(cpts) and np.array_equal(ckeep, clean["centre"] & ~clean["larger"] & ~clean["tie"])
                lagged = keep != ckeep                               # decisions that differ between the two readings of the oracle
                assert int((lagged & ~cs["wide"]).sum()) >= 20
                if name == "C":
                    assert int((lagged & cs["wide"]).sum()) >= 20
                    nw, nn = int((cs["centre"] & cs["wide"]).sum()), int((cs["centre"] & ~cs["wide"]).sum())
                    assert nw > 0 and nn > 0 and 1 / 3 <= nw / nn <= 3          # both radius classes in every stretch of the list
                else:
                    assert not cs["wide"].any()
            if pop == "distinct":
                assert not (cs["tie"] & ~cs["larger"] & cs["centre"]).any() or dens == 1.0
            if name == "D":
                xs = np.nonzero(keep.any(axis=0))[0]
                assert (xs < 4096).any() and (xs >= 4096).any()      # survivors in both passes of k_emit's word loop


def test_reading_variant_is_the_clean_disc(okz):
    """the census' lag switch is the oracle's own alternative reading (okz_reading_variant & 1), survivor by survivor, on the dense
    four-valued map of C as well (test_seeded_maps_census does the same on the sparse maps it counts on)"""
    s = dt.CC.sched(okz)
    w, h, _ = s.whp[0]
    words, layer = dt.seeded_maps(s, dt.CC, "four", 1.0)
    clean = dt.nms_census(s, words, layer, lag=False)
    okz.lib().okz_set_reading_variant(1)
    try:
        pts, total = dt.records(okz, s, dt.oracle_maps(s, words, layer))
    finally:
        okz.lib().okz_set_reading_variant(0)
    keep = np.zeros((h, w), bool)
    keep[pts["y"].astype(np.int64), pts["x"].astype(np.int64)] = True
    assert total == len(pts) and np.array_equal(keep, clean["centre"] & ~clean["larger"] & ~clean["tie"])


def test_refinement_has_weak_and_refined_points(okz, walks):
    """both branches of gRefine, at least 50 keypoints each.  Noise alone does not reach the weak one (1 keypoint of 3072 on A; 1 to 3
    of ~3000 on blurred, streaked and quantised noise as well): a strict 3 x 3 maximum of an unstructured plane almost never has its
    Newton step beyond one pixel.  detector_tail.painted_patches plants patches that do, at every level it can"""
    s = dt.A.sched(okz)
    e = walks(dt.A, dt.noise)
    refined, weak = dt.weak_census(okz, s, e.maps, e.dets)
    assert refined >= 50 and weak >= 1, (refined, weak)
    for ctx in (dt.A, dt.B, dt.CC):
        s = ctx.sched(okz)
        refined = weak = 0
        for l in dt.painted_levels(s):
            e = dt.walk(okz, s, {l: ("L", dt.painted_patches(s, l))}, THR)
            r, k = dt.weak_census(okz, s, e.maps, e.dets)
            refined, weak = refined + r, weak + k
        assert refined >= 50 and weak >= 50, (ctx.name, refined, weak)


def test_value_domain_planes_reach_nan_and_inf_determinants(okz):
    s = dt.B.sched(okz)
    nan = inf = 0
    for name in dt.VALUE_DOMAIN:
        dets = dt.det_planes(okz, s, dt.value_domain_case(s, name))
        nan += sum(int(np.isnan(d).sum()) for d in dets.values())
        inf += sum(int(np.isinf(d).sum()) for d in dets.values())
    assert nan >= 100 and inf >= 100


def _fails_by_a_tie_alone(d, dom, thr):
    """pixels of the domain above the threshold that are >= all eight neighbours but not > all of them"""
    x0, x1, y0, y1 = dom
    c = d[y0:y1 + 1, x0:x1 + 1]
    ge, gt = np.ones(c.shape, bool), np.ones(c.shape, bool)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            if i or j:
                nb = d[y0 + i:y1 + 1 + i, x0 + j:x1 + 1 + j]
                ge &= c >= nb
                gt &= c > nb
    return int(((c > thr) & ge & ~gt).sum()), int(((c > thr) & gt).sum())


def test_fast_planes_tie(okz):
    s = dt.A.sched(okz)
    for thr in dt.FAST_THRESHOLDS:
        e = dt.walk(okz, s, dt.fast_case(s, "small_range"), thr, fast=True)
        n = 0
        for l in s.levels():
            t, m = _fails_by_a_tie_alone(e.dets[l][:, :s.whp[l // dt.MS][0]], s.domain(l), thr)
            assert m == e.per_level[l]
            n += t
        assert n >= 100 and len(e.cand) >= 1000, (thr, n)
    for name in dt.FAST_FAMILIES:
        n65, n0 = (len(dt.walk(okz, s, dt.fast_case(s, name), thr, fast=True).cand) for thr in dt.FAST_THRESHOLDS)
        assert 20 <= n65 <= n0, (name, n65, n0)


def test_walk_reproduces_the_pipeline_oracle(okz):
    """the same walk over the arena planes of a whole-image run gives okz.detect_and_compute's keypoints"""
    ctx = dt.A
    s = ctx.sched(okz)
    w, h, p = s.whp[0]
    img = np.zeros((h, p), np.float32)
    img[:, :w] = dt.white_noise_image(w, h, 0)
    r = okz.detect_and_compute(img, w, ctx.params(okz), max_pts=dt.MAX_PTS, desc=False, keep_arena=True)
    case = {l: ("det", np.ascontiguousarray(okz.plane(r, 1, l // dt.MS, l % dt.MS))) for l in s.levels()}
    e = dt.walk(okz, s, case, THR)
    pts, total = dt.records(okz, s, e.maps, e.dets)
    assert total == len(r.points) > 300
    for f in ("x", "y", "octave", "response", "size"):
        assert np.array_equal(pts[f].view(np.uint32) if pts[f].dtype.kind == "f" else pts[f],
                              r.points[f].view(np.uint32) if pts[f].dtype.kind == "f" else r.points[f]), f

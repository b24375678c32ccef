"""Stage parity of the keypoint kernels (csrc/kernels_describe.hip: k_orient<float|int>, k_describe_runs<float|int>,
k_describe<float|int>, k_desc_perm) against the oracle's point functions, on the planted keypoints of tests/keypoint_stage.py.

Float path: hak_op_orient_describe -- orientation + MLDB (mode "orient"), MLDB alone with planted angles ("angles"), and upright
contexts.  FAST path: hak_op_fast_orient_describe -- refinement + orientation + MLDB, and refinement + MLDB in upright contexts.
Every plane family x descriptor pattern size x HAK_DESC_PLAN 0 / 1; all records of a case go in one call.  Whole records are
compared, bit for bit (value_domain.same_bits for an angle: NaN against NaN): the fields no kernel may touch must come back as they
went in.  tests/test_keypoint_stage_cpu.py asserts, on the oracle alone, which edges these cases reach.

The knobs are read by hak_create, so a context is made per (pattern size, upright, HAK_DESC_PLAN, HAK_DESC_SORT) and kept for the module."""
import pytest

import keypoint_stage as ks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sched(okz):
    return ks.oracle_sched(okz)


@pytest.fixture(scope="module")
def contexts():
    cache = {}
    yield cache
    for det, _ in cache.values():
        det.close()


@pytest.fixture(scope="module")
def expected():
    return {}


def _context(ah, sched, cache, monkeypatch, pat, upright, plan, sort=None):
    key = (pat, upright, plan, sort)
    if key not in cache:
        monkeypatch.setenv("HAK_DESC_PLAN", plan)
        if sort is not None:
            monkeypatch.setenv("HAK_DESC_SORT", sort)
        det = ah.Akazer()
        det.init((ks.W, ks.H, ah.iAlignUp(ks.W, 128)), noctaves=ks.NOCT, max_scale=ks.MS, descriptor_pattern_size=pat, upright=upright,
                 max_pts=ks.MAX_PTS)
        assert ks.det_sched(det).same(sched), "the context's schedule is not the oracle's"
        cache[key] = [det, None]
    return cache[key]


def _load(entry, sched, tag, planes):
    """the planes of a family into the context's arena (once per context and family)"""
    det = entry[0]
    if entry[1] != tag:
        for l, lv in enumerate(planes):
            o, s = divmod(l, ks.MS)
            w = sched.whp[o][0]
            for kind, key in ((0, "lt"), (2, "lx"), (3, "ly")):
                det.set_plane(kind, o, s, lv[key][:, :w])
        entry[1] = tag
    return det


def _expect(okz, sched, expected, kind, family, pat, mode, planes, rec, tag="case"):
    key = (kind, family, pat, mode, tag)
    if key not in expected:
        expected[key] = ks.oracle_walk(okz, sched, rec, planes, mode, pat, kind == "fast")
    return expected[key]


def _check(got, want, rec, what):
    diff = ks.first_difference(got, want)
    if diff is not None:
        i, f = diff
        pytest.fail(f"{what}: record {i} (level {int(rec['octave'][i])}, x {rec['x'][i]!r}, y {rec['y'][i]!r}) differs first in `{f}`: "
                    f"got {got[f][i]!r}, oracle {want[f][i]!r}")


@pytest.mark.parametrize("mode", ks.MODES)
@pytest.mark.parametrize("plan", ["1", "0"], ids=["plan", "noplan"])
@pytest.mark.parametrize("pat", ks.PATTERNS)
@pytest.mark.parametrize("family", ks.FLOAT_FAMILIES)
def test_float_orient_describe(ah, okz, sched, contexts, expected, monkeypatch, family, pat, plan, mode):
    rec, _ = ks.records(okz, sched, "float")
    planes = ks.float_planes(okz, family)
    det = _load(_context(ah, sched, contexts, monkeypatch, pat, mode == "upright", plan), sched, ("float", family), planes)
    want = _expect(okz, sched, expected, "float", family, pat, mode, planes, rec)
    got = det.orient_describe(rec.view(ah.POINT_DTYPE), desc=2 if mode == "angles" else 1).view(okz.POINT_DTYPE)
    _check(got, want, rec, f"{family}, pattern {pat}, {mode}")


@pytest.mark.parametrize("mode", ["orient", "upright"])
@pytest.mark.parametrize("plan", ["1", "0"], ids=["plan", "noplan"])
@pytest.mark.parametrize("pat", ks.PATTERNS)
@pytest.mark.parametrize("family", ks.FAST_FAMILIES)
def test_fast_refine_orient_describe(ah, okz, sched, contexts, expected, monkeypatch, family, pat, plan, mode):
    rec, _ = ks.records(okz, sched, "fast")
    planes = ks.fast_planes(okz, family)
    det = _load(_context(ah, sched, contexts, monkeypatch, pat, mode == "upright", plan), sched, ("fast", family), planes)
    want = _expect(okz, sched, expected, "fast", family, pat, mode, planes, rec)
    got = det.fast_orient_describe(rec.view(ah.POINT_DTYPE), desc=1).view(okz.POINT_DTYPE)
    _check(got, want, rec, f"FAST {family}, pattern {pat}, {mode}")


def test_fast_refinement_alone(ah, okz, sched, contexts, monkeypatch):
    """desc = 0: k_orient<int> runs for the refinement alone and nothing else of the record changes"""
    rec, _ = ks.records(okz, sched, "fast")
    planes = ks.fast_planes(okz, "int_min_block")
    det = _load(_context(ah, sched, contexts, monkeypatch, 10, False, "1"), sched, ("fast", "int_min_block"), planes)
    want = ks.oracle_walk(okz, sched, rec, planes, "orient", 10, True)
    for f in ("angle", "features"):
        want[f] = rec[f]
    got = det.fast_orient_describe(rec.view(ah.POINT_DTYPE), desc=0).view(okz.POINT_DTYPE)
    _check(got, want, rec, "FAST refinement alone")


@pytest.mark.parametrize("kind,family", [("float", "rotating"), ("fast", "full_range")])
def test_launch_shape_and_visiting_order(ah, okz, sched, contexts, expected, monkeypatch, kind, family):
    """more records than either grid has blocks (1024 for k_orient, 4096 for the MLDB kernels), all levels in mixed order: both
    kernels loop.  With HAK_DESC_SORT=2 they visit the records level by level through k_desc_perm's permutation, with 0 in output
    order: identical results, equal to the oracle's."""
    fast = kind == "fast"
    rec = ks.many_records(okz, sched, kind)
    assert len(rec) > 4096 and len(rec) <= ks.MAX_PTS
    planes = ks.fast_planes(okz, family) if fast else ks.float_planes(okz, family)
    want = _expect(okz, sched, expected, kind, family, 10, "orient", planes, rec, "many")
    got = {}
    for sort in ("2", "0"):
        det = _load(_context(ah, sched, contexts, monkeypatch, 10, False, "1", sort), sched, (kind, family), planes)
        got[sort] = det.orient_describe(rec.view(ah.POINT_DTYPE), desc=1, fast=fast).view(okz.POINT_DTYPE)
        _check(got[sort], want, rec, f"{kind} {family}, {len(rec)} records, HAK_DESC_SORT={sort}")
    assert ks.first_difference(got["2"], got["0"]) is None

"""k_describe_runs gathers its samples in image-row order (the order table of the keypoint's angle bin, HAK_DESC_GATHER=1, the
default) or in window order (HAK_DESC_GATHER=0) and sums them in the reference's order either way: whole records must be bit-identical
to the oracle's and to each other, on the small planes and the planted keypoints of tests/keypoint_stage.py.

Added to those records: keypoints in the four image corners and on the four image edges of every level (both clamps of the sample
position fire, in x and in y), and planted angles that reach every row of the table and every way a float can miss one: each bin
centre, the float32 values one ulp either side of each bin edge, 0, -0.0, +-pi, the value just below 2 pi, negative angles, NaN,
+-inf, +-1e30 and a denormal.  The float path takes them as they are (MLDB alone, mode "angles"); the FAST path always runs k_orient<int>
first (it carries the refinement), so its angles are the orientation kernel's own and its image-corner keypoints sit one pixel inside,
where the refinement's 3 x 3 neighbourhood exists.  Pattern size 12 goes through the generic k_describe: the knob must be inert there.

The knobs are read by hak_create: a context per (pattern size, upright, HAK_DESC_GATHER, HAK_DESC_SORT), kept for the module."""
import numpy as np
import pytest

import keypoint_stage as ks

pytestmark = pytest.mark.gpu
f32 = np.float32
NB = 32
FAMILY = {"float": "hdr", "fast": "full_range"}


def planted_angles():
    a = [f32(b * 2 * np.pi / NB) for b in range(NB)]
    for b in range(NB):
        e = f32((b + 0.5) * 2 * np.pi / NB)
        a += [np.nextafter(e, f32(-np.inf)), np.nextafter(e, f32(np.inf))]
    a += [f32(0.0), f32(-0.0), f32(np.pi), f32(-np.pi), np.nextafter(f32(2 * np.pi), f32(0)), f32(-0.3), f32(-1.0), f32(-5.0)]
    a += [f32(np.nan), f32(np.inf), f32(-np.inf), f32(1e30), f32(-1e30), f32(1e-45)]
    return a


def planted_records(okz, sched, kind):
    """ks.records + eight keypoints per level in the image corners and on the image edges; float records carry planted_angles()"""
    rec, _ = ks.records(okz, sched, kind)
    inset = 1 if kind == "fast" else 0
    extra = []
    for l in range(ks.NOCT * ks.MS):
        o = l // ks.MS
        w, h, _ = sched.whp[o]
        x0, x1, y0, y1 = inset, w - 1 - inset, inset, h - 1 - inset
        for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1), (w // 2, y0), (w // 2, y1), (x0, h // 2), (x1, h // 2)):
            r = rec[0].copy()
            r["x"], r["y"], r["octave"], r["size"] = f32(x << o), f32(y << o), l, sched.sizes[l]
            extra.append(r)
    out = np.concatenate([rec, np.array(extra, rec.dtype)])
    out["response"] = np.arange(len(out), dtype=np.float32) + f32(0.5)
    angles = planted_angles()
    assert len(out) >= 2 * len(angles)
    for i in range(len(out)):                   # the image-corner records come last: stride 1 gives them consecutive angles
        out["angle"][i] = angles[(i * 37) % len(angles)] if i < len(rec) else angles[(i * 5 + 3) % len(angles)]
    return out


def many_planted(okz, sched, kind, n=4400):
    """more records than the grid has blocks (4096), every level in mixed order"""
    rec = planted_records(okz, sched, kind)
    rng = np.random.default_rng([ks.SEED, 4301])
    out = rec[rng.integers(0, len(rec), n)].copy()
    out["response"] = np.arange(n, dtype=np.float32) + f32(0.5)
    assert 4096 < n <= ks.MAX_PTS and len(set(out["octave"][:64])) == ks.NOCT * ks.MS
    return out


@pytest.fixture(scope="module")
def sched(okz):
    return ks.oracle_sched(okz)


@pytest.fixture(scope="module")
def contexts():
    cache = {}
    yield cache
    for det, _ in cache.values():
        det.close()


def _context(ah, sched, cache, monkeypatch, pat, upright, gather, sort=None):
    key = (pat, upright, gather, sort)
    if key not in cache:
        monkeypatch.setenv("HAK_DESC_GATHER", gather)
        monkeypatch.setenv("HAK_DESC_PLAN", "1")
        if sort is None:
            monkeypatch.delenv("HAK_DESC_SORT", raising=False)
        else:
            monkeypatch.setenv("HAK_DESC_SORT", sort)
        det = ah.Akazer()
        det.init((ks.W, ks.H, ah.iAlignUp(ks.W, 128)), noctaves=ks.NOCT, max_scale=ks.MS, descriptor_pattern_size=pat, upright=upright,
                 max_pts=ks.MAX_PTS)
        assert ks.det_sched(det).same(sched), "the context's schedule is not the oracle's"
        cache[key] = [det, None]
    return cache[key]


def _load(entry, sched, tag, planes):
    det = entry[0]
    if entry[1] != tag:
        for l, lv in enumerate(planes):
            o, s = divmod(l, ks.MS)
            w = sched.whp[o][0]
            for kind, key in ((0, "lt"), (2, "lx"), (3, "ly")):
                det.set_plane(kind, o, s, lv[key][:, :w])
        entry[1] = tag
    return det


def _run(ah, okz, sched, contexts, monkeypatch, kind, mode, pat, rec, sorts=(None,)):
    """the records through every (HAK_DESC_GATHER, HAK_DESC_SORT) context: each result equal to the oracle's, all equal to each other"""
    fast = kind == "fast"
    planes = ks.fast_planes(okz, FAMILY[kind]) if fast else ks.float_planes(okz, FAMILY[kind])
    want = ks.oracle_walk(okz, sched, rec, planes, mode, pat, fast)
    got = []
    for gather in ("1", "0"):
        for sort in sorts:
            det = _load(_context(ah, sched, contexts, monkeypatch, pat, mode == "upright", gather, sort), sched, kind, planes)
            out = det.orient_describe(rec.view(ah.POINT_DTYPE), desc=2 if mode == "angles" else 1, fast=fast).view(okz.POINT_DTYPE)
            diff = ks.first_difference(out, want)
            if diff is not None:
                i, f = diff
                pytest.fail(f"{kind}, pattern {pat}, {mode}, HAK_DESC_GATHER={gather}, HAK_DESC_SORT={sort}: record {i} (level "
                            f"{int(rec['octave'][i])}, x {rec['x'][i]!r}, y {rec['y'][i]!r}, planted angle {rec['angle'][i]!r}) differs "
                            f"first in `{f}`: got {out[f][i]!r}, oracle {want[f][i]!r}")
            got.append(out)
    for out in got[1:]:
        assert ks.first_difference(out, got[0]) is None
    return want


CASES = [("float", "orient"), ("float", "angles"), ("float", "upright"), ("fast", "orient"), ("fast", "upright")]


@pytest.mark.parametrize("kind,mode", CASES)
def test_gather_order_is_bit_exact(ah, okz, sched, contexts, monkeypatch, kind, mode):
    rec = planted_records(okz, sched, kind)
    want = _run(ah, okz, sched, contexts, monkeypatch, kind, mode, 10, rec)
    if mode == "angles":                        # the planted angles reached the kernel and came back untouched, every bin among them
        assert np.array_equal(want["angle"].view(np.uint32), rec["angle"].view(np.uint32))
        assert {ah.describe_order_bin(float(a)) for a in rec["angle"]} == set(range(NB))
        assert len({bytes(f) for f in want["features"]}) > len(rec) // 2


@pytest.mark.parametrize("kind,mode", [("float", "angles"), ("fast", "orient")])
def test_knob_is_inert_on_the_generic_kernel(ah, okz, sched, contexts, monkeypatch, kind, mode):
    assert not ah.describe_plan(12)[0]
    _run(ah, okz, sched, contexts, monkeypatch, kind, mode, 12, planted_records(okz, sched, kind))


@pytest.mark.parametrize("kind,mode", [("float", "angles"), ("fast", "orient")])
def test_more_records_than_blocks_in_both_visiting_orders(ah, okz, sched, contexts, monkeypatch, kind, mode):
    _run(ah, okz, sched, contexts, monkeypatch, kind, mode, 10, many_planted(okz, sched, kind), sorts=("0", "2"))

"""CPU twin of tests/test_gpu_keypoint_stage.py: the planted-keypoint cases of tests/keypoint_stage.py on the oracle alone.

  * the generator is pinned: the same seed gives the same bytes (a checksum of one small case);
  * the stage harness is tied to the pipeline oracle: on one float and one FAST run of detect_and_compute(keep_arena=True) the walk of
    keypoint_stage.oracle_walk (and okz_refine_point on the float path) on the arena planes, from the NMS output, reproduces the
    pipeline's x, y, angle and features bit for bit -- the plane, octave, width and pitch conventions the GPU module relies on;
  * the census: which narrow places of the point functions the cases reach, counted by the oracle itself (OkzCensus) and asserted, so
    that a change of the generator cannot silently stop exercising an edge.  The minimums below are the counts observed with
    keypoint_stage.SEED = 11 (printed by `pytest -s`); no case is filtered or skipped.
"""
import ctypes as C

import numpy as np
import pytest

import keypoint_stage as ks

f32 = np.float32


@pytest.fixture(scope="module")
def sched(okz):
    return ks.oracle_sched(okz)


# ------------------------------------------------------------------------------------------------ the generator
def test_geometry_is_the_smallest_with_eight_domains(okz, sched):
    assert sched.whp == [(265, 245, 384), (132, 122, 256)] and all(p != w for w, _, p in sched.whp)
    doms = [ks.domain(sched, l) for l in range(ks.NOCT * ks.MS)]
    assert doms[0] == (29, 235, 29, 215) and doms[7] == (58, 73, 58, 63)          # the 0.72 px argument starts at column 29
    assert all(x1 - x0 >= 2 and y1 - y0 >= 2 for x0, x1, y0, y1 in doms)
    # one row less at octave 1 and its sublevel 3 (border 56.57) has no room for "one inside the limit" any more
    assert f32(56.5) < sched.borders[7] < f32(56.6) and doms[7][3] - doms[7][2] == 5


def test_generator_is_pinned(okz, sched):
    rec, tags = ks.records(okz, sched, "float")
    rec2, _ = ks.records(okz, sched, "float")
    assert rec.tobytes() == rec2.tobytes() and len(rec) == 241
    frec, _ = ks.records(okz, sched, "fast")
    assert ks.digest(rec, ks.float_planes(okz, "rotating")) == ks.digest(rec2, ks.float_planes.__wrapped__(okz, "rotating"))
    assert ks.digest(frec, ks.fast_planes(okz, "ramp_x")) == PIN_FAST_RAMP_X
    assert ks.digest(rec, ks.float_planes(okz, "lobes")) == PIN_FLOAT_LOBES
    many = ks.many_records(okz, sched, "fast")
    assert len(many) > 4096 and many.tobytes() == ks.many_records(okz, sched, "fast").tobytes()


PIN_FAST_RAMP_X = "c3be2191f72fa56577d2ae8c17a137849bb801f208dbe99094f883f33860343d"
PIN_FLOAT_LOBES = "fd1fa829514ee63310b748b7c5181f21166a2706b36ca631ab367ea9a1a243bd"


def test_positions_cover_limits_corners_parities_and_fractions(okz, sched):
    rec, tags = ks.records(okz, sched, "float")
    frec, _ = ks.records(okz, sched, "fast")
    pos = ks.positions(sched)
    for l in range(ks.NOCT * ks.MS):
        x0, x1, y0, y1 = ks.domain(sched, l)
        mine = [(x, y, t) for ll, x, y, t in pos if ll == l]
        assert all(x0 <= x <= x1 and y0 <= y <= y1 for x, y, _ in mine)
        for lim, axis in ((x0, 0), (x1, 0), (y0, 1), (y1, 1)):                        # every level has keypoints on each of its four limits
            assert sum(p[axis] == lim for p in mine) >= 4, (l, lim)
        assert {(x0, y0), (x1, y0), (x0, y1), (x1, y1)} <= {(x, y) for x, y, _ in mine}
        assert {(x0 + 1, y0 + 1), (x1 - 1, y1 - 1)} <= {(x, y) for x, y, _ in mine}
        assert sum(t == "interior" for _, _, t in mine) == 6
    o1 = frec["octave"] >= ks.MS
    assert {(int(x) & 1, int(y) & 1) for x, y in zip(frec["x"][o1], frec["y"][o1])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert np.all(frec["x"] == np.floor(frec["x"])) and np.all(frec["y"] == np.floor(frec["y"]))
    # float path: level coordinates off the integer on both sides, and after the + 0.5f of the orientation on both sides of .5
    lvl = rec["x"] / (1 << (rec["octave"] // ks.MS)).astype(f32)
    frac = lvl - np.floor(lvl)
    assert (frac == 0.5).sum() >= 8 and ((frac > 0.4999) & (frac < 0.5)).sum() >= 8 and ((frac > 0.5) & (frac < 0.5001)).sum() >= 8
    ang = set(rec["angle"].view(np.uint32).tolist())
    for v in ks.angle_sweep()[:23]:
        assert int(f32(v).view(np.uint32)) in ang, v


# ------------------------------------------------------------------------------------------------ the tie to the pipeline oracle
def _arena_planes(okz, r, dtype):
    out = []
    for l in range(r.noct * r.ms):
        o, s = divmod(l, r.ms)
        w, h, p = (int(v) for v in r.owhps[3 * o:3 * o + 3])
        pl = {}
        for key, kind in (("lt", 0), ("det", 1), ("lx", 2), ("ly", 3)):
            base = int(r.offsets[o]) + (kind * r.ms + s) * int(r.osizes[o])
            pl[key] = r.arena[base:base + h * p].reshape(h, p).view(dtype)
        out.append(pl)
    return out


def _maps(r, dtype):
    n = int(r.osizes[0])
    h, p = int(r.owhps[1]), int(r.owhps[2])
    return r.arena[:n].view(dtype).reshape(h, p), r.arena[n:2 * n].view(np.float32).reshape(h, p), r.arena[2 * n:3 * n].view(np.int32).reshape(h, p)


@pytest.mark.parametrize("fast", [False, True], ids=["float", "FAST"])
@pytest.mark.parametrize("upright", [False, True], ids=["oriented", "upright"])
def test_stage_walk_reproduces_the_pipeline_oracle(okz, sched, fast, upright):
    from akaze_hip import synth
    u8 = synth.scene(ks.W, ks.H, 3, nshapes=200)
    prm = ks.params(okz, 10, upright)
    p = sched.whp[0][2]
    if fast:
        r = okz.fast_detect_and_compute(u8, prm, max_pts=4000, keep_arena=True)
    else:
        r = okz.detect_and_compute(synth.to_float(u8, p), ks.W, prm, max_pts=4000, keep_arena=True)
    assert [tuple(int(v) for v in r.owhps[3 * o:3 * o + 3]) for o in range(r.noct)] == sched.whp
    assert len(r.points) > 300 and len(set(r.points["octave"].tolist())) == 6          # (no image reaches the two narrowest levels)
    # the unrefined keypoints: the NMS once more on the maps the run left in the arena
    resp, size, layer = _maps(r, np.int32 if fast else np.float32)
    _, _, _, psz = okz.schedule(prm, r.noct)
    raw, total = okz.nms(np.ascontiguousarray(resp), np.ascontiguousarray(size), np.ascontiguousarray(layer), ks.W, psz, 4000, fast=fast)
    assert total == len(r.points)
    assert np.array_equal(raw["size"].view(np.uint32), sched.sizes[raw["octave"]].view(np.uint32))        # okz_schedule is the run's schedule
    for pt in raw:                                                       # and `accepted` is the run's border rule: no keypoint outside it
        l = int(pt["octave"])
        x0, x1, y0, y1 = ks.domain(sched, l)
        assert x0 <= int(pt["x"]) >> (l // ks.MS) <= x1 and y0 <= int(pt["y"]) >> (l // ks.MS) <= y1
    planes = _arena_planes(okz, r, np.int32 if fast else np.float32)
    raw["match"], raw["distance"], raw["match_x"], raw["match_y"] = -1, -1, -1, -1
    if not fast:
        for i in range(len(raw)):
            l = int(raw["octave"][i])
            okz.lib().okz_refine_point(C.c_void_p(raw.ctypes.data + i * raw.itemsize), C.c_void_p(planes[l]["det"].ctypes.data),
                                       C.c_int(l // ks.MS), C.c_int(sched.whp[l // ks.MS][2]))
    got = ks.oracle_walk(okz, sched, raw, planes, "upright" if upright else "orient", 10, fast)
    assert ks.first_difference(got, r.points) is None
    assert got.tobytes() == r.points.tobytes()


# ------------------------------------------------------------------------------------------------ the census
def _census(okz, sched, kind, families, planes_of, modes, patterns):
    rec, tags = ks.records(okz, sched, kind)
    out = {}
    for fam in families:
        pl = planes_of(okz, fam)
        for pat in patterns:
            for mode in modes:
                got, rows = ks.oracle_walk(okz, sched, rec, pl, mode, pat, kind == "fast", census=True)
                out[fam, pat, mode] = (got, rows)
    return rec, out


@pytest.fixture(scope="module")
def float_census(okz, sched):
    return _census(okz, sched, "float", ks.FLOAT_FAMILIES, ks.float_planes, ks.MODES, ks.PATTERNS)


@pytest.fixture(scope="module")
def fast_census(okz, sched):
    return _census(okz, sched, "fast", ks.FAST_FAMILIES, ks.fast_planes, ("orient", "upright"), ks.PATTERNS)


def _clamps(cen, pat, fams=None):
    rows = [r for (f, p, m), (_, rs) in cen.items() if p == pat and (fams is None or f in fams) for r in rs]
    return np.array([r[0] for r in rows]).sum(0), min(r[1] for r in rows)


def test_census_sample_positions(float_census, fast_census):
    """pattern 12 clamps on all four sides; pattern 10 never does, with under 1 px to spare (6 and 8 stay further inside)"""
    for name, (_, cen), finite in (("float", float_census, ks.vd.TIERS["A"] + list(ks.ORIENT_FAMILIES)), ("FAST", fast_census, None)):
        c12, _ = _clamps(cen, 12, finite)
        c10, e10 = _clamps(cen, 10, finite)
        c8, e8 = _clamps(cen, 8, finite)
        c6, e6 = _clamps(cen, 6, finite)
        print(name, "clamped samples at pattern 12 (left, right, top, bottom):", c12.tolist(), "| min edge distance at 10, 8, 6:", e10, e8, e6)
        assert np.all(c12 >= np.array(CLAMP12_MIN[name])), c12
        assert not c10.any() and not c8.any() and not c6.any()
        assert e10 < 1.0 and e10 < e8 < e6
    assert _clamps(float_census[1], 10, ks.vd.TIERS["A"] + list(ks.ORIENT_FAMILIES))[1] < 0.0       # a refined keypoint rounds onto column 0


CLAMP12_MIN = {"float": [2780, 4165, 3966, 3383], "FAST": [374, 837, 421, 934]}      # observed (left, right, top, bottom)


def test_census_orientation_histogram(float_census):
    _, cen = float_census
    win = {f: [r[6] for r in cen[f, 10, "orient"][1]] for f in ks.FLOAT_FAMILIES}
    assert set(win["rotating"]) == set(range(42))                       # every window start wins, the wrapping ones included
    assert sum(k >= 36 for k in win["rotating"]) >= 6
    hi = {f: sum(r[2] for r in cen[f, 10, "orient"][1]) for f in ks.FLOAT_FAMILIES}
    lo = {f: sum(r[3] for r in cen[f, 10, "orient"][1]) for f in ks.FLOAT_FAMILIES}
    bin0 = {f: sum(r[4] for r in cen[f, 10, "orient"][1]) for f in ks.FLOAT_FAMILIES}
    bin41 = {f: sum(r[5] for r in cen[f, 10, "orient"][1]) for f in ks.FLOAT_FAMILIES}
    ties = {f: sum(r[9] > 0 for r in cen[f, 10, "orient"][1]) for f in ks.FLOAT_FAMILIES}
    print("clamped from above 41:", hi["lobes"], "| bin 0:", bin0["rotating"], "| bin 41:", bin41["rotating"], "| ties:", ties["lobes"],
          "| below 0:", sum(lo.values()))
    assert hi["lobes"] >= HI_MIN and bin0["rotating"] >= BIN0_MIN and bin41["rotating"] >= BIN41_MIN
    # a < 0 cannot happen for an angle in [-pi, pi] (the conversion truncates toward zero and NaN gives bin 21): the lower clamp is dead
    # code in the reference too, and bin 0 is reached by the angle -pi alone
    assert sum(lo.values()) == 0
    assert ties["lobes"] >= TIES_MIN                                    # two windows of equal weight, different angle: first from 0 wins
    got = cen["zero", 10, "orient"][0]
    assert np.all(got["angle"] == 0) and not np.signbit(got["angle"]).any()


HI_MIN, BIN0_MIN, BIN41_MIN, TIES_MIN = 9196, 293, 687, 49                   # observed; 49 = every cell of `lobes`


def test_census_fast_refinement_and_saturation(okz, sched, fast_census):
    rec, cen = fast_census
    acc = rej = sat_full = 0
    moved = np.zeros(4, int)
    for (fam, pat, mode), (got, rows) in cen.items():
        if pat != 10 or mode != "orient":
            continue
        acc += sum(r[7] == 1 for r in rows)
        rej += sum(r[7] == 0 for r in rows)
        ratio = (1 << (rec["octave"] // ks.MS)).astype(f32)
        cx, cy = np.floor(rec["x"] / ratio) * ratio, np.floor(rec["y"] / ratio) * ratio    # (int)x >> o, back at full resolution
        ok = np.array([r[7] == 1 for r in rows])
        moved += [int((got["x"][ok] < cx[ok]).sum()), int((got["x"][ok] > cx[ok]).sum()), int((got["y"][ok] < cy[ok]).sum()), int((got["y"][ok] > cy[ok]).sum())]
        if fam == "raw_full_range":
            sat_full += sum(r[8] for r in rows)
        else:
            assert not sum(r[8] for r in rows), fam                     # derivatives out of gDerivate are 16-bit numbers
    print("FAST refinement accepted / rejected:", acc, rej, "| moved left, right, up, down:", moved.tolist(), "| saturated (raw_full_range):", sat_full)
    assert acc >= ACC_MIN and rej >= REJ_MIN and np.all(moved >= np.array(MOVED_MIN)) and sat_full >= SAT_MIN
    # `unit_step`: the first accepted corner of every level takes a step of exactly +1.0 level pixel in x, and it is accepted
    got, rows = cen["unit_step", 10, "orient"]
    for l in range(ks.NOCT * ks.MS):
        i = int(np.argmax(rec["octave"] == l))
        ratio = 1 << (l // ks.MS)
        assert rows[i][7] == 1 and got["x"][i] == np.floor(rec["x"][i] / ratio) * ratio + ratio and got["y"][i] == np.floor(rec["y"][i] / ratio) * ratio
    hi = sum(r[2] for r in cen["ramp_x", 10, "orient"][1])
    assert hi >= 109 * 100                                              # Ly = 0, Lx < 0: every sample of most records takes the clamp a > 41
    winners = {r[6] for (f, p, m), (_, rs) in cen.items() if m == "orient" for r in rs}
    print("FAST winning windows:", len(winners))
    assert len(winners) >= FAST_WINNERS_MIN


def test_fast_det_restates_the_oracle(okz, sched):
    """keypoint_stage.fast_det (the determinant of `raw_full_range`) against fkz_hessian, on derivatives that come from there"""
    for fam in ("full_range", "ramp_blown"):
        for l, lv in enumerate(ks.fast_planes(okz, fam)):
            w = sched.whp[l // ks.MS][0]
            assert np.array_equal(ks.fast_det(okz, lv["lx"], lv["ly"], w, int(sched.sigma_size[l]))[:, :w], lv["det"][:, :w]), (fam, l)


ACC_MIN, REJ_MIN, MOVED_MIN, SAT_MIN, FAST_WINNERS_MIN = 1179, 749, [241, 260, 223, 256], 16216, 41         # observed


def test_census_descriptors_are_not_degenerate(float_census, fast_census):
    for name, (_, cen) in (("float", float_census), ("FAST", fast_census)):
        feats = np.concatenate([got["features"] for got, _ in cen.values()])
        bits = np.unpackbits(feats, axis=1, bitorder="little")[:, :486]
        assert bits.min(0).max() == 0 and bits.max(0).min() == 1, name             # every one of the 486 bits takes both values
        assert not np.unpackbits(feats[:, 60], bitorder="little").reshape(-1, 8)[:, 6:].any()      # byte 60 holds 6 bits

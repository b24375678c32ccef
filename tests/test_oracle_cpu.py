"""CPU suite, part 1: the oracle against every pinned quantity.

The reference ships no tests; what can be pinned is: the FED tau tables (against the reference's
own fed.cpp, compiled into oracle/_ref and frozen in tests/golden/fed_tau.json), the constants the
survey derived from the reference source (hex KATs), the struct layout, and the oracle's own
frozen outputs on the reference's bundled left.pgm/right.pgm (regression pin).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_fed_tau_matches_reference_golden(okz):
    cases = json.load(open(os.path.join(GOLDEN, "fed_tau.json")))["cases"]
    assert len(cases) >= 100
    for c in cases:
        tau = okz.fed_tau(c["T"], c["M"], c["tau_max"], c["reordering"])
        assert [int(v) for v in tau.view(np.uint32)] == c["tau_bits"], c["T"]


def test_fed_tau_matches_live_reference_build(okz):
    """300 seeded random process times: the reference's fed.cpp tables are frozen in tests/golden/fed_tau_random.npz
    (make_golden.py fed_random_golden); where oracle/_ref/libfedref.so is built, the live reference must give them too"""
    g = np.load(os.path.join(GOLDEN, "fed_tau_random.npz"))
    rng = np.random.default_rng(5)
    ts = rng.uniform(0.01, 300.0, 300).astype(np.float32)
    assert np.array_equal(ts.view(np.uint32), g["T"].view(np.uint32))
    live = okz.ref_lib() is not None
    for reorder in (0, 1):
        bits, offs = g[f"tau_bits_{reorder}"], np.concatenate([[0], np.cumsum(g[f"tau_len_{reorder}"])])
        for i, T in enumerate(ts):
            want = bits[offs[i]:offs[i + 1]]
            assert np.array_equal(okz.fed_tau(float(T), 1, 0.25, reorder).view(np.uint32), want), (float(T), reorder)
            if live:
                assert np.array_equal(okz.ref_fed_tau(float(T), 1, 0.25, reorder).view(np.uint32), want), (float(T), reorder)


def test_fed_schedule_kats(okz):
    # steps per (octave, sublevel) and first tau vectors
    ttimes = [0.530193, 0.749807, 1.060387, 1.499614, 2.120772, 2.999228, 4.241547, 5.998454, 8.483089,
              11.996912, 16.966187, 23.993816, 33.932358, 47.987648, 67.864746, 95.975266, 135.729431,
              191.950592, 271.458984]
    lens = [len(okz.fed_tau(t)) for t in ttimes]
    assert lens == [3, 3, 4, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 29, 34, 40, 48, 57]
    np.testing.assert_allclose(okz.fed_tau(0.530193), [0.0697266981, 0.108422101, 0.352044374], rtol=2e-6)
    np.testing.assert_allclose(okz.fed_tau(1.060387), [0.106038667, 0.679864287, 0.0820016563, 0.192482203], rtol=2e-6)
    np.testing.assert_allclose(okz.fed_tau(1.499614), [0.149961352, 0.961473405, 0.115967877, 0.272210985], rtol=2e-6)


def test_gauss_taps_kat(okz):
    k = okz.gauss_taps(1.0, 2)
    assert [bits(v) for v in k] == [0x3ECE2433, 0x3E7A0FEA, 0x3D5F2F86]
    k = okz.gauss_taps(float(np.float32(1.6) * np.float32(1.6)), 4)
    np.testing.assert_allclose(k, [0.250404447, 0.205977082, 0.114643514, 0.043175146, 0.0110020069], rtol=1e-6)


def test_derivative_factors_kat(okz):
    f1, f2 = okz.deriv_factors()
    assert bits(f1) == 0x3DC00001 and bits(f2) == 0x3EA00001


def test_point_struct_layout(okz):
    assert okz.lib().okz_sizeof_point() == 104
    d = okz.POINT_DTYPE
    offs = {n: d.fields[n][1] for n in d.names}
    assert offs == dict(x=0, y=4, octave=8, response=12, size=16, angle=20, features=24, _pad=85, match=88,
                        distance=92, match_x=96, match_y=100)


def test_mldb_pair_table(okz):
    a, b = okz.compare_indices()
    assert (a[:486] < b[:486]).all() and ((b[:486] - a[:486]) % 3 == 0).all()
    # 18 + 108 + 360 pairs, channel-major inside each grid
    assert a[0] == 0 and b[0] == 3 and a[6] == 1 and a[18] == 12 and b[18] == 15 and a[126] == 39
    assert len({(int(x), int(y)) for x, y in zip(a[:486], b[:486])}) == 486


def test_oracle_on_reference_images_is_frozen(okz, golden):
    """regression pin on data/left.pgm, right.pgm (also the survey's independent smoke datum: 3544 / 4695 under its misread clean-disc NMS and true-maximum hmax; 3634 / 4831 with the reference's cursor lag, Q1; 3631 / 4834 with the lattice maximum and the histogram guard of hScharrContrast as well, round 5)"""
    from akaze_hip import synth
    for name, key, n in (("left", "pts1", 3631), ("right", "pts2", 4834)):
        u8 = golden.lr_u8[name]
        r = okz.detect_and_compute(synth.to_float(u8, 1280), 1280)
        g = golden.lr[key]
        assert len(r.points) == n == len(g)
        for f in ("x", "y", "octave", "response", "size", "angle", "features"):
            assert np.array_equal(r.points[f], g[f]), f
    kc = golden.lr["kc"]
    np.testing.assert_allclose(kc, [0.663032, 0.948956], rtol=1e-5)          # (0.65252 / 0.95842 with the true maximum, rounds 1-4)


def test_oracle_match_frozen_and_rules(okz, golden):
    p1, p2 = golden.lr["pts1"].copy(), golden.lr["pts2"].copy()
    want = p1.copy()
    p1["match"] = 0
    okz.match(p1, p2)
    for f in ("match", "distance", "match_x", "match_y"):
        assert np.array_equal(p1[f], want[f])
    acc = p1["match"] >= 0
    assert acc.sum() == 2464 and (p1["distance"][acc] < 96).all() and (p1["distance"][~acc] == -1).all()
    # brute-force check of the accept rule on a subset with numpy
    f1, f2 = p1["features"][:200], p2["features"]
    d = np.unpackbits(f1[:, None, :] ^ f2[None, :, :], axis=2).sum(axis=2)
    for q in range(200):
        dm = d[q].min()
        idx = np.nonzero(d[q] == dm)[0]
        ok = dm < 96 and len(set(idx % 16)) == 1
        assert (p1["match"][q] == (idx[0] if ok else -1)) and (p1["distance"][q] == (dm if ok else -1))


def test_oracle_match_edge_cases(okz):
    from akaze_hip import synth
    a = synth.random_descriptors(40, 1, okz.POINT_DTYPE)
    b = a[:5].copy()                                    # n2 < 16
    okz.match(a, b)
    assert (a["match"][:5] == np.arange(5)).all() and (a["distance"][:5] == 0).all()
    okz.match(a, b[:0])                                 # n2 == 0
    assert (a["match"] == -1).all()
    # duplicate train descriptors in different residue classes -> rejected; same class -> first wins
    b = np.concatenate([a[:1], a[:1]])                  # j = 0 and 1: classes differ
    okz.match(a[:1], b)
    assert a["match"][0] == -1
    b = synth.random_descriptors(17, 2, okz.POINT_DTYPE)
    b[0] = a[0]; b[16] = a[0]                           # j = 0 and 16: same class
    okz.match(a[:1], b)
    assert a["match"][0] == 0 and a["distance"][0] == 0


def test_oracle_synth_frozen(okz, golden):
    from akaze_hip import synth
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    for name, w, h, seed, kw in mg.SYNTH_CASES:
        r = mg.run_oracle(mg.case_scene(w, h, seed), **kw)
        g = golden.synth[name + "_pts"]
        assert len(g) > 20 and r.points.tobytes() == g.tobytes(), name


def test_stage_properties(okz):
    rng = np.random.default_rng(3)
    w, h, p = 150, 97, 192
    img = np.zeros((h, p), np.float32)
    img[:, :w] = rng.uniform(0, 1, (h, w)).astype(np.float32)
    # a constant image is a fixed point of every smoothing / diffusion stage
    c = np.zeros((h, p), np.float32); c[:, :w] = 0.25
    lp = okz.lowpass(c, w, 1.0, 2)
    assert np.abs(lp[:, :w] - 0.25).max() < 1e-6
    g = okz.flow(okz.lowpass(img, w, 1.0, 2), w, 1, 0.5)
    assert (g[:, :w] > 0).all() and (g[:, :w] <= 1).all()
    out = okz.nld_steps(c, g, w, [0.2, 5.0, 0.7])
    assert np.array_equal(out[:, :w], c[:, :w])
    # tau = 0 is the identity; a stable step (tau <= 0.25, g <= 1) obeys the maximum principle
    assert np.array_equal(okz.nld_steps(img, g, w, [0.0])[:, :w], img[:, :w])
    out = okz.nld_steps(img, g, w, [0.2, 0.25])
    assert out[:, :w].min() >= img[:, :w].min() - 1e-6 and out[:, :w].max() <= img[:, :w].max() + 1e-6
    # separable Gaussian == numpy reference with reflect-101 padding (fp tolerance)
    k = okz.gauss_taps(1.0, 2).astype(np.float64)
    full = np.concatenate([k[:0:-1], k])
    pad = np.pad(img[:, :w].astype(np.float64), 2, mode="reflect")
    rows = sum(full[i] * pad[:, i:i + w] for i in range(5))
    ref = sum(full[i] * rows[i:i + h, :] for i in range(5))
    assert np.abs(okz.lowpass(img, w, 1.0, 2)[:, :w] - ref).max() < 1e-6


# ----------------------------------------------------------------- integer FAST path oracle (akaze_oracle_fast.c)
def test_fast_oracle_fixed_point_kats(okz):
    """16.16 weights: ik = (int)(k * 65536 + 0.5f) of the float taps (akazed.cu:3896-3921)"""
    import ctypes as C
    L = okz.lib()
    ik = np.zeros(8, np.int32)
    for var, R in ((1.0, 2), (1.6 * 1.6, 3), (1.2 * 1.2, 3), (2.0 * 2.0, 5)):
        L.fkz_gauss_taps(C.c_float(var), R, ik.ctypes.data_as(C.POINTER(C.c_int)))
        k = okz.gauss_taps(var, R)
        want = (k.astype(np.float32) * np.float32(65536) + np.float32(0.5)).astype(np.int32)
        assert np.array_equal(ik[:R + 1], want)
        assert abs(int(ik[0]) + 2 * int(ik[1:R + 1].sum()) - 65536) <= R + 1
    f1, f2 = C.c_int(), C.c_int()
    L.fkz_deriv_factors(C.byref(f1), C.byref(f2))
    a, b = okz.deriv_factors()
    assert f1.value == int(np.float32(a) * np.float32(65536) + np.float32(0.5))
    assert f2.value == int(np.float32(b) * np.float32(65536) + np.float32(0.5))


def test_fast_oracle_is_frozen(okz, golden):
    g = np.load(os.path.join(golden.dir, "fast_oracle.npz"))
    for name, n, kc in (("left", 3798, 168), ("right", 5169, 248)):
        r = okz.fast_detect_and_compute(golden.lr_u8[name])
        assert len(r.points) == n and r.kcontrast == kc == int(g[name + "_kc"][0])
        for f in ("x", "y", "octave", "response", "size", "angle", "features"):
            assert np.array_equal(r.points[f], g[name + "_pts"][f]), f
        # integer determinants above the fixed threshold 65 (akaze.cpp:559), stored as floats
        resp = r.points["response"]
        assert (resp == np.floor(resp)).all() and (resp > 65).all()


def test_fast_oracle_flat_and_tiny_images(okz):
    flat = np.full((128, 160), 77, np.uint8)
    assert len(okz.fast_detect_and_compute(flat).points) == 0
    r = okz.fast_detect_and_compute(np.zeros((96, 96), np.uint8))
    assert len(r.points) == 0


# ----------------------------------------------------------------- match post-processing
def _brute_knn2(p1, p2, ratio, cross, max_dist):
    f1, f2 = p1["features"], p2["features"]
    d = np.unpackbits(f1[:, None, :] ^ f2[None, :, :], axis=2).sum(axis=2).astype(np.int64)
    out = []
    rev = d.argmin(axis=0)                      # first minimum = smallest query index
    for i in range(len(p1)):
        j1 = int(d[i].argmin())
        d1 = int(d[i, j1])
        rest = np.delete(d[i], j1)
        d2 = int(rest.min()) if rest.size else 512
        ok = d1 < max_dist and d1 * ratio[1] < d2 * ratio[0] and (not cross or rev[j1] == i)
        if ok:
            out.append((i, j1, d1, d2))
    return out


@pytest.mark.parametrize("ratio,cross", [((1, 1), False), ((1, 1), True), ((4, 5), True), ((3, 5), False)])
def test_oracle_knn2_against_numpy_brute_force(okz, ratio, cross):
    from akaze_hip import synth
    p2 = synth.random_descriptors(300, 3, okz.POINT_DTYPE)
    p1 = synth.random_descriptors(260, 4, okz.POINT_DTYPE, planted_from=p2, nplanted=150, maxflip=60)
    p1[7]["features"] = p1[3]["features"]           # duplicate queries: the cross-check keeps only the first
    p2[11]["features"] = p2[5]["features"]          # duplicate train points: d1 == d2 fails the ratio test
    got = okz.match_knn2(p1, p2, ratio, cross)
    want = _brute_knn2(p1, p2, ratio, cross, 96)
    assert [(int(r["query"]), int(r["train"]), int(r["distance"]), int(r["second"])) for r in got] == want
    assert len(want) > 20
    acc = p1["match"] >= 0
    assert acc.sum() == len(got) and np.array_equal(np.nonzero(acc)[0], got["query"])
    assert np.array_equal(p1["match_x"][acc], p2["x"][got["train"]]) and (p1["distance"][~acc] == -1).all()
    assert np.array_equal(got["x1"], p1["x"][got["query"]]) and np.array_equal(got["y2"], p2["y"][got["train"]])


def test_oracle_knn2_edge_cases(okz):
    from akaze_hip import synth
    p1 = synth.random_descriptors(5, 1, okz.POINT_DTYPE)
    assert len(okz.match_knn2(p1, p1[:0].copy())) == 0 and (p1["match"] == -1).all()
    one = p1[:1].copy()
    q = p1.copy()
    got = okz.match_knn2(q, one, cross=False)        # single train point: d2 = 512, query 0 is identical (d1 = 0)
    assert got[0]["query"] == 0 and got[0]["distance"] == 0 and got[0]["second"] == 512
    got = okz.match_knn2(q, one, cross=True)
    assert len(got) == 1


def test_hmax_racy_remainder_is_inert_on_every_fixture(okz, golden):
    """gFindMaxContrastU4's deterministic core is the lattice maximum (what the oracle takes); its racy remainder -- thread 0 of a block
    also compares with eight pixels of the image's top-left tile, which other blocks lower and block (0, 0) raises -- can add at most
    max(grad[0..31][0..31]) (akazed.cu:859-873).  On every input the goldens, the bench and the statistical pin use,
    that bound lies BELOW the lattice maximum: there the reference's hmax is the oracle's exactly, whatever the race does."""
    import os
    from akaze_hip import synth
    from conftest import GOLDEN
    rec = np.load(os.path.join(GOLDEN, "ref_recon_1080p_u8.npz"))
    imgs = [golden.lr_u8["left"], golden.lr_u8["right"], rec["img1"], rec["img2"]]
    for seed in (1, 2, 3, 9, 16):
        imgs += list(synth.pair(1920, 1080, seed))
    for seed in (1, 8):
        imgs += list(synth.pair(1280, 720, seed))
    for u8 in imgs:
        h, w = u8.shape
        p = (w + 127) // 128 * 128
        g = okz.scharr_grad(okz.lowpass(synth.to_float(u8, p), w, 1.0, 2), w)[:, :w]
        lattice = max(np.float32(0.03), g[::16, ::16].max())
        assert g[:32, :32].max() <= lattice, (u8.shape, float(g[:32, :32].max()), float(lattice))
        _, hmax, _ = okz.kcontrast(okz.scharr_grad(okz.lowpass(synth.to_float(u8, p), w, 1.0, 2), w), w, 0.7)
        assert hmax == lattice



def test_constant_image_both_oracles(okz):
    """hmax == 0: hfactor = inf and every bin index is 0 * inf = NaN, which the device cast turns into bin 0 (akazed.cu:924; a C cast is
    undefined there and x86 would index the histogram with INT_MIN) -- no keypoints, no crash, in both pipelines"""
    r = okz.detect_and_compute(np.full((240, 384), 0.25, np.float32), 320)
    assert len(r.points) == 0
    rf = okz.fast_detect_and_compute(np.full((240, 320), 64, np.uint8))
    assert len(rf.points) == 0 and rf.kcontrast == 0

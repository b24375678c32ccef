"""GPU suite: RANSAC homography (hak_find_homography / hak_find_homography_batch, kernels_homography.hip) bit for bit against
its numpy statement tests/homography_ref.py -- every H bit, inliers, hypothesis, refined and every mask byte -- on planted
models, degenerate inputs, ragged batches, the detect -> 2-NN -> RANSAC chain at 1080p and the demo's --homography leg."""
import os
import subprocess

import numpy as np
import pytest

import homography_ref as hr
from conftest import ROOT
from test_homography_cpu import corner_error, planted, synth_warp_H

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from akaze_hip import synth
    return synth


def as_pairs(ah, recs):
    """(n, 4) float32 records -> MATCH_PAIR_DTYPE array (query = index, the other ints fixed)"""
    m = np.zeros(len(recs), ah.MATCH_PAIR_DTYPE)
    m["query"] = np.arange(len(recs))
    m["train"] = np.arange(len(recs))[::-1]
    m["distance"], m["second"] = 17, 40
    for k, f in enumerate(("x1", "y1", "x2", "y2")):
        m[f] = recs[:, k]
    return m


def upload(torch, pairs):
    return torch.from_numpy(np.ascontiguousarray(pairs).view(np.uint8).reshape(-1).copy()).cuda() if len(pairs) else \
        torch.zeros(32, dtype=torch.uint8, device="cuda")


def gpu_single(ah, torch, pairs, iterations, threshold, seed, refine, ctx=None):
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    rec = np.zeros((), ah.HOMOGRAPHY_DTYPE)
    ah.check(ah.lib.hak_find_homography(ctx, d.data_ptr(), n, iterations, threshold, seed, refine, mask.data_ptr(), rec.ctypes.data))
    return rec, mask[:n].cpu().numpy()


def assert_same(got, gmask, want, wmask, what=""):
    assert np.array_equal(got["H"].view(np.uint32), want["H"].view(np.uint32)), (what, got, want)
    for f in ("inliers", "hypothesis", "refined", "n"):
        assert int(got[f]) == int(want[f]), (what, f, got, want)
    assert np.array_equal(gmask, wmask), (what, "mask", int((gmask != wmask).sum()))


def case_records(n, seed, outlier_rate=0.4, nan_rows=True):
    recs, _, _ = planted(n, seed, outlier_rate=outlier_rate, w=1920, h=1080)
    if nan_rows and n >= 10:
        recs[n // 3, 1] = np.nan
        recs[n // 2, 2] = np.inf
    return recs


@pytest.mark.parametrize("n", [0, 3, 4, 5, 63, 64, 65, 1000, 10000, 25000])
def test_single_call_bit_exact(ah, torch, n):
    pairs = as_pairs(ah, case_records(n, 100 + n))
    for k, iters in enumerate((1, 64, 1000, 4096)):
        thr = (1.0, 3.0)[k % 2]
        for refine in (0, 1):
            got, gm = gpu_single(ah, torch, pairs, iters, thr, 11 + k, refine)
            want, wm = hr.find_homography(pairs, iters, thr, 11 + k, bool(refine))
            assert_same(got, gm, want, wm, (n, iters, thr, refine))
            if n >= 1000 and iters >= 1000:
                assert got["hypothesis"] >= 0 and got["refined"] == refine


def test_degenerate_inputs_bit_exact(ah, torch):
    quad = np.array([[0, 0, 10, 5], [100, 0, 112, 4], [100, 80, 108, 90], [0, 80, 9, 83]], np.float32)
    t = np.linspace(0, 500, 200, dtype=np.float32)
    cases = {
        "quad": quad,
        "collinear": np.stack([t, 2 * t + 3, t + np.float32(7) * (t % 3), t * 0.5 + (t % 5)], axis=1).astype(np.float32),
        "duplicates": np.repeat(quad[:3], [70, 70, 60], axis=0),
        "all_nan": np.full((50, 4), np.nan, np.float32),
        "half_nan": np.where(np.arange(300)[:, None] % 2 == 0, np.nan, case_records(300, 5, nan_rows=False)).astype(np.float32),
    }
    for name, recs in cases.items():
        pairs = as_pairs(ah, recs)
        for refine in (0, 1):
            got, gm = gpu_single(ah, torch, pairs, 256, 2.0, 3, refine)
            want, wm = hr.find_homography(pairs, 256, 2.0, 3, bool(refine))
            assert_same(got, gm, want, wm, name)
    got, _ = gpu_single(ah, torch, as_pairs(ah, cases["collinear"]), 256, 2.0, 3, 1)
    assert got["hypothesis"] == -1 and np.array_equal(got["H"], np.eye(3, dtype=np.float32).ravel())


def test_batch_ragged_equals_single_calls(ah, torch, synth):
    """a batch with ragged counts (0, 3, large, clamped to the stride) equals the single calls slot by slot; ctx = NULL equals a
    context; the batch runs asynchronously on the context's stream"""
    stride = 6000
    counts = [0, 3, 5000, 64, 2000, 7000, 700]                          # 7000 > stride: clamped
    np_ = len(counts)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    lists = []
    for k, c in enumerate(counts):
        recs = case_records(stride, 40 + k)
        allp[k * stride:(k + 1) * stride] = as_pairs(ah, recs)
        lists.append(allp[k * stride:k * stride + min(c, stride)].copy())
    w, h = 640, 480
    det = ah.Akazer()
    det.init((w, h, ah.iAlignUp(w, 128)), max_pts=100, batch=2)
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(np_ * ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    for refine in (1, 0):
        ah.check(ah.lib.hak_find_homography_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, 1024, 2.5, 77, refine,
                                                  d_out.data_ptr(), d_mask.data_ptr()))
        ah.check(ah.lib.hak_sync(det.ctx))
        out = d_out.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
        masks = d_mask.cpu().numpy().reshape(np_, stride)
        for k, lst in enumerate(lists):
            n = len(lst)
            s1, m1 = gpu_single(ah, torch, lst, 1024, 2.5, 77, refine)
            s2, m2 = gpu_single(ah, torch, lst, 1024, 2.5, 77, refine, ctx=det.ctx)
            assert_same(out[k], masks[k, :n], s1, m1, ("batch vs single", k))
            assert_same(s2, m2, s1, m1, ("ctx vs NULL", k))
            assert (masks[k, n:] == 0xEE).all()                         # nothing written past the pair's count
            if k == 2:
                want, wm = hr.find_homography(lst, 1024, 2.5, 77, bool(refine))
                assert_same(s1, m1, want, wm, "reference")
    det.close()


def test_end_to_end_1080p_batch(ah, okz, torch, synth):
    """hak_detect_and_compute_batch -> hak_match_knn2_batch -> hak_find_homography_batch on three synth.pair(1920, 1080) seeds:
    equal to the reference on the downloaded lists and within 1 px of synth.warp's map at the corners (1 px threshold; measured
    with the oracle when written: 0.61 / 0.35 / 0.32 px)"""
    w, h = 1920, 1080
    p = ah.iAlignUp(w, 128)
    seeds = (1, 2, 3)
    imgs = []
    for s in seeds:
        imgs += list(synth.pair(w, h, s))
    B = len(imgs)
    mp = 10000
    host = np.stack([synth.to_float(u, p) for u in imgs])
    dimg = torch.from_numpy(host).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=mp, batch=B)
    pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
    num = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
    hom = torch.zeros(B // 2 * ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    masks = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
    ah.check(ah.lib.hak_match_knn2_batch(det.ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()))
    ah.check(ah.lib.hak_find_homography_batch(det.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 1024, 1.0, 0, 1, hom.data_ptr(),
                                              masks.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    cnts = cnt.cpu().numpy()
    lists = out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    recs = hom.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
    mk = masks.cpu().numpy().reshape(B // 2, mp)
    corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    for k in range(B // 2):
        lst = lists[k, :cnts[k]]
        assert len(lst) > 1000
        want, wm = hr.find_homography(lst, 1024, 1.0, 0, True)
        assert_same(recs[k], mk[k, :cnts[k]], want, wm, k)
        assert recs[k]["refined"] == 1 and recs[k]["inliers"] > len(lst) // 2
        assert corner_error(recs[k]["H"], synth_warp_H(w, h), corners) <= 1.0
    det.close()


def test_demo_homography_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --homography` on left/right.pgm: its H, inlier count and mask equal the Python call on the same matches"""
    from test_gpu_dropin import write_pgm
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    r = subprocess.run([DEMO, "0", left, right, "1", "--dump", dump, "--homography"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Homography (RANSAC" in r.stdout
    raw = open(dump, "rb").read()
    off = 0
    for _ in range(2):                                                  # the float and the FAST path's point sections
        n1, n2 = np.frombuffer(raw, np.int32, 2, off)
        off += 8 + 104 * int(n1 + n2)
    n, inl = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    off += 8
    H = np.frombuffer(raw, np.float32, 9, off).copy()
    off += 36
    lst = np.frombuffer(raw, ah.MATCH_PAIR_DTYPE, n, off).copy()
    off += 32 * n
    mask = np.frombuffer(raw, np.uint8, n, off).copy()
    assert off + n == len(raw) and n > 100
    got, gm = ah.findHomography(lst)
    assert np.array_equal(H.view(np.uint32), got["H"].view(np.uint32)) and inl == got["inliers"] and np.array_equal(mask, gm)
    want, wm = hr.find_homography(lst, 1024, 3.0, 0, True)
    assert_same(got, gm, want, wm, "demo")
    assert inl > n // 2


def test_randomised_parity(ah, torch):
    """~200 seeded cases: sizes, outlier rates, NaN rows, iterations, thresholds, seeds, refine"""
    rng = np.random.default_rng(2026)
    fails = []
    for c in range(200):
        n = int(rng.choice([int(rng.integers(0, 12)), int(rng.integers(12, 300)), int(rng.integers(300, 4000))]))
        recs = case_records(n, 1000 + c, outlier_rate=float(rng.uniform(0.0, 0.9)), nan_rows=bool(rng.integers(0, 2)))
        if n and rng.random() < 0.2:                                    # a share of exact duplicates
            recs[rng.integers(0, n, n // 4)] = recs[0]
        iters = int(rng.choice([1, 7, 64, 100, 256, 513, 1024]))
        thr = float(np.float32(rng.uniform(0.2, 8.0)))
        seed = int(rng.integers(0, 2**32))
        refine = int(rng.integers(0, 2))
        pairs = as_pairs(ah, recs)
        got, gm = gpu_single(ah, torch, pairs, iters, thr, seed, refine)
        want, wm = hr.find_homography(pairs, iters, thr, seed, bool(refine))
        try:
            assert_same(got, gm, want, wm, c)
        except AssertionError as e:
            fails.append(str(e)[:300])
    assert not fails, f"{len(fails)} of 200 differ: " + "; ".join(fails[:3])


def test_randomised_families(ah, torch):
    """the cases of test_homography_cpu.all_parity_cases -- 150 drawn from six scene families (planted projective, similarity,
    integer lattice at unit and coarse spacing, mirrored image 2, a model whose wz = 0 line crosses the cloud, collinear), with
    outliers, NaN / inf rows, duplicates up to all-equal, coordinates scaled by 2^-20 .. 2^20 and offset by +-16000, n from 0,
    iterations 1 .. 257, thresholds 0.2 .. 8, seeds 0 and 0xFFFFFFFF, plus the hand-made singular refits -- record and mask byte for
    byte against the statement with the refit off and on, with and without a context; every third block of eight also as one
    ragged hak_find_homography_batch call per refit setting.  What the cases reach (no model, ties, refit accepted / rejected / singular, records
    behind the wz = 0 line, samples the orientation test rejects) is asserted in test_homography_cpu.py."""
    from test_homography_cpu import all_parity_cases
    fails = []
    cases = all_parity_cases()
    det = ah.Akazer()
    det.init((256, 192, 256), max_pts=500, batch=2)
    wants = []
    for k, c in enumerate(cases):
        pairs = as_pairs(ah, c["recs"])
        wants.append({})
        for refine in (0, 1):
            want, wm = wants[k][refine] = hr.find_homography(pairs, c["iterations"], c["threshold"], c["seed"], bool(refine))
            got, gm = gpu_single(ah, torch, pairs, c["iterations"], c["threshold"], c["seed"], refine, ctx=det.ctx if c["ctx"] else None)
            try:
                assert_same(got, gm, want, wm, (k, c["scene"], refine))
            except AssertionError as e:
                fails.append(str(e)[:300])
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    for g in groups:
        ks = [k for k, c in enumerate(cases) if c["group"] == g]
        c0 = cases[ks[0]]
        stride = max(1, max(len(cases[k]["recs"]) for k in ks))
        allp = np.zeros(len(ks) * stride, ah.MATCH_PAIR_DTYPE)
        for f in ("x1", "y1", "x2", "y2"):
            allp[f] = np.nan                                            # records past a pair's count are not the call's business
        for slot, k in enumerate(ks):
            allp[slot * stride:slot * stride + len(cases[k]["recs"])] = as_pairs(ah, cases[k]["recs"])
        d = upload(torch, allp)
        d_cnt = torch.tensor([len(cases[k]["recs"]) for k in ks], dtype=torch.int32, device="cuda")
        for refine in (0, 1):
            d_out = torch.zeros(len(ks) * ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_mask = torch.full((len(ks) * stride,), 0xEE, dtype=torch.uint8, device="cuda")
            ah.check(ah.lib.hak_find_homography_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), len(ks), c0["iterations"],
                                                      c0["threshold"], c0["seed"], refine, d_out.data_ptr(), d_mask.data_ptr()))
            ah.check(ah.lib.hak_sync(det.ctx))
            out = d_out.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
            masks = d_mask.cpu().numpy().reshape(len(ks), stride)
            for slot, k in enumerate(ks):
                n = len(cases[k]["recs"])
                want, wm = wants[k][refine]
                try:
                    assert_same(out[slot], masks[slot, :n], want, wm, ("batch", g, k, refine))
                    assert (masks[slot, n:] == 0xEE).all(), ("batch", g, k, "written past the count")
                except AssertionError as e:
                    fails.append(str(e)[:300])
    det.close()
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_bad_arguments(ah, torch):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    rec = np.zeros((), ah.HOMOGRAPHY_DTYPE)
    lib = ah.lib
    assert lib.hak_find_homography(None, d.data_ptr() + 4, 10, 64, 3.0, 0, 1, None, rec.ctypes.data) != 0     # misaligned
    assert lib.hak_find_homography(None, d.data_ptr(), -1, 64, 3.0, 0, 1, None, rec.ctypes.data) != 0
    assert lib.hak_find_homography(None, d.data_ptr(), 10, 64, -1.0, 0, 1, None, rec.ctypes.data) != 0
    assert lib.hak_find_homography(None, d.data_ptr(), 10, 64, 3.0, 0, 1, None, None) != 0
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.hak_find_homography_batch(None, d.data_ptr(), 64, cnt.data_ptr(), 1, 64, 3.0, 0, 1, d.data_ptr(), None) != 0

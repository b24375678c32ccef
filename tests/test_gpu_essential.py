"""GPU suite: five-point RANSAC essential matrix (hak_find_essential / hak_find_essential_batch, kernels_essential.hip) bit for bit
against its numpy statement tests/essential_ref.py -- every F bit, inliers, hypothesis, root, n and every mask byte -- on planted
two-view scenes, bad records, ragged batches, the detect -> 2-NN -> essential -> pose -> pose refit chain, the Python wrapper, the
demo's --essential leg and the committed randomised cases."""
import os
import subprocess

import numpy as np
import pytest

import essential_ref as er
from conftest import ROOT
from test_essential_cpu import PARITY_CASES, parity_case
from test_gpu_fundamental import as_pairs, assert_same, det, synth, torch, upload  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
SIZES = [0, 4, 5, 6, 63, 64, 65, 1023, 1024, 1025, 2500]               # n < 5, the first usable size, wave and LDS chunk edges
ITERATIONS = [1, 5, 6, 7, 11, 12, 13, 85, 86, 255, 256, 257, 1024]     # six hypotheses per wave; score blocks in virtual hypotheses
SEEDS = [0, 1, 0xFFFFFFFF]
K_A = (1500.0, 1500.0, 960.0, 540.0)                                    # two_view_matches' camera
K_B = (1480.0, 1530.0, 950.5, 548.25)                                   # a second one, fx != fy


def gpu_single(ah, torch, pairs, K1, K2, iterations, threshold, seed, ctx=None, with_mask=True):
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    k1, k2 = ah.intrinsics(K1), ah.intrinsics(K2)
    ah.check(ah.lib.hak_find_essential(ctx, d.data_ptr(), n, k1.ctypes.data, k2.ctypes.data, iterations, threshold, seed,
                                       mask.data_ptr() if with_mask else None, rec.ctypes.data))
    return rec, mask[:n].cpu().numpy()


def scene(synth, n, seed):
    """n records: 70 % planted two-view inliers with 0.3 px Gaussian noise, the rest uniformly random"""
    n_in = n * 7 // 10
    return synth.two_view_matches(n_in, n - n_in, seed, noise=0.3)[0]


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, n):
    pairs = as_pairs(ah, scene(synth, n, 100 + n))
    for k, iters in enumerate(ITERATIONS):
        seed = SEEDS[(k + n) % 3]
        thr = (1.0, 2.5)[k % 2]
        K2 = (K_A, K_B)[k % 2]
        got, gm = gpu_single(ah, torch, pairs, K_A, K2, iters, thr, seed)
        want, wm = er.find_essential(pairs, K_A, K2, iters, thr, seed)
        assert_same(got, gm, want, wm, (n, iters, thr, seed))
        if n >= 1023 and iters >= 255 and K2 == K_A:
            assert got["hypothesis"] >= 0 and got["inliers"] >= n // 2 and 16 <= got["root"] <= 25
        if n < 5:
            assert got["hypothesis"] == -1 and not got["F"].any() and not gm.any() and got["root"] == 0


def test_bad_and_duplicate_records_bit_exact(ah, torch, synth):
    base = scene(synth, 600, 9)
    nan = base.copy()
    nan[::5, 0] = np.nan
    nan[3::11, 3] = np.inf
    nan[7::13, 2] = -np.inf
    nan[1::17, 1] = np.nan
    sparse = np.full((40, 4), np.nan, np.float32)
    sparse[[1, 5, 11, 33]] = base[:4]
    cases = {
        "nan_inf": nan,
        "all_nan": np.full((50, 4), np.nan, np.float32),
        "four_finite": sparse,
        "five_copies": np.tile(base[:1], (5, 1)),
        "duplicates": np.repeat(base[:7], 30, axis=0),                  # 210 records, seven distinct
        "few_distinct": np.repeat(base[:4], 40, axis=0),                # four distinct: every sample repeats a point
    }
    for name, recs in cases.items():
        pairs = as_pairs(ah, recs)
        for seed in SEEDS:
            got, gm = gpu_single(ah, torch, pairs, K_A, K_A, 256, 1.0, seed)
            want, wm = er.find_essential(pairs, K_A, K_A, 256, 1.0, seed)
            assert_same(got, gm, want, wm, (name, seed))
        if name in ("all_nan", "four_finite", "five_copies"):
            assert got["hypothesis"] == -1 and not gm.any()
    got, gm = gpu_single(ah, torch, as_pairs(ah, nan), K_A, K_A, 256, 1.0, 0)
    assert got["hypothesis"] >= 0 and not gm[~np.isfinite(nan).all(axis=1)].any()


def test_null_context_and_null_mask(ah, torch, synth, det):
    for n in (6, 700, 1500):
        pairs = as_pairs(ah, scene(synth, n, 30 + n))
        a, am = gpu_single(ah, torch, pairs, K_A, K_B, 300, 1.0, 5)
        b, bm = gpu_single(ah, torch, pairs, K_A, K_B, 300, 1.0, 5, ctx=det.ctx)
        assert_same(b, bm, a, am, ("ctx vs NULL", n))
        for ctx in (None, det.ctx):
            c, cm = gpu_single(ah, torch, pairs, K_A, K_B, 300, 1.0, 5, ctx=ctx, with_mask=False)
            assert c.tobytes() == a.tobytes() and (cm == 0xEE).all()    # d_mask = NULL: the record is unchanged


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    """counts {0, 3, 5, 900, stride + 50} at stride 1100: every record and mask equals the single call on the same list, the bytes
    of a mask beyond a pair's count stay untouched, d_masks = NULL works; asynchronous on the context's stream"""
    stride = 1100
    counts = [0, 3, 5, 900, stride + 50]
    np_ = len(counts)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    lists = []
    for k, c in enumerate(counts):
        allp[k * stride:(k + 1) * stride] = as_pairs(ah, scene(synth, stride, 40 + k))
        lists.append(allp[k * stride:k * stride + min(c, stride)].copy())
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    k1, k2 = ah.intrinsics(K_A), ah.intrinsics(K_B)
    singles = [gpu_single(ah, torch, lst, K_A, K_B, 1024, 1.0, 77) for lst in lists]
    want, wm = er.find_essential(lists[3], K_A, K_B, 1024, 1.0, 77)
    assert_same(singles[3][0], singles[3][1], want, wm, "reference")
    for with_masks in (True, False):
        d_out = torch.zeros(np_ * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
        ah.check(ah.lib.hak_find_essential_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, k1.ctypes.data, k2.ctypes.data, 1024,
                                                 1.0, 77, d_out.data_ptr(), d_mask.data_ptr() if with_masks else None))
        ah.check(ah.lib.hak_sync(det.ctx))
        out = d_out.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
        masks = d_mask.cpu().numpy().reshape(np_, stride)
        for k, lst in enumerate(lists):
            n = len(lst)
            s, m = singles[k]
            if with_masks:
                assert_same(out[k], masks[k, :n], s, m, ("batch vs single", k))
                assert (masks[k, n:] == 0xEE).all()                     # nothing written past the pair's count
            else:
                assert out[k].tobytes() == s.tobytes() and (masks[k] == 0xEE).all()
    assert out[4]["n"] == stride and out[0]["hypothesis"] == -1 and out[1]["hypothesis"] == -1 and out[2]["n"] == 5


def test_chain_detect_match_essential_pose(ah, torch, synth):
    """hak_detect_and_compute_batch -> hak_match_knn2_batch -> hak_find_essential_batch -> hak_recover_pose_batch ->
    hak_refine_pose_batch on two synth pairs at 256 x 192 with no host synchronisation in between: equal to the single calls on
    the downloaded lists, and the essential record to the statement"""
    w, h = 256, 192
    p = ah.iAlignUp(w, 128)
    imgs = []
    for s in (1, 2):
        imgs += list(synth.pair(w, h, s))
    B, mp = len(imgs), 1000
    K = ah.intrinsics((300.0, 310.0, 128.0, 96.0))
    kp = K.ctypes.data
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    dt = ah.Akazer()
    dt.init((w, h, p), max_pts=mp, batch=B)
    pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
    num = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
    ess = torch.zeros(B // 2 * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    masks = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
    pose = torch.zeros(B // 2 * ah.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    pmask = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
    xyz = torch.zeros(B // 2 * mp * 3, dtype=torch.float32, device="cuda")
    lib = ah.lib
    ah.check(lib.hak_detect_and_compute_batch(dt.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
    ah.check(lib.hak_match_knn2_batch(dt.ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()))
    ah.check(lib.hak_find_essential_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, kp, kp, 256, 1.0, 0, ess.data_ptr(),
                                          masks.data_ptr()))
    ah.check(lib.hak_recover_pose_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, ess.data_ptr(), kp, kp, 1.0, 50.0,
                                        pose.data_ptr(), pmask.data_ptr(), xyz.data_ptr()))
    mid = torch.zeros_like(pose)
    mid.copy_(pose)                                                     # (a device copy on the same stream order; no host sync)
    ah.check(lib.hak_refine_pose_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, kp, kp, 2.0, 50.0, 3, pose.data_ptr(),
                                       pmask.data_ptr(), xyz.data_ptr()))
    ah.check(lib.hak_sync(dt.ctx))
    cnts = cnt.cpu().numpy()
    lists = out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    recs = ess.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
    mk = masks.cpu().numpy().reshape(B // 2, mp)
    poses = pose.cpu().numpy().view(ah.POSE_DTYPE)
    pm = pmask.cpu().numpy().reshape(B // 2, mp)
    for k in range(B // 2):
        lst = lists[k, :cnts[k]].copy()
        assert len(lst) >= 5
        s, m = gpu_single(ah, torch, lst, K, K, 256, 1.0, 0)
        assert_same(recs[k], mk[k, :cnts[k]], s, m, k)
        want, wm = er.find_essential(lst, K, K, 256, 1.0, 0)
        assert_same(s, m, want, wm, ("reference", k))
        assert recs[k]["hypothesis"] >= 0 and recs[k]["inliers"] > len(lst) // 2
        p0, m0, _ = ah.recoverPose(lst, s, K, None, 1.0, 50.0)
        p1, m1, _ = ah.refinePose(lst, K, p0, None, 2.0, 50.0, 3)
        assert poses[k].tobytes() == p1.tobytes() and np.array_equal(pm[k, :cnts[k]], m1)
    dt.close()


def test_python_wrapper(ah, torch, synth):
    pairs = as_pairs(ah, scene(synth, 500, 4))
    got, gm = ah.findEssential(pairs, K_A, K_B, 256, 1.0, 3)
    want, wm = er.find_essential(pairs, K_A, K_B, 256, 1.0, 3)
    assert got.dtype == ah.FUNDAMENTAL_DTYPE
    assert_same(got, gm, want, wm, "wrapper")
    dev, dm = ah.findEssential(upload(torch, pairs), K_A, K_B, 256, 1.0, 3)      # a device tensor is used in place
    assert_same(dev, dm, want, wm, "wrapper, device list")
    one, om = ah.findEssential(pairs, np.array([[1500.0, 0, 960], [0, 1500, 540], [0, 0, 1]]), None, 256, 1.0, 3)
    want1, wm1 = er.find_essential(pairs, K_A, None, 256, 1.0, 3)
    assert_same(one, om, want1, wm1, "wrapper, K2 omitted")


def test_demo_essential_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --essential FX FY CX CY --pose FX FY CX CY --epipolar 3` on left/right.pgm: its F, inlier count and mask equal
    the Python call on the same matches, the pose leg behind it runs on that F (the dumped record equals recoverPose on it), and
    the epipolar leg re-matches under that F and estimates the essential matrix of the new list"""
    from test_gpu_dropin import write_pgm
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    h, w = golden.lr_u8["left"].shape
    K = (1.2 * w, 1.2 * w, w / 2.0, h / 2.0)
    ks = [repr(float(v)) for v in K]
    r = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--essential", *ks, "--pose", *ks, "--epipolar", "3"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Essential matrix as F (RANSAC" in r.stdout and "Fundamental matrix (RANSAC" not in r.stdout
    assert "Relative pose from the fundamental matrix" in r.stdout
    assert "Essential matrix of the epipolar matches: " in r.stdout and "Fundamental matrix of the epipolar matches" not in r.stdout
    raw = open(dump, "rb").read()
    off = 0
    for _ in range(2):                                                  # the float and the FAST path's point sections
        n1, n2 = np.frombuffer(raw, np.int32, 2, off)
        off += 8 + 104 * int(n1 + n2)
    n, inl = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    off += 8
    F = np.frombuffer(raw, np.float32, 9, off).copy()
    off += 36
    lst = np.frombuffer(raw, ah.MATCH_PAIR_DTYPE, n, off).copy()
    off += 32 * n
    mask = np.frombuffer(raw, np.uint8, n, off).copy()
    off += n
    pose = np.frombuffer(raw, ah.POSE_DTYPE, 1, off)[0]
    off += 64
    front = np.frombuffer(raw, np.uint8, n, off).copy()
    assert off + n + 12 * n == len(raw) and n > 100
    got, gm = ah.findEssential(lst, K)
    assert np.array_equal(F.view(np.uint32), got["F"].view(np.uint32)) and inl == got["inliers"] and np.array_equal(mask, gm)
    want, wm = er.find_essential(lst, K, None, 1024, 1.0, 0)
    assert_same(got, gm, want, wm, "demo")
    p0, m0, _ = ah.recoverPose(lst, got, K)
    assert pose.tobytes() == p0.tobytes() and np.array_equal(front, m0) and pose["candidate"] >= 0


def test_randomised_parity(ah, torch, det):
    """the committed cases of test_essential_cpu.parity_case -- sizes from 0 to 3000, seven scene families, outliers, NaN / inf rows,
    duplicates up to all-equal, intrinsics from fx = 300 to 3000 with fx != fy and K1 != K2, seeds 0 and 0xFFFFFFFF -- record and mask
    byte for byte against the statement, with and without a context; every third block of eight also as one ragged
    hak_find_essential_batch call.  What the cases reach is asserted in test_essential_cpu.py."""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    wants = []
    for k, c in enumerate(cases):
        pairs = as_pairs(ah, c["recs"])
        want, wm = er.find_essential(pairs, c["K1"], c["K2"], c["iterations"], c["threshold"], c["seed"])
        wants.append((want, wm))
        got, gm = gpu_single(ah, torch, pairs, c["K1"], c["K2"], c["iterations"], c["threshold"], c["seed"], ctx=det.ctx if c["ctx"] else None)
        try:
            assert_same(got, gm, want, wm, (k, c["scene"]))
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
        d_out = torch.zeros(len(ks) * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_mask = torch.full((len(ks) * stride,), 0xEE, dtype=torch.uint8, device="cuda")
        k1, k2 = ah.intrinsics(c0["K1"]), ah.intrinsics(c0["K2"])
        ah.check(ah.lib.hak_find_essential_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), len(ks), k1.ctypes.data, k2.ctypes.data,
                                                 c0["iterations"], c0["threshold"], c0["seed"], d_out.data_ptr(), d_mask.data_ptr()))
        ah.check(ah.lib.hak_sync(det.ctx))
        out = d_out.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
        masks = d_mask.cpu().numpy().reshape(len(ks), stride)
        for slot, k in enumerate(ks):
            n = len(cases[k]["recs"])
            try:
                assert_same(out[slot], masks[slot, :n], wants[k][0], wants[k][1], ("batch", g, k))
                assert (masks[slot, n:] == 0xEE).all(), ("batch", g, k, "written past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 4
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    K = ah.intrinsics(K_A)
    bad = K.copy()
    bad["fy"] = 0.0
    lib, out, k, b = ah.lib, rec.ctypes.data, K.ctypes.data, bad.ctypes.data
    assert lib.hak_find_essential(None, d.data_ptr() + 4, 10, k, k, 64, 1.0, 0, None, out) != 0      # misaligned
    assert lib.hak_find_essential(None, d.data_ptr(), -1, k, k, 64, 1.0, 0, None, out) != 0
    assert lib.hak_find_essential(None, d.data_ptr(), 10, k, k, 0, 1.0, 0, None, out) != 0
    assert lib.hak_find_essential(det.ctx, d.data_ptr(), 10, k, k, 64, -1.0, 0, None, out) != 0
    assert lib.hak_find_essential(det.ctx, d.data_ptr(), 10, k, k, 64, 1.0, 0, None, None) != 0
    assert lib.hak_find_essential(det.ctx, d.data_ptr(), 10, None, k, 64, 1.0, 0, None, out) != 0
    assert lib.hak_find_essential(det.ctx, d.data_ptr(), 10, k, b, 64, 1.0, 0, None, out) != 0
    batch = lib.hak_find_essential_batch
    assert batch(None, d.data_ptr(), 64, cnt.data_ptr(), 1, k, k, 64, 1.0, 0, d.data_ptr(), None) != 0      # no context
    assert batch(det.ctx, d.data_ptr(), 64, None, 1, k, k, 64, 1.0, 0, d.data_ptr(), None) != 0             # no counts
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, k, k, 64, 1.0, 0, None, None) != 0           # no d_out
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 0, k, k, 64, 1.0, 0, d.data_ptr(), None) != 0   # npairs < 1
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, k, k, 65537, 1.0, 0, d.data_ptr(), None) != 0
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, k, k, 64, float("nan"), 0, d.data_ptr(), None) != 0
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, b, k, 64, 1.0, 0, d.data_ptr(), None) != 0
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, k, None, 64, 1.0, 0, d.data_ptr(), None) != 0
    assert lib.hak_last_error().decode() != ""

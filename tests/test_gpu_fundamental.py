"""GPU suite: RANSAC fundamental matrix (hak_find_fundamental / hak_find_fundamental_batch, kernels_fundamental.hip) bit for bit
against its numpy statement tests/fundamental_ref.py -- every F bit, inliers, hypothesis, root, n and every mask byte -- on
planted two-view scenes, the golden pair's matches, bad records, ragged batches, the detect -> 2-NN -> RANSAC chain, the Python
wrapper and the demo's --fundamental leg."""
import os
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
from conftest import ROOT
from test_fundamental_cpu import GOLDEN_INLIERS, GOLDEN_SEED, PARITY_CASES, golden_records, parity_case

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
SIZES = [0, 6, 7, 8, 63, 64, 65, 1023, 1024, 1025, 2500]               # n < 7, the first usable size, wave and LDS chunk edges
ITERATIONS = [1, 15, 16, 17, 255, 256, 257, 1024]                       # block and slot boundaries
SEEDS = [0, 1, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from akaze_hip import synth
    return synth


@pytest.fixture(scope="module")
def det(ah, torch):
    """a small context for the calls that take one"""
    d = ah.Akazer()
    d.init((256, 192, 256), max_pts=2000, batch=4)
    yield d
    d.close()


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


def gpu_single(ah, torch, pairs, iterations, threshold, seed, ctx=None, with_mask=True):
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    ah.check(ah.lib.hak_find_fundamental(ctx, d.data_ptr(), n, iterations, threshold, seed, mask.data_ptr() if with_mask else None,
                                         rec.ctypes.data))
    return rec, mask[:n].cpu().numpy()


def assert_same(got, gmask, want, wmask, what=""):
    assert np.array_equal(got["F"].view(np.uint32), want["F"].view(np.uint32)), (what, got, want)
    for f in ("inliers", "hypothesis", "root", "n"):
        assert int(got[f]) == int(want[f]), (what, f, got, want)
    assert np.array_equal(gmask, wmask), (what, "mask", int((gmask != wmask).sum()))


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
        got, gm = gpu_single(ah, torch, pairs, iters, thr, seed)
        want, wm = fr.find_fundamental(pairs, iters, thr, seed)
        assert_same(got, gm, want, wm, (n, iters, thr, seed))
        if n >= 1023 and iters >= 255:
            assert got["hypothesis"] >= 0 and got["inliers"] >= n // 2
        if n < 7:
            assert got["hypothesis"] == -1 and not got["F"].any() and not gm.any()


@pytest.mark.parametrize("seed", SEEDS)
def test_golden_pair_bit_exact(ah, torch, seed):
    pairs = as_pairs(ah, golden_records())
    got, gm = gpu_single(ah, torch, pairs, 1024, 1.0, seed)
    want, wm = fr.find_fundamental(pairs, 1024, 1.0, seed)
    assert_same(got, gm, want, wm, seed)
    if seed == GOLDEN_SEED:
        assert got["inliers"] == GOLDEN_INLIERS


def test_bad_and_duplicate_records_bit_exact(ah, torch, synth):
    base = scene(synth, 600, 9)
    nan = base.copy()
    nan[::5, 0] = np.nan
    nan[3::11, 3] = np.inf
    nan[7::13, 2] = -np.inf
    nan[1::17, 1] = np.nan
    one = np.tile(base[:1], (7, 1))
    sparse = np.full((40, 4), np.nan, np.float32)
    sparse[[1, 5, 11, 20, 33, 39]] = base[:6]
    cases = {
        "nan_inf": nan,
        "all_nan": np.full((50, 4), np.nan, np.float32),
        "six_finite": sparse,
        "seven_copies": one,
        "duplicates": np.repeat(base[:9], 30, axis=0),                  # 270 records, nine distinct
        "few_distinct": np.repeat(base[:5], 40, axis=0),                # five distinct: every sample repeats a point
    }
    for name, recs in cases.items():
        pairs = as_pairs(ah, recs)
        for seed in SEEDS:
            got, gm = gpu_single(ah, torch, pairs, 256, 1.0, seed)
            want, wm = fr.find_fundamental(pairs, 256, 1.0, seed)
            assert_same(got, gm, want, wm, (name, seed))
        if name in ("all_nan", "six_finite", "seven_copies"):
            assert got["hypothesis"] == -1 and not gm.any()
    got, gm = gpu_single(ah, torch, as_pairs(ah, nan), 256, 1.0, 0)
    assert got["hypothesis"] >= 0 and not gm[~np.isfinite(nan).all(axis=1)].any()


def test_null_context_and_null_mask(ah, torch, synth, det):
    for n in (8, 700, 1500):
        pairs = as_pairs(ah, scene(synth, n, 30 + n))
        a, am = gpu_single(ah, torch, pairs, 300, 1.0, 5)
        b, bm = gpu_single(ah, torch, pairs, 300, 1.0, 5, ctx=det.ctx)
        assert_same(b, bm, a, am, ("ctx vs NULL", n))
        for ctx in (None, det.ctx):
            c, cm = gpu_single(ah, torch, pairs, 300, 1.0, 5, ctx=ctx, with_mask=False)
            assert c.tobytes() == a.tobytes() and (cm == 0xEE).all()    # d_mask = NULL: the record is unchanged


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    """counts {0, 3, 7, 900, stride + 50} at stride 1100: every record and mask equals the single call on the same list, the bytes
    of a mask beyond a pair's count stay untouched, d_masks = NULL works; asynchronous on the context's stream"""
    stride = 1100
    counts = [0, 3, 7, 900, stride + 50]
    np_ = len(counts)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    lists = []
    for k, c in enumerate(counts):
        allp[k * stride:(k + 1) * stride] = as_pairs(ah, scene(synth, stride, 40 + k))
        lists.append(allp[k * stride:k * stride + min(c, stride)].copy())
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    singles = [gpu_single(ah, torch, lst, 1024, 1.0, 77) for lst in lists]
    want, wm = fr.find_fundamental(lists[3], 1024, 1.0, 77)
    assert_same(singles[3][0], singles[3][1], want, wm, "reference")
    for with_masks in (True, False):
        d_out = torch.zeros(np_ * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
        ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, 1024, 1.0, 77,
                                                   d_out.data_ptr(), d_mask.data_ptr() if with_masks else None))
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
    assert out[4]["n"] == stride and out[0]["hypothesis"] == -1 and out[1]["hypothesis"] == -1


def test_chain_detect_match_fundamental(ah, torch, synth):
    """hak_detect_and_compute_batch -> hak_match_knn2_batch -> hak_find_fundamental_batch on two synth pairs at 256 x 192 with no
    host synchronisation in between: equal to the single calls on the downloaded lists"""
    w, h = 256, 192
    p = ah.iAlignUp(w, 128)
    imgs = []
    for s in (1, 2):
        imgs += list(synth.pair(w, h, s))
    B, mp = len(imgs), 1000
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    dt = ah.Akazer()
    dt.init((w, h, p), max_pts=mp, batch=B)
    pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
    num = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
    fund = torch.zeros(B // 2 * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    masks = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
    ah.check(ah.lib.hak_detect_and_compute_batch(dt.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
    ah.check(ah.lib.hak_match_knn2_batch(dt.ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()))
    ah.check(ah.lib.hak_find_fundamental_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 256, 1.0, 0, fund.data_ptr(),
                                               masks.data_ptr()))
    ah.check(ah.lib.hak_sync(dt.ctx))
    cnts = cnt.cpu().numpy()
    lists = out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    recs = fund.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
    mk = masks.cpu().numpy().reshape(B // 2, mp)
    for k in range(B // 2):
        lst = lists[k, :cnts[k]].copy()
        assert len(lst) >= 7
        s, m = gpu_single(ah, torch, lst, 256, 1.0, 0)
        assert_same(recs[k], mk[k, :cnts[k]], s, m, k)
        want, wm = fr.find_fundamental(lst, 256, 1.0, 0)
        assert_same(s, m, want, wm, ("reference", k))
        assert recs[k]["hypothesis"] >= 0 and recs[k]["inliers"] > len(lst) // 2
    dt.close()


def test_python_wrapper(ah, torch, synth):
    pairs = as_pairs(ah, scene(synth, 500, 4))
    got, gm = ah.findFundamental(pairs, 256, 1.0, 3)
    want, wm = fr.find_fundamental(pairs, 256, 1.0, 3)
    assert got.dtype == ah.FUNDAMENTAL_DTYPE
    assert_same(got, gm, want, wm, "wrapper")
    dev, dm = ah.findFundamental(upload(torch, pairs), 256, 1.0, 3)     # a device tensor is used in place
    assert_same(dev, dm, want, wm, "wrapper, device list")


def test_demo_fundamental_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --fundamental` on left/right.pgm: its F, inlier count and mask equal the Python call on the same matches"""
    from test_gpu_dropin import write_pgm
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    r = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--fundamental"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fundamental matrix (RANSAC" in r.stdout and "Homography (RANSAC" not in r.stdout
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
    assert off + n == len(raw) and n > 100
    got, gm = ah.findFundamental(lst)
    assert np.array_equal(F.view(np.uint32), got["F"].view(np.uint32)) and inl == got["inliers"] and np.array_equal(mask, gm)
    want, wm = fr.find_fundamental(lst, 1024, 1.0, 0)
    assert_same(got, gm, want, wm, "demo")
    assert inl > n // 2


def test_randomised_parity(ah, torch, det):
    """the 150 seeded cases of test_fundamental_cpu.parity_case -- sizes from 0 to 3000, five scene families (general, planar,
    pure translation, integer lattice, collinear), outliers, NaN / inf rows, duplicates up to all-equal, coordinates scaled by
    2^-20 .. 2^20 and offset by +-16000, iterations, thresholds, seeds 0 and 0xFFFFFFFF -- record and mask byte for byte against
    the statement, with and without a context; every third block of eight also as one ragged hak_find_fundamental_batch call.
    What the cases reach (ties, later roots, no model, one- and three-root cubics) is asserted in test_fundamental_cpu.py.
    Measured on an MI355X box: 0.4 s, most of it the numpy statement."""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    wants = []
    for k, c in enumerate(cases):
        pairs = as_pairs(ah, c["recs"])
        want, wm = fr.find_fundamental(pairs, c["iterations"], c["threshold"], c["seed"])
        wants.append((want, wm))
        got, gm = gpu_single(ah, torch, pairs, c["iterations"], c["threshold"], c["seed"], ctx=det.ctx if c["ctx"] else None)
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
        ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), len(ks), c0["iterations"], c0["threshold"],
                                                   c0["seed"], d_out.data_ptr(), d_mask.data_ptr()))
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
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    lib, out = ah.lib, rec.ctypes.data
    assert lib.hak_find_fundamental(None, d.data_ptr() + 4, 10, 64, 1.0, 0, None, out) != 0          # misaligned
    assert lib.hak_find_fundamental(None, d.data_ptr(), -1, 64, 1.0, 0, None, out) != 0
    assert lib.hak_find_fundamental(None, d.data_ptr(), 10, 0, 1.0, 0, None, out) != 0
    assert lib.hak_find_fundamental(det.ctx, d.data_ptr(), 10, 64, -1.0, 0, None, out) != 0
    assert lib.hak_find_fundamental(det.ctx, d.data_ptr(), 10, 64, 1.0, 0, None, None) != 0
    batch = lib.hak_find_fundamental_batch
    assert batch(None, d.data_ptr(), 64, cnt.data_ptr(), 1, 64, 1.0, 0, d.data_ptr(), None) != 0      # no context
    assert batch(det.ctx, d.data_ptr(), 64, None, 1, 64, 1.0, 0, d.data_ptr(), None) != 0             # no counts
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 64, 1.0, 0, None, None) != 0           # no d_out
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 0, 64, 1.0, 0, d.data_ptr(), None) != 0   # npairs < 1
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 65537, 1.0, 0, d.data_ptr(), None) != 0
    assert batch(det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 64, float("nan"), 0, d.data_ptr(), None) != 0
    assert lib.hak_last_error().decode() != ""

"""GPU suite: rank-2 refit of the fundamental matrix (hak_refine_fundamental / hak_refine_fundamental_batch,
kernels_fundrefit.hip) bit for bit against its numpy statement tests/fundamental_refit_ref.py -- every F bit, inliers,
hypothesis, root, n and every mask byte.  The inputs are the STATEMENT's RANSAC records (fundamental_ref), so the device's own
RANSAC can neither mask nor cause a difference."""
import os
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
from conftest import ROOT
from test_fundamental_cpu import PARITY_CASES, parity_case
from test_gpu_fundamental import as_pairs, assert_same, det, scene, synth, torch, upload  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
SIZES = [0, 7, 8, 9, 63, 64, 65, 129, 1025]         # the first usable inlier count, the wave edges of the summation order
ROUNDS = [1, 3, 8]


def gpu_refine(ah, torch, pairs, record, threshold, rounds, ctx=None, with_mask=True):
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    rec = np.array(record, ah.FUNDAMENTAL_DTYPE).reshape(())
    ah.check(ah.lib.hak_refine_fundamental(ctx, d.data_ptr(), n, threshold, rounds, mask.data_ptr() if with_mask else None,
                                           rec.ctypes.data))
    return rec, mask[:n].cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    pairs = as_pairs(ah, scene(synth, n, 100 + n))
    refined = 0
    for thr in (1.0, 2.5):
        rec0, _ = fr.find_fundamental(pairs, 256, thr, n)
        for rounds in ROUNDS:
            want, wm = rr.refine_fundamental(pairs, rec0, thr, rounds)
            for ctx in (None, det.ctx):
                got, gm = gpu_refine(ah, torch, pairs, rec0, thr, rounds, ctx=ctx)
                assert_same(got, gm, want, wm, (n, thr, rounds, ctx is not None))
            got, gm = gpu_refine(ah, torch, pairs, rec0, thr, rounds, with_mask=False)
            assert got.tobytes() == want.tobytes() and (gm == 0xEE).all()   # d_mask = NULL: same record, buffer untouched
            refined += int(want["root"]) == 3
    if n < 7:
        assert want["hypothesis"] == -1 and not want["F"].any()
    if n >= 63:
        assert refined > 0


def test_refining_a_refined_record_again(ah, torch, synth):
    pairs = as_pairs(ah, scene(synth, 700, 12))
    rec0, _ = fr.find_fundamental(pairs, 256, 1.0, 1)
    a, _ = gpu_refine(ah, torch, pairs, rec0, 1.0, 1)
    assert a["root"] == 3
    b, bm = gpu_refine(ah, torch, pairs, a, 1.0, 2)
    want, wm = rr.refine_fundamental(pairs, a, 1.0, 2)
    assert_same(b, bm, want, wm, "second refit")
    assert b["inliers"] >= a["inliers"] and b["root"] == 3
    c, cm = gpu_refine(ah, torch, pairs, b, 2.5, 1)                     # another threshold: counted at this call's
    want, wm = rr.refine_fundamental(pairs, b, 2.5, 1)
    assert_same(c, cm, want, wm, "third refit")


def _batch(ah, torch, det, lists, stride, records, thr, rounds, extra=1, counts=None):
    """one hak_refine_fundamental_batch call over `lists`; `counts` = the counts the device reads (default: the lists' lengths);
    `extra` records past npairs are sentinels"""
    np_ = len(lists)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    for f in ("x1", "y1", "x2", "y2"):
        allp[f] = np.nan
    for k, lst in enumerate(lists):
        allp[k * stride:k * stride + len(lst)] = lst
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts if counts is not None else [len(lst) for lst in lists], dtype=torch.int32, device="cuda")
    size = ah.FUNDAMENTAL_DTYPE.itemsize
    host = np.full((np_ + extra) * size, 0xEE, np.uint8)
    host[:np_ * size] = np.array(records, ah.FUNDAMENTAL_DTYPE).view(np.uint8)
    d_io = torch.from_numpy(host).cuda()
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, thr, rounds, d_io.data_ptr(),
                                                 d_mask.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_io.cpu().numpy()
    assert (raw[np_ * size:] == 0xEE).all()                             # records past npairs are untouched
    return raw[:np_ * size].view(ah.FUNDAMENTAL_DTYPE), d_mask.cpu().numpy().reshape(np_, stride)


def test_randomised_parity(ah, torch, det):
    """the 150 parity_case inputs as single calls (rounds 1 + k % 3 and each case's own threshold), and every third group as one
    ragged batch call"""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    recs0, pairs_of = [], []
    for k, c in enumerate(cases):
        pairs = as_pairs(ah, c["recs"])
        pairs_of.append(pairs)
        rec0, _ = fr.find_fundamental(pairs, c["iterations"], c["threshold"], c["seed"])
        recs0.append(rec0)
        want, wm = rr.refine_fundamental(pairs, rec0, c["threshold"], 1 + k % 3)
        got, gm = gpu_refine(ah, torch, pairs, rec0, c["threshold"], 1 + k % 3, ctx=det.ctx if c["ctx"] else None)
        try:
            assert_same(got, gm, want, wm, (k, c["scene"]))
        except AssertionError as e:
            fails.append(str(e)[:300])
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    for g in groups:
        ks = [k for k, c in enumerate(cases) if c["group"] == g]
        thr = cases[ks[0]]["threshold"]
        stride = max(1, max(len(pairs_of[k]) for k in ks))
        out, masks = _batch(ah, torch, det, [pairs_of[k] for k in ks], stride, [recs0[k] for k in ks], thr, 3)
        for slot, k in enumerate(ks):
            n = len(pairs_of[k])
            want, wm = rr.refine_fundamental(pairs_of[k], recs0[k], thr, 3)
            try:
                assert_same(out[slot], masks[slot, :n], want, wm, ("batch", g, k))
                assert (masks[slot, n:] == 0xEE).all(), ("batch", g, k, "written past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    stride = 1100
    counts = [0, 3, 8, 900, stride + 50, 900, 900]
    lists, records = [], []
    for k, c in enumerate(counts):
        lst = as_pairs(ah, scene(synth, stride, 40 + k))[:min(c, stride)]
        lists.append(lst)
        records.append(fr.find_fundamental(lst, 256, 1.0, 77)[0])
    records[5] = records[5].copy()
    records[5]["hypothesis"] = -1                                       # a no-model record with a usable F
    records[6] = records[6].copy()
    records[6]["F"][4] = np.nan                                         # a NaN in F
    # the device reads the raw counts: stride + 50 is clamped to the stride there, and pair 5's list and mask stay as they are
    out, masks = _batch(ah, torch, det, lists, stride, records, 1.0, 3, counts=counts)
    for k, lst in enumerate(lists):
        n = len(lst)
        s, m = gpu_refine(ah, torch, lst, records[k], 1.0, 3)
        assert_same(out[k], masks[k, :n], s, m, ("batch vs single", k))
        want, wm = rr.refine_fundamental(lst, records[k], 1.0, 3)
        assert_same(s, m, want, wm, ("reference", k))
        assert (masks[k, n:] == 0xEE).all()
    assert out[4]["n"] == stride and out[3]["root"] == 3
    for k in (0, 1, 5, 6):
        assert out[k]["hypothesis"] == -1 and not out[k]["F"].any() and out[k]["inliers"] == 0 and not masks[k, :len(lists[k])].any()


def test_chain_detect_match_fundamental_refine_epipolar(ah, torch, synth):
    """detect -> knn2 -> find_fundamental_batch -> refine_batch -> match_epipolar_batch with one hak_sync at the end equals the
    same calls made one at a time with downloads in between; every accepted epipolar match lies in the refined F's band"""
    w, h = 256, 192
    p = ah.iAlignUp(w, 128)
    imgs = []
    for s in (1, 2):
        imgs += list(synth.pair(w, h, s))
    B, mp, radius = len(imgs), 1000, 2.0
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    dt = ah.Akazer()
    dt.init((w, h, p), max_pts=mp, batch=B)
    size = ah.FUNDAMENTAL_DTYPE.itemsize

    def run(sync_between):
        pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
        num = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
        fund = torch.zeros(B // 2 * size, dtype=torch.uint8, device="cuda")
        masks = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
        eout = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
        ecnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
        got = []
        steps = [
            lambda: ah.lib.hak_detect_and_compute_batch(dt.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1),
            lambda: ah.lib.hak_match_knn2_batch(dt.ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()),
            lambda: ah.lib.hak_find_fundamental_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 256, 1.0, 0, fund.data_ptr(),
                                                      None),
            lambda: ah.lib.hak_refine_fundamental_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 1.0, 3, fund.data_ptr(),
                                                        masks.data_ptr()),
            lambda: ah.lib.hak_match_epipolar_batch(dt.ctx, pts.data_ptr(), num.data_ptr(), B // 2, fund.data_ptr(), radius, 4, 5, 1, 0,
                                                    eout.data_ptr(), ecnt.data_ptr()),
        ]
        for step in steps:
            ah.check(step())
            if sync_between:
                ah.check(ah.lib.hak_sync(dt.ctx))
                got.append([t.cpu().numpy().copy() for t in (out, cnt, fund, masks)])
        ah.check(ah.lib.hak_sync(dt.ctx))
        return [t.cpu().numpy() for t in (out, cnt, fund, masks, eout, ecnt)], got

    chain, _ = run(False)
    stepwise, downloads = run(True)
    for a, b in zip(chain, stepwise):
        assert np.array_equal(a, b)
    out, cnt, fund, masks, eout, ecnt = chain
    lists = out.view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    before = downloads[2][2].view(ah.FUNDAMENTAL_DTYPE)                  # the records hak_find_fundamental_batch wrote
    recs = fund.view(ah.FUNDAMENTAL_DTYPE)
    elists = eout.view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    for k in range(B // 2):
        lst = lists[k, :cnt[k]].copy()
        want, wm = rr.refine_fundamental(lst, before[k], 1.0, 3)
        assert_same(recs[k], masks.reshape(B // 2, mp)[k, :cnt[k]], want, wm, ("chain", k))
        assert recs[k]["inliers"] >= before[k]["inliers"] and recs[k]["hypothesis"] >= 0
        # the epipolar gate is the point-to-line distance in image 2, e e < r2 (a a + b b); the Sampson denominator adds
        # p p + q q >= 0, so every accepted match is a Sampson inlier of the same F at threshold = radius up to float32 rounding
        em = fr.records(elists[k, :ecnt[k]]).astype(np.float64)
        assert len(em) > 0
        F = recs[k]["F"].astype(np.float64).reshape(3, 3)
        l2 = np.concatenate([em[:, :2], np.ones((len(em), 1))], axis=1) @ F.T
        dist = np.abs((l2 * np.concatenate([em[:, 2:], np.ones((len(em), 1))], axis=1)).sum(axis=1)) / np.hypot(l2[:, 0], l2[:, 1])
        assert (dist < radius * (1 + 1e-4)).all()
        assert (fr.sampson(F, em) < radius * (1 + 1e-4)).all()
    dt.close()


def test_python_wrapper(ah, torch, synth):
    pairs = as_pairs(ah, scene(synth, 500, 4))
    rec0, _ = fr.find_fundamental(pairs, 256, 1.0, 3)
    keep = rec0.copy()
    want, wm = rr.refine_fundamental(pairs, rec0, 1.0, 3)
    got, gm = ah.refineFundamental(pairs, rec0)
    assert got.dtype == ah.FUNDAMENTAL_DTYPE and rec0.tobytes() == keep.tobytes()
    assert_same(got, gm, want, wm, "wrapper")
    dev, dm = ah.refineFundamental(upload(torch, pairs), rec0, 1.0, 3)  # a device tensor is used in place
    assert_same(dev, dm, want, wm, "wrapper, device list")
    assert got["root"] == 3 and got["inliers"] >= rec0["inliers"]


def _demo_dump(ah, raw):
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
    return n, inl, F, lst, mask


def test_demo_refine_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --fundamental --refine 3`: the dumped F, count and mask equal refineFundamental on the dumped list; without
    --refine the output has no refit line and the dump holds the RANSAC model"""
    from test_gpu_dropin import write_pgm
    left, right = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    dumps = {}
    for name, extra in (("plain", []), ("refined", ["--refine", "3"])):
        dump = str(tmp_path / (name + ".bin"))
        r = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--fundamental"] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Refit of the fundamental matrix" in r.stdout) == bool(extra)
        dumps[name] = _demo_dump(ah, open(dump, "rb").read())
    n, inl0, F0, lst, mask0 = dumps["plain"]
    rec0, m0 = ah.findFundamental(lst)
    assert np.array_equal(F0.view(np.uint32), rec0["F"].view(np.uint32)) and inl0 == rec0["inliers"] and np.array_equal(mask0, m0)
    n2, inl, F, lst2, mask = dumps["refined"]
    assert n2 == n and lst2.tobytes() == lst.tobytes()
    got, gm = ah.refineFundamental(lst, rec0, 1.0, 3)
    assert np.array_equal(F.view(np.uint32), got["F"].view(np.uint32)) and inl == got["inliers"] and np.array_equal(mask, gm)
    want, wm = rr.refine_fundamental(lst, fr.find_fundamental(lst, 1024, 1.0, 0)[0], 1.0, 3)
    assert_same(got, gm, want, wm, "demo")
    assert inl >= inl0


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    lib, io = ah.lib, rec.ctypes.data
    one, batch = lib.hak_refine_fundamental, lib.hak_refine_fundamental_batch
    refused = [
        (one, (None, d.data_ptr(), 10, 1.0, 0, None, io)), (one, (None, d.data_ptr(), 10, 1.0, 9, None, io)),       # rounds
        (one, (None, d.data_ptr(), 10, float("nan"), 3, None, io)), (one, (None, d.data_ptr(), 10, float("inf"), 3, None, io)),
        (one, (det.ctx, d.data_ptr(), 10, 0.0, 3, None, io)), (one, (det.ctx, d.data_ptr(), 10, -1.0, 3, None, io)),
        (one, (None, d.data_ptr(), -1, 1.0, 3, None, io)),                                                 # n < 0
        (one, (None, None, 5, 1.0, 3, None, io)),                                                          # no list
        (one, (None, d.data_ptr() + 4, 10, 1.0, 3, None, io)),                                             # misaligned
        (one, (det.ctx, d.data_ptr(), 10, 1.0, 3, None, None)),                                            # no h_inout
        (batch, (None, d.data_ptr(), 64, cnt.data_ptr(), 1, 1.0, 3, d.data_ptr(), None)),                  # no context
        (batch, (det.ctx, d.data_ptr(), 64, None, 1, 1.0, 3, d.data_ptr(), None)),                         # no counts
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 1.0, 3, None, None)),                       # no d_inout
        (batch, (det.ctx, None, 64, cnt.data_ptr(), 1, 1.0, 3, d.data_ptr(), None)),                       # no list
        (batch, (det.ctx, d.data_ptr() + 4, 64, cnt.data_ptr(), 1, 1.0, 3, d.data_ptr(), None)),           # misaligned
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 0, 1.0, 3, d.data_ptr(), None)),               # npairs < 1
        (batch, (det.ctx, d.data_ptr(), 0, cnt.data_ptr(), 1, 1.0, 3, d.data_ptr(), None)),                # stride < 1
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 1.0, 0, d.data_ptr(), None)),               # rounds
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 1.0, 9, d.data_ptr(), None)),
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, float("nan"), 3, d.data_ptr(), None)),      # threshold
        (batch, (det.ctx, d.data_ptr(), 64, cnt.data_ptr(), 1, 0.0, 3, d.data_ptr(), None)),
    ]
    for k, (fn, args) in enumerate(refused):
        ah.check(one(None, d.data_ptr(), 0, 1.0, 1, None, io))          # a call that succeeds in between: no stale message counts
        assert fn(*args) != 0, (k, args)
        assert lib.hak_last_error().decode() != "", (k, args)
    assert not d.any()                                                  # nothing was written through a refused call's pointers

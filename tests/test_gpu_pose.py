"""GPU suite: relative pose from the fundamental matrix (hak_recover_pose / hak_recover_pose_batch, kernels_pose.hip) bit for bit
against its numpy statement tests/pose_ref.py -- every byte of the record, the front mask and the points.  The input F values are
the STATEMENTS' (the planted F, fundamental_ref, fundamental_refit_ref), never the device's, so the device's own RANSAC and refit
can neither mask nor cause a difference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import pose_ref as pr
from conftest import ROOT
from test_gpu_fundamental import as_pairs, det, synth, torch, upload  # noqa: F401 (fixtures)
from test_pose_cpu import PARITY_CASES, TABLE, f32_model, first_winners, parity_case, table_case

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
BLOCK = 512                                                             # k_pose's threads per pair (PO_BLOCK): 8 waves
SIZES = [0, 1, 7, 8, 63, 64, 65, 129, BLOCK - 1, BLOCK, BLOCK + 1, 1025]
INF = float("inf")
_fp = C.POINTER(C.c_float)


def scene(synth, n, seed, **kw):
    """n records: 70 % planted two-view inliers with 0.3 px noise at depths of 4 .. 12 baselines, the rest uniformly random;
    -> (pairs, planted F as a hak_fundamental holds it, K)"""
    n_in = n * 7 // 10
    recs, _, F, K = synth.two_view_scene(n_in, n - n_in, seed, noise=0.3, **kw)[:4]
    return recs, f32_model(F), K


def gpu_pose(ah, torch, pairs, F, K1, K2=None, threshold=1.0, max_depth=INF, ctx=None, with_mask=True, with_xyz=True):
    """one hak_recover_pose call -> (record, the whole 0xEE-prefilled mask buffer, the whole xyz buffer as bytes)"""
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    xyz = torch.full((12 * max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K1)
    k2 = k1 if K2 is None else ah.intrinsics(K2)
    f = np.ascontiguousarray(np.asarray(F, np.float32).reshape(9))
    rec = np.zeros((), ah.POSE_DTYPE)
    ah.check(ah.lib.hak_recover_pose(ctx, d.data_ptr(), n, f.ctypes.data_as(_fp), k1.ctypes.data, k2.ctypes.data, threshold, max_depth,
                                     mask.data_ptr() if with_mask else None, xyz.data_ptr() if with_xyz else None, rec.ctypes.data))
    return rec, mask.cpu().numpy(), xyz.cpu().numpy()


def assert_same(got, gmask, gxyz, want, wmask, wxyz, what=""):
    """got: a record and the n mask bytes and 12 n xyz bytes the device wrote"""
    assert got.tobytes() == np.array(want, got.dtype).tobytes(), (what, got, want)
    assert np.array_equal(gmask, wmask), (what, "mask", int((gmask != wmask).sum()))
    assert gxyz.tobytes() == wxyz.tobytes(), (what, "xyz")


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    recs, F_true, K = scene(synth, n, 300 + n)
    pairs = as_pairs(ah, recs)
    models = [(1.0, F_true)]
    if n >= 8:
        rec0 = fr.find_fundamental(pairs, 256, 2.5, n)[0]
        models.append((2.5, rr.refine_fundamental(pairs, rec0, 2.5, 1)[0]["F"]))      # the statements' noisy model
    poses = fronts = 0
    for thr, F in models:
        for md in (INF, 8.0):
            want, wm, wx = pr.recover_pose(pairs, F, K, None, thr, md)
            for ctx in (None, det.ctx):
                got, gm, gx = gpu_pose(ah, torch, pairs, F, K, None, thr, md, ctx=ctx)
                assert_same(got, gm[:n], gx[:12 * n], want, wm, wx, (n, thr, md, ctx is not None))
            got, gm, gx = gpu_pose(ah, torch, pairs, F, K, None, thr, md, with_mask=False)
            assert (gm == 0xEE).all()                                   # d_mask = NULL: same record and points, buffer untouched
            assert_same(got, wm, gx[:12 * n], want, wm, wx, (n, thr, md, "no mask"))
            got, gm, gx = gpu_pose(ah, torch, pairs, F, K, None, thr, md, ctx=det.ctx, with_xyz=False)
            assert (gx == 0xEE).all()
            assert_same(got, gm[:n], wx, want, wm, wx, (n, thr, md, "no xyz"))
            got, gm, gx = gpu_pose(ah, torch, pairs, F, K, None, thr, md, with_mask=False, with_xyz=False)
            assert (gm == 0xEE).all() and (gx == 0xEE).all() and got.tobytes() == np.array(want, got.dtype).tobytes()
            poses += int(want["candidate"]) >= 0 and F is F_true
            fronts += int(want["in_front"])
    assert poses == 2                                                   # the planted F always gives a pose, even at n = 0
    if n >= 63:
        assert fronts > n and int(want["in_front"]) < int(want["inliers"])          # max_depth = 8 cuts the 4 .. 12 scene


def test_two_cameras_and_degenerate_models(ah, torch, synth):
    recs, F, K = scene(synth, 300, 5)
    pairs = as_pairs(ah, recs)
    cx, cy = K[0, 2], K[1, 2]
    two = recs.copy()
    two[:, 2], two[:, 3] = (recs[:, 2] - cx) * 2 + cx + 7, (recs[:, 3] - cy) * 2 + cy - 3
    S = np.array([[0.5, 0, (cx - 7) / 2], [0, 0.5, (cy + 3) / 2], [0, 0, 1.0]])
    F2 = f32_model(S.T @ F.astype(np.float64).reshape(3, 3))
    K2 = (2 * K[0, 0], 2 * K[1, 1], cx + 7, cy - 3)
    want, wm, wx = pr.recover_pose(as_pairs(ah, two), F2, K, K2)
    got, gm, gx = gpu_pose(ah, torch, as_pairs(ah, two), F2, K, K2)
    assert_same(got, gm[:300], gx[:3600], want, wm, wx, "K1 != K2")
    assert want["in_front"] > 150
    bad = F.copy()
    bad[4] = np.nan
    rank1 = np.zeros(9, np.float32)
    rank1[0] = 1.0
    nonfinite = pairs.copy()
    nonfinite["x2"] = np.nan
    for what, lst, f, k in (("NaN in F", pairs, bad, K), ("zero F", pairs, np.zeros(9, np.float32), K),
                            ("rank-1 E", pairs, rank1, (1.0, 1.0, 0.0, 0.0)), ("non-finite records", nonfinite, F, K)):
        want, wm, wx = pr.recover_pose(lst, f, k)
        got, gm, gx = gpu_pose(ah, torch, lst, f, k)
        assert_same(got, gm[:300], gx[:3600], want, wm, wx, what)
        assert (want["candidate"] == -1) == (what != "non-finite records") and want["in_front"] == 0 and not gm[:300].any()


def test_every_candidate_wins(ah, torch, synth):
    runs = []
    for k in range(len(TABLE)):
        recs, F, K, R, t, z = table_case(synth, k)
        runs.append((recs, F, K, R, t, z, pr.recover_pose(recs, F, K)))
        if len(first_winners(runs)) == 4:
            break
    first = first_winners(runs)
    assert sorted(first) == [0, 1, 2, 3]
    for c, k in first.items():
        recs, F, K, _, _, _, (want, wm, wx) = runs[k]
        got, gm, gx = gpu_pose(ah, torch, as_pairs(ah, recs), F, K)
        assert_same(got, gm[:len(recs)], gx[:12 * len(recs)], want, wm, wx, ("candidate", c, k))
        assert got["candidate"] == c and got["in_front"] == len(recs)


def _batch(ah, torch, det, lists, stride, records, K, thr, md, counts, extra=1, with_out=True, K2=None):
    """one hak_recover_pose_batch call; `extra` records past npairs are sentinels -> (records, masks, xyz bytes)"""
    np_ = len(lists)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    for f in ("x1", "y1", "x2", "y2"):
        allp[f] = np.nan
    for k, lst in enumerate(lists):
        allp[k * stride:k * stride + len(lst)] = lst
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_F = torch.from_numpy(np.array(records, ah.FUNDAMENTAL_DTYPE).view(np.uint8).copy()).cuda()
    size = ah.POSE_DTYPE.itemsize
    d_out = torch.full(((np_ + extra) * size,), 0xEE, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    d_xyz = torch.full((np_ * stride * 12,), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K)
    k2 = k1 if K2 is None else ah.intrinsics(K2)
    ah.check(ah.lib.hak_recover_pose_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, d_F.data_ptr(), k1.ctypes.data,
                                           k2.ctypes.data, thr, md, d_out.data_ptr(), d_mask.data_ptr() if with_out else None,
                                           d_xyz.data_ptr() if with_out else None))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_out.cpu().numpy()
    assert (raw[np_ * size:] == 0xEE).all()                             # records past npairs are untouched
    return raw[:np_ * size].view(ah.POSE_DTYPE), d_mask.cpu().numpy().reshape(np_, stride), d_xyz.cpu().numpy().reshape(np_, stride * 12)


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    stride = 1100
    counts = [0, 3, 8, 900, stride + 50, 900, 900]
    lists, records = [], []
    for k, c in enumerate(counts):
        recs, F, K = scene(synth, stride, 40 + k)
        lst = as_pairs(ah, recs)[:min(c, stride)]
        lists.append(lst)
        rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
        rec["F"], rec["hypothesis"], rec["n"] = F, 7, len(lst)
        if k in (3, 4):
            rec = rr.refine_fundamental(lst, fr.find_fundamental(lst, 256, 1.0, 77)[0], 1.0, 1)[0]       # the statements' model
        records.append(rec)
    records[5]["hypothesis"] = -1                                       # a no-model record with a usable F
    records[6]["F"][4] = np.nan                                         # a NaN in F
    # the device reads the raw counts: stride + 50 is clamped to the stride there
    for md in (INF, 9.0):
        out, masks, xyz = _batch(ah, torch, det, lists, stride, records, K, 1.0, md, counts)
        for k, lst in enumerate(lists):
            n = len(lst)
            want, wm, wx = pr.recover_pose(lst, records[k], K, None, 1.0, md)
            assert_same(out[k], masks[k, :n], xyz[k, :12 * n], want, wm, wx, ("batch vs statement", k, md))
            f = records[k]["F"] if records[k]["hypothesis"] >= 0 else np.full(9, np.nan, np.float32)
            s, sm, sx = gpu_pose(ah, torch, lst, f, K, None, 1.0, md)
            assert_same(out[k], masks[k, :n], xyz[k, :12 * n], s, sm[:n], sx[:12 * n], ("batch vs single", k, md))
            assert (masks[k, n:] == 0xEE).all() and (xyz[k, 12 * n:] == 0xEE).all()     # nothing past a count
        assert out[4]["n"] == stride and out[3]["in_front"] > 300 and out[0]["candidate"] >= 0 and out[0]["n"] == 0
        for k in (5, 6):
            assert out[k]["candidate"] == -1 and out[k]["inliers"] == 0 and not masks[k, :900].any() and not xyz[k, :12 * 900].any()
    bare = _batch(ah, torch, det, lists, stride, records, K, 1.0, 9.0, counts, with_out=False)
    assert bare[0].tobytes() == out.tobytes() and (bare[1] == 0xEE).all() and (bare[2] == 0xEE).all()


def test_randomised_parity(ah, torch, det):
    """the 150 seeded cases of test_pose_cpu.parity_case -- sizes from 0 to 3000 with the block and chunk edges, six scene families
    (general, sideways and forward translation, nearly pure rotation, planar, integer lattice under K = (1, 1, 0, 0)), matches at
    infinity and behind the cameras, six kinds of model (planted, the statements' RANSAC and refit records, random, rank 1, zero),
    negated, scaled by 2^-100 .. 2^100, with NaN / inf entries, K1 = K2 or not over five cameras, five depth limits, NaN rows,
    duplicates, coordinates offset by +-16000 -- record, mask and points byte for byte against the statement, with and without a
    context; every third block of eight also as one ragged hak_recover_pose_batch call with the records on the device, the ones
    with hypothesis -1 included.  What the cases reach (every candidate, ties, every j3, every cause of "no pose", det <= 0, the
    depth limit) is asserted in test_pose_cpu.py."""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    for k, c in enumerate(cases):
        n = len(c["recs"])
        pairs = as_pairs(ah, c["recs"])
        F = c["record"]["F"]
        want, wm, wx = pr.recover_pose(pairs, F, c["K1"], c["K2"], c["threshold"], c["max_depth"])
        got, gm, gx = gpu_pose(ah, torch, pairs, F, c["K1"], c["K2"], c["threshold"], c["max_depth"], ctx=det.ctx if c["ctx"] else None)
        try:
            assert_same(got, gm[:n], gx[:12 * n], want, wm, wx, (k, c["scene"], c["model"], c["depth"]))
            assert (gm[n:] == 0xEE).all() and (gx[12 * n:] == 0xEE).all(), (k, "written past the count")
        except AssertionError as e:
            fails.append(str(e)[:300])
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    broken = 0
    for g in groups:
        ks = [k for k, c in enumerate(cases) if c["group"] == g]
        c0 = cases[ks[0]]
        lists = [as_pairs(ah, cases[k]["recs"]) for k in ks]
        records = [cases[k]["record"] for k in ks]
        stride = max(1, max(len(lst) for lst in lists))
        out, masks, xyz = _batch(ah, torch, det, lists, stride, records, c0["K1"], c0["threshold"], c0["max_depth"],
                                 [len(lst) for lst in lists], K2=c0["K2"])
        for slot, k in enumerate(ks):
            n = len(lists[slot])
            broken += records[slot]["hypothesis"] < 0
            want, wm, wx = pr.recover_pose(lists[slot], records[slot], c0["K1"], c0["K2"], c0["threshold"], c0["max_depth"])
            try:
                assert_same(out[slot], masks[slot, :n], xyz[slot, :12 * n], want, wm, wx, ("batch", g, k))
                assert (masks[slot, n:] == 0xEE).all() and (xyz[slot, 12 * n:] == 0xEE).all(), ("batch", g, k, "written past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 5 and broken >= 3
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_chain_detect_match_fundamental_refine_pose(ah, torch, synth):
    """detect -> knn2 -> find_fundamental_batch -> refine_batch -> recover_pose_batch with one hak_sync at the end equals the same
    calls made one at a time with downloads in between, and the statement on the downloaded lists and records"""
    w, h = 256, 192
    p = ah.iAlignUp(w, 128)
    imgs = []
    for s in (1, 2):
        imgs += list(synth.pair(w, h, s))
    B, mp = len(imgs), 1000
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    dt = ah.Akazer()
    dt.init((w, h, p), max_pts=mp, batch=B)
    size = ah.FUNDAMENTAL_DTYPE.itemsize
    K = ah.intrinsics((300.0, 310.0, 128.0, 96.0))

    def run(sync_between):
        pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
        num = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
        fund = torch.zeros(B // 2 * size, dtype=torch.uint8, device="cuda")
        pose = torch.zeros(B // 2 * 64, dtype=torch.uint8, device="cuda")
        masks = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
        xyz = torch.zeros(B // 2 * mp * 3, dtype=torch.float32, device="cuda")
        steps = [
            lambda: ah.lib.hak_detect_and_compute_batch(dt.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1),
            lambda: ah.lib.hak_match_knn2_batch(dt.ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()),
            lambda: ah.lib.hak_find_fundamental_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 256, 1.0, 0, fund.data_ptr(),
                                                      None),
            lambda: ah.lib.hak_refine_fundamental_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 1.0, 3, fund.data_ptr(), None),
            lambda: ah.lib.hak_recover_pose_batch(dt.ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, fund.data_ptr(), K.ctypes.data,
                                                  K.ctypes.data, 1.0, 50.0, pose.data_ptr(), masks.data_ptr(), xyz.data_ptr()),
        ]
        for step in steps:
            ah.check(step())
            if sync_between:
                ah.check(ah.lib.hak_sync(dt.ctx))
                _ = [t.cpu() for t in (out, cnt, fund)]
        ah.check(ah.lib.hak_sync(dt.ctx))
        return [t.cpu().numpy() for t in (out, cnt, fund, pose, masks, xyz)]

    chain = run(False)
    stepwise = run(True)
    for a, b in zip(chain, stepwise):
        assert a.tobytes() == b.tobytes()
    out, cnt, fund, pose, masks, xyz = chain
    lists = out.view(ah.MATCH_PAIR_DTYPE).reshape(B // 2, mp)
    recs, poses = fund.view(ah.FUNDAMENTAL_DTYPE), pose.view(ah.POSE_DTYPE)
    for k in range(B // 2):
        n = int(cnt[k])
        assert n > 0
        want, wm, wx = pr.recover_pose(lists[k, :n].copy(), recs[k], K, None, 1.0, 50.0)
        assert_same(poses[k], masks.reshape(B // 2, mp)[k, :n], xyz.reshape(B // 2, mp * 3)[k, :3 * n], want, wm, wx, ("chain", k))
        assert (poses[k]["candidate"] >= 0) == (recs[k]["hypothesis"] >= 0) and poses[k]["inliers"] == recs[k]["inliers"]
    assert (poses["candidate"] >= 0).any() and poses["in_front"].sum() > 0
    dt.close()


def test_python_wrapper(ah, torch, synth):
    recs, F, K = scene(synth, 500, 4)
    pairs = as_pairs(ah, recs)
    want, wm, wx = pr.recover_pose(pairs, F, K)
    got, gm, gx = ah.recoverPose(pairs, F, K)
    assert got.dtype == ah.POSE_DTYPE and gm.dtype == np.uint8 and gx.dtype == np.float32 and gx.shape == (500, 3)
    assert_same(got, gm, gx, want, wm, wx, "wrapper")
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    rec["F"], rec["hypothesis"] = F, 3
    dev = ah.recoverPose(upload(torch, pairs), rec, ah.intrinsics(K), K, 1.0, 9.0)  # a device tensor is used in place; a record
    assert_same(*dev, *pr.recover_pose(pairs, rec, K, K, 1.0, 9.0), "wrapper, device list")
    assert 0 < dev[0]["in_front"] < got["in_front"]
    rec["hypothesis"] = -1
    none = ah.recoverPose(pairs, rec, K)
    assert_same(*none, *pr.recover_pose(pairs, rec, K), "wrapper, no model")
    assert none[0]["candidate"] == -1


def test_demo_pose_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --fundamental --refine 3 --pose FX FY CX CY`: the dumped pose record, mask and points equal recoverPose and the
    statement on the dumped list and F; without --pose the output has no pose line"""
    from test_gpu_dropin import write_pgm
    left, right = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    hh, ww = golden.lr_u8["left"].shape
    K = (1.2 * ww, 1.2 * ww, ww / 2.0, hh / 2.0)
    dump = str(tmp_path / "pose.bin")
    r = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--refine", "3", "--pose"] +
                       [repr(float(v)) for v in K], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Relative pose from the fundamental matrix" in r.stdout and "Refit of the fundamental matrix" in r.stdout
    raw = open(dump, "rb").read()
    off = 0
    for _ in range(2):                                                  # the float and the FAST path's point sections
        n1, n2 = np.frombuffer(raw, np.int32, 2, off)
        off += 8 + 104 * int(n1 + n2)
    n, inl = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    F = np.frombuffer(raw, np.float32, 9, off + 8).copy()
    off += 44
    lst = np.frombuffer(raw, ah.MATCH_PAIR_DTYPE, n, off).copy()
    off += 33 * n                                                       # the list and the refit's mask
    rec = np.frombuffer(raw, ah.POSE_DTYPE, 1, off)[0]
    mask = np.frombuffer(raw, np.uint8, n, off + 64).copy()
    xyz = np.frombuffer(raw, np.float32, 3 * n, off + 64 + n).copy().reshape(n, 3)
    assert off + 64 + 13 * n == len(raw) and n > 100
    got, gm, gx = ah.recoverPose(lst, F, K)
    assert_same(rec, mask, xyz, got, gm, gx, "demo vs wrapper")
    assert_same(rec, mask, xyz, *pr.recover_pose(lst, F, K), "demo vs statement")
    assert rec["n"] == n and rec["inliers"] == inl and rec["candidate"] >= 0
    plain = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--fundamental"], capture_output=True, text=True)
    assert plain.returncode == 0 and "Relative pose" not in plain.stdout


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    dF = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rec, ok_rec = np.zeros((), ah.POSE_DTYPE), np.zeros((), ah.POSE_DTYPE)
    F = np.zeros(9, np.float32)
    F[5], F[7] = -1.0, 1.0
    K = ah.intrinsics((300.0, 300.0, 128.0, 96.0))

    def k_with(**kw):
        b = K.copy()
        for f, v in kw.items():
            b[f] = v
        return b

    nan = float("nan")
    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=INF), k_with(cx=nan), k_with(cy=-INF)]
    lib, io, fp, kp, p = ah.lib, rec.ctypes.data, F.ctypes.data_as(_fp), K.ctypes.data, d.data_ptr()
    one, batch = lib.hak_recover_pose, lib.hak_recover_pose_batch
    refused = [(one, (None, p, 10, fp, kp, kp, thr, INF, p, p, io)) for thr in (0.0, -1.0, nan, INF)]
    refused += [(one, (det.ctx, p, 10, fp, kp, kp, 1.0, md, p, p, io)) for md in (0.0, -3.0, nan)]
    refused += [(one, (None, p, 10, fp, b.ctypes.data, kp, 1.0, INF, p, p, io)) for b in bad_k]
    refused += [(one, (None, p, 10, fp, kp, b.ctypes.data, 1.0, INF, p, p, io)) for b in bad_k]
    refused += [
        (one, (None, p, 10, None, kp, kp, 1.0, INF, p, p, io)),                                            # no F
        (one, (None, p, 10, fp, None, kp, 1.0, INF, p, p, io)), (one, (None, p, 10, fp, kp, None, 1.0, INF, p, p, io)),    # no K
        (one, (det.ctx, p, 10, fp, kp, kp, 1.0, INF, p, p, None)),                                         # no h_out
        (one, (None, p, -1, fp, kp, kp, 1.0, INF, p, p, io)),                                              # n < 0
        (one, (None, None, 5, fp, kp, kp, 1.0, INF, p, p, io)),                                            # no list
        (one, (None, p + 4, 10, fp, kp, kp, 1.0, INF, p, p, io)),                                          # misaligned
        (batch, (None, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),               # no context
        (batch, (det.ctx, p, 64, None, 1, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),                      # no counts
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, None, kp, kp, 1.0, INF, p, p, p)),                     # no d_F
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, INF, None, p, p)),         # no d_out
        (batch, (det.ctx, None, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),         # no list
        (batch, (det.ctx, p + 4, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),        # misaligned
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 0, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),            # npairs < 1
        (batch, (det.ctx, p, 0, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, INF, p, p, p)),             # stride < 1
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), None, kp, 1.0, INF, p, p, p)),          # no K
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, None, 1.0, INF, p, p, p)),
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, nan, INF, p, p, p)),            # threshold
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 0.0, INF, p, p, p)),
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, nan, p, p, p)),            # max_depth
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, kp, 1.0, 0.0, p, p, p)),
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), bad_k[0].ctypes.data, kp, 1.0, INF, p, p, p)),
        (batch, (det.ctx, p, 64, cnt.data_ptr(), 1, dF.data_ptr(), kp, bad_k[4].ctypes.data, 1.0, INF, p, p, p)),
    ]
    for k, (fn, args) in enumerate(refused):
        ah.check(one(None, p, 0, fp, kp, kp, 1.0, INF, None, None, ok_rec.ctypes.data))   # a call that succeeds in between
        assert ok_rec["candidate"] == 0 and ok_rec["n"] == 0
        assert fn(*args) != 0, (k, args)
        assert lib.hak_last_error().decode() != "", (k, args)
    ah.check(lib.hak_sync(det.ctx))
    assert not d.any() and not rec.tobytes().strip(b"\0")               # nothing was written through a refused call's pointers
    ah.check(one(None, p, 10, fp, kp, kp, 1.0, INF, None, None, io))    # +inf max_depth and the same pointers are accepted
    assert rec["n"] == 10

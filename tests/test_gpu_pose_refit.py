"""GPU suite: calibrated Gauss-Newton refit of the relative pose (hak_refine_pose / hak_refine_pose_batch, kernels_poserefit.hip)
bit for bit against its numpy statement tests/pose_refit_ref.py -- every R / t bit, inliers, in_front, candidate, n, every mask byte
and every xyz bit.  The inputs are the STATEMENT's records (pose_ref), so the device's own earlier stages can neither mask nor cause
a difference."""
import os
import subprocess

import numpy as np
import pytest

import pose_ref as pr
import pose_refit_ref as pz
import projected_match_ref as pm
import triangulate_ref as tr
from conftest import ROOT
from test_gpu_fundamental import as_pairs, det, synth, torch, upload  # noqa: F401 (fixtures)
from test_gpu_pose import assert_same, scene
from test_pose_cpu import PARITY_CASES, f32_model, noisy_case, parity_case
from test_pose_refit_cpu import FAMILY_CASES, family_case, refusals

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
SIZES = [0, 4, 5, 6, 63, 64, 65, 129, 1340]        # the first usable counts, the wave edges of the summation order
ROUNDS = [1, 3, 8]
INF = float("inf")
SIZE = 64                                          # sizeof(hak_pose)


def gpu_refine(ah, torch, pairs, K1, record, K2=None, threshold=1.0, max_depth=INF, rounds=3, ctx=None, with_mask=True, with_xyz=True):
    """one hak_refine_pose call -> (record, the whole 0xEE-prefilled mask buffer, the whole xyz buffer as bytes)"""
    n = len(pairs)
    d = upload(torch, pairs)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    xyz = torch.full((12 * max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K1)
    k2 = k1 if K2 is None else ah.intrinsics(K2)
    rec = np.array(record, ah.POSE_DTYPE).reshape(())
    ah.check(ah.lib.hak_refine_pose(ctx, d.data_ptr(), n, k1.ctypes.data, k2.ctypes.data, threshold, max_depth, rounds,
                                    mask.data_ptr() if with_mask else None, xyz.data_ptr() if with_xyz else None, rec.ctypes.data))
    return rec, mask.cpu().numpy(), xyz.cpu().numpy()


def _pairs(ah, recs):
    return recs if recs.dtype.names else as_pairs(ah, recs)


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    if n < 7:                                                           # every match planted: the first usable counts
        recs, _, F, K = synth.two_view_scene(n, 0, 300 + n, noise=0.3)[:4]
        F = f32_model(F)
    else:
        recs, F, K = scene(synth, n, 300 + n)
    pairs = as_pairs(ah, recs)
    refined = 0
    for thr in (1.0, 2.5):
        rec0 = pr.recover_pose(pairs, F, K, None, thr, INF)[0]
        assert rec0["candidate"] >= 0
        for rounds in ROUNDS:
            want, wm, wx = pz.refine_pose(pairs, K, rec0, None, thr, INF, rounds)
            for ctx in (None, det.ctx):
                got, gm, gx = gpu_refine(ah, torch, pairs, K, rec0, None, thr, INF, rounds, ctx=ctx)
                assert_same(got, gm[:n], gx[:12 * n], want, wm, wx, (n, thr, rounds, ctx is not None))
                assert (gm[n:] == 0xEE).all() and (gx[12 * n:] == 0xEE).all()        # untouched past n
            got, gm, gx = gpu_refine(ah, torch, pairs, K, rec0, None, thr, INF, rounds, with_mask=False)
            assert (gm == 0xEE).all()                                   # d_mask = NULL: same record and points, buffer untouched
            assert_same(got, wm, gx[:12 * n], want, wm, wx, (n, thr, rounds, "no mask"))
            got, gm, gx = gpu_refine(ah, torch, pairs, K, rec0, None, thr, INF, rounds, ctx=det.ctx, with_xyz=False)
            assert (gx == 0xEE).all()
            assert_same(got, gm[:n], wx, want, wm, wx, (n, thr, rounds, "no xyz"))
            got, gm, gx = gpu_refine(ah, torch, pairs, K, rec0, None, thr, INF, rounds, with_mask=False, with_xyz=False)
            assert (gm == 0xEE).all() and (gx == 0xEE).all() and got.tobytes() == np.array(want, got.dtype).tobytes()
            refined += int(want["candidate"]) == pz.REFINED_CANDIDATE
    if n < 5:
        assert refined == 0 and want["in_front"] <= n                   # a model, and too few matches for a round
    if n >= 63:
        assert refined > 0 and want["in_front"] > n // 2


def test_refining_a_refined_record_again(ah, torch, synth):
    recs, flags, rec1, K, R, t = noisy_case(synth, 1000, 0.6, 6)
    pairs = as_pairs(ah, recs)
    rec0 = pr.recover_pose(pairs, rec1, K, None, 1.0, 50.0)[0]
    a, _, _ = gpu_refine(ah, torch, pairs, K, rec0, None, 1.0, 50.0, 1)
    assert a["candidate"] == 4
    b, bm, bx = gpu_refine(ah, torch, pairs, K, a, None, 1.0, 50.0, 2)
    assert_same(b, bm, bx, *pz.refine_pose(pairs, K, a, None, 1.0, 50.0, 2), "second refit")
    assert b["in_front"] >= a["in_front"] and b["candidate"] == 4
    c, cm, cx = gpu_refine(ah, torch, pairs, K, b, None, 2.0, 50.0, 8)  # another threshold: counted at this call's
    assert_same(c, cm, cx, *pz.refine_pose(pairs, K, b, None, 2.0, 50.0, 8), "third refit")
    assert c["in_front"] > b["in_front"]


def _batch(ah, torch, det, lists, stride, records, K1, K2, thr, md, rounds, extra=1, counts=None):
    """one hak_refine_pose_batch call over `lists`; `counts` = the counts the device reads (default: the lists' lengths); `extra`
    records past npairs are sentinels -> (records, masks, xyz bytes)"""
    np_ = len(lists)
    allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
    for f in ("x1", "y1", "x2", "y2"):
        allp[f] = np.nan                                                # past a count: must not be read as usable
    for k, lst in enumerate(lists):
        allp[k * stride:k * stride + len(lst)] = lst
    d = upload(torch, allp)
    d_cnt = torch.tensor(counts if counts is not None else [len(lst) for lst in lists], dtype=torch.int32, device="cuda")
    host = np.full((np_ + extra) * SIZE, 0xEE, np.uint8)
    host[:np_ * SIZE] = np.array(records, ah.POSE_DTYPE).view(np.uint8)
    d_io = torch.from_numpy(host).cuda()
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    d_xyz = torch.full((np_ * stride * 12,), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K1)
    k2 = k1 if K2 is None else ah.intrinsics(K2)
    ah.check(ah.lib.hak_refine_pose_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, k1.ctypes.data, k2.ctypes.data, thr, md,
                                          rounds, d_io.data_ptr(), d_mask.data_ptr(), d_xyz.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_io.cpu().numpy()
    assert (raw[np_ * SIZE:] == 0xEE).all()                             # records past npairs are untouched
    return raw[:np_ * SIZE].view(ah.POSE_DTYPE), d_mask.cpu().numpy().reshape(np_, stride), d_xyz.cpu().numpy().reshape(np_, stride * 12)


def test_randomised_parity(ah, torch, det):
    """the family of test_pose_refit_cpu.family_case -- the parity_case inputs of test_pose_cpu with their statement records at the
    case's own threshold and at 0.3 of it, and the built members -- as single calls, with and without a context, and every group
    of the first part as one ragged batch call.  What the family reaches is asserted in test_pose_refit_cpu.py"""
    fails = []
    posed = []
    for k in range(PARITY_CASES):
        c = parity_case(k)
        posed.append(pr.recover_pose(c["recs"], c["record"], c["K1"], c["K2"], c["threshold"], c["max_depth"])[0])
    members = [family_case(j, posed) for j in range(FAMILY_CASES)]
    for m in members:
        m["pairs"] = _pairs(ah, m["recs"])
    for j, m in enumerate(members):
        n = len(m["pairs"])
        want = pz.refine_pose(m["pairs"], m["K1"], m["record"], m["K2"], m["threshold"], m["max_depth"], m["rounds"])
        got, gm, gx = gpu_refine(ah, torch, m["pairs"], m["K1"], m["record"], m["K2"], m["threshold"], m["max_depth"], m["rounds"],
                                 ctx=det.ctx if m["ctx"] else None)
        try:
            assert_same(got, gm[:n], gx[:12 * n], *want, (j, m["kind"]))
            assert (gm[n:] == 0xEE).all() and (gx[12 * n:] == 0xEE).all(), (j, "written past the count")
        except AssertionError as e:
            fails.append(str(e)[:300])
    groups = sorted({m["group"] for m in members if m["group"] >= 0})
    for g in groups:
        ms = [m for m in members if m["group"] == g]
        m0 = ms[0]
        lists = [m["pairs"] for m in ms]
        stride = max(1, max(len(lst) for lst in lists))
        out, masks, xyz = _batch(ah, torch, det, lists, stride, [m["record"] for m in ms], m0["K1"], m0["K2"], m0["threshold"],
                                 m0["max_depth"], m0["rounds"])
        for slot, m in enumerate(ms):
            n = len(lists[slot])
            want = pz.refine_pose(lists[slot], m0["K1"], m["record"], m0["K2"], m0["threshold"], m0["max_depth"], m0["rounds"])
            try:
                assert_same(out[slot], masks[slot, :n], xyz[slot, :12 * n], *want, ("batch", g, slot))
                assert (masks[slot, n:] == 0xEE).all() and (xyz[slot, 12 * n:] == 0xEE).all(), ("batch", g, slot, "past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    stride = 1100
    counts = [0, 4, 5, 900, stride + 50, 900, 900]
    lists, records = [], []
    for k, c in enumerate(counts):
        recs, F, K = scene(synth, stride, 40 + k)
        lst = as_pairs(ah, recs)[:min(c, stride)]
        lists.append(lst)
        records.append(pr.recover_pose(as_pairs(ah, recs), F, K, None, 1.0, 50.0)[0])
    records[5] = records[5].copy()
    records[5]["candidate"] = -1                                        # a no-pose record with a usable R
    records[6] = records[6].copy()
    records[6]["R"][4] = np.nan                                         # a NaN in R
    # the device reads the raw counts: stride + 50 is clamped to the stride there
    out, masks, xyz = _batch(ah, torch, det, lists, stride, records, K, None, 1.0, 50.0, 3, counts=counts)
    for k, lst in enumerate(lists):
        n = len(lst)
        s, m, x = gpu_refine(ah, torch, lst, K, records[k], None, 1.0, 50.0, 3)
        assert_same(out[k], masks[k, :n], xyz[k, :12 * n], s, m[:n], x[:12 * n], ("batch vs single", k))
        assert_same(s, m[:n], x[:12 * n], *pz.refine_pose(lst, K, records[k], None, 1.0, 50.0, 3), ("reference", k))
        assert (masks[k, n:] == 0xEE).all() and (xyz[k, 12 * n:] == 0xEE).all()
    assert out[4]["n"] == stride and out[3]["candidate"] == 4 and out[4]["candidate"] == 4
    ident = np.eye(3, dtype=np.float32).reshape(9)
    for k in (5, 6):
        assert out[k]["candidate"] == -1 and np.array_equal(out[k]["R"], ident) and not out[k]["t"].any()
        assert out[k]["inliers"] == 0 and out[k]["in_front"] == 0 and not masks[k, :len(lists[k])].any()
    assert out[0]["candidate"] == records[0]["candidate"] and out[0]["n"] == 0 and out[0]["in_front"] == 0


def test_chain_without_syncs(ah, torch, synth, det):
    """two three-view scenes as four lists in hak_match_knn2_batch's layout: find_fundamental_batch -> refine_fundamental_batch ->
    recover_pose_batch -> refine_pose_batch -> link_tracks_batch -> solve_pnp_batch with one hak_sync at the end equals the same
    calls made one at a time with downloads in between, and every refined record, mask and xyz equals the statement applied to
    the downloaded hak_recover_pose_batch record"""
    mp = 2000
    scenes = [synth.three_view_scene(1, 400, 0.5, 0.3), synth.three_view_scene(2, 300, 0.3, 0.2)]
    lists = np.zeros(4 * mp, ah.MATCH_PAIR_DTYPE)
    counts = np.zeros(4, np.int32)
    for j, sc in enumerate(scenes):
        for side, lst in enumerate((sc[3], sc[4])):
            lists[(2 * j + side) * mp:(2 * j + side) * mp + len(lst)] = lst
            counts[2 * j + side] = len(lst)
    K = ah.intrinsics(scenes[0][0])
    d_l, d_c = upload(torch, lists), torch.from_numpy(counts).cuda()
    lib, ctx, kp = ah.lib, det.ctx, K.ctypes.data

    def run(sync_between):
        fund = torch.zeros(4 * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        pose = torch.zeros(4 * SIZE, dtype=torch.uint8, device="cuda")
        pmask = torch.full((4 * mp,), 0xEE, dtype=torch.uint8, device="cuda")
        xyz = torch.full((4 * mp * 12,), 0xEE, dtype=torch.uint8, device="cuda")
        corr = torch.full((2 * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        ncorr = torch.zeros(2, dtype=torch.int32, device="cuda")
        absp = torch.zeros(2 * 64, dtype=torch.uint8, device="cuda")
        steps = [
            lambda: lib.hak_find_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 256, 1.0, 5, fund.data_ptr(), None),
            lambda: lib.hak_refine_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 1.0, 3, fund.data_ptr(), None),
            lambda: lib.hak_recover_pose_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, fund.data_ptr(), kp, kp, 1.0, 50.0,
                                               pose.data_ptr(), pmask.data_ptr(), xyz.data_ptr()),
            lambda: lib.hak_refine_pose_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, kp, kp, 2.0, 50.0, 8, pose.data_ptr(),
                                              pmask.data_ptr(), xyz.data_ptr()),
            lambda: lib.hak_link_tracks_batch(ctx, d_l.data_ptr(), 2 * mp, d_c.data_ptr(), 2, pmask.data_ptr(), xyz.data_ptr(),
                                              d_l.data_ptr() + 32 * mp, 2 * mp, d_c.data_ptr() + 4, 2, 2, corr.data_ptr(), mp,
                                              ncorr.data_ptr()),
            lambda: lib.hak_solve_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), 2, kp, 64, 2.0, 9, absp.data_ptr(), None),
        ]
        got = []
        for step in steps:
            ah.check(step())
            if sync_between:
                ah.check(lib.hak_sync(ctx))
                got.append(pose.cpu().numpy().copy())
        ah.check(lib.hak_sync(ctx))
        return [t.cpu().numpy() for t in (pose, pmask, xyz, corr, ncorr, absp)], got

    chain, _ = run(False)
    stepwise, downloads = run(True)
    for a, b in zip(chain, stepwise):
        assert np.array_equal(a, b)
    pose, pmask, xyz, corr, ncorr, absp = chain
    before = downloads[2].view(ah.POSE_DTYPE)                           # the records hak_recover_pose_batch wrote
    recs = pose.view(ah.POSE_DTYPE)
    for k in range(4):
        n = int(counts[k])
        lst = lists[k * mp:k * mp + n]
        want = pz.refine_pose(lst, K, before[k], None, 2.0, 50.0, 8)
        assert_same(recs[k], pmask[k * mp:k * mp + n], xyz[12 * k * mp:12 * (k * mp + n)], *want, ("chain", k))
        assert (pmask[k * mp + n:(k + 1) * mp] == 0xEE).all() and (xyz[12 * (k * mp + n):12 * (k + 1) * mp] == 0xEE).all()
        assert before[k]["candidate"] >= 0 and recs[k]["candidate"] == 4 and recs[k]["in_front"] >= before[k]["in_front"] > 100
    ab = absp.view(ah.ABS_POSE_DTYPE)
    assert (ab["hypothesis"] >= 0).all() and (ncorr > 100).all() and (ab["inliers"] > 40).all()


def test_refitted_record_is_a_view_for_what_follows(ah, torch, synth, det):
    """the refitted record, left on the device by hak_refine_pose_batch, read there as HAK_VIEW_RELATIVE by hak_triangulate_batch
    and hak_match_projected_batch: each equals its own statement given the same record, so candidate = 4 reads as a model"""
    from test_gpu_projected_match import upload as upload_any
    from test_gpu_triangulate import REC
    from test_gpu_triangulate import assert_same as assert_tri
    from test_guided_match_cpu import IDENTITY, build_pair
    from test_projected_match_cpu import K_LIFT, identity_list, lift, shuffled
    mp = 1100
    recs, flags, rec1, K, R, t = noisy_case(synth, 1000, 0.6, 6)
    m = as_pairs(ah, recs)
    rec0 = pr.recover_pose(m, rec1, K, None, 1.0, 50.0)[0]
    d, d_cnt = upload(torch, m), torch.tensor([len(m)], dtype=torch.int32, device="cuda")
    pose = upload(torch, np.array([rec0], ah.POSE_DTYPE))
    k1 = ah.intrinsics(K)
    ah.check(ah.lib.hak_refine_pose_batch(det.ctx, d.data_ptr(), mp, d_cnt.data_ptr(), 1, k1.ctypes.data, k1.ctypes.data, 2.0, 50.0, 8,
                                          pose.data_ptr(), None, None))
    mask = torch.full((mp,), 0xEE, dtype=torch.uint8, device="cuda")
    xyz = torch.full((12 * mp,), 0xEE, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    ah.check(ah.lib.hak_triangulate_batch(det.ctx, d.data_ptr(), mp, d_cnt.data_ptr(), 1, 1, None, ah.VIEW_IDENTITY, 0, pose.data_ptr(),
                                          ah.VIEW_RELATIVE, 1, k1.ctypes.data, k1.ctypes.data, 2.0, 50.0, 0.0, out.data_ptr(),
                                          mask.data_ptr(), xyz.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    prec = pose.cpu().numpy().view(ah.POSE_DTYPE)[0]
    assert prec.tobytes() == np.array(pz.refine_pose(m, K, rec0, None, 2.0, 50.0, 8)[0], ah.POSE_DTYPE).tobytes()
    assert prec["candidate"] == 4
    want = tr.triangulate(m, None, prec, K, None, 2.0, 50.0, 0.0)
    raw = out.cpu().numpy()
    assert_tri((raw[:REC].view(ah.TRIANGULATION_DTYPE)[0], mask.cpu().numpy(), xyz.cpu().numpy()), want, len(m), "refitted view")
    assert want[0]["model"] == 1 and want[0]["kept"] > 600
    # landmarks lifted under the refitted pose, re-matched under the record on the device
    nA = n2 = 300
    M = np.concatenate([prec["R"], prec["t"]]).astype(np.float32)
    q, tt = build_pair(nA, n2, 300, ah.POINT_DTYPE, H=IDENTITY)
    pts, _ = lift(synth, q, 310, M=M)
    A, D, lmask = shuffled(identity_list(nA), pts, q, 320)
    dA, dX, dD, dT = (upload_any(torch, a) for a in (A, pts, D, tt))
    dM = upload_any(torch, lmask, np.uint8)
    cA, cT = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (nA, n2))
    d_out = torch.full((nA * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    kl = ah.intrinsics(K_LIFT)
    ah.check(ah.lib.hak_match_projected_batch(det.ctx, dA.data_ptr(), nA, cA.data_ptr(), 1, dM.data_ptr(), dX.data_ptr(), dD.data_ptr(),
                                              nA, cA.data_ptr(), 1, dT.data_ptr(), n2, cT.data_ptr(), 1, 1, pose.data_ptr(),
                                              ah.VIEW_RELATIVE, 1, kl.ctypes.data, 3.0, 4, 5, 1, 0, d_out.data_ptr(), nA, cnt.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    ref, _ = pm.match_projected(A, lmask, pts, D, tt, prec, K_LIFT, 3.0, (4, 5), True, 0)
    got, c = d_out.cpu().numpy(), cnt.cpu().numpy()
    assert c[0] == len(ref) > 50 and c[1] == -7
    assert got[:32 * len(ref)].tobytes() == ref.tobytes() and (got[32 * len(ref):] == 0xEE).all()


def test_python_wrapper(ah, torch, synth):
    recs, flags, rec1, K, R, t = noisy_case(synth, 400, 0.5, 7)
    pairs = as_pairs(ah, recs)
    rec0 = pr.recover_pose(pairs, rec1, K, None, 1.0, 50.0)[0]
    keep = rec0.copy()
    want = pz.refine_pose(pairs, K, rec0, None, 2.0, 50.0, 8)
    got, gm, gx = ah.refinePose(pairs, K, rec0, None, 2.0, 50.0, 8)
    assert got.dtype == ah.POSE_DTYPE and gm.dtype == np.uint8 and gx.dtype == np.float32 and gx.shape == (len(pairs), 3)
    assert rec0.tobytes() == keep.tobytes()
    assert_same(got, gm, gx, *want, "wrapper")
    dev = ah.refinePose(upload(torch, pairs), ah.intrinsics(K), rec0, threshold=2.0, max_depth=50.0, rounds=8)    # used in place
    assert_same(*dev, *want, "wrapper, device list")
    assert got["candidate"] == 4 and got["in_front"] >= pz.count_under(pairs, rec0, K, None, 2.0, 50.0)
    plain = ah.refinePose(pairs, K, rec0)                               # the defaults: 1 px, no depth limit, 3 rounds
    assert_same(*plain, *pz.refine_pose(pairs, K, rec0), "wrapper, defaults")


def test_demo_pose_refine_leg(ah, golden, tmp_path):
    """`hipakaze_demo --refine 3 --pose FX FY CX CY --pose-refine 3` (akaze::cuRefinePose): the dumped refitted R, t, count and mask
    equal the statement on the dumped list and pose; without --pose-refine the output has no such line"""
    from test_gpu_dropin import write_pgm
    left, right = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    hh, ww = golden.lr_u8["left"].shape
    K = (1.2 * ww, 1.2 * ww, ww / 2.0, hh / 2.0)
    dump = str(tmp_path / "pose.bin")
    cmd = ["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--refine", "3", "--pose"] + \
          [repr(float(v)) for v in K]
    r = subprocess.run(cmd + ["--pose-refine", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Relative pose from the fundamental matrix" in r.stdout and "Refit of the relative pose" in r.stdout
    raw = open(dump, "rb").read()
    off = 0
    for _ in range(2):                                                  # the float and the FAST path's point sections
        n1, n2 = np.frombuffer(raw, np.int32, 2, off)
        off += 8 + 104 * int(n1 + n2)
    n = int(np.frombuffer(raw, np.int32, 1, off)[0])
    off += 44
    lst = np.frombuffer(raw, ah.MATCH_PAIR_DTYPE, n, off).copy()
    off += 33 * n                                                       # the list and the fundamental refit's mask
    rec = np.frombuffer(raw, ah.POSE_DTYPE, 1, off)[0].copy()
    off += 64 + 13 * n                                                  # the pose record, its mask and points
    R = np.frombuffer(raw, np.float32, 9, off)
    t = np.frombuffer(raw, np.float32, 3, off + 36)
    count = int(np.frombuffer(raw, np.int32, 1, off + 48)[0])
    mask = np.frombuffer(raw, np.uint8, n, off + 52)
    assert off + 52 + n == len(raw) and n > 100 and rec["candidate"] >= 0
    rec["candidate"] = 0                                                # cuRefinePose hands R and t over, not the record
    want, wm, _ = pz.refine_pose(lst, K, rec, None, 1.0, INF, 3)
    assert R.tobytes() == want["R"].tobytes() and t.tobytes() == want["t"].tobytes() and count == want["in_front"]
    assert np.array_equal(mask, wm) and count >= pz.count_under(lst, rec, K, None, 1.0, INF)
    plain = subprocess.run(cmd, capture_output=True, text=True)
    assert plain.returncode == 0 and "Refit of the relative pose" not in plain.stdout and "Relative pose" in plain.stdout


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls, keep, rec = refusals(ah, det.ctx, d.data_ptr(), cnt.data_ptr())
    assert len(calls) >= 47
    ok = np.zeros((), ah.POSE_DTYPE)
    K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))
    for k, (fn, args) in enumerate(calls):
        ah.check(ah.lib.hak_refine_pose(None, d.data_ptr(), 0, K.ctypes.data, K.ctypes.data, 1.0, INF, 1, None, None,
                                        ok.ctypes.data))               # succeeds in between
        assert ok["n"] == 0 and ok["candidate"] == -1                   # (an all-zero record: t = 0 has no F)
        ok["candidate"] = 0
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    ah.check(ah.lib.hak_sync(det.ctx))
    assert not d.any() and not cnt.any() and not rec.tobytes().strip(b"\0")

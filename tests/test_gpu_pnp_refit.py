"""GPU suite: Gauss-Newton refit of the absolute pose (hak_refine_pnp / hak_refine_pnp_batch, kernels_pnprefit.hip) bit for bit
against its numpy statement tests/pnp_refit_ref.py -- every R / t bit, inliers, hypothesis, solution, n and every mask byte.  The
inputs are the STATEMENT's RANSAC records (pnp_ref), so the device's own RANSAC can neither mask nor cause a difference."""
import numpy as np
import pytest

import pnp_ref as pn
import pnp_refit_ref as pf
from test_gpu_fundamental import det, synth, torch, upload  # noqa: F401 (fixtures)
from test_gpu_pnp import POSE_SIZE, assert_same, scene
from test_pnp_cpu import K_TABLE, PARITY_CASES, parity_case
from test_pnp_refit_cpu import FAMILY_CASES, family_case, refusals

pytestmark = pytest.mark.gpu

SIZES = [0, 2, 3, 4, 5, 63, 64, 65, 129, 1340]     # the first usable counts, the wave edges of the summation order
ROUNDS = [1, 3, 8]


def gpu_refine(ah, torch, corr, K, record, threshold, rounds, ctx=None, with_mask=True):
    """one hak_refine_pnp call -> (record, the whole 0xEE-prefilled mask buffer)"""
    n = len(corr)
    d = upload(torch, corr)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    k = ah.intrinsics(K)
    rec = np.array(record, ah.ABS_POSE_DTYPE).reshape(())
    ah.check(ah.lib.hak_refine_pnp(ctx, d.data_ptr(), n, k.ctypes.data, threshold, rounds, mask.data_ptr() if with_mask else None,
                                   rec.ctypes.data))
    return rec, mask.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    corr = scene(synth, n, n)
    refined = 0
    for thr in (1.0, 2.5):
        rec0, _ = pn.solve_pnp(corr, K_TABLE, 64, thr, n)
        for rounds in ROUNDS:
            want, wm = pf.refine_pnp(corr, K_TABLE, rec0, thr, rounds)
            for ctx in (None, det.ctx):
                got, gm = gpu_refine(ah, torch, corr, K_TABLE, rec0, thr, rounds, ctx=ctx)
                assert_same(got, gm[:n], want, wm, (n, thr, rounds, ctx is not None))
                assert (gm[n:] == 0xEE).all()
            got, gm = gpu_refine(ah, torch, corr, K_TABLE, rec0, thr, rounds, with_mask=False)
            assert got.tobytes() == want.tobytes() and (gm == 0xEE).all()   # d_mask = NULL: same record, buffer untouched
            refined += int(want["solution"]) == pf.REFINED_SOLUTION
    if n < 3:
        assert want["hypothesis"] == -1 and want["inliers"] == 0
    if n == 3:
        assert want["hypothesis"] >= 0 and want["solution"] != pf.REFINED_SOLUTION      # a model, and too few inliers for a round
    if n >= 63:
        assert refined > 0


def test_refining_a_refined_record_again(ah, torch, synth):
    corr = scene(synth, 700, 12)
    rec0, _ = pn.solve_pnp(corr, K_TABLE, 64, 2.0, 1)
    a, _ = gpu_refine(ah, torch, corr, K_TABLE, rec0, 2.0, 1)
    assert a["solution"] == 4
    b, bm = gpu_refine(ah, torch, corr, K_TABLE, a, 2.0, 2)
    want, wm = pf.refine_pnp(corr, K_TABLE, a, 2.0, 2)
    assert_same(b, bm, want, wm, "second refit")
    assert b["inliers"] >= a["inliers"] and b["solution"] == 4
    c, cm = gpu_refine(ah, torch, corr, K_TABLE, b, 0.8, 1)              # another threshold: counted at this call's
    want, wm = pf.refine_pnp(corr, K_TABLE, b, 0.8, 1)
    assert_same(c, cm, want, wm, "third refit")


def _batch(ah, torch, det, lists, stride, records, K, thr, rounds, extra=1, counts=None):
    """one hak_refine_pnp_batch call over `lists`; `counts` = the counts the device reads (default: the lists' lengths); `extra`
    records past npairs are sentinels"""
    np_ = len(lists)
    allc = np.zeros(np_ * stride, ah.CORR3D_DTYPE)
    allc["X"] = np.nan                                                  # past a count: must not be read as usable
    for k, lst in enumerate(lists):
        allc[k * stride:k * stride + len(lst)] = lst
    d = upload(torch, allc)
    d_cnt = torch.tensor(counts if counts is not None else [len(lst) for lst in lists], dtype=torch.int32, device="cuda")
    host = np.full((np_ + extra) * POSE_SIZE, 0xEE, np.uint8)
    host[:np_ * POSE_SIZE] = np.array(records, ah.ABS_POSE_DTYPE).view(np.uint8)
    d_io = torch.from_numpy(host).cuda()
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K)
    ah.check(ah.lib.hak_refine_pnp_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, k1.ctypes.data, thr, rounds,
                                         d_io.data_ptr(), d_mask.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_io.cpu().numpy()
    assert (raw[np_ * POSE_SIZE:] == 0xEE).all()                        # records past npairs are untouched
    return raw[:np_ * POSE_SIZE].view(ah.ABS_POSE_DTYPE), d_mask.cpu().numpy().reshape(np_, stride)


def test_randomised_parity(ah, torch, det):
    """the family of test_pnp_refit_cpu.family_case -- the parity_case inputs of test_pnp_cpu with their statement records at the
    case's own threshold and at 0.3 of it, and the built on-axis members -- as single calls, with and without a context, and every
    group of the first part as one ragged batch call.  What the family reaches (every exit of the rule) is asserted in
    test_pnp_refit_cpu.py"""
    fails = []
    solved = [pn.solve_pnp(c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"])[0]
              for c in (parity_case(k) for k in range(PARITY_CASES))]
    members = [family_case(j, solved) for j in range(FAMILY_CASES)]
    for j, m in enumerate(members):
        n = len(m["corr"])
        want, wm = pf.refine_pnp(m["corr"], m["K"], m["record"], m["threshold"], m["rounds"])
        got, gm = gpu_refine(ah, torch, m["corr"], m["K"], m["record"], m["threshold"], m["rounds"], ctx=det.ctx if m["ctx"] else None)
        try:
            assert_same(got, gm[:n], want, wm, (j, m["kind"]))
            assert (gm[n:] == 0xEE).all(), (j, "written past the count")
        except AssertionError as e:
            fails.append(str(e)[:300])
    groups = sorted({m["group"] for m in members if m["group"] >= 0})
    for g in groups:
        ms = [m for m in members if m["group"] == g]
        m0 = ms[0]
        lists = [m["corr"] for m in ms]
        stride = max(1, max(len(lst) for lst in lists))
        out, masks = _batch(ah, torch, det, lists, stride, [m["record"] for m in ms], m0["K"], m0["threshold"], 3)
        for slot, m in enumerate(ms):
            n = len(lists[slot])
            want, wm = pf.refine_pnp(lists[slot], m0["K"], m["record"], m0["threshold"], 3)
            try:
                assert_same(out[slot], masks[slot, :n], want, wm, ("batch", g, slot))
                assert (masks[slot, n:] == 0xEE).all(), ("batch", g, slot, "written past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    stride = 1100
    counts = [0, 3, 4, 900, stride + 50, 900, 900]
    lists, records = [], []
    for k, c in enumerate(counts):
        lst = scene(synth, stride, 40 + k)[:min(c, stride)]
        lists.append(lst)
        records.append(pn.solve_pnp(lst, K_TABLE, 64, 2.0, 77)[0])
    records[5] = records[5].copy()
    records[5]["hypothesis"] = -1                                       # a no-model record with a usable R
    records[6] = records[6].copy()
    records[6]["R"][4] = np.nan                                         # a NaN in R
    # the device reads the raw counts: stride + 50 is clamped to the stride there
    out, masks = _batch(ah, torch, det, lists, stride, records, K_TABLE, 2.0, 3, counts=counts)
    for k, lst in enumerate(lists):
        n = len(lst)
        s, m = gpu_refine(ah, torch, lst, K_TABLE, records[k], 2.0, 3)
        assert_same(out[k], masks[k, :n], s, m[:n], ("batch vs single", k))
        want, wm = pf.refine_pnp(lst, K_TABLE, records[k], 2.0, 3)
        assert_same(s, m[:n], want, wm, ("reference", k))
        assert (masks[k, n:] == 0xEE).all()
    assert out[4]["n"] == stride and out[3]["solution"] == 4 and out[4]["solution"] == 4
    ident = np.eye(3, dtype=np.float32).reshape(9)
    for k in (0, 5, 6):
        assert out[k]["hypothesis"] == -1 and np.array_equal(out[k]["R"], ident) and not out[k]["t"].any()
        assert out[k]["inliers"] == 0 and out[k]["solution"] == 0 and not masks[k, :len(lists[k])].any()


def test_chain_fundamental_refine_pose_link_pnp_refine(ah, torch, synth, det):
    """the chain of test_gpu_pnp.test_chain_fundamental_refine_pose_link_pnp (two three-view scenes as four lists in
    hak_match_knn2_batch's layout) with hak_refine_pnp_batch appended: one hak_sync at the end equals the same calls made one at a
    time with downloads in between, and every refined record equals the statement applied to the downloaded list and the downloaded
    hak_solve_pnp_batch record"""
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
        pose = torch.zeros(4 * 64, dtype=torch.uint8, device="cuda")
        pmask = torch.zeros(4 * mp, dtype=torch.uint8, device="cuda")
        xyz = torch.zeros(4 * mp * 3, dtype=torch.float32, device="cuda")
        corr = torch.full((2 * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        ncorr = torch.zeros(2, dtype=torch.int32, device="cuda")
        absp = torch.zeros(2 * POSE_SIZE, dtype=torch.uint8, device="cuda")
        amask = torch.full((2 * mp,), 0xEE, dtype=torch.uint8, device="cuda")
        steps = [
            lambda: lib.hak_find_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 256, 1.0, 5, fund.data_ptr(), None),
            lambda: lib.hak_refine_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 1.0, 3, fund.data_ptr(), None),
            lambda: lib.hak_recover_pose_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, fund.data_ptr(), kp, kp, 1.0, 50.0,
                                               pose.data_ptr(), pmask.data_ptr(), xyz.data_ptr()),
            lambda: lib.hak_link_tracks_batch(ctx, d_l.data_ptr(), 2 * mp, d_c.data_ptr(), 2, pmask.data_ptr(), xyz.data_ptr(),
                                              d_l.data_ptr() + 32 * mp, 2 * mp, d_c.data_ptr() + 4, 2, 2, corr.data_ptr(), mp,
                                              ncorr.data_ptr()),
            lambda: lib.hak_solve_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), 2, kp, 64, 2.0, 9, absp.data_ptr(), None),
            lambda: lib.hak_refine_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), 2, kp, 2.0, 3, absp.data_ptr(),
                                             amask.data_ptr()),
        ]
        got = []
        for step in steps:
            ah.check(step())
            if sync_between:
                ah.check(lib.hak_sync(ctx))
                got.append(absp.cpu().numpy().copy())
        ah.check(lib.hak_sync(ctx))
        return [t.cpu().numpy() for t in (corr, ncorr, absp, amask)], got

    chain, _ = run(False)
    stepwise, downloads = run(True)
    for a, b in zip(chain, stepwise):
        assert np.array_equal(a, b)
    corr, ncorr, absp, amask = chain
    clists = corr.view(ah.CORR3D_DTYPE).reshape(2, mp)
    before = downloads[4].view(ah.ABS_POSE_DTYPE)                       # the records hak_solve_pnp_batch wrote
    recs = absp.view(ah.ABS_POSE_DTYPE)
    for j, sc in enumerate(scenes):
        n = int(ncorr[j])
        lst = clists[j, :n].copy()
        assert pn.solve_pnp(lst, K, 64, 2.0, 9)[0].tobytes() == before[j].tobytes()
        want, wm = pf.refine_pnp(lst, K, before[j], 2.0, 3)
        assert_same(recs[j], amask[j * mp:j * mp + n], want, wm, ("chain", j))
        assert (amask[j * mp + n:(j + 1) * mp] == 0xEE).all()
        assert before[j]["hypothesis"] >= 0 and recs[j]["inliers"] >= before[j]["inliers"] > 40 and recs[j]["n"] == n > 100
        assert recs[j]["solution"] == 4


def test_python_wrapper(ah, torch, synth):
    corr = scene(synth, 500, 4)
    rec0, _ = pn.solve_pnp(corr, K_TABLE, 64, 2.0, 3)
    keep = rec0.copy()
    want, wm = pf.refine_pnp(corr, K_TABLE, rec0, 2.0, 3)
    got, gm = ah.refinePnP(corr, K_TABLE, rec0)
    assert got.dtype == ah.ABS_POSE_DTYPE and gm.dtype == np.uint8 and rec0.tobytes() == keep.tobytes()
    assert_same(got, gm, want, wm, "wrapper")
    dev, dm = ah.refinePnP(upload(torch, corr), ah.intrinsics(K_TABLE), rec0, 2.0, 3)     # a device tensor is used in place
    assert_same(dev, dm, want, wm, "wrapper, device list")
    assert got["solution"] == 4 and got["inliers"] >= rec0["inliers"]


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls, keep, rec = refusals(ah, det.ctx, d.data_ptr(), cnt.data_ptr())
    assert len(calls) >= 34
    ok = np.zeros((), ah.ABS_POSE_DTYPE)
    K = ah.intrinsics(K_TABLE)
    for k, (fn, args) in enumerate(calls):
        ah.check(ah.lib.hak_refine_pnp(None, d.data_ptr(), 0, K.ctypes.data, 1.0, 1, None, ok.ctypes.data))     # succeeds in between
        assert ok["n"] == 0
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    ah.check(ah.lib.hak_sync(det.ctx))
    assert not d.any() and not cnt.any() and not rec.tobytes().strip(b"\0")


def test_chain_from_images(ah, torch, synth):
    """the whole chain on 256 x 192 synth images -- two triples (I0, I1, I1, I2), the middle image detected twice: detect -> knn2 ->
    find_fundamental_batch -> refine_fundamental_batch -> recover_pose_batch -> link_tracks_batch -> solve_pnp_batch ->
    refine_pnp_batch with one hak_sync at the end equals the same calls made one at a time with downloads in between; each refined
    record equals the statement applied to the downloaded list and the downloaded hak_solve_pnp_batch record"""
    w, h = 256, 192
    p = ah.iAlignUp(w, 128)
    imgs = []
    for s in (1, 2):
        a, b = synth.pair(w, h, s)
        imgs += [a, b, b, synth.warp(b, -2.0, 0.97, (-6.0, 9.0))]
    B, mp, nt = len(imgs), 1000, len(imgs) // 4
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    dt = ah.Akazer()
    dt.init((w, h, p), max_pts=mp, batch=B)
    K = ah.intrinsics((300.0, 300.0, w / 2.0, h / 2.0))
    lib, ctx, kp = ah.lib, dt.ctx, K.ctypes.data

    def run(sync_between):
        pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
        num = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.zeros(B // 2 * mp * 32, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B // 2, dtype=torch.int32, device="cuda")
        fund = torch.zeros(B // 2 * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        pose = torch.zeros(B // 2 * 64, dtype=torch.uint8, device="cuda")
        front = torch.zeros(B // 2 * mp, dtype=torch.uint8, device="cuda")
        xyz = torch.zeros(B // 2 * mp * 3, dtype=torch.float32, device="cuda")
        corr = torch.zeros(nt * mp * 32, dtype=torch.uint8, device="cuda")
        ncorr = torch.zeros(nt, dtype=torch.int32, device="cuda")
        absp = torch.zeros(nt * POSE_SIZE, dtype=torch.uint8, device="cuda")
        amask = torch.full((nt * mp,), 0xEE, dtype=torch.uint8, device="cuda")
        steps = [
            lambda: lib.hak_detect_and_compute_batch(ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1),
            lambda: lib.hak_match_knn2_batch(ctx, pts.data_ptr(), num.data_ptr(), B // 2, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()),
            lambda: lib.hak_find_fundamental_batch(ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 256, 1.0, 0, fund.data_ptr(), None),
            lambda: lib.hak_refine_fundamental_batch(ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, 1.0, 3, fund.data_ptr(), None),
            lambda: lib.hak_recover_pose_batch(ctx, out.data_ptr(), mp, cnt.data_ptr(), B // 2, fund.data_ptr(), kp, kp, 1.0, 50.0,
                                               pose.data_ptr(), front.data_ptr(), xyz.data_ptr()),
            lambda: lib.hak_link_tracks_batch(ctx, out.data_ptr(), 2 * mp, cnt.data_ptr(), 2, front.data_ptr(), xyz.data_ptr(),
                                              out.data_ptr() + 32 * mp, 2 * mp, cnt.data_ptr() + 4, 2, nt, corr.data_ptr(), mp,
                                              ncorr.data_ptr()),
            lambda: lib.hak_solve_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), nt, kp, 256, 2.0, 9, absp.data_ptr(), None),
            lambda: lib.hak_refine_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), nt, kp, 2.0, 3, absp.data_ptr(),
                                             amask.data_ptr()),
        ]
        got = []
        for step in steps:
            ah.check(step())
            if sync_between:
                ah.check(lib.hak_sync(ctx))
                got.append(absp.cpu().numpy().copy())
        ah.check(lib.hak_sync(ctx))
        return [t.cpu().numpy() for t in (corr, ncorr, absp, amask)], got

    chain, _ = run(False)
    stepwise, downloads = run(True)
    for a, b in zip(chain, stepwise):
        assert np.array_equal(a, b)
    corr, ncorr, absp, amask = chain
    lists = corr.view(ah.CORR3D_DTYPE).reshape(nt, mp)
    before = downloads[6].view(ah.ABS_POSE_DTYPE)                       # the records hak_solve_pnp_batch wrote
    recs = absp.view(ah.ABS_POSE_DTYPE)
    for k in range(nt):
        n = int(ncorr[k])
        want, wm = pf.refine_pnp(lists[k, :n].copy(), K, before[k], 2.0, 3)
        assert_same(recs[k], amask.reshape(nt, mp)[k, :n], want, wm, ("image chain", k))
        assert (amask.reshape(nt, mp)[k, n:] == 0xEE).all()
        print(f"image chain {k}: {n} correspondences, inliers {before[k]['inliers']} -> {recs[k]['inliers']}, hypothesis "
              f"{before[k]['hypothesis']}, solution {before[k]['solution']} -> {recs[k]['solution']}")
        assert recs[k]["inliers"] >= before[k]["inliers"] and recs[k]["n"] == n
    dt.close()

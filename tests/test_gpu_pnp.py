"""GPU suite: track linking and RANSAC absolute pose (hak_link_tracks(_batch), hak_solve_pnp(_batch), kernels_pnp.hip) byte for
byte against their numpy statements tests/link_ref.py and tests/pnp_ref.py -- every byte of the record, the mask, the
correspondences and the counts.

Launch shapes (hak_homography_blocks, shared with the other RANSAC estimators): a single list takes hp = 16 hypotheses per score
block at every iteration count, so ITERATIONS covers 1, 4, 4, 5 and 64 score blocks and 1, 1, 1, 2 and 16 model blocks (63 and 65
leave a partly filled block of each kind); the ragged batch of five lists takes hp = 32, 64, 128 and 256 at BATCH_ITERATIONS
(each test asks the library's launch rule, hak_op_ransac_shape, whether it still does).
The link's scatter takes 1 .. 64 blocks of 256 matches per pair: the single-call sizes give 1, 3, 4, 6, 20 and (20000 matches) the cap
of 64, the batch 16; its gather walks 1024 matches per step: 1023, 1024, 1025 and 2500 matches are one, one, two and three steps."""
import ctypes as C

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import link_ref as lr
import pnp_ref as pn
import pose_ref as pr
from test_gpu_fundamental import det, synth, torch, upload  # noqa: F401 (fixtures)
from test_pnp_cpu import K_TABLE, FOCAL, H, W, PARITY_CASES, corr_array, pairs, parity_case, refusals
from test_ransac_shapes_cpu import shape_of

pytestmark = pytest.mark.gpu

SIZES = [0, 2, 3, 4, 63, 64, 65, 129, 1340]
ITERATIONS = [1, 63, 64, 65, 1024]
BATCH_ITERATIONS = [(400, 32), (1024, 64), (1664, 128), (3200, 256)]    # (iterations, the hp five lists get)
POSE_SIZE = 64


def scene(synth, n, seed, noise=0.3, outliers=0.3):
    """n correspondences of one planted pose: 70 % projections with `noise` px of Gaussian noise, the rest uniformly random
    observations"""
    rng = np.random.default_rng(7000 + seed)
    R, t = synth.rotation_zyx(rng.uniform(-20, 20, 3)), rng.uniform(-1, 1, 3)
    z = rng.uniform(4.0, 12.0, n)
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)
    Xc = np.stack([(uv[:, 0] - W / 2.0) / FOCAL * z, (uv[:, 1] - H / 2.0) / FOCAL * z, z], axis=1)
    obs = uv + rng.normal(0.0, noise, uv.shape)
    out = rng.random(n) < outliers
    obs[out] = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)[out]
    return corr_array((Xc - t) @ R, obs)


def gpu_pnp(ah, torch, corr, K, iterations, threshold, seed, ctx=None, with_mask=True):
    """one hak_solve_pnp call -> (record, the whole 0xEE-prefilled mask buffer)"""
    n = len(corr)
    d = upload(torch, corr)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    k = ah.intrinsics(K)
    rec = np.zeros((), ah.ABS_POSE_DTYPE)
    ah.check(ah.lib.hak_solve_pnp(ctx, d.data_ptr(), n, k.ctypes.data, iterations, threshold, seed,
                                  mask.data_ptr() if with_mask else None, rec.ctypes.data))
    return rec, mask.cpu().numpy()


def assert_same(got, gmask, want, wmask, what=""):
    assert got.tobytes() == np.array(want, got.dtype).tobytes(), (what, got, want)
    assert np.array_equal(gmask, wmask), (what, "mask", int((gmask != wmask).sum()))


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    corr = scene(synth, n, n)
    assert shape_of(ah, 1, 256) == (16, 16)
    want, wm = pn.solve_pnp(corr, K_TABLE, 256, 1.5, n)
    for ctx in (None, det.ctx):
        got, gm = gpu_pnp(ah, torch, corr, K_TABLE, 256, 1.5, n, ctx=ctx)
        assert_same(got, gm[:n], want, wm, (n, ctx is not None))
    got, gm = gpu_pnp(ah, torch, corr, K_TABLE, 256, 1.5, n, with_mask=False)
    assert (gm == 0xEE).all() and got.tobytes() == np.array(want, got.dtype).tobytes()      # d_mask = NULL: buffer untouched
    assert (want["hypothesis"] >= 0) == (n >= 3)
    if n >= 63:
        assert want["inliers"] > 0.5 * n


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_iteration_counts_bit_exact(ah, torch, synth, det, iterations):
    corr = scene(synth, 300, 50)
    assert shape_of(ah, 1, iterations) == (16, (iterations + 15) // 16)  # the launch rule still gives what the docstring says
    for seed in (0, 0xFFFFFFFF):
        want, wm = pn.solve_pnp(corr, K_TABLE, iterations, 1.0, seed)
        got, gm = gpu_pnp(ah, torch, corr, K_TABLE, iterations, 1.0, seed, ctx=det.ctx if seed else None)
        assert_same(got, gm[:300], want, wm, (iterations, seed))
        assert want["hypothesis"] < iterations


def test_degenerate_and_non_finite_records(ah, torch, synth):
    corr = scene(synth, 200, 9, outliers=0.0)
    line = corr[:3].copy()
    for f in ("X", "Y", "Z"):
        line[f][2] = 0.5 * (line[f][0] + line[f][1])
    same = corr.copy()
    for f in ("X", "Y", "Z", "u", "v"):
        same[f] = same[f][0]
    cases = [("collinear", line), ("identical", same)]
    for f, bad in (("X", np.nan), ("Y", np.inf), ("Z", -np.inf), ("u", np.nan), ("v", np.inf)):
        some = corr.copy()
        some[f][::2] = bad
        cases.append(("half " + f, some))
        allbad = corr.copy()
        allbad[f] = bad
        cases.append(("all " + f, allbad))
    behind = corr.copy()
    for f in ("X", "Y", "Z"):
        behind[f][::3] = -behind[f][::3]                                # wrong points: mostly behind the camera
    cases.append(("behind", behind))
    for what, lst in cases:
        want, wm = pn.solve_pnp(lst, K_TABLE, 64, 1.0, 5)
        got, gm = gpu_pnp(ah, torch, lst, K_TABLE, 64, 1.0, 5)
        assert_same(got, gm[:len(lst)], want, wm, what)
        if what in ("collinear", "identical") or what.startswith("all"):
            assert want["hypothesis"] == -1 and not gm[:len(lst)].any()
        if what.startswith("half"):
            assert want["hypothesis"] >= 0 and not gm[:200:2].any() and gm[1:200:2].sum() > 90


def _pnp_batch(ah, torch, det, lists, stride, counts, K, iterations, thr, seed, with_mask=True):
    """one hak_solve_pnp_batch call; a record past npairs is a sentinel -> (records, masks)"""
    np_ = len(lists)
    allc = np.zeros(np_ * stride, ah.CORR3D_DTYPE)
    allc["X"] = np.nan                                                  # past a count: must not be read as usable
    for k, lst in enumerate(lists):
        allc[k * stride:k * stride + len(lst)] = lst
    d = upload(torch, allc)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_out = torch.full(((np_ + 1) * POSE_SIZE,), 0xEE, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((np_ * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K)
    ah.check(ah.lib.hak_solve_pnp_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, k1.ctypes.data, iterations, thr, seed,
                                        d_out.data_ptr(), d_mask.data_ptr() if with_mask else None))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_out.cpu().numpy()
    assert (raw[np_ * POSE_SIZE:] == 0xEE).all()
    return raw[:np_ * POSE_SIZE].view(ah.ABS_POSE_DTYPE), d_mask.cpu().numpy().reshape(np_, stride)


@pytest.fixture(scope="module")
def ragged(synth):
    stride = 800
    counts = [0, 3, 64, 700, stride + 50]                               # the device reads the raw counts: the last is clamped
    return stride, counts, [scene(synth, stride, 20 + k)[:min(c, stride)] for k, c in enumerate(counts)]


@pytest.mark.parametrize("iterations,hp", BATCH_ITERATIONS)
def test_batch_ragged_bit_exact(ah, torch, det, ragged, iterations, hp):
    stride, counts, lists = ragged
    assert shape_of(ah, len(lists), iterations) == (hp, (iterations + hp - 1) // hp)
    out, masks = _pnp_batch(ah, torch, det, lists, stride, counts, K_TABLE, iterations, 1.0, 11)
    for k, lst in enumerate(lists):
        n = len(lst)
        want, wm = pn.solve_pnp(lst, K_TABLE, iterations, 1.0, 11)
        assert_same(out[k], masks[k, :n], want, wm, ("batch vs statement", k, iterations))
        assert (masks[k, n:] == 0xEE).all()                             # nothing past a count
    assert out[4]["n"] == stride and out[0]["hypothesis"] == -1 and out[0]["n"] == 0 and out[3]["inliers"] > 350
    if hp == 64:
        for k, lst in enumerate(lists):
            s, sm = gpu_pnp(ah, torch, lst, K_TABLE, iterations, 1.0, 11)
            assert_same(out[k], masks[k, :len(lst)], s, sm[:len(lst)], ("batch vs single", k))
        bare = _pnp_batch(ah, torch, det, lists, stride, counts, K_TABLE, iterations, 1.0, 11, with_mask=False)
        assert bare[0].tobytes() == out.tobytes() and (bare[1] == 0xEE).all()


def test_randomised_parity(ah, torch, det):
    """the 150 seeded cases of test_pnp_cpu.parity_case -- sizes from 0 to 3000 and the LDS chunk edge, six scene families (general,
    coplanar and rings, collinear, integer lattice, near or behind the centre of projection, far), five cameras, outliers, NaN / inf
    rows, duplicates up to all-equal, the world scaled by 2^-20 .. 2^20 and offset by +-16000, iterations, thresholds, seeds 0 and
    0xFFFFFFFF -- record and mask byte for byte against the statement, with and without a context; every third block of eight also
    as one ragged hak_solve_pnp_batch call.  What the cases reach (0 .. 4 solutions, every rejection, ties, later solutions, no
    model) is asserted in test_pnp_cpu.py; every hypothesis of them is compared in test_gpu_ransac_trace.py."""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    wants = []
    for k, c in enumerate(cases):
        n = len(c["corr"])
        want, wm = pn.solve_pnp(c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"])
        wants.append((want, wm))
        got, gm = gpu_pnp(ah, torch, c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"], ctx=det.ctx if c["ctx"] else None)
        try:
            assert_same(got, gm[:n], want, wm, (k, c["scene"], c["camera"]))
            assert (gm[n:] == 0xEE).all(), (k, "written past the count")
        except AssertionError as e:
            fails.append(str(e)[:300])
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    for g in groups:
        ks = [k for k, c in enumerate(cases) if c["group"] == g]
        c0 = cases[ks[0]]
        lists = [cases[k]["corr"] for k in ks]
        stride = max(1, max(len(lst) for lst in lists))
        out, masks = _pnp_batch(ah, torch, det, lists, stride, [len(lst) for lst in lists], c0["K"], c0["iterations"], c0["threshold"],
                                c0["seed"])
        for slot, k in enumerate(ks):
            n = len(lists[slot])
            try:
                assert_same(out[slot], masks[slot, :n], wants[k][0], wants[k][1], ("batch", g, k))
                assert (masks[slot, n:] == 0xEE).all(), ("batch", g, k, "written past the count")
            except AssertionError as e:
                fails.append(str(e)[:300])
    assert len(groups) >= 5
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:3])


# ------------------------------------------------------------------------------------------------------------------- link
def gpu_link(ah, torch, A, mask, xyz, B, max_index, ctx=None, with_host=True):
    """one hak_link_tracks call -> (count, the whole 0xEE-prefilled device list as bytes, the host list)"""
    nA, nB = len(A), len(B)
    dA, dB = upload(torch, A), upload(torch, B)
    dx = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1).copy()).cuda() if nA else \
        torch.zeros(4, dtype=torch.float32, device="cuda")
    dm = None if mask is None else (torch.from_numpy(np.ascontiguousarray(mask, np.uint8).copy()).cuda() if nA else
                                    torch.zeros(4, dtype=torch.uint8, device="cuda"))
    d_out = torch.full((max(nB, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(nB, 1), ah.CORR3D_DTYPE)
    cnt = C.c_int(-1)
    ah.check(ah.lib.hak_link_tracks(ctx, dA.data_ptr(), nA, None if dm is None else dm.data_ptr(), dx.data_ptr(), dB.data_ptr(), nB,
                                    max_index, d_out.data_ptr(), C.byref(cnt), h_out.ctypes.data if with_host else None))
    return cnt.value, d_out.cpu().numpy(), h_out


def assert_link(ah, got, want, what=""):
    count, raw, h_out = got
    assert count == len(want), (what, count, len(want))
    assert raw[:32 * count].tobytes() == want.tobytes(), what
    assert (raw[32 * count:] == 0xEE).all(), what                       # nothing past the count
    if h_out is not None:
        assert h_out[:count].tobytes() == want.tobytes() and not h_out[count:].tobytes().strip(b"\0"), what


def random_lists(nA, nB, nkp, seed, with_mask=True):
    """two lists over nkp keypoints of the shared image: repeated trains, indices out of range, a mask that removes a third"""
    rng = np.random.default_rng(seed)
    A = pairs(np.arange(nA), rng.integers(-2, nkp + 3, nA))
    B = pairs(np.sort(rng.integers(-2, nkp + 3, nB)), rng.integers(0, nkp, nB), x2=rng.uniform(0, 1920, nB))
    xyz = rng.normal(0, 5, (nA, 3)).astype(np.float32)
    if nA:
        xyz[rng.integers(0, nA)] = np.nan                               # linked all the same
    mask = (rng.random(nA) < 0.67).astype(np.uint8) * rng.integers(1, 255, nA).astype(np.uint8) if with_mask else None
    return A, mask, xyz, B


@pytest.mark.parametrize("nA,nB", [(0, 0), (0, 50), (50, 0), (1, 1), (63, 65), (700, 1023), (1340, 1024), (900, 1025), (5000, 2500), (20000, 1500)])
def test_link_single_call_byte_exact(ah, torch, det, nA, nB):
    nkp = max(4, (nA + nB) // 3)
    A, mask, xyz, B = random_lists(nA, nB, nkp, nA + nB)
    for m in (None, mask):
        want = lr.link_tracks(A, m, xyz, B, nkp)
        for ctx in (None, det.ctx):
            assert_link(ah, gpu_link(ah, torch, A, m, xyz, B, nkp, ctx=ctx), want, (nA, nB, m is not None, ctx is not None))
    count, raw, h = gpu_link(ah, torch, A, mask, xyz, B, nkp, with_host=False)
    assert_link(ah, (count, raw, None), want, "no host list")
    if nA >= 63 and nB >= 63:
        full = lr.link_tracks(A, None, xyz, B, nkp)
        assert 0 < len(want) < len(full) < nB                           # the mask and the range both remove links
        tr = A["train"][full["src3d"]]
        assert (np.bincount(A["train"][(A["train"] >= 0) & (A["train"] < nkp)])[tr] > 1).any()     # repeated trains were resolved


def test_link_rule_cases_on_the_device(ah, torch):
    A = pairs([0, 1, 2, 3, 4, 5, 6], [5, 9, 5, 2, 9, 40, -1])
    xyz = np.arange(21, dtype=np.float32).reshape(7, 3) + 100
    B = pairs([9, 5, 7, 2, 40, 5, -1, 41], [1, 2, 3, 4, 5, 6, 7, 8])
    mask = np.array([0, 1, 1, 1, 1, 1, 1], np.uint8)
    for m, mi in ((None, 40), (None, 41), (mask, 40), (mask, 1), (None, 2000000)):
        want = lr.link_tracks(A, m, xyz, B, mi)
        assert_link(ah, gpu_link(ah, torch, A, m, xyz, B, mi), want, (m is not None, mi))
    assert lr.link_tracks(A, None, xyz, B, 40)["src3d"].tolist() == [1, 0, 3, 0]


def test_link_batch_knn2_layout(ah, torch, det):
    """three links over six lists in hak_match_knn2_batch's layout (list k at k * max_pts, count k): list 2j links to list 2j + 1
    with base offsets 0 and max_pts, strides 2 max_pts and count steps 2; a count above the stride is clamped"""
    mp = 2000                                                           # det's max_pts: the batch form's max_index
    rng = np.random.default_rng(3)
    sizes = [(700, 1500), (0, 40), (1999, 2000)]
    lists = np.zeros(6 * mp, ah.MATCH_PAIR_DTYPE)
    lists["train"] = lists["query"] = 1                                 # past a count: would link if read
    masks = np.full(6 * mp, 1, np.uint8)
    xyz = rng.normal(0, 3, (6 * mp, 3)).astype(np.float32)
    counts = np.zeros(6, np.int32)
    parts = []
    for j, (nA, nB) in enumerate(sizes):
        A, mask, _, B = random_lists(nA, nB, mp, 100 + j)
        lists[2 * j * mp:2 * j * mp + nA] = A
        lists[(2 * j + 1) * mp:(2 * j + 1) * mp + nB] = B
        masks[2 * j * mp:2 * j * mp + nA] = mask
        counts[2 * j], counts[2 * j + 1] = nA, nB
        parts.append((A, mask, xyz[2 * j * mp:2 * j * mp + nA], B))
    counts[5] = 4 * mp + 7                                              # clamped to min(strideB, out_stride) = max_pts on the device
    parts[2] = parts[2][:3] + (lists[5 * mp:6 * mp].copy(),)
    d_l, d_m = upload(torch, lists), torch.from_numpy(masks).cuda()
    d_x, d_c = torch.from_numpy(xyz.reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
    for with_mask in (True, False):
        d_out = torch.full((3 * mp * 32 + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        d_n = torch.full((4,), -9, dtype=torch.int32, device="cuda")
        ah.check(ah.lib.hak_link_tracks_batch(det.ctx, d_l.data_ptr(), 2 * mp, d_c.data_ptr(), 2, d_m.data_ptr() if with_mask else None,
                                              d_x.data_ptr(), d_l.data_ptr() + 32 * mp, 2 * mp, d_c.data_ptr() + 4, 2, 3,
                                              d_out.data_ptr(), mp, d_n.data_ptr()))
        ah.check(ah.lib.hak_sync(det.ctx))
        raw, n = d_out.cpu().numpy(), d_n.cpu().numpy()
        assert n[3] == -9 and (raw[3 * mp * 32:] == 0xEE).all()
        for j, (A, mask, x, B) in enumerate(parts):
            want = lr.link_tracks(A, mask if with_mask else None, x, B, mp)
            assert_link(ah, (int(n[j]), raw[j * mp * 32:(j + 1) * mp * 32], None), want, ("batch", j, with_mask))
            assert_link(ah, gpu_link(ah, torch, A, mask if with_mask else None, x, B, mp, ctx=det.ctx), want, ("single", j))
        assert n[0] > 100 and n[1] == 0 and n[2] > 100


def test_chain_fundamental_refine_pose_link_pnp(ah, torch, synth, det):
    """two three-view scenes as four lists in hak_match_knn2_batch's layout: find_fundamental_batch -> refine_batch ->
    recover_pose_batch -> link_tracks_batch -> solve_pnp_batch with one hak_sync at the end equals the statement chain"""
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
    fund = torch.zeros(4 * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    pose = torch.zeros(4 * 64, dtype=torch.uint8, device="cuda")
    pmask = torch.zeros(4 * mp, dtype=torch.uint8, device="cuda")
    xyz = torch.zeros(4 * mp * 3, dtype=torch.float32, device="cuda")
    corr = torch.full((2 * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    ncorr = torch.zeros(2, dtype=torch.int32, device="cuda")
    absp = torch.zeros(2 * POSE_SIZE, dtype=torch.uint8, device="cuda")
    amask = torch.full((2 * mp,), 0xEE, dtype=torch.uint8, device="cuda")
    lib, ctx, kp = ah.lib, det.ctx, K.ctypes.data
    ah.check(lib.hak_find_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 256, 1.0, 5, fund.data_ptr(), None))
    ah.check(lib.hak_refine_fundamental_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, 1.0, 3, fund.data_ptr(), None))
    ah.check(lib.hak_recover_pose_batch(ctx, d_l.data_ptr(), mp, d_c.data_ptr(), 4, fund.data_ptr(), kp, kp, 1.0, 50.0, pose.data_ptr(),
                                        pmask.data_ptr(), xyz.data_ptr()))
    ah.check(lib.hak_link_tracks_batch(ctx, d_l.data_ptr(), 2 * mp, d_c.data_ptr(), 2, pmask.data_ptr(), xyz.data_ptr(),
                                       d_l.data_ptr() + 32 * mp, 2 * mp, d_c.data_ptr() + 4, 2, 2, corr.data_ptr(), mp, ncorr.data_ptr()))
    ah.check(lib.hak_solve_pnp_batch(ctx, corr.data_ptr(), mp, ncorr.data_ptr(), 2, kp, 512, 2.0, 9, absp.data_ptr(), amask.data_ptr()))
    ah.check(lib.hak_sync(ctx))
    raw, n, got, gmask = corr.cpu().numpy(), ncorr.cpu().numpy(), absp.cpu().numpy().view(ah.ABS_POSE_DTYPE), amask.cpu().numpy()
    for j, sc in enumerate(scenes):
        A, B = sc[3], sc[4]
        rec0, _ = fr.find_fundamental(A, 256, 1.0, 5)
        rec1, _ = rr.refine_fundamental(A, rec0, 1.0, 3)
        wpose, wpm, wxyz = pr.recover_pose(A, rec1, K, None, 1.0, 50.0)
        want = lr.link_tracks(A, wpm, wxyz, B, mp)
        assert_link(ah, (int(n[j]), raw[j * mp * 32:(j + 1) * mp * 32], None), want, ("chain link", j))
        wrec, wmask = pn.solve_pnp(want, K, 512, 2.0, 9)
        assert_same(got[j], gmask[j * mp:j * mp + len(want)], wrec, wmask, ("chain pnp", j))
        assert (gmask[j * mp + len(want):(j + 1) * mp] == 0xEE).all()
        assert wrec["hypothesis"] >= 0 and wrec["inliers"] > 40 and len(want) > 100


def test_python_wrappers(ah, torch, synth):
    K, _, _, A, B, fa, fb, X0, pa, pb = synth.three_view_scene(3, 300, 0.0, 0.2)
    xyz = X0.astype(np.float32)
    mask = fa.astype(np.uint8)
    want = lr.link_tracks(A, mask, xyz, B, 600)
    got = ah.linkTracks(A, xyz, B, mask, 600)
    assert got.dtype == ah.CORR3D_DTYPE and got.tobytes() == want.tobytes() and len(want) > 150
    assert ah.linkTracks(A, xyz, B).tobytes() == lr.link_tracks(A, None, xyz, B, int(A["train"].max()) + 1).tobytes()
    dev = ah.linkTracks(upload(torch, A), torch.from_numpy(xyz).cuda(), upload(torch, B), torch.from_numpy(mask).cuda(), 600)
    assert dev.tobytes() == want.tobytes()                              # device tensors are used in place
    wrec, wmask = pn.solve_pnp(want, K, 256, 1.0, 4)
    rec, m = ah.solvePnP(want, K, 256, 1.0, 4)                          # a 3 x 3 K
    assert rec.dtype == ah.ABS_POSE_DTYPE and m.dtype == np.uint8
    assert_same(rec, m, wrec, wmask, "wrapper")
    rec, m = ah.solvePnP(upload(torch, want), ah.intrinsics(K), 256, 1.0, 4)
    assert_same(rec, m, wrec, wmask, "wrapper, device list")
    # noise-free: the absolute pose of image 2 in image 0's frame is the composition of the two planted relative poses
    (R01, t01), (R12, t12) = synth.three_view_scene(3, 300, 0.0, 0.2)[1:3]
    assert np.abs(rec["R"].reshape(3, 3) - R12 @ R01).max() < 1e-3 and np.abs(rec["t"] - (R12 @ t01 + t12)).max() < 1e-2
    assert len(ah.linkTracks(A[:0], xyz[:0], B)) == 0 and ah.solvePnP(want[:2], K)[0]["hypothesis"] == -1


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls, keep, rec, count = refusals(ah, det.ctx, d.data_ptr(), cnt.data_ptr())
    assert len(calls) >= 60
    ok = np.zeros((), ah.ABS_POSE_DTYPE)
    K = ah.intrinsics(K_TABLE)
    for k, (fn, args) in enumerate(calls):
        ah.check(ah.lib.hak_solve_pnp(None, d.data_ptr(), 0, K.ctypes.data, 64, 1.0, 0, None, ok.ctypes.data))     # succeeds in between
        assert ok["hypothesis"] == -1 and ok["n"] == 0
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    ah.check(ah.lib.hak_sync(det.ctx))
    assert not d.any() and not cnt.any() and not rec.tobytes().strip(b"\0") and count.value == -7

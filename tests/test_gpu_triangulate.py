"""GPU suite: triangulation under two known views (hak_triangulate(_batch), kernels_triangulate.hip) byte for byte against its
numpy statement tests/triangulate_ref.py -- every byte of the record, of the whole mask buffer and of the whole point buffer, both
prefilled with 0xEE.

Launch shape: k_pose's, one block of BLOCK = 512 threads per list, one match per thread per step; the sizes give a partly filled
wave, a full wave, one lane of a second wave, one thread short of a step, a full step, one match of a second step, and three steps."""
import numpy as np
import pytest

import link_ref as lr
import pnp_ref as pn
import pose_ref as pr
import triangulate_ref as tr
from test_gpu_fundamental import det, synth, torch, upload  # noqa: F401 (fixtures)
from test_pnp_cpu import FOCAL, H, K_TABLE, TABLE, W
from test_triangulate_cpu import B_SIDE, _abs_record, _pose_record, chain, gate_cases, match_array, project, refusals, rt12

pytestmark = pytest.mark.gpu

BLOCK = 512                                                             # TR_BLOCK of kernels_triangulate.hip
SIZES = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1340]
PAR = (1.0, 11.0, 0.02)                                                 # threshold, max_depth, min_sin of the scenes below
REC = tr.TRIANGULATION_DTYPE.itemsize


def scene(synth, n, seed, ka=4, kb=32):
    """n matches of a cloud seen by two views of the pose table: 0.4 px of noise, a fifth wrong matches, some behind or beyond
    max_depth, every 37th with a non-finite coordinate -- every gate has members -> (matches, MA, MB)"""
    rng = np.random.default_rng(9000 + seed)
    MA = rt12(synth.rotation_zyx(TABLE[ka][0]), TABLE[ka][1])
    MB = rt12(synth.rotation_zyx(TABLE[kb][0]), TABLE[kb][1])
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(3, 14, n)], axis=1)
    pA = project(X, MA[:9].reshape(3, 3), MA[9:].astype(np.float64))[0] + rng.normal(0, 0.4, (n, 2))
    pB = project(X, MB[:9].reshape(3, 3), MB[9:].astype(np.float64))[0] + rng.normal(0, 0.4, (n, 2))
    wrong = rng.random(n) < 0.2
    pB[wrong] = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)[wrong]
    m = match_array(pA, pB)
    for i in range(36, n, 37):
        m[("x1", "y1", "x2", "y2")[i % 4]][i] = (np.nan, np.inf, -np.inf)[i % 3]
    return m, MA, MB


def fp(ah, M):
    import ctypes as C
    return None if M is None else M.ctypes.data_as(C.POINTER(C.c_float))


def gpu_single(ah, torch, m, MA, MB, K, par, ctx=None, with_mask=True, with_xyz=True):
    """one hak_triangulate call -> (record, the whole 0xEE-prefilled mask buffer, the whole 0xEE-prefilled point buffer as bytes)"""
    n = len(m)
    d = upload(torch, m)
    mask = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    xyz = torch.full((12 * max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    k = ah.intrinsics(K)
    rec = np.zeros((), ah.TRIANGULATION_DTYPE)
    MA = None if MA is None else np.ascontiguousarray(MA, np.float32)
    MB = None if MB is None else np.ascontiguousarray(MB, np.float32)
    ah.check(ah.lib.hak_triangulate(ctx, d.data_ptr(), n, fp(ah, MA), fp(ah, MB), k.ctypes.data, k.ctypes.data, par[0], par[1], par[2],
                                    mask.data_ptr() if with_mask else None, xyz.data_ptr() if with_xyz else None, rec.ctypes.data))
    return rec, mask.cpu().numpy(), xyz.cpu().numpy()


def assert_same(got, want, n, what=""):
    """got = (record, whole mask buffer, whole point buffer as bytes), want = the statement's (record, mask, xyz) of n matches"""
    rec, mask, xyz = got
    wrec, wmask, wxyz = want
    assert rec.tobytes() == np.array(wrec, rec.dtype).tobytes(), (what, rec, wrec)
    assert np.array_equal(mask[:n], wmask), (what, "mask", int((mask[:n] != wmask).sum()))
    assert xyz[:12 * n].tobytes() == wxyz.tobytes(), (what, "xyz", int((xyz[:12 * n].view(np.float32).reshape(n, 3) != wxyz).any(axis=1).sum()))
    assert (mask[n:] == 0xEE).all() and (xyz[12 * n:] == 0xEE).all(), (what, "written past the count")


@pytest.mark.parametrize("n", SIZES)
def test_single_call_bit_exact(ah, torch, synth, det, n):
    m, MA, MB = scene(synth, n, n)
    want = tr.triangulate(m, MA, MB, K_TABLE, None, *PAR)
    for ctx in (None, det.ctx):
        assert_same(gpu_single(ah, torch, m, MA, MB, K_TABLE, PAR, ctx=ctx), want, n, (n, ctx is not None))
    rec, mask, xyz = gpu_single(ah, torch, m, MA, MB, K_TABLE, PAR, with_mask=False)      # d_mask = NULL: its stand-in untouched
    assert (mask == 0xEE).all()
    assert_same((rec, np.concatenate([want[1], mask[n:]]), xyz), want, n, (n, "no mask"))
    rec, mask, xyz = gpu_single(ah, torch, m, MA, MB, K_TABLE, PAR, ctx=det.ctx, with_xyz=False)
    assert (xyz == 0xEE).all()
    assert_same((rec, mask, np.concatenate([want[2].view(np.uint8).reshape(-1), xyz[12 * n:]])), want, n, (n, "no xyz"))
    if n >= BLOCK - 1:
        assert want[0]["kept"] > 0.3 * n and (want[0]["rejected"] > 0).all()      # every gate has members


def _kind(ah, v):
    """(kind, record array of one, host view) of a view as the CPU cases give it"""
    if v is None:
        return ah.VIEW_IDENTITY, None, None
    if getattr(v, "dtype", None) is not None and v.dtype.names:
        rel = "candidate" in v.dtype.names
        host = np.concatenate([v["R"].reshape(9), v["t"].reshape(3)]).astype(np.float32)
        return (ah.VIEW_RELATIVE if rel else ah.VIEW_ABSOLUTE), np.array([v], v.dtype), host
    return ah.VIEW_ABSOLUTE, np.array([_abs_record(np.asarray(v, np.float32))], pn.ABS_POSE_DTYPE), np.asarray(v, np.float32)


def gpu_batch(ah, torch, det, lists, counts, mp, slot, nslots, viewA, viewB, K, par, with_mask=True, with_xyz=True, bufs=None):
    """one hak_triangulate_batch call over len(lists) lists in a layout of `nslots` lists of mp records per chain, list k in slot
    `slot` of chain k: stride nslots * mp, count step nslots, base offset slot * mp.  viewA, viewB: (kind, record array or None,
    step).  Every list slot holds usable matches and every count slot a positive count, so a wrong stride or step shows.
    -> (records (npairs,), mask buffer (npairs * nslots, mp), point buffer (npairs * nslots, 12 mp) as bytes), a record past
    npairs is a sentinel"""
    np_ = len(lists)
    filler = lists[int(np.argmax([len(lst) for lst in lists]))]
    allm = np.zeros(np_ * nslots * mp, ah.MATCH_PAIR_DTYPE)
    for s in range(np_ * nslots):
        allm[s * mp:s * mp + min(len(filler), mp)] = filler[:mp]        # past a count, and in the other slots: usable if read
    cnt = np.full(np_ * nslots, min(len(filler), mp), np.int32)
    for k, lst in enumerate(lists):
        allm[(k * nslots + slot) * mp:(k * nslots + slot) * mp + len(lst)] = lst
        cnt[k * nslots + slot] = counts[k]
    d, d_cnt = upload(torch, allm), torch.from_numpy(cnt).cuda()
    d_out = torch.full(((np_ + 1) * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_mask, d_xyz = bufs if bufs is not None else (torch.full((np_ * nslots * mp,), 0xEE, dtype=torch.uint8, device="cuda"),
                                                   torch.full((np_ * nslots * mp * 12,), 0xEE, dtype=torch.uint8, device="cuda"))
    dv = [None if v[1] is None else upload(torch, v[1]) for v in (viewA, viewB)]
    k1 = ah.intrinsics(K)
    ah.check(ah.lib.hak_triangulate_batch(det.ctx, d.data_ptr() + 32 * slot * mp, nslots * mp, d_cnt.data_ptr() + 4 * slot, nslots, np_,
                                          None if dv[0] is None else dv[0].data_ptr(), viewA[0], viewA[2],
                                          None if dv[1] is None else dv[1].data_ptr(), viewB[0], viewB[2], k1.ctypes.data, k1.ctypes.data,
                                          par[0], par[1], par[2], d_out.data_ptr(),
                                          d_mask.data_ptr() + slot * mp if with_mask else None,
                                          d_xyz.data_ptr() + 12 * slot * mp if with_xyz else None))
    ah.check(ah.lib.hak_sync(det.ctx))
    raw = d_out.cpu().numpy()
    assert (raw[np_ * REC:] == 0xEE).all()
    return (raw[:np_ * REC].view(ah.TRIANGULATION_DTYPE), d_mask.cpu().numpy().reshape(np_ * nslots, mp),
            d_xyz.cpu().numpy().reshape(np_ * nslots, 12 * mp))


def test_every_gate_and_no_model_case(ah, torch, det):
    cases = gate_cases()
    assert len(cases) >= 20
    for c in cases:
        m, n = c["matches"], len(c["matches"])
        want = tr.triangulate(m, c["A"], c["B"], K_TABLE, None, *c["par"])
        assert want[0]["kept"] == c["kept"] and want[0]["model"] == c["model"], c["name"]
        (ka, ra, ha), (kb, rb, hb) = _kind(ah, c["A"]), _kind(ah, c["B"])
        mp = max(n, 1)
        out, masks, xyz = gpu_batch(ah, torch, det, [m], [n], mp, 0, 1, (ka, ra, 1), (kb, rb, 1), K_TABLE, c["par"])
        assert_same((out[0], masks[0], xyz[0]), want, n, ("batch", c["name"]))
        if c["model"]:                                                  # the synchronous form takes views with a model only
            for ctx in (None, det.ctx):
                assert_same(gpu_single(ah, torch, m, ha, hb, K_TABLE, c["par"], ctx=ctx), want, n, ("single", c["name"]))


def test_view_kinds_and_steps(ah, torch, synth, det):
    """IDENTITY / RELATIVE / ABSOLUTE in both positions, as hak_pose and hak_abs_pose arrays with view steps 0, 1 and 3; the records
    a step skips are NaN-filled with a model flag set: read, they would give another result"""
    mp, np_ = 600, 3
    views = [rt12(synth.rotation_zyx(TABLE[k][0]), TABLE[k][1]) for k in (8, 25, 39, 18, 11, 32)]
    lists = [scene(synth, 500 + 17 * k, 60 + k)[0] for k in range(np_)]

    def array(kind, Ms, step):
        if kind == ah.VIEW_IDENTITY:
            return None
        make, dt = (_pose_record, pr.POSE_DTYPE) if kind == ah.VIEW_RELATIVE else (_abs_record, pn.ABS_POSE_DTYPE)
        arr = np.zeros(max(step, 1) * np_, dt)
        arr["R"], arr["t"] = np.nan, np.nan
        for k in range(np_ if step else 1):
            arr[k * step] = make(Ms[k])
        return arr

    tried = 0
    for kindA, kindB, stepA, stepB in [(0, 1, 0, 1), (0, 2, 0, 3), (1, 0, 1, 0), (2, 0, 3, 0), (1, 2, 3, 1), (2, 1, 1, 3), (1, 1, 1, 1),
                                       (2, 2, 3, 3), (1, 2, 0, 1), (2, 1, 1, 0)]:
        MsA, MsB = views[:3], views[3:]
        arrA, arrB = array(kindA, MsA, stepA), array(kindB, MsB, stepB)
        out, masks, xyz = gpu_batch(ah, torch, det, lists, [len(lst) for lst in lists], mp, 0, 1, (kindA, arrA, stepA),
                                    (kindB, arrB, stepB), K_TABLE, (2.0, np.inf, 0.0))
        for k, lst in enumerate(lists):
            va = None if kindA == 0 else MsA[k if stepA else 0]
            vb = None if kindB == 0 else MsB[k if stepB else 0]
            want = tr.triangulate(lst, va, vb, K_TABLE, None, 2.0, np.inf, 0.0)
            assert want[0]["model"] == 1
            assert_same((out[k], masks[k], xyz[k]), want, len(lst), (kindA, kindB, stepA, stepB, k))
            tried += 1
    assert tried == 30


@pytest.fixture(scope="module")
def ragged(synth):
    mp = 1400
    counts = [0, 3, 64, 700, 1340]
    sc = [scene(synth, 1400, 30 + k) for k in range(5)]
    return mp, counts, [s[0] for s in sc], sc[0][1], sc[0][2]


def test_ragged_batch_in_the_six_image_layout(ah, torch, synth, det, ragged):
    """five chains of three lists: the lists of pairs 3j + 1 (stride 3 mp, count step 3, base offset mp), view A from an array of
    hak_pose with step 3, view B from an array of hak_abs_pose with step 1; the view of list 2 has no model; the slots of pairs 3j
    and 3j + 2 must come back untouched.  Then the same lists at stride mp with the count of the last above the stride: it is
    clamped (in the six-image layout the stride spans three slots, so there the clamp cannot be what protects a neighbour)"""
    mp, counts, full, MA, MB = ragged
    lists = [f[:c] for f, c in zip(full, counts)]
    poses = np.zeros(15, pr.POSE_DTYPE)
    poses["R"], poses["t"] = np.nan, np.nan
    absp = np.zeros(5, pn.ABS_POSE_DTYPE)
    for k in range(5):
        poses[3 * k] = _pose_record(MA, k % 4)
        absp[k] = _abs_record(MB, -1 if k == 2 else 7)
    for with_mask, with_xyz in ((True, True), (False, True), (True, False)):
        out, masks, xyz = gpu_batch(ah, torch, det, lists, counts, mp, 1, 3, (ah.VIEW_RELATIVE, poses, 3), (ah.VIEW_ABSOLUTE, absp, 1),
                                    K_TABLE, PAR, with_mask, with_xyz)
        for k, lst in enumerate(lists):
            want = tr.triangulate(lst, poses[3 * k], absp[k], K_TABLE, None, *PAR)
            n = len(lst)
            gm = masks[3 * k + 1] if with_mask else np.concatenate([want[1], masks[3 * k + 1][n:]])
            gx = xyz[3 * k + 1] if with_xyz else np.concatenate([want[2].view(np.uint8).reshape(-1), xyz[3 * k + 1][12 * n:]])
            assert_same((out[k], gm, gx), want, n, ("ragged", k, with_mask, with_xyz))
            for other in (3 * k, 3 * k + 2):                            # the neighbouring pairs' slots
                assert (masks[other] == 0xEE).all() and (xyz[other] == 0xEE).all(), (k, other)
        if not with_mask:
            assert (masks == 0xEE).all()
        if not with_xyz:
            assert (xyz == 0xEE).all()
        assert out[2]["model"] == 0 and out[2]["n"] == 64 and out[4]["n"] == 1340 and out[0]["n"] == 0 and out[0]["model"] == 1
        assert out[3]["kept"] > 200 and out[1]["kept"] + out[1]["rejected"].sum() == 3
    lists[4] = full[4][:mp]
    out, masks, xyz = gpu_batch(ah, torch, det, lists, counts[:4] + [3 * mp + 9], mp, 0, 1, (ah.VIEW_RELATIVE, poses, 3),
                                (ah.VIEW_ABSOLUTE, absp, 1), K_TABLE, PAR)
    for k, lst in enumerate(lists):
        assert_same((out[k], masks[k], xyz[k]), tr.triangulate(lst, poses[3 * k], absp[k], K_TABLE, None, *PAR), len(lst), ("clamped", k))
    assert out[4]["n"] == mp


def test_in_place_over_the_pose_outputs(ah, torch, synth, det):
    """mask and points written over the buffers hak_recover_pose_batch just filled for the same pair, with view A the identity and
    view B the pair's own hak_pose, read on the device"""
    mp = 700
    recs, flags, F, K, R, t, z = synth.two_view_scene(450, 150, 12, noise=0.3)
    m = match_array(recs[:, :2], recs[:, 2:])
    d, d_cnt = upload(torch, m), torch.tensor([len(m)], dtype=torch.int32, device="cuda")
    fund = np.zeros(1, ah.FUNDAMENTAL_DTYPE)
    fund["F"], fund["hypothesis"] = F.reshape(9), 0
    d_f = upload(torch, fund)
    pose = torch.zeros(64, dtype=torch.uint8, device="cuda")
    mask = torch.full((mp,), 0xEE, dtype=torch.uint8, device="cuda")
    xyz = torch.full((12 * mp,), 0xEE, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    k1 = ah.intrinsics(K)
    ah.check(ah.lib.hak_recover_pose_batch(det.ctx, d.data_ptr(), mp, d_cnt.data_ptr(), 1, d_f.data_ptr(), k1.ctypes.data, k1.ctypes.data,
                                           1.0, 50.0, pose.data_ptr(), mask.data_ptr(), xyz.data_ptr()))
    ah.check(ah.lib.hak_triangulate_batch(det.ctx, d.data_ptr(), mp, d_cnt.data_ptr(), 1, 1, None, ah.VIEW_IDENTITY, 0, pose.data_ptr(),
                                          ah.VIEW_RELATIVE, 1, k1.ctypes.data, k1.ctypes.data, 1.0, 50.0, 0.0, out.data_ptr(),
                                          mask.data_ptr(), xyz.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    prec = pose.cpu().numpy().view(ah.POSE_DTYPE)[0]
    wpose, wpm, wxyz = pr.recover_pose(m, fund[0], K, None, 1.0, 50.0)
    assert prec.tobytes() == np.array(wpose, ah.POSE_DTYPE).tobytes() and prec["candidate"] >= 0
    want = tr.triangulate(m, None, prec, K, None, 1.0, 50.0, 0.0)
    raw = out.cpu().numpy()
    assert (raw[REC:] == 0xEE).all()
    assert_same((raw[:REC].view(ah.TRIANGULATION_DTYPE)[0], mask.cpu().numpy(), xyz.cpu().numpy()), want, len(m), "in place")
    # close to hak_recover_pose's own points, not identical: nearly every planted match is kept by both, the points agree to 1e-3
    both = (wpm == 1) & (want[1] == 1)
    assert both.sum() > 400 and np.abs(want[2][both] - wxyz[both]).max() < 0.05 and not np.array_equal(want[2][both], wxyz[both])


def test_four_view_chain_on_the_device(ah, torch, synth, det):
    """two chains of four_view_scene in the six-image layout (pairs 3j, 3j + 1, 3j + 2 = (I0, I1), (I1, I2), (I2, I3)): the whole
    sequence from hak_find_fundamental_batch to the hak_refine_pnp_batch for I3 with one hak_sync at the end equals the
    statements' chain, byte for byte"""
    mp, seed = 2000, 5
    legs = [(400, 0.3, 1), (400, 0.5, 3)]
    want = [chain(synth, n, noise, s, ransac_seed=seed, max_index=mp) for n, noise, s in legs]
    lists = np.zeros(6 * mp, ah.MATCH_PAIR_DTYPE)
    counts = np.zeros(6, np.int32)
    for j, w in enumerate(want):
        for side, lst in enumerate((w["scene"][3], w["scene"][4], w["scene"][11])):
            lists[(3 * j + side) * mp:(3 * j + side) * mp + len(lst)] = lst
            counts[3 * j + side] = len(lst)
    K = ah.intrinsics(want[0]["scene"][0])
    d_l, d_c = upload(torch, lists), torch.from_numpy(counts).cuda()
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    fill = lambda nbytes: torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
    fund, pose = zeros(6 * ah.FUNDAMENTAL_DTYPE.itemsize), zeros(6 * 64)
    pmask, xyz = fill(6 * mp), fill(6 * mp * 12)
    corr2, corr3 = fill(2 * mp * 32), fill(2 * mp * 32)
    n2, n3 = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    abs2, abs3, tri = zeros(2 * 64), zeros(2 * 64), fill(3 * REC)
    am2, am3 = fill(2 * mp), fill(2 * mp)
    lib, ctx, kp, L, Cn = ah.lib, det.ctx, K.ctypes.data, d_l.data_ptr(), d_c.data_ptr()
    ah.check(lib.hak_find_fundamental_batch(ctx, L, mp, Cn, 6, 256, 1.0, seed, fund.data_ptr(), None))
    ah.check(lib.hak_refine_fundamental_batch(ctx, L, mp, Cn, 6, 1.0, 3, fund.data_ptr(), None))
    ah.check(lib.hak_recover_pose_batch(ctx, L, mp, Cn, 6, fund.data_ptr(), kp, kp, 1.0, 50.0, pose.data_ptr(), pmask.data_ptr(),
                                        xyz.data_ptr()))
    ah.check(lib.hak_link_tracks_batch(ctx, L, 3 * mp, Cn, 3, pmask.data_ptr(), xyz.data_ptr(), L + 32 * mp, 3 * mp, Cn + 4, 3, 2,
                                       corr2.data_ptr(), mp, n2.data_ptr()))
    ah.check(lib.hak_solve_pnp_batch(ctx, corr2.data_ptr(), mp, n2.data_ptr(), 2, kp, 256, 2.0, seed, abs2.data_ptr(), None))
    ah.check(lib.hak_refine_pnp_batch(ctx, corr2.data_ptr(), mp, n2.data_ptr(), 2, kp, 2.0, 3, abs2.data_ptr(), am2.data_ptr()))
    ah.check(lib.hak_triangulate_batch(ctx, L + 32 * mp, 3 * mp, Cn + 4, 3, 2, pose.data_ptr(), ah.VIEW_RELATIVE, 3, abs2.data_ptr(),
                                       ah.VIEW_ABSOLUTE, 1, kp, kp, 2.0, 50.0, 0.01, tri.data_ptr(), pmask.data_ptr() + mp,
                                       xyz.data_ptr() + 12 * mp))
    ah.check(lib.hak_link_tracks_batch(ctx, L + 32 * mp, 3 * mp, Cn + 4, 3, pmask.data_ptr() + mp, xyz.data_ptr() + 12 * mp,
                                       L + 64 * mp, 3 * mp, Cn + 8, 3, 2, corr3.data_ptr(), mp, n3.data_ptr()))
    ah.check(lib.hak_solve_pnp_batch(ctx, corr3.data_ptr(), mp, n3.data_ptr(), 2, kp, 256, 2.0, seed, abs3.data_ptr(), None))
    ah.check(lib.hak_refine_pnp_batch(ctx, corr3.data_ptr(), mp, n3.data_ptr(), 2, kp, 2.0, 3, abs3.data_ptr(), am3.data_ptr()))
    ah.check(lib.hak_sync(ctx))
    g = dict(pose=pose.cpu().numpy().view(ah.POSE_DTYPE), pmask=pmask.cpu().numpy().reshape(6, mp), xyz=xyz.cpu().numpy().reshape(6, 12 * mp),
             corr2=corr2.cpu().numpy().reshape(2, mp * 32), corr3=corr3.cpu().numpy().reshape(2, mp * 32), n2=n2.cpu().numpy(),
             n3=n3.cpu().numpy(), abs2=abs2.cpu().numpy().view(ah.ABS_POSE_DTYPE), abs3=abs3.cpu().numpy().view(ah.ABS_POSE_DTYPE),
             am2=am2.cpu().numpy().reshape(2, mp), am3=am3.cpu().numpy().reshape(2, mp), tri=tri.cpu().numpy())
    assert (g["tri"][2 * REC:] == 0xEE).all()
    tri_rec = g["tri"][:2 * REC].view(ah.TRIANGULATION_DTYPE)

    def same_record(got, wanted, what):
        assert got.tobytes() == np.array(wanted, got.dtype).tobytes(), (what, got, wanted)

    def same_list(raw, count, wanted, what):
        assert count == len(wanted) and raw[:32 * count].tobytes() == wanted.tobytes() and (raw[32 * count:] == 0xEE).all(), (what, count)

    for j, w in enumerate(want):
        n = len(w["scene"][3])
        same_record(g["pose"][3 * j], w["pose"], ("pose", j))
        assert np.array_equal(g["pmask"][3 * j][:n], w["pmask"]) and g["xyz"][3 * j][:12 * n].tobytes() == w["xyz"].tobytes(), ("pose points", j)
        same_list(g["corr2"][j], int(g["n2"][j]), w["corr2"], ("link to I2", j))
        same_record(g["abs2"][j], w["ref2"], ("pose of I2", j))
        assert np.array_equal(g["am2"][j][:len(w["corr2"])], w["mask2"]), ("inliers of I2", j)
        assert_same((tri_rec[j], g["pmask"][3 * j + 1], g["xyz"][3 * j + 1]), (w["tri"], w["tmask"], w["txyz"]), n, ("triangulation", j))
        same_list(g["corr3"][j], int(g["n3"][j]), w["corr3"], ("link to I3", j))
        same_record(g["abs3"][j], w["ref3"], ("pose of I3", j))
        assert np.array_equal(g["am3"][j][:len(w["corr3"])], w["mask3"]) and (g["am3"][j][len(w["corr3"]):] == 0xEE).all(), ("inliers of I3", j)
        assert w["tri"]["kept"] > 250 and w["ref3"]["hypothesis"] >= 0 and w["ref3"]["inliers"] > 100


def test_python_wrapper(ah, torch, synth, det):
    m, MA, MB = scene(synth, 300, 77)
    want = tr.triangulate(m, MA, MB, K_TABLE, None, *PAR)
    for args in ((m, MA, MB, K_TABLE, None), (upload(torch, m), _pose_record(MA), _abs_record(MB), ah.intrinsics(K_TABLE), K_TABLE)):
        rec, mask, xyz = ah.triangulate(*args, threshold=PAR[0], max_depth=PAR[1], min_sin=PAR[2])
        assert rec.dtype == ah.TRIANGULATION_DTYPE and mask.dtype == np.uint8 and xyz.dtype == np.float32 and xyz.shape == (300, 3)
        assert rec.tobytes() == want[0].tobytes() and np.array_equal(mask, want[1]) and xyz.tobytes() == want[2].tobytes()
    rec, mask, xyz = ah.triangulate(m, None, MB, K_TABLE, akazer=det)
    w = tr.triangulate(m, None, MB, K_TABLE)
    assert rec.tobytes() == w[0].tobytes() and np.array_equal(mask, w[1]) and xyz.tobytes() == w[2].tobytes()
    rec, mask, xyz = ah.triangulate(m, _pose_record(MA, -1), MB, K_TABLE)                     # step 1 of the rule
    w = tr.triangulate(m, _pose_record(MA, -1), MB, K_TABLE)
    assert rec.tobytes() == w[0].tobytes() and rec["model"] == 0 and not mask.any() and not xyz.any() and len(mask) == 300
    assert ah.triangulate(m[:0], MA, MB, K_TABLE)[0]["n"] == 0


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls, keep, rec = refusals(ah, det.ctx, d.data_ptr(), cnt.data_ptr())
    assert len(calls) >= 50
    ok = np.zeros((), ah.TRIANGULATION_DTYPE)
    K = ah.intrinsics(K_TABLE)
    for k, (fn, args, word) in enumerate(calls):
        ah.check(ah.lib.hak_triangulate(None, d.data_ptr(), 0, None, None, K.ctypes.data, K.ctypes.data, 1.0, 5.0, 0.0, None, None,
                                        ok.ctypes.data))                # succeeds in between
        assert ok["model"] == 1 and ok["n"] == 0
        assert fn(*args) != 0, (k, args)
        assert word in ah.lib.hak_last_error().decode(), (k, word)
    ah.check(ah.lib.hak_sync(det.ctx))
    assert not d.any() and not cnt.any() and not rec.tobytes().strip(b"\0")

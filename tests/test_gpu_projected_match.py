"""GPU suite: projection-guided matching (hak_match_projected / hak_match_projected_batch, kernels_projected.hip) bit for bit
against its numpy statement tests/projected_match_ref.py -- the list, the count, and nothing written past the count -- on the guided
fixture lifted into 3-D, the boundary cases of the gate, landmarks behind the camera, sets outside any extent, ties, ragged batches
with every kind of view, and the detect-layout chain 2-NN -> F -> refit -> pose -> link -> PnP -> refit -> re-match -> refit."""
import ctypes as C

import numpy as np
import pytest

import guided_match_ref as gr
import projected_match_ref as pm
from test_guided_match_cpu import IDENTITY, SIZES, build_pair, random_points
from test_projected_match_cpu import (CHAIN_RADIUS, K_LIFT, build_lifted, chain, fixture_shares, identity_list, lift, refusals, rt12,
                                      shuffled)

pytestmark = pytest.mark.gpu

RADII = (0.5, 3.0, 20.0)
EYE = rt12(np.eye(3), (0.0, 0.0, 0.0))


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
    """a context for the calls that take one (the geometry does not matter to the matcher): seven lists of 600"""
    d = ah.Akazer()
    d.init((640, 480, ah.iAlignUp(640, 128)), max_pts=600, batch=14)
    yield d
    d.close()


def upload(torch, a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(128, dtype=torch.uint8, device="cuda")


def fp(M):
    return None if M is None else M.ctypes.data_as(C.POINTER(C.c_float))


class Case:
    """a landmark set and a train set on the device, for any number of calls"""

    def __init__(self, torch, A, mask, xyz, D, T):
        self.torch, self.A, self.mask, self.xyz, self.D, self.T = torch, A, mask, np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), D, T
        self.dA, self.dx, self.dD, self.dT = upload(torch, A), upload(torch, self.xyz), upload(torch, D), upload(torch, T)
        self.dm = None if mask is None else upload(torch, mask, np.uint8)
        self.dist = pm.distances(A, mask, D, T)

    def gpu(self, ah, M, K, radius, ratio=(4, 5), cross=True, max_dist=0, ctx=None):
        """one synchronous call -> the list; the device list equals the host copy and nothing is written past the count"""
        nA = len(self.A)
        d_out = self.torch.full((max(nA, 1) * 32,), 0xEE, dtype=self.torch.uint8, device="cuda")
        h_out = np.zeros(max(nA, 1), ah.CORR3D_DTYPE)
        cnt = C.c_int(-1)
        k = ah.intrinsics(K)
        M = None if M is None else np.ascontiguousarray(M, np.float32)
        ah.check(ah.lib.hak_match_projected(ctx, self.dA.data_ptr(), nA, None if self.dm is None else self.dm.data_ptr(), self.dx.data_ptr(),
                                            self.dD.data_ptr(), len(self.D), self.dT.data_ptr(), len(self.T), fp(M), k.ctypes.data,
                                            float(radius), ratio[0], ratio[1], int(cross), max_dist, d_out.data_ptr(), C.byref(cnt),
                                            h_out.ctypes.data))
        dev = d_out.cpu().numpy().view(ah.CORR3D_DTYPE)
        assert 0 <= cnt.value <= nA
        assert np.array_equal(dev[:cnt.value].view(np.uint8), h_out[:cnt.value].view(np.uint8))
        assert (dev[cnt.value:].view(np.uint8) == 0xEE).all()                # nothing written past the count
        only = C.c_int(-1)                                                   # d_out = NULL: the count alone
        ah.check(ah.lib.hak_match_projected(ctx, self.dA.data_ptr(), nA, None if self.dm is None else self.dm.data_ptr(), self.dx.data_ptr(),
                                            self.dD.data_ptr(), len(self.D), self.dT.data_ptr(), len(self.T), fp(M), k.ctypes.data,
                                            float(radius), ratio[0], ratio[1], int(cross), max_dist, None, C.byref(only), None))
        assert only.value == cnt.value
        return h_out[:cnt.value].copy()

    def check(self, ah, M, K, radii, what, ctxs=(None,), ratios=((4, 5),), crosses=(True,), dists=(0,)):
        """the calls against the statement; returns the number of correspondences seen"""
        total = 0
        for radius in radii:
            found = pm.search(self.A, self.mask, self.xyz, self.D, self.T, M, K, radius, dist=self.dist)
            for ratio in ratios:
                for cross in crosses:
                    for md in dists:
                        want, _ = pm.accept(found, self.xyz, self.T, ratio, cross, md)
                        for ctx in ctxs:
                            got = self.gpu(ah, M, K, radius, ratio, cross, md, ctx)
                            assert len(got) == len(want), (what, radius, ratio, cross, md, ctx is not None, len(got), len(want))
                            assert got.tobytes() == want.tobytes(), (what, radius, ratio, cross, md, ctx is not None)
                            total += len(want)
        return total


@pytest.mark.parametrize("nA,n2", SIZES)
def test_lifted_fixture_bit_exact(ah, torch, synth, det, nA, n2):
    """build_lifted (the guided fixture's partners, in-gate decoys, closer out-of-gate decoys and rivals, lifted under the planted
    view) at every size x radius x ratio x cross-check x max_dist x {no context, a context}; again with a shuffled list A (`train` a
    permutation, D reordered) and a mask that drops every fifth landmark.  At the sizes that can carry them the fixture's shares
    are asserted on the statement (the same bars and seeds: test_projected_match_cpu.py)."""
    A, xyz, D, T, M = build_lifted(synth, nA, n2, ah.POINT_DTYPE)
    if nA >= 300:
        s = fixture_shares(A, xyz, D, T, M)
        assert s["accepted"] >= 0.25 and s["differs"] >= 0.05 and s["ratio"] >= 0.05 and s["cross"] >= 0.01, s
    kw = dict(ctxs=(None, det.ctx), ratios=((1, 1), (4, 5)), crosses=(False, True), dists=(0, 40))
    total = Case(torch, A, None, xyz, D, T).check(ah, M, K_LIFT, RADII, (nA, n2), **kw)
    A2, D2, mask = shuffled(A, xyz, D, 11 + nA)
    total2 = Case(torch, A2, mask, xyz, D2, T).check(ah, M, K_LIFT, RADII, (nA, n2, "shuffled"), **kw)
    if nA >= 63 and n2 >= 63:
        assert total > 0 and 0 < total2 < total


def test_gate_boundary_is_strict(ah, torch):
    """R = I, integer t, K = (1, 1, 0, 0), Z = 1, integer coordinates: dx dx + dy dy == r2 exactly for the offsets (3, 4), (5, 0),
    (0, -5), (-4, 3) at radius 5 -- the strict < rejects them; (2, 4) and (4, 2) are inside.  Repeated at nextafter(5, 6)"""
    M = rt12(np.eye(3), (30.0, -20.0, 0.0))
    offs = [(3, 4), (5, 0), (0, -5), (-4, 3), (2, 4), (4, 2)]
    rng = np.random.default_rng(1)
    q = random_points(rng, 6 * 20, ah.POINT_DTYPE)
    q["x"] = (20 + 25 * (np.arange(len(q)) % 24)).astype(np.float32)
    q["y"] = (30 + 40 * (np.arange(len(q)) // 24)).astype(np.float32)
    t = q.copy()
    for i in range(len(q)):
        t["x"][i] = q["x"][i] + 30 + offs[i % 6][0]
        t["y"][i] = q["y"][i] - 20 + offs[i % 6][1]
    xyz = np.stack([q["x"], q["y"], np.ones(len(q), np.float32)], axis=1)
    A = identity_list(len(q))
    K1 = (1.0, 1.0, 0.0, 0.0)
    g = pm.gate(A, None, xyz, len(q), t, M, K1, 5.0)
    on, inside = np.arange(len(q)) % 6 < 4, np.arange(len(q)) % 6 >= 4
    assert not g[on, on].any() and g[inside, inside].all()
    case = Case(torch, A, None, xyz, q, t)
    got = case.gpu(ah, M, K1, 5.0)
    assert np.array_equal(got["src3d"], np.nonzero(inside)[0]) and np.array_equal(got["src2d"], got["src3d"])
    up = np.nextafter(np.float32(5), np.float32(6))
    assert pm.gate(A, None, xyz, len(q), t, M, K1, up)[on, on].all()
    assert case.check(ah, M, K1, (5.0, up), "boundary") == 40 + 120


def test_behind_the_camera_and_non_finite_records(ah, torch, synth, det):
    """a pose that puts about half the landmarks behind the camera -- mirrored through its centre, so they project onto their
    partner's pixel from behind -- and some at exactly zc = 0; NaN / +-inf in xyz and in T; a train set with no finite point"""
    M = rt12(synth.rotation_zyx((1.0, -2.0, 0.5)), (0.2, -0.1, -8.0))
    q, t = build_pair(400, 500, 5, ah.POINT_DTYPE, H=IDENTITY)
    xyz, _ = lift(synth, q, 31, M=M, depth=(-8.0, 8.0))
    flat = rt12(np.eye(3), (0.0, 0.0, -8.0))                                # zc = Z - 8: exactly 0 where Z = 8
    xyz2, _ = lift(synth, q, 32, M=flat, depth=(-8.0, 8.0))
    xyz2[::13, 2] = 8.0
    A = identity_list(len(q))
    for pts, view in ((xyz, M), (xyz2, flat)):
        zc = pm.project(pts, view, K_LIFT)[2]
        assert (zc <= 0).sum() > 100 and (zc > 0).sum() > 100
        case = Case(torch, A, None, pts, q, t)
        assert case.check(ah, view, K_LIFT, (3.0, 50.0), "behind", ctxs=(None, det.ctx)) > 100
        got = case.gpu(ah, view, K_LIFT, 3.0, (1, 1), False)
        assert (zc[got["src3d"]] > 0).all()
    assert (pm.project(xyz2, flat, K_LIFT)[2] == 0).sum() >= 30
    A, xyz, D, T, M = build_lifted(synth, 400, 500, ah.POINT_DTYPE, seed=6)
    xyz[::7, 0], xyz[3::11, 1], xyz[5::13, 2], xyz[6::17, 2] = np.nan, np.inf, -np.inf, np.nan
    T["x"][::5], T["y"][1::9], T["y"][2::17] = np.inf, np.nan, -np.inf
    assert Case(torch, A, None, xyz, D, T).check(ah, M, K_LIFT, (3.0, 50.0), "non-finite", ctxs=(None, det.ctx)) > 50
    T["x"][:], T["y"][:] = np.nan, np.nan                                    # no finite train point at all
    assert len(Case(torch, A, None, xyz, D, T).gpu(ah, M, K_LIFT, 3.0)) == 0


def test_points_outside_any_extent(ah, torch, synth, det):
    """projections and train points around -800 px and at 1e5, and a train set that also holds points at 1e5, 3e6 and 1e30:
    whatever extent the binning assumes, every gated point is found"""
    for k, (sx, sy) in enumerate(((-800.0, -900.0), (1e5, 1e5))):
        H = np.array([1, 0, sx, 0, 1, sy, 0, 0, 1], np.float32)
        q, t = build_pair(500, 800, 20 + k, ah.POINT_DTYPE, H=H)
        px, py, _ = gr.project(q, H)
        xyz, M = lift(synth, np.stack([px, py], axis=1), 40 + k)
        if k == 0:
            t["x"][::10] += np.float32(1e5)                              # far outliers stretch or leave the box
            t["y"][5::10] = 3e6
            t["x"][7::50] = 1e30
        case = Case(torch, identity_list(len(q)), None, xyz, q, t)
        assert len(pm.match_projected(case.A, None, xyz, q, t, M, K_LIFT, 3.0)[0]) > 100
        case.check(ah, M, K_LIFT, RADII, ("shift", k), ctxs=(None, det.ctx))


def test_one_cell_duplicates_and_ties(ah, torch):
    """every train point at one of two positions (one cell, J_m of hundreds) and descriptors from a few prototypes: equal distances
    inside a gate go to the smallest index, in both directions; two landmarks with the same `train` (the same descriptor) and the
    same point: the cross-check keeps the smaller m"""
    rng = np.random.default_rng(3)
    q = random_points(rng, 100, ah.POINT_DTYPE)
    t = random_points(rng, 500, ah.POINT_DTYPE)
    t["x"], t["y"] = np.where(np.arange(500) % 2, 320.0, 320.5).astype(np.float32), 240.0
    q["x"] = (320 + rng.uniform(-1, 1, 100)).astype(np.float32)
    q["y"] = (240 + rng.uniform(-1, 1, 100)).astype(np.float32)
    t["features"] = t["features"][rng.integers(0, 5, 500)]
    q["features"] = q["features"][rng.integers(0, 3, 100)]
    for i in range(0, 100, 3):                                           # some landmarks close to a train prototype
        q["features"][i] = t["features"][i % 5]
        q["features"][i][i % 61] ^= 1
    xyz = np.stack([q["x"], q["y"], np.ones(100, np.float32)], axis=1)
    A = identity_list(100)
    K1 = (1.0, 1.0, 0.0, 0.0)
    assert pm.gate(A, None, xyz, 100, t, None, K1, 3.0).sum(axis=1).min() >= 250
    case = Case(torch, A, None, xyz, q, t)
    assert case.check(ah, None, K1, (0.9, 3.0), "ties", ratios=((1, 1), (4, 5), (1000, 1)), crosses=(False, True)) > 0
    assert len(pm.match_projected(A, None, xyz, q, t, None, K1, 3.0, (1000, 1), True, 0)[0]) > 0
    # twins: landmarks 0 and 1 are the same point with the same descriptor, one train point at their projection
    q2 = random_points(rng, 4, ah.POINT_DTYPE)
    t2 = q2[:3].copy()
    A2 = identity_list(4)
    A2["train"][1] = 0
    xyz2 = np.array([[10, 10, 1], [10, 10, 1], [200, 50, 1], [90, 300, 1]], np.float32)
    t2["x"], t2["y"] = xyz2[[0, 2, 3], 0], xyz2[[0, 2, 3], 1]
    t2["features"] = q2["features"][[0, 2, 3]]
    twins = Case(torch, A2, None, xyz2, q2, t2)
    both = twins.gpu(ah, None, K1, 2.0, (4, 5), False)
    kept = twins.gpu(ah, None, K1, 2.0, (4, 5), True)
    assert both["src3d"].tolist() == [0, 1, 2, 3] and both["src2d"].tolist() == [0, 0, 1, 2]
    assert kept["src3d"].tolist() == [0, 2, 3]
    twins.check(ah, None, K1, (2.0,), "twins", crosses=(False, True))


@pytest.mark.parametrize("n1,n2", [(1, 1), (65, 63), (300, 1000)])
def test_identity_view_equals_guided_matching(ah, torch, det, n1, n2):
    """a property that needs no statement: R = I, t = 0, K = (1, 1, 0, 0), Z = 1, an identity list A and |coordinates| <= 4096 --
    the projection is the query's position, and the list equals hak_match_guided's under H = identity field for field"""
    from test_gpu_guided_match import gpu_guided
    q, t = build_pair(n1, n2, 70 + n1, ah.POINT_DTYPE, H=IDENTITY)
    q["x"] *= 4.0
    q["y"] *= -5.0
    t["x"] *= 4.0
    t["y"] *= -5.0
    assert max(np.abs(q["x"]).max(), np.abs(t["y"]).max()) <= 4096.0
    xyz = np.stack([q["x"], q["y"], np.ones(n1, np.float32)], axis=1)
    case = Case(torch, identity_list(n1), None, xyz, q, t)
    seen = 0
    for radius, ratio, cross, md in ((3.0, (4, 5), True, 0), (20.0, (1, 1), True, 0), (1.5, (4, 5), False, 40), (1e5, (4, 5), True, 0)):
        for ctx in (None, det.ctx):
            got = case.gpu(ah, None, (1.0, 1.0, 0.0, 0.0), radius, ratio, cross, md, ctx)
            _, glist, _ = gpu_guided(ah, torch, q, t, IDENTITY, radius, ratio, cross, md, ctx)
            assert np.array_equal(got["src3d"], glist["query"]) and np.array_equal(got["src2d"], glist["train"])
            assert np.array_equal(got["u"].view(np.uint32), glist["x2"].view(np.uint32))
            assert np.array_equal(got["v"].view(np.uint32), glist["y2"].view(np.uint32))
            assert np.array_equal(got["X"].view(np.uint32), glist["x1"].view(np.uint32)) and not got["pad"].any()
            seen += len(got)
    assert seen > 0 or n1 < 65                                               # (a single random pair has no partner to accept)


def _record(ah, kind, M, flag):
    rec = np.zeros((), ah.POSE_DTYPE if kind == ah.VIEW_RELATIVE else ah.ABS_POSE_DTYPE)
    rec["R"], rec["t"], rec["inliers"], rec["n"] = M[:9], M[9:], 5, 9
    rec["candidate" if kind == ah.VIEW_RELATIVE else "hypothesis"] = flag
    return rec


def test_batch_ragged_equals_single_calls(ah, torch, synth, det):
    """seven lists at max_pts = 600 with ragged counts (0, 1, 600, one with an empty T, one above its stride: clamped), views of
    every kind with view steps 0 and 1 and count steps 1 and 3; with a view per list, one without a model and one with a NaN in R
    give count 0.  Every slot equals its single call; the 0xEE-prefilled buffers are untouched past the counts"""
    mp, npairs = 600, 7
    shapes = [(0, 50), (1, 1), (600, 600), (300, 0), (600, 500), (200, 500), (100, 100)]        # (landmarks = descriptors, train points)
    over = {4: (650, 700, 500)}                                          # the counts list 4 reports: above the strides
    NO_MODEL, NAN_R = 5, 6
    runs = [(ah.VIEW_IDENTITY, 0, 1, False), (ah.VIEW_RELATIVE, 1, 3, True), (ah.VIEW_ABSOLUTE, 1, 1, False), (ah.VIEW_ABSOLUTE, 0, 3, True),
            (ah.VIEW_RELATIVE, 0, 1, False)]
    K = ah.intrinsics(K_LIFT)
    for kind, vstep, cstep, with_mask in runs:
        views = [EYE if kind == ah.VIEW_IDENTITY else rt12(synth.rotation_zyx((1.0 + k, -2.0, 0.5 * k)), (0.1 * k, -0.2, 0.3))
                 for k in range(npairs)]
        if vstep == 0:
            views = [views[0]] * npairs
        hA = np.zeros((npairs, mp), ah.MATCH_PAIR_DTYPE)
        hX = np.full((npairs, mp, 3), np.nan, np.float32)
        hM = np.ones((npairs, mp), np.uint8)
        hD, hT = np.zeros((npairs, mp), ah.POINT_DTYPE), np.zeros((npairs, mp), ah.POINT_DTYPE)
        cA, cD, cT = (np.full(npairs * cstep, 77, np.int32) for _ in range(3))      # the slots a step skips: decoys
        cases = []
        for k, (nA, n2) in enumerate(shapes):
            nD = nA
            q, t = build_pair(nA, n2, 300 + k, ah.POINT_DTYPE, H=IDENTITY)
            xyz, _ = lift(synth, q, 310 + k, M=views[k])
            A, D, mask = shuffled(identity_list(nA), xyz, q, 320 + k)
            hA[k, :nA], hX[k, :nA], hD[k, :nD], hT[k, :n2] = A, xyz, D, t
            hA[k, nA:]["train"] = 3                                      # records past a count are not the call's business
            if with_mask:
                hM[k, :nA] = mask
            cases.append((A, mask if with_mask else None, xyz, D, t))
            cA[k * cstep], cD[k * cstep], cT[k * cstep] = over.get(k, (nA, nD, n2))
        recs = None
        if kind != ah.VIEW_IDENTITY:
            recs = np.zeros(npairs if vstep else 1, ah.POSE_DTYPE if kind == ah.VIEW_RELATIVE else ah.ABS_POSE_DTYPE)
            for k in range(len(recs)):
                recs[k] = _record(ah, kind, views[k], 3 + k)
            if vstep:
                recs[NO_MODEL]["candidate" if kind == ah.VIEW_RELATIVE else "hypothesis"] = -1
                recs[NAN_R]["R"][4] = np.nan
        dA, dX, dM, dD, dT = upload(torch, hA), upload(torch, hX), upload(torch, hM), upload(torch, hD), upload(torch, hT)
        dcA, dcD, dcT = (torch.from_numpy(c).cuda() for c in (cA, cD, cT))
        dV = None if recs is None else upload(torch, recs)
        for cross in (1, 0):
            d_out = torch.full((npairs * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
            d_cnt = torch.full((npairs + 1,), -7, dtype=torch.int32, device="cuda")
            ah.check(ah.lib.hak_match_projected_batch(det.ctx, dA.data_ptr(), mp, dcA.data_ptr(), cstep, dM.data_ptr() if with_mask else None,
                                                      dX.data_ptr(), dD.data_ptr(), mp, dcD.data_ptr(), cstep, dT.data_ptr(), mp,
                                                      dcT.data_ptr(), cstep, npairs, None if dV is None else dV.data_ptr(), kind, vstep,
                                                      K.ctypes.data, 3.0, 4, 5, cross, 0, d_out.data_ptr(), mp, d_cnt.data_ptr()))
            ah.check(ah.lib.hak_sync(det.ctx))
            lists = d_out.cpu().numpy().reshape(npairs, mp * 32)
            cnts = d_cnt.cpu().numpy()
            assert cnts[npairs] == -7
            for k, (A, mask, xyz, D, t) in enumerate(cases):
                no_model = vstep == 1 and kind != ah.VIEW_IDENTITY and k in (NO_MODEL, NAN_R)
                if no_model:
                    want = np.zeros(0, ah.CORR3D_DTYPE)
                    assert len(pm.match_projected(A, mask, xyz, D, t, recs[k], K_LIFT, 3.0, (4, 5), bool(cross), 0)[0]) == 0
                else:
                    want = Case(torch, A, mask, xyz, D, t).gpu(ah, views[k], K_LIFT, 3.0, (4, 5), bool(cross), 0)
                assert cnts[k] == len(want), (kind, vstep, cstep, cross, k, int(cnts[k]), len(want))
                assert lists[k, :32 * len(want)].tobytes() == want.tobytes(), (kind, vstep, cstep, cross, k)
                assert (lists[k, 32 * len(want):] == 0xEE).all(), (kind, vstep, cstep, cross, k)
                if k == 2:
                    ref, _ = pm.match_projected(A, mask, xyz, D, t, views[k], K_LIFT, 3.0, (4, 5), bool(cross), 0)
                    assert want.tobytes() == ref.tobytes() and len(ref) > 100
        # the inputs are only read
        for dev, host in ((dA, hA), (dX, hX), (dD, hD), (dT, hT)):
            assert dev.cpu().numpy().tobytes() == np.ascontiguousarray(host).tobytes()


def test_chain_without_host_round_trip(ah, torch, synth):
    """two three-view scenes in the four-image layout (I0, I1, I1, I2): hak_match_knn2_batch -> hak_find_fundamental_batch ->
    hak_refine_fundamental_batch -> hak_recover_pose_batch -> hak_link_tracks_batch -> hak_solve_pnp_batch -> hak_refine_pnp_batch ->
    hak_match_projected_batch -> hak_refine_pnp_batch, all enqueued before ONE hak_sync, equals the statements' chain"""
    mp, seed, n = 1000, 5, 400
    legs = [(n, 0.5, 1), (n, 0.5, 2)]
    want = [chain(synth, nn, noise, s, ransac_seed=seed, max_index=mp) for nn, noise, s in legs]
    pts = np.zeros((8, mp), ah.POINT_DTYPE)
    num = np.zeros(8, np.int32)
    for j, w in enumerate(want):
        for slot, img in enumerate((0, 1, 1, 2)):
            pts[4 * j + slot, :2 * n] = w["scene"][3][img]
            num[4 * j + slot] = 2 * n
    det = ah.Akazer()
    det.init((640, 480, ah.iAlignUp(640, 128)), max_pts=mp, batch=8)
    K = ah.intrinsics(want[0]["scene"][0])
    d_p, d_n = upload(torch, pts), torch.from_numpy(num).cuda()
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    fill = lambda nbytes: torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
    lists, cnt = fill(4 * mp * 32), torch.zeros(4, dtype=torch.int32, device="cuda")
    fund, pose = zeros(4 * ah.FUNDAMENTAL_DTYPE.itemsize), zeros(4 * 64)
    pmask, xyz = fill(4 * mp), fill(4 * mp * 12)
    corr, corrp = fill(2 * mp * 32), fill(2 * mp * 32)
    nc, ncp = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    absp, am, amp = zeros(2 * 64), fill(2 * mp), fill(2 * mp)
    lib, ctx, kp, L, Cn, P, N = ah.lib, det.ctx, K.ctypes.data, lists.data_ptr(), cnt.data_ptr(), d_p.data_ptr(), d_n.data_ptr()
    ah.check(lib.hak_match_knn2_batch(ctx, P, N, 4, 4, 5, 1, 0, L, Cn))
    ah.check(lib.hak_find_fundamental_batch(ctx, L, mp, Cn, 4, 256, 1.0, seed, fund.data_ptr(), None))
    ah.check(lib.hak_refine_fundamental_batch(ctx, L, mp, Cn, 4, 1.0, 3, fund.data_ptr(), None))
    ah.check(lib.hak_recover_pose_batch(ctx, L, mp, Cn, 4, fund.data_ptr(), kp, kp, 1.0, 50.0, pose.data_ptr(), pmask.data_ptr(), xyz.data_ptr()))
    ah.check(lib.hak_link_tracks_batch(ctx, L, 2 * mp, Cn, 2, pmask.data_ptr(), xyz.data_ptr(), L + 32 * mp, 2 * mp, Cn + 4, 2, 2,
                                       corr.data_ptr(), mp, nc.data_ptr()))
    ah.check(lib.hak_solve_pnp_batch(ctx, corr.data_ptr(), mp, nc.data_ptr(), 2, kp, 256, 2.0, seed, absp.data_ptr(), None))
    ah.check(lib.hak_refine_pnp_batch(ctx, corr.data_ptr(), mp, nc.data_ptr(), 2, kp, 2.0, 3, absp.data_ptr(), am.data_ptr()))
    ah.check(lib.hak_match_projected_batch(ctx, L, 2 * mp, Cn, 2, pmask.data_ptr(), xyz.data_ptr(), P + 104 * mp, 4 * mp, N + 4, 4,
                                           P + 104 * 3 * mp, 4 * mp, N + 12, 4, 2, absp.data_ptr(), ah.VIEW_ABSOLUTE, 1, kp, CHAIN_RADIUS,
                                           4, 5, 1, 0, corrp.data_ptr(), mp, ncp.data_ptr()))
    ah.check(lib.hak_refine_pnp_batch(ctx, corrp.data_ptr(), mp, ncp.data_ptr(), 2, kp, 2.0, 3, absp.data_ptr(), amp.data_ptr()))
    ah.check(lib.hak_sync(ctx))
    g_lists, g_cnt = lists.cpu().numpy().reshape(4, mp * 32), cnt.cpu().numpy()
    g_corr, g_corrp = corr.cpu().numpy().reshape(2, mp * 32), corrp.cpu().numpy().reshape(2, mp * 32)
    g_nc, g_ncp = nc.cpu().numpy(), ncp.cpu().numpy()
    g_abs = absp.cpu().numpy().view(ah.ABS_POSE_DTYPE)
    g_pose = pose.cpu().numpy().view(ah.POSE_DTYPE)
    g_am, g_amp = am.cpu().numpy().reshape(2, mp), amp.cpu().numpy().reshape(2, mp)

    def same_list(raw, count, wanted, what):
        assert count == len(wanted), (what, count, len(wanted))
        assert raw[:32 * count].tobytes() == wanted.tobytes() and (raw[32 * count:] == 0xEE).all(), what

    for j, w in enumerate(want):
        same_list(g_lists[2 * j], int(g_cnt[2 * j]), w["A"], ("2-NN (I0, I1)", j))
        same_list(g_lists[2 * j + 1], int(g_cnt[2 * j + 1]), w["B"], ("2-NN (I1, I2)", j))
        assert g_pose[2 * j].tobytes() == np.array(w["pose"], ah.POSE_DTYPE).tobytes(), ("pose", j)
        same_list(g_corr[j], int(g_nc[j]), w["corr"], ("link", j))
        assert np.array_equal(g_am[j][:len(w["corr"])], w["mask2"]), ("inliers before the re-match", j)
        same_list(g_corrp[j], int(g_ncp[j]), w["corrp"], ("re-match", j))
        assert g_abs[j].tobytes() == np.array(w["ref3"], ah.ABS_POSE_DTYPE).tobytes(), ("pose of I2 after the re-match", j, g_abs[j], w["ref3"])
        assert np.array_equal(g_amp[j][:len(w["corrp"])], w["mask3"]) and (g_amp[j][len(w["corrp"]):] == 0xEE).all(), ("inliers", j)
        assert w["ref2"]["hypothesis"] >= 0 and len(w["corrp"]) > 100
        # more inliers after the re-match is a property of the data, not of the kernel: asserted only where the statement says so
        if w["ref3"]["inliers"] >= w["ref2"]["inliers"]:
            assert g_abs[j]["inliers"] >= w["ref2"]["inliers"]
    det.close()


def test_python_wrapper(ah, torch, synth, det):
    A, xyz, D, T, M = build_lifted(synth, 300, 1000, ah.POINT_DTYPE)
    A2, D2, mask = shuffled(A, xyz, D, 4)
    res = []
    for recs in (D2, T):
        data = ah.AkazeData()
        ah.initAkazeData(data, len(recs), False, True)
        ah.check(ah.lib.hak_memcpy_h2d(data.d_data, np.ascontiguousarray(recs).ctypes.data, recs.nbytes))
        data.num_pts = len(recs)
        res.append(data)
    try:
        want, _ = pm.match_projected(A2, mask, xyz, D2, T, M, K_LIFT, 3.0, (4, 5), True, 0)
        absr = _record(ah, ah.VIEW_ABSOLUTE, M, 0)
        for args, kw in (((A2, xyz, res[0], res[1], M, K_LIFT), dict(radius=3.0, maskA=mask)),
                         ((upload(torch, A2), torch.from_numpy(xyz).cuda(), res[0], res[1], absr, ah.intrinsics(K_LIFT)),
                          dict(radius=3.0, maskA=torch.from_numpy(mask).cuda(), akazer=det)),
                         ((A2, xyz, res[0], res[1], _record(ah, ah.VIEW_RELATIVE, M, 2), K_LIFT), dict(radius=3.0, maskA=mask))):
            got = ah.matchProjected(*args, **kw)
            assert got.dtype == ah.CORR3D_DTYPE and got.tobytes() == want.tobytes() and len(want) > 50
        w8, _ = pm.match_projected(A2, None, xyz, D2, T, M, K_LIFT, 8.0, (1, 1), False, 40)
        assert ah.matchProjected(A2, xyz, res[0], res[1], M, K_LIFT, ratio=(1, 1), cross_check=False, max_dist=40).tobytes() == w8.tobytes()
        assert len(ah.matchProjected(A2, xyz, res[0], res[1], _record(ah, ah.VIEW_ABSOLUTE, M, -1), K_LIFT)) == 0     # step 7 of the rule
        assert len(ah.matchProjected(A2[:0], xyz[:0], res[0], res[1], M, K_LIFT)) == 0
    finally:
        for data in res:
            ah.freeAkazeData(data)


def test_bad_arguments(ah, torch, det):
    d = torch.zeros(64 * 104, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls, keep, hcnt = refusals(ah, det.ctx, d.data_ptr(), cnt.data_ptr())
    assert len(calls) >= 60
    K = ah.intrinsics(K_LIFT)
    ok = C.c_int(-1)
    for k, (fn, args, word) in enumerate(calls):
        ah.check(ah.lib.hak_match_projected(None, d.data_ptr(), 4, None, d.data_ptr(), d.data_ptr(), 4, d.data_ptr(), 4, None, K.ctypes.data,
                                            8.0, 4, 5, 1, 0, None, C.byref(ok), None))      # succeeds in between
        assert ok.value >= 0
        assert fn(*args) != 0, (k, args)
        assert word in ah.lib.hak_last_error().decode(), (k, word)
    ah.check(ah.lib.hak_sync(det.ctx))
    assert not d.any() and not cnt.any() and hcnt.value == -5

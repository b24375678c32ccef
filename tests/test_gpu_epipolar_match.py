"""GPU suite: epipolar guided matching (hak_match_epipolar / hak_match_epipolar_batch, kernels_epipolar.hip) bit for bit against its
numpy statement tests/epipolar_match_ref.py -- the match fields of every query, the match list and the count -- on planted pairs
with decoys, the boundary of the band, every line orientation, train sets that defeat the binning, the rule's domain, ragged
batches, the 2-NN -> RANSAC -> epipolar chain and the demo's --epipolar leg."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import epipolar_match_ref as er
from conftest import ROOT
from test_epipolar_match_cpu import F_XSHIFT, build_pair_epipolar, scene_F
from test_guided_match_cpu import SIZES, random_points
from test_gpu_guided_match import FIELDS, assert_same, gpu_guided, upload

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
F_YSHIFT = np.array([0, 0, 1, 0, 0, 0, -1, 0, 0], np.float32)           # the line of (x, y) is x2 = x
F_DIAG = np.array([0, 0, 1, 0, 0, -1, -1, 1, 0], np.float32)            # a = 1, b = -1 exactly: y2 = x2 + (y - x)
F_FORWARD = np.array([0, -1, 240, 1, 0, -320, -240, 320, 0], np.float32)   # epipole (320, 240) in both images


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def det(ah):
    """a context for the calls that take one (the geometry does not matter to the matcher)"""
    d = ah.Akazer()
    d.init((640, 480, ah.iAlignUp(640, 128)), max_pts=600, batch=14)
    yield d
    d.close()


def gpu_epipolar(ah, torch, q, t, F, radius, ratio=(4, 5), cross=True, max_dist=0, ctx=None):
    """one synchronous call: (pts1 with the match fields the call copied to the host, match list, the device's point records)"""
    n1, n2 = len(q), len(t)
    d1, d2 = upload(torch, q), upload(torch, t)
    d_out = torch.full((max(n1, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(n1, 1), ah.MATCH_PAIR_DTYPE)
    out = q.copy()
    cnt = C.c_int(-1)
    f = np.ascontiguousarray(F, np.float32)
    ah.check(ah.lib.hak_match_epipolar(ctx, d1.data_ptr(), n1, d2.data_ptr(), n2, f.ctypes.data_as(C.POINTER(C.c_float)), float(radius),
                                       ratio[0], ratio[1], int(cross), max_dist, out.ctypes.data, d_out.data_ptr(), C.byref(cnt),
                                       h_out.ctypes.data))
    dev = d1.cpu().numpy().view(ah.POINT_DTYPE)[:n1] if n1 else q.copy()
    lst_dev = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE)
    assert 0 <= cnt.value <= n1
    assert np.array_equal(lst_dev[:cnt.value].view(np.uint8), h_out[:cnt.value].view(np.uint8))
    assert (lst_dev[cnt.value:].view(np.uint8) == 0xEE).all()            # nothing written past the count
    return out, h_out[:cnt.value].copy(), dev


def check_against_statement(ah, torch, q, t, F, radii, what, ctxs=(None,), ratios=((4, 5),), crosses=(True,), dists=(0,)):
    """every combination against the statement; returns the statement's list lengths"""
    d = er.hamming(q, t) if len(q) and len(t) else None
    counts = []
    for radius in radii:
        for ratio in ratios:
            for cross in crosses:
                for md in dists:
                    wout, wlist, _ = er.match_epipolar(q, t, F, radius, ratio, cross, md, dist=d)
                    counts.append(len(wlist))
                    for ctx in ctxs:
                        got = gpu_epipolar(ah, torch, q, t, F, radius, ratio, cross, md, ctx)
                        assert_same(got, (wout, wlist), (what, radius, ratio, cross, md, ctx is not None))
    return counts


@pytest.mark.parametrize("n1,n2", SIZES)
def test_planted_pairs_bit_exact(ah, torch, det, n1, n2):
    """build_pair_epipolar (true partners on the line, in-band decoys, closer off-line decoys, off-line look-alikes, rivals) at
    every size x radius x ratio x cross-check x {no context, a context}; what the fixture holds is asserted on the statement in
    test_epipolar_match_cpu.py (the same seeds)"""
    q, t = build_pair_epipolar(n1, n2, 100 + n1, ah.POINT_DTYPE)
    counts = check_against_statement(ah, torch, q, t, scene_F(), (0.5, 2.0, 8.0), (n1, n2), ctxs=(None, det.ctx), ratios=((1, 1), (4, 5)),
                                     crosses=(False, True))
    if n1 >= 300:
        assert min(counts) >= n1 // 4
        check_against_statement(ah, torch, q, t, scene_F(), (2.0,), (n1, n2, "max_dist"), dists=(40,))


def test_band_boundary_is_strict(ah, torch):
    """pure sideways translation, integer coordinates: the line of (x, y) is y2 = y, e = y - y2 and den = 1 exactly.  At radius 2
    the train points at y - 2 and y + 2 are out (e e == r2 den), their float32 neighbours towards the line are in"""
    rng = np.random.default_rng(1)
    n = 40
    q = random_points(rng, n, ah.POINT_DTYPE)
    q["y"] = (16 + 10 * np.arange(n)).astype(np.float32)
    t = random_points(rng, 4 * n, ah.POINT_DTYPE)
    for i in range(n):
        y = q["y"][i]
        t["y"][4 * i:4 * i + 4] = [y - 2, y + 2, np.nextafter(np.float32(y - 2), y), np.nextafter(np.float32(y + 2), y)]
        t["features"][4 * i + 2 + i % 2] = q["features"][i]
    g = er.gate(q, t, F_XSHIFT, 2.0)
    own = np.repeat(np.arange(n), 4)
    assert np.array_equal(g, (own[None, :] == np.arange(n)[:, None]) & (np.arange(4 * n) % 4 >= 2)[None, :])
    out, lst, _ = gpu_epipolar(ah, torch, q, t, F_XSHIFT, 2.0)
    assert np.array_equal(out["match"], 4 * np.arange(n) + 2 + np.arange(n) % 2) and (out["distance"] == 0).all()
    check_against_statement(ah, torch, q, t, F_XSHIFT, (2.0, np.nextafter(np.float32(2), np.float32(3)), 1.9999), "boundary",
                            ratios=((1, 1), (4, 5)), crosses=(False, True))


@pytest.mark.parametrize("name,F", [("x-shift", F_XSHIFT), ("y-shift", F_YSHIFT), ("diagonal", F_DIAG), ("forward", F_FORWARD)])
def test_line_orientations(ah, torch, det, name, F):
    """horizontal lines (columns are walked), vertical lines (rows), the exact diagonal |a| == |b|, and the pencil of lines through
    an epipole inside the image -- every slope, and a query AT the epipole, which has a = b = 0 and no band"""
    q, t = build_pair_epipolar(400, 500, 30, ah.POINT_DTYPE, F=F)
    a, b, _, den = er.line(q, F)
    if name == "diagonal":
        assert (np.abs(a) == np.abs(b)).all()
    if name == "forward":
        q["x"][5], q["y"][5] = 320.0, 240.0
        q["x"][6], q["y"][6] = np.nextafter(np.float32(320), np.float32(321)), 240.0      # one float32 step away: a band again
        den = er.line(q, F)[3]
        assert den[5] == 0 and den[6] >= er.DEN_MIN and (np.abs(a) > np.abs(b)).sum() > 50 and (np.abs(a) < np.abs(b)).sum() > 50
    counts = check_against_statement(ah, torch, q, t, F, (0.5, 2.0, 8.0), name, ctxs=(None, det.ctx))
    assert min(counts) > 100
    if name == "forward":
        out, _, _ = gpu_epipolar(ah, torch, q, t, F, 1e4)
        assert out["match"][5] == -1


def test_lines_that_miss_the_box_and_box_corners(ah, torch):
    """train points confined to [100, 200]^2 with points exactly at its corners: most lines miss the box altogether (nothing to
    find, nothing to fault on), and on the exact diagonal the lines of (150, 50) and (50, 150) touch it at one corner only"""
    rng = np.random.default_rng(4)
    t = random_points(rng, 300, ah.POINT_DTYPE, w=100.0, h=100.0)
    t["x"] += 100
    t["y"] += 100
    t["x"][:4], t["y"][:4] = [100, 200, 100, 200], [100, 100, 200, 200]
    q = random_points(rng, 300, ah.POINT_DTYPE)
    q["x"][:2], q["y"][:2] = [150, 50], [50, 150]
    q["features"][0], q["features"][1] = t["features"][1], t["features"][2]
    for F in (F_XSHIFT, F_YSHIFT, F_DIAG, scene_F()):
        g = er.gate(q, t, F, 2.0)
        assert (~g.any(axis=1)).sum() > 50
        check_against_statement(ah, torch, q, t, F, (0.5, 2.0, 8.0), "box", ratios=((1, 1),), crosses=(False, True))
    g = er.gate(q, t, F_DIAG, 0.5)
    assert g[0, 1] and g[1, 2]
    out, _, _ = gpu_epipolar(ah, torch, q, t, F_DIAG, 0.5, (1000, 1), False)
    assert out["match"][0] == 1 and out["match"][1] == 2


def test_binning_independence(ah, torch, det):
    """train sets that collapse into one cell, that lie on one straight line (zero extent on an axis), duplicates with descriptor
    ties, and the planted set with one far-away in-domain train point that stretches the box and changes the cell side"""
    F = scene_F()
    rng = np.random.default_rng(3)
    q = random_points(rng, 100, ah.POINT_DTYPE)
    t = random_points(rng, 500, ah.POINT_DTYPE)
    t["features"] = t["features"][rng.integers(0, 5, 500)]
    q["features"] = q["features"][rng.integers(0, 3, 100)]
    for i in range(0, 100, 3):                                           # some queries close to a train prototype
        q["features"][i] = t["features"][i % 5]
        q["features"][i][i % 61] ^= 1
    t["x"], t["y"] = np.where(np.arange(500) % 2, 320.0, 320.5).astype(np.float32), 240.0                  # two positions, one cell
    check_against_statement(ah, torch, q, t, F, (2.0, 300.0), "one cell", ratios=((1, 1), (1000, 1)), crosses=(False, True))
    assert len(er.match_epipolar(q, t, F, 300.0, (1000, 1), True, 0)[1]) > 0
    t["x"] = rng.uniform(0, 640, 500).astype(np.float32)                                                # a horizontal row of points
    check_against_statement(ah, torch, q, t, F, (0.5, 8.0), "row", ratios=((1, 1), (1000, 1)), crosses=(False, True))
    t["y"], t["x"] = t["x"].copy(), np.float32(100.25)                                                   # a vertical one
    check_against_statement(ah, torch, q, t, F, (0.5, 8.0), "column", ratios=((1, 1), (1000, 1)), crosses=(False, True))
    # the planted set, then the same with a far point appended: it changes the grid, and nothing else
    q, t = build_pair_epipolar(300, 599, 400, ah.POINT_DTYPE)
    far = random_points(rng, 1, ah.POINT_DTYPE)
    far["x"], far["y"] = 16000.0, -16000.0
    t2 = np.concatenate([t, far])
    for radius in (0.5, 2.0):
        base = gpu_epipolar(ah, torch, q, t, F, radius, ctx=det.ctx)
        wide = gpu_epipolar(ah, torch, q, t2, F, radius, ctx=det.ctx)
        assert_same(wide, er.match_epipolar(q, t2, F, radius)[:2], ("far point", radius))
        untouched = ~er.gate(q, far, F, radius)[:, 0]
        assert untouched.sum() >= 290
        for f in FIELDS:
            assert np.array_equal(base[0][f][untouched].view(np.uint32), wide[0][f][untouched].view(np.uint32)), f


def test_domain(ah, torch, det):
    """records with NaN or inf, coordinates just inside and just outside +-16384, at 2^20 and at 1e30, on both sides; F scaled so
    that den lands on either side of 2^-100"""
    F = scene_F()
    q, t = build_pair_epipolar(400, 500, 6, ah.POINT_DTYPE)
    q["x"][::7], q["y"][3::11], q["x"][5::13] = np.nan, np.inf, -np.inf
    t["x"][::5], t["y"][1::9], t["y"][2::17] = np.inf, np.nan, -np.inf
    check_against_statement(ah, torch, q, t, F, (2.0, 50.0), "non-finite", ctxs=(None, det.ctx))
    t["x"][:], t["y"][:] = np.nan, np.nan                                # no finite train point at all
    out, lst, _ = gpu_epipolar(ah, torch, q, t, F, 2.0)
    assert (out["match"] == -1).all() and len(lst) == 0
    # the bounds: under the sideways translation a train point (x2, y) is on the line of (x, y) whatever x2 is
    edge = np.float32(16384)
    vals = np.array([edge, -edge, np.nextafter(edge, np.float32(np.inf)), -np.nextafter(edge, np.float32(np.inf)),
                     np.nextafter(edge, np.float32(0)), 2.0 ** 20, -2.0 ** 20, 1e30, -1e30, 2.0 ** 20 + 1], np.float32)
    rng = np.random.default_rng(8)
    n = 4 * len(vals)
    q = random_points(rng, n, ah.POINT_DTYPE)
    q["y"] = (8 + 11 * np.arange(n)).astype(np.float32)
    t = q.copy()
    t["x"][:len(vals)] = vals                                            # train x at the bound
    t["y"][len(vals):2 * len(vals)] = vals                               # train y at the bound (and the query's y follows)
    q["y"][len(vals):2 * len(vals)] = vals
    q["x"][2 * len(vals):3 * len(vals)] = vals                           # query x at the bound
    g = er.gate(q, t, F_XSHIFT, 2.0)
    inside = np.abs(vals) <= edge
    for blk in range(3):
        assert np.array_equal(np.diag(g)[blk * len(vals):(blk + 1) * len(vals)], inside), blk
    assert np.diag(g)[3 * len(vals):].all()
    check_against_statement(ah, torch, q, t, F_XSHIFT, (2.0, 50.0), "bounds", ctxs=(None, det.ctx), ratios=((1, 1), (4, 5)))
    # den = b b with b = -s: exactly 2^-100 is in the domain, one float32 step below is not
    q, t = build_pair_epipolar(200, 300, 7, ah.POINT_DTYPE, F=F_XSHIFT)
    at = F_XSHIFT * np.float32(2.0 ** -50)
    below = at.copy()
    below[5] = np.nextafter(at[5], np.float32(0))
    assert (er.line(q, at)[3] == er.DEN_MIN).all() and (er.line(q, below)[3] < er.DEN_MIN).all()
    counts = check_against_statement(ah, torch, q, t, at, (0.5, 2.0), "den at the floor")
    assert min(counts) > 50
    assert check_against_statement(ah, torch, q, t, below, (0.5, 2.0, 1e5), "den below the floor") == [0, 0, 0]


@pytest.mark.parametrize("n1,n2", [(1, 1), (65, 63), (300, 1000), (1500, 1500)])
def test_huge_radius_equals_knn2(ah, torch, det, n1, n2):
    """a property that needs no statement: radius 1e5, every den in the domain -- every pair is gated, and the call's output is
    byte-identical to hak_match_knn2's"""
    q, t = build_pair_epipolar(n1, n2, 70 + n1, ah.POINT_DTYPE)
    F = scene_F()
    assert (er.line(q, F)[3] >= er.DEN_MIN).all()
    for ratio, cross, md in (((1, 1), True, 0), ((4, 5), True, 0), ((4, 5), False, 40)):
        for ctx in (None, det.ctx):
            gout, glist, gdev = gpu_epipolar(ah, torch, q, t, F, 1e5, ratio, cross, md, ctx)
            kout, klist, kdev = gpu_guided(ah, torch, q, t, None, 0.0, ratio, cross, md, ctx, knn2=True)
            assert np.array_equal(gdev.view(np.uint8), kdev.view(np.uint8)) and np.array_equal(gout.view(np.uint8), kout.view(np.uint8))
            assert np.array_equal(glist.view(np.uint8), klist.view(np.uint8))
    if n1 >= 300:
        assert len(glist) > 0


def batch_buffers(ah, torch, host, num, recs, npairs, mp):
    return (upload(torch, host), torch.from_numpy(num).cuda(), upload(torch, recs),
            torch.full((npairs * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda"),
            torch.full((npairs,), -7, dtype=torch.int32, device="cuda"))


def test_batch_ragged_equals_single_calls(ah, torch, det):
    """seven pairs with ragged counts (0, 1, max_pts), one record without a model (hypothesis = -1) and one with a NaN in F: equal
    to the single calls slot by slot, count 0 and every query rejected for those two; enqueued on the context's stream and
    synchronised once.  A NULL d_F is refused."""
    mp = 600
    shapes = [(0, 50), (1, 1), (600, 600), (300, 0), (200, 500), (100, 100), (50, 60)]
    npairs = len(shapes)
    host = np.zeros((2 * npairs, mp), ah.POINT_DTYPE)
    num = np.zeros(2 * npairs, np.int32)
    recs = np.zeros(npairs, ah.FUNDAMENTAL_DTYPE)
    for k, (n1, n2) in enumerate(shapes):
        F = (scene_F(), F_XSHIFT, F_DIAG, F_FORWARD)[k % 4]
        q, t = build_pair_epipolar(n1, n2, 200 + k, ah.POINT_DTYPE, F=F)
        host[2 * k, :n1], host[2 * k + 1, :n2] = q, t
        host[2 * k, n1:]["x"] = np.nan                                    # records past the counts are not the call's business
        num[2 * k], num[2 * k + 1] = n1, n2
        recs[k]["F"], recs[k]["hypothesis"], recs[k]["inliers"], recs[k]["n"] = F, 3 + k, 10, 20
    recs[4]["hypothesis"] = -1
    recs[5]["F"][4] = np.nan
    for cross in (1, 0):
        d_pts, d_num, d_F, d_out, d_cnt = batch_buffers(ah, torch, host, num, recs, npairs, mp)
        assert ah.lib.hak_match_epipolar_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, None, 2.0, 4, 5, cross, 0,
                                               d_out.data_ptr(), d_cnt.data_ptr()) != 0
        ah.check(ah.lib.hak_match_epipolar_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, d_F.data_ptr(), 2.0, 4, 5, cross, 0,
                                                 d_out.data_ptr(), d_cnt.data_ptr()))
        ah.check(ah.lib.hak_sync(det.ctx))
        got = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(2 * npairs, mp)
        lists = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(npairs, mp)
        cnts = d_cnt.cpu().numpy()
        assert np.array_equal(got[1::2].view(np.uint8), host[1::2].view(np.uint8))         # the train sets are only read
        for k, (n1, n2) in enumerate(shapes):
            q, t = host[2 * k, :n1].copy(), host[2 * k + 1, :n2].copy()
            if k in (4, 5):
                assert cnts[k] == 0
                assert (got[2 * k, :n1]["match"] == -1).all() and (got[2 * k, :n1]["distance"] == -1).all()
                assert (got[2 * k, :n1]["match_x"] == -1).all() and (got[2 * k, :n1]["match_y"] == -1).all()
                continue
            sout, slist, _ = gpu_epipolar(ah, torch, q, t, recs[k]["F"], 2.0, (4, 5), bool(cross), 0)
            assert cnts[k] == len(slist), (k, cnts[k], len(slist))
            assert np.array_equal(lists[k, :cnts[k]].view(np.uint8), slist.view(np.uint8)), k
            assert (lists[k, cnts[k]:].view(np.uint8) == 0xEE).all()
            for f in FIELDS:
                assert np.array_equal(got[2 * k, :n1][f].view(np.uint32), sout[f].view(np.uint32)), (k, f)
            if k == 2:
                wout, wlist, _ = er.match_epipolar(q, t, recs[k]["F"], 2.0, (4, 5), bool(cross), 0)
                assert_same((sout, slist, got[2 * k, :n1]), (wout, wlist), "batch vs statement")
                assert len(wlist) > 100


def test_chain_without_host_round_trip(ah, torch, det):
    """uploaded planted sets -> hak_match_knn2_batch -> hak_find_fundamental_batch -> hak_match_epipolar_batch, all enqueued before
    ONE hak_sync: the epipolar result equals the statement applied to the F records read back afterwards"""
    mp, npairs = 600, 3
    host = np.zeros((2 * npairs, mp), ah.POINT_DTYPE)
    num = np.zeros(2 * npairs, np.int32)
    for k, (n1, n2) in enumerate(((300, 600), (600, 600), (5, 5))):
        host[2 * k, :n1], host[2 * k + 1, :n2] = build_pair_epipolar(n1, n2, 300 + k, ah.POINT_DTYPE)
        num[2 * k], num[2 * k + 1] = n1, n2
    d_pts, d_num, d_F, d_out, d_cnt = batch_buffers(ah, torch, host, num, np.zeros(npairs, ah.FUNDAMENTAL_DTYPE), npairs, mp)
    k_out = torch.zeros(npairs * mp * 32, dtype=torch.uint8, device="cuda")
    k_cnt = torch.zeros(npairs, dtype=torch.int32, device="cuda")
    ah.check(ah.lib.hak_match_knn2_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, 4, 5, 1, 0, k_out.data_ptr(), k_cnt.data_ptr()))
    ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, k_out.data_ptr(), mp, k_cnt.data_ptr(), npairs, 512, 1.0, 0, d_F.data_ptr(), None))
    ah.check(ah.lib.hak_match_epipolar_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, d_F.data_ptr(), 2.0, 4, 5, 1, 0,
                                             d_out.data_ptr(), d_cnt.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    recs = d_F.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
    got = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(2 * npairs, mp)
    lists = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(npairs, mp)
    cnts = d_cnt.cpu().numpy()
    assert recs[0]["hypothesis"] >= 0 and recs[1]["hypothesis"] >= 0 and recs[2]["hypothesis"] == -1
    for k in range(npairs):
        n1, n2 = num[2 * k], num[2 * k + 1]
        q, t = host[2 * k, :n1], host[2 * k + 1, :n2]
        wout, wlist, _ = er.match_epipolar(q, t, recs[k]["F"], 2.0, (4, 5), True, 0, model=recs[k]["hypothesis"] >= 0)
        assert_same((got[2 * k, :n1], lists[k, :cnts[k]], got[2 * k, :n1]), (wout, wlist), ("chain", k))
    assert cnts[0] > 50 and cnts[1] > 100 and cnts[2] == 0


def test_python_wrapper(ah, torch):
    q, t = build_pair_epipolar(300, 400, 11, ah.POINT_DTYPE)
    r1, r2 = ah.AkazeData(), ah.AkazeData()
    for r, pts in ((r1, q), (r2, t)):
        ah.initAkazeData(r, len(pts), True, True)
        ah.check(ah.lib.hak_memcpy_h2d(r.d_data, np.ascontiguousarray(pts).ctypes.data, pts.nbytes))
        r.h_data[:], r.num_pts = pts, len(pts)
    lst = ah.cuMatchEpipolar(r1, r2, scene_F())
    wout, wlist, _ = er.match_epipolar(q, t, scene_F(), 2.0)
    assert_same((r1.h_data, lst, r1.h_data), (wout, wlist), "wrapper")
    assert len(lst) > 50
    ah.freeAkazeData(r1)
    ah.freeAkazeData(r2)


def test_demo_epipolar_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --epipolar 2` on left/right.pgm prints the two new lines (and implies --fundamental); their counts equal what
    the Python calls compute from the dumped points and the dumped F"""
    from test_gpu_dropin import write_pgm
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    r = subprocess.run(["timeout", "-k", "10", "300", DEMO, "0", left, right, "1", "--dump", dump, "--epipolar", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fundamental matrix (RANSAC" in r.stdout
    m = re.search(r"^Epipolar matches \(radius 2 px, ratio 0.8 \+ cross-check\): (\d+) against (\d+) of the 2-NN match", r.stdout, re.M)
    m2 = re.search(r"^Fundamental matrix of the epipolar matches: (\d+) inliers of (\d+) against (\d+) of (\d+)", r.stdout, re.M)
    assert m and m2, r.stdout
    raw = open(dump, "rb").read()
    n1, n2 = (int(v) for v in np.frombuffer(raw, np.int32, 2, 0))
    pts = np.frombuffer(raw, ah.POINT_DTYPE, n1 + n2, 8).copy()
    off = 8 + 104 * (n1 + n2)
    f1, f2 = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    off += 8 + 104 * (f1 + f2)
    n, inl = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    F = np.frombuffer(raw, np.float32, 9, off + 8).copy()
    _, lst, _ = gpu_epipolar(ah, torch, pts[:n1], pts[n1:], F, 2.0)
    rec, _ = ah.findFundamental(lst)
    assert (int(m.group(1)), int(m.group(2))) == (len(lst), n)
    assert [int(v) for v in m2.groups()] == [int(rec["inliers"]), len(lst), inl, n]
    assert len(lst) > 100
    wout, wlist, _ = er.match_epipolar(pts[:n1], pts[n1:], F, 2.0)
    assert np.array_equal(lst.view(np.uint8), np.ascontiguousarray(wlist).view(np.uint8))

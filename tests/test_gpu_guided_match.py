"""GPU suite: guided matching (hak_match_guided / hak_match_guided_batch, kernels_guided.hip) bit for bit against its numpy
statement tests/guided_match_ref.py -- the match fields of every query, the match list and the count -- on planted pairs with
decoys, the boundary cases of the gate, ragged batches, the detect -> 2-NN -> RANSAC -> guided chain and the demo's --guided leg."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guided_match_ref as gr
from conftest import ROOT
from test_guided_match_cpu import H_MILD, IDENTITY, SIZES, build_pair, fixture_shares, random_points

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
FIELDS = ("match", "distance", "match_x", "match_y")


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


def upload(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda() if len(recs) else \
        torch.zeros(128, dtype=torch.uint8, device="cuda")


def gpu_guided(ah, torch, q, t, H, radius, ratio=(4, 5), cross=True, max_dist=0, ctx=None, knn2=False):
    """one synchronous call: (pts1 with the match fields the call copied to the host, match list, the device's point records)"""
    n1, n2 = len(q), len(t)
    d1, d2 = upload(torch, q), upload(torch, t)
    d_out = torch.full((max(n1, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(n1, 1), ah.MATCH_PAIR_DTYPE)
    out = q.copy()
    cnt = C.c_int(-1)
    if knn2:
        ah.check(ah.lib.hak_match_knn2(ctx, d1.data_ptr(), n1, d2.data_ptr(), n2, ratio[0], ratio[1], int(cross), max_dist,
                                       out.ctypes.data, d_out.data_ptr(), C.byref(cnt), h_out.ctypes.data))
    else:
        h = np.ascontiguousarray(H, np.float32)
        ah.check(ah.lib.hak_match_guided(ctx, d1.data_ptr(), n1, d2.data_ptr(), n2, h.ctypes.data_as(C.POINTER(C.c_float)), float(radius),
                                         ratio[0], ratio[1], int(cross), max_dist, out.ctypes.data, d_out.data_ptr(), C.byref(cnt),
                                         h_out.ctypes.data))
    dev = d1.cpu().numpy().view(ah.POINT_DTYPE)[:n1] if n1 else q.copy()
    lst_dev = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE)
    assert 0 <= cnt.value <= n1
    assert np.array_equal(lst_dev[:cnt.value].view(np.uint8), h_out[:cnt.value].view(np.uint8))
    assert (lst_dev[cnt.value:].view(np.uint8) == 0xEE).all()            # nothing written past the count
    return out, h_out[:cnt.value].copy(), dev


def assert_same(got, want, what):
    (gout, glist, gdev), (wout, wlist) = got, want
    for f in FIELDS:
        assert np.array_equal(gout[f].view(np.uint32), wout[f].view(np.uint32)), (what, f, int((gout[f] != wout[f]).sum()))
        assert np.array_equal(gdev[f].view(np.uint32), wout[f].view(np.uint32)), (what, "device", f)
    assert len(glist) == len(wlist), (what, "count", len(glist), len(wlist))
    assert np.array_equal(glist.view(np.uint8), np.ascontiguousarray(wlist).view(np.uint8)), (what, "list")


def check_against_statement(ah, torch, q, t, H, radii, what, ctxs=(None,), ratios=((4, 5),), crosses=(True,), dists=(0,)):
    d = gr.hamming(q, t) if len(q) and len(t) else None
    for radius in radii:
        for ratio in ratios:
            for cross in crosses:
                for md in dists:
                    wout, wlist, _ = gr.match_guided(q, t, H, radius, ratio, cross, md, dist=d)
                    for ctx in ctxs:
                        got = gpu_guided(ah, torch, q, t, H, radius, ratio, cross, md, ctx)
                        assert_same(got, (wout, wlist), (what, radius, ratio, cross, md, ctx is not None))


@pytest.mark.parametrize("n1,n2", SIZES)
def test_planted_pairs_bit_exact(ah, torch, det, n1, n2):
    """build_pair (true partners, in-gate decoys, closer out-of-gate decoys, rivals) at every size x radius x ratio x cross-check x
    max_dist x {no context, a context}.  At the sizes that can carry them the fixture's shares are asserted on the statement at
    radius 3, ratio 4/5, cross-check on: >= 25 % accepted, >= 5 % matched differently from the ungated 2-NN rule, >= 5 % rejected
    by the ratio test inside the gate, >= 1 % by the cross-check alone (the same seeds: test_guided_match_cpu.py)."""
    q, t = build_pair(n1, n2, 100 + n1, ah.POINT_DTYPE)
    if n1 >= 300:
        s = fixture_shares(q, t)
        assert s["accepted"] >= 0.25 and s["differs"] >= 0.05 and s["ratio"] >= 0.05 and s["cross"] >= 0.01, s
    check_against_statement(ah, torch, q, t, H_MILD, (0.5, 3.0, 20.0), (n1, n2), ctxs=(None, det.ctx), ratios=((1, 1), (4, 5)),
                            crosses=(False, True), dists=(0, 40))


def test_gate_boundary_is_strict(ah, torch):
    """integer translation, integer coordinates: dx dx + dy dy == r2 exactly for the offsets (3, 4), (5, 0), (0, -5), (-4, 3) at
    radius 5 -- the strict < rejects them; (2, 4) and (4, 2) are inside"""
    H = np.array([1, 0, 30, 0, 1, -20, 0, 0, 1], np.float32)
    offs = [(3, 4), (5, 0), (0, -5), (-4, 3), (2, 4), (4, 2)]
    rng = np.random.default_rng(1)
    q = random_points(rng, 6 * 20, ah.POINT_DTYPE)
    q["x"] = (20 + 25 * (np.arange(len(q)) % 24)).astype(np.float32)
    q["y"] = (30 + 40 * (np.arange(len(q)) // 24)).astype(np.float32)
    t = q.copy()
    for i in range(len(q)):
        t["x"][i] = q["x"][i] + 30 + offs[i % 6][0]
        t["y"][i] = q["y"][i] - 20 + offs[i % 6][1]
    g = gr.gate(q, t, H, 5.0)
    on, inside = np.arange(len(q)) % 6 < 4, np.arange(len(q)) % 6 >= 4
    assert not g[on, on].any() and g[inside, inside].all()
    out, lst, _ = gpu_guided(ah, torch, q, t, H, 5.0)
    assert (out["match"][on] == -1).all() and np.array_equal(out["match"][inside], np.nonzero(inside)[0])
    check_against_statement(ah, torch, q, t, H, (5.0, np.nextafter(np.float32(5), np.float32(6))), "boundary")


def test_wz_not_positive_and_non_finite_records(ah, torch, det):
    q, t = build_pair(400, 500, 5, ah.POINT_DTYPE)
    H = H_MILD.copy()
    H[6], H[7] = np.float32(-1.0 / 320.0), 0.0                           # wz <= 0 right of x = 320 (and exactly 0 somewhere near it)
    q["x"][7] = 320.0
    _, _, wz = gr.project(q, H)
    assert (wz <= 0).sum() > 50 and (wz > 0).sum() > 50
    check_against_statement(ah, torch, q, t, H, (3.0, 50.0), "wz", ctxs=(None, det.ctx))
    q, t = build_pair(400, 500, 6, ah.POINT_DTYPE)
    q["x"][::7], q["y"][3::11], q["x"][5::13] = np.nan, np.inf, -np.inf
    t["x"][::5], t["y"][1::9], t["y"][2::17] = np.inf, np.nan, -np.inf
    check_against_statement(ah, torch, q, t, H_MILD, (3.0, 50.0), "non-finite", ctxs=(None, det.ctx))
    t["x"][:], t["y"][:] = np.nan, np.nan                                # no finite train point at all
    out, lst, _ = gpu_guided(ah, torch, q, t, H_MILD, 3.0)
    assert (out["match"] == -1).all() and len(lst) == 0


def test_points_outside_any_extent(ah, torch, det):
    """sets shifted through H to around -500 and to 1e5, and a train set that also holds points at 1e5, 3e6 and 1e30: whatever
    extent the binning assumes, every gated point is found"""
    for k, (sx, sy) in enumerate(((-800.0, -900.0), (1e5, 1e5))):
        H = np.array([1, 0, sx, 0, 1, sy, 0, 0, 1], np.float32)
        q, t = build_pair(500, 800, 20 + k, ah.POINT_DTYPE, H=H)
        if k == 0:
            t["x"][::10] += np.float32(1e5)                              # far outliers stretch or leave the box
            t["y"][5::10] = 3e6
            t["x"][7::50] = 1e30
        _, lst, _ = gr.match_guided(q, t, H, 3.0)
        assert len(lst) > 100
        check_against_statement(ah, torch, q, t, H, (0.5, 3.0, 20.0), ("shift", k), ctxs=(None, det.ctx))


def test_one_cell_duplicates_and_ties(ah, torch):
    """every train point at one of two positions (one cell, J_i of hundreds) and descriptors from a few prototypes: equal distances
    inside a gate go to the smallest index, in both directions"""
    rng = np.random.default_rng(3)
    q = random_points(rng, 100, ah.POINT_DTYPE)
    t = random_points(rng, 500, ah.POINT_DTYPE)
    t["x"], t["y"] = np.where(np.arange(500) % 2, 320.0, 320.5).astype(np.float32), 240.0
    q["x"] = (320 + rng.uniform(-1, 1, 100)).astype(np.float32)
    q["y"] = (240 + rng.uniform(-1, 1, 100)).astype(np.float32)
    t["features"] = t["features"][rng.integers(0, 5, 500)]
    q["features"] = q["features"][rng.integers(0, 3, 100)]
    for i in range(0, 100, 3):                                           # some queries close to a train prototype
        q["features"][i] = t["features"][i % 5]
        q["features"][i][i % 61] ^= 1
    g = gr.gate(q, t, IDENTITY, 3.0)
    assert g.sum(axis=1).min() >= 250
    check_against_statement(ah, torch, q, t, IDENTITY, (0.9, 3.0), "ties", ratios=((1, 1), (4, 5), (1000, 1)), crosses=(False, True))
    out, lst, _ = gr.match_guided(q, t, IDENTITY, 3.0, (1000, 1), True, 0)
    assert len(lst) > 0


@pytest.mark.parametrize("n1,n2", [(1, 1), (65, 63), (300, 1000), (1500, 1500)])
def test_identity_huge_radius_equals_knn2(ah, torch, det, n1, n2):
    """a property that needs no statement: H = identity, |coordinates| <= 4096, radius 1e5 -- every pair is gated, and the call's
    output is byte-identical to hak_match_knn2's"""
    q, t = build_pair(n1, n2, 70 + n1, ah.POINT_DTYPE)
    q["x"] *= 4.0
    t["y"] *= -5.0
    assert max(np.abs(q["x"]).max(), np.abs(t["y"]).max()) <= 4096.0
    for ratio, cross, md in (((1, 1), True, 0), ((4, 5), True, 0), ((4, 5), False, 40)):
        for ctx in (None, det.ctx):
            gout, glist, gdev = gpu_guided(ah, torch, q, t, IDENTITY, 1e5, ratio, cross, md, ctx)
            kout, klist, kdev = gpu_guided(ah, torch, q, t, None, 0.0, ratio, cross, md, ctx, knn2=True)
            assert np.array_equal(gdev.view(np.uint8), kdev.view(np.uint8)) and np.array_equal(gout.view(np.uint8), kout.view(np.uint8))
            assert np.array_equal(glist.view(np.uint8), klist.view(np.uint8))
    if n1 >= 300:
        assert len(glist) > 0


def test_batch_ragged_equals_single_calls(ah, torch, det):
    """seven pairs with ragged counts (0, 1, max_pts), one record without a model (hypothesis = -1) and one with a NaN in H: equal
    to the single calls slot by slot, count 0 and every query rejected for those two; enqueued on the context's stream and
    synchronised once"""
    mp = 600
    shapes = [(0, 50), (1, 1), (600, 600), (300, 0), (200, 500), (100, 100), (50, 60)]
    npairs = len(shapes)
    host = np.zeros((2 * npairs, mp), ah.POINT_DTYPE)
    num = np.zeros(2 * npairs, np.int32)
    recs = np.zeros(npairs, ah.HOMOGRAPHY_DTYPE)
    for k, (n1, n2) in enumerate(shapes):
        H = H_MILD.copy()
        H[2] += k
        q, t = build_pair(n1, n2, 200 + k, ah.POINT_DTYPE, H=H)
        host[2 * k, :n1], host[2 * k + 1, :n2] = q, t
        host[2 * k, n1:]["x"] = np.nan                                    # records past the counts are not the call's business
        num[2 * k], num[2 * k + 1] = n1, n2
        recs[k]["H"], recs[k]["hypothesis"], recs[k]["inliers"], recs[k]["n"] = H, 3 + k, 10, 20
    recs[4]["hypothesis"] = -1
    recs[5]["H"][4] = np.nan
    for cross in (1, 0):
        d_pts = upload(torch, host)
        d_num = torch.from_numpy(num).cuda()
        d_H = upload(torch, recs)
        d_out = torch.full((npairs * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((npairs,), -7, dtype=torch.int32, device="cuda")
        ah.check(ah.lib.hak_match_guided_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, d_H.data_ptr(), 3.0, 4, 5, cross, 0,
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
            sout, slist, _ = gpu_guided(ah, torch, q, t, recs[k]["H"], 3.0, (4, 5), bool(cross), 0)
            assert cnts[k] == len(slist), (k, cnts[k], len(slist))
            assert np.array_equal(lists[k, :cnts[k]].view(np.uint8), slist.view(np.uint8)), k
            assert (lists[k, cnts[k]:].view(np.uint8) == 0xEE).all()
            for f in FIELDS:
                assert np.array_equal(got[2 * k, :n1][f].view(np.uint32), sout[f].view(np.uint32)), (k, f)
            if k == 2:
                wout, wlist, _ = gr.match_guided(q, t, recs[k]["H"], 3.0, (4, 5), bool(cross), 0)
                assert_same((sout, slist, got[2 * k, :n1]), (wout, wlist), "batch vs statement")
                assert len(wlist) > 100


def test_chain_without_host_round_trip(ah, torch):
    """detect batch -> hak_match_knn2_batch -> hak_find_homography_batch -> hak_match_guided_batch on synth.pair(640, 480), all
    enqueued before ONE hak_sync: the guided result equals the statement applied to the downloaded points and H"""
    from akaze_hip import synth
    w, h = 640, 480
    p = ah.iAlignUp(w, 128)
    mp, B = 4000, 2
    imgs = list(synth.pair(w, h, 3))
    dimg = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=mp, batch=B)
    pts = torch.zeros(B * mp * 104, dtype=torch.uint8, device="cuda")
    num = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(mp * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    gout = torch.zeros(mp * 32, dtype=torch.uint8, device="cuda")
    gcnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    hom = torch.zeros(ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, dimg.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
    ah.check(ah.lib.hak_match_knn2_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1, 4, 5, 1, 0, out.data_ptr(), cnt.data_ptr()))
    ah.check(ah.lib.hak_find_homography_batch(det.ctx, out.data_ptr(), mp, cnt.data_ptr(), 1, 1024, 3.0, 0, 1, hom.data_ptr(), None))
    ah.check(ah.lib.hak_match_guided_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1, hom.data_ptr(), 8.0, 4, 5, 1, 0, gout.data_ptr(),
                                           gcnt.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    n = num.cpu().numpy()
    allp = pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(B, mp)
    rec = hom.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)[0]
    q, t = allp[0, :n[0]], allp[1, :n[1]]
    assert n[0] > 100 and n[1] > 100 and rec["hypothesis"] >= 0
    wout, wlist, _ = gr.match_guided(q, t, rec["H"], 8.0, (4, 5), True, 0)
    ng = int(gcnt.cpu().numpy()[0])
    glist = gout.cpu().numpy().view(ah.MATCH_PAIR_DTYPE)[:ng]
    assert_same((q, glist, q), (wout, wlist), "chain")
    # guided matching should recover at least the inliers RANSAC found in the 2-NN list; asserted only where the statement itself
    # says so for this pair (it is a property of the data, not of the kernel)
    if len(wlist) >= int(rec["inliers"]):
        assert ng >= int(rec["inliers"])
    det.close()


def mask_times(text):
    return re.sub(r"\d+(\.\d+)?(e[-+]?\d+)?( ms\))", "T\\3", re.sub(r"(Time[^:]*:\s*)\S+", r"\1T", text))


def test_demo_guided_leg(ah, golden, torch, tmp_path):
    """`hipakaze_demo --homography --guided 8` prints the two new lines; without --guided every line is what it was (timings aside)"""
    from test_gpu_dropin import write_pgm
    left, right = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    runs = {}
    for name, extra in (("plain", []), ("guided", ["--guided", "8"])):
        r = subprocess.run([DEMO, "0", left, right, "1", "--homography"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = r.stdout
    new = [ln for ln in runs["guided"].splitlines() if ln.startswith("Guided matches (radius 8 px") or ln.startswith("Homography of the guided matches:")]
    assert len(new) == 2, runs["guided"]
    assert "Guided" not in runs["plain"] and "guided" not in runs["plain"]
    kept = [ln for ln in runs["guided"].splitlines() if ln not in new]
    assert mask_times("\n".join(kept)) == mask_times(runs["plain"].rstrip("\n"))
    m = re.match(r"Guided matches \(radius 8 px, ratio 0.8 \+ cross-check\): (\d+) against (\d+) of the 2-NN match", new[0])
    assert m and int(m.group(1)) > 0
    m2 = re.match(r"Homography of the guided matches: (\d+) inliers of (\d+) against (\d+) of (\d+)", new[1])
    assert m2 and int(m2.group(2)) == int(m.group(1)) and int(m2.group(4)) == int(m.group(2))

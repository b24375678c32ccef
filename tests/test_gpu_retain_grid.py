"""GPU suite: the grid selection (hak_set_retain_grid, kernels_grid_select.hip).  Every case compares whole 104-byte records with the
numpy statement tests/retain_grid_ref.py applied to the unclamped list and to INTEGER positions that do not come from the code
under test: the planted lattice of the hand-made maps, the oracle's own full-resolution maps everywhere else
(retain_grid_ref.oracle_positions).  Planted maps through hak_op_tail_seed / _finish (float and FAST; cells that straddle bitmap
words and partial edge cells; a crowded cell; cells with more survivors than the kernel stages in LDS), a 640x480 scene end to end
on both paths, a mixed batch captured and replayed, the modes switched on one context, a pair call with its match, a 1080p frame
and the demo's --retain-grid flag."""
import os
import subprocess

import numpy as np
import pytest

import retain_best_ref as rb
import retain_grid_ref as rg
from conftest import ROOT, assert_points_equal
from test_gpu_dropin import read_dump, write_pgm

pytestmark = pytest.mark.gpu

ALL = ("x", "y", "octave", "response", "size", "angle", "features", "match", "distance", "match_x", "match_y")
BIG = 1 << 19                                    # room for every survivor: the oracle's unclamped list
DEMO = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from akaze_hip import synth
    return synth


def same_bytes(a, b):
    assert len(a) == len(b), (len(a), len(b))
    assert a.tobytes() == b.tobytes(), int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1).sum())


def detect(ah, det, img, w, h, p, cap, data=None):
    own = data is None
    if own:
        data = ah.AkazeData()
        ah.initAkazeData(data, cap, True, True)
    try:
        det.detectAndCompute(img.data_ptr(), data, (w, h, p), True)
        return data.h_data[:data.num_pts].copy()
    finally:
        if own:
            ah.freeAkazeData(data)


def fast_detect(ah, det, img, w, h, p, cap):
    data = ah.AkazeData()
    ah.initAkazeData(data, cap, True, True)
    try:
        det.fastDetectAndCompute(img.data_ptr(), data, (w, h, p), True)
        return data.h_data[:data.num_pts].copy()
    finally:
        ah.freeAkazeData(data)


class Ref:
    """the oracle's unclamped list of an image and the integer positions of its entries"""

    def __init__(self, okz, synth, u8, p, fast=False):
        self.w, self.fast = u8.shape[1], fast
        if fast:
            r = okz.fast_detect_and_compute(u8, max_pts=BIG, keep_arena=True)
        else:
            r = okz.detect_and_compute(synth.to_float(u8, p), self.w, okz.default_params(), max_pts=BIG, keep_arena=True)
        self.full = r.points
        self.x, self.y = rg.line_up(rg.oracle_positions(okz, r, self.w, fast=fast), self.full) if len(self.full) else (np.zeros(0), np.zeros(0))

    def idx(self, C, G):
        return rg.retained(self.x, self.y, self.full["response"], self.w, C, G, self.fast)

    def retain(self, C, G):
        return self.full[self.idx(C, G)].copy()

    def quota(self, C, G):
        return rg.quota(np.unique(rg.cells(self.x, self.y, self.w, G), return_counts=True)[1], C)


@pytest.fixture(scope="module")
def scene640(okz, synth):
    w, h = 640, 480
    u8 = synth.scene(w, h, 1, nshapes=400)
    return u8, Ref(okz, synth, u8, 640), Ref(okz, synth, u8, 640, fast=True)


@pytest.fixture(scope="module")
def golden_refs(okz, synth, golden):
    """float and FAST references of the golden left / right pair (1280 x 960)"""
    out = {}
    for name in ("left", "right"):
        u8 = golden.lr_u8[name]
        out[name] = Ref(okz, synth, u8, 1280)
        out["fast_" + name] = Ref(okz, synth, u8, 1280, fast=True)
    assert_points_equal(out["left"].full, golden.lr["pts1"])
    assert_points_equal(out["right"].full, golden.lr["pts2"])
    return out


# ------------------------------------------------------------------- planted response maps (hak_op_tail_seed / _finish)
PW, PH = 320, 240


def planted(kind, fast):
    """isolated layer-0 candidates (every one survives the NMS: its disc reaches 2 px), responses by `kind`; returns the maps and
    the planted positions in raster order"""
    resp = np.zeros((PH, PW), np.int32 if fast else np.float32)
    layer = np.full((PH, PW), -1, np.int32)
    rng = np.random.default_rng(11)
    if kind == "crowded":                                   # an 8-px lattice, and a 3-px lattice inside the 32-px cell at (96, 96)
        ys, xs = np.meshgrid(np.arange(40, PH - 40, 8), np.arange(40, PW - 40, 8), indexing="ij")
        cy, cx = np.meshgrid(np.arange(96, 128, 3), np.arange(96, 128, 3), indexing="ij")
        keep = ~((ys >= 92) & (ys < 132) & (xs >= 92) & (xs < 132))
        ys, xs = np.concatenate([ys[keep], cy.ravel()]), np.concatenate([xs[keep], cx.ravel()])
    elif kind == "dense":                                   # a 3-px lattice all over: 128-px cells hold more than 512 survivors
        ys, xs = (a.ravel() for a in np.meshgrid(np.arange(40, PH - 40, 3), np.arange(40, PW - 40, 3), indexing="ij"))
    else:
        ys, xs = (a.ravel() for a in np.meshgrid(np.arange(40, PH - 40, 8), np.arange(40, PW - 40, 8), indexing="ij"))
    order = np.argsort(ys * PW + xs)
    ys, xs = ys[order], xs[order]
    n = ys.size
    if kind == "groups":
        v = rng.choice(np.array([700, 500, 300], np.int32) if fast else np.array([0.5, 0.25, 0.125], np.float32), n)
    elif kind == "equal":
        v = np.full(n, 400 if fast else 0.3, resp.dtype)
    elif kind == "signs":                                   # negative, -0.0 and positive, with ties
        v = rng.choice(np.array([-7, -1, 3, 9], np.int32) if fast else np.array([-0.5, -0.0, -1e-20, 0.25, 2.0], np.float32), n)
    else:                                                   # crowded, dense: a few ties among mostly distinct values
        v = rng.integers(66, 66 + n // 2, n).astype(np.int32) if fast else (rng.integers(1, n // 2, n) / np.float32(n)).astype(np.float32)
    resp[ys, xs] = v
    layer[ys, xs] = 0
    return resp, layer, xs, ys


@pytest.mark.parametrize("fast", [False, True], ids=["float", "fast"])
@pytest.mark.parametrize("kind", ["groups", "equal", "signs", "crowded", "dense"])
def test_planted_maps(ah, fast, kind):
    det = ah.Akazer()
    det.init((PW, PH, ah.iAlignUp(PW, 128)), max_pts=8192)
    resp, layer, xs, ys = planted(kind, fast)
    n = len(xs)

    def run(C):
        det.tail_begin()
        det.tail_seed(resp, layer)
        return det.tail_finish(max_pts=C, refine=False, fast=fast)

    full, total = run(8192)
    assert total == n == len(full)                                            # every planted candidate is a survivor ...
    assert np.array_equal(full["x"], xs) and np.array_equal(full["y"], ys)    # ... at its planted position, in raster order
    if kind == "crowded":
        assert ((xs >= 96) & (xs < 128) & (ys >= 96) & (ys < 128)).sum() == 121
    for G in (8, 24, 32, 128):
        det.set_retain_grid(G)
        counts = np.unique(rg.cells(xs, ys, PW, G), return_counts=True)[1]
        if kind == "dense" and G == 128:
            assert counts.max() > 512                                         # (ranked out of global memory)
        occupied = len(counts)
        # clamps: 1, fewer than the occupied cells, the first (above the occupied cells) with R == 0 and with R > 0, n - 1, n
        Cs = {1, max(occupied // 2, 1), n - 1, n}
        zero = next((C for C in range(occupied, n) if rg.quota(counts, C)[1] == 0), None)
        some = next((C for C in range(occupied + 1, n) if rg.quota(counts, C)[1] > 0), None)
        assert counts.max() == 1 or (zero is not None and some is not None)   # (one survivor per cell: q = 0, R = C for every clamp)
        Cs |= {C for C in (zero, some) if C}
        for C in sorted(Cs):
            got, num = run(C)
            want = full[rg.retained(xs, ys, full["response"], PW, C, G, fast)]
            assert num == len(want) == min(C, n)
            same_bytes(got, want)
    det.set_retain_grid(0)
    same_bytes(run(n // 2)[0], full[:n // 2])                                 # off again: the raster-order prefix
    det.close()


# ------------------------------------------------------------------------------------------------ scenes end to end
def test_scene_float(ah, torch, synth, scene640):
    u8, ref, _ = scene640
    w, h, p = 640, 480, 640
    S = len(ref.full)
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p))
    for G in (16, 64):
        det.set_retain_grid(G)
        for C in (250, 900):
            assert S > C
            idx = ref.idx(C, G)
            assert not np.array_equal(idx, np.arange(C)) and not np.array_equal(idx, rb.retained(ref.full, C))
            got = detect(ah, det, img, w, h, p, C)
            assert len(got) == C
            assert_points_equal(got, ref.full[idx])
            same_bytes(got, ref.full[idx])
    same_bytes(detect(ah, det, img, w, h, p, S), ref.full)                    # S == C: everything
    det.close()


def test_scene_fast(ah, torch, synth, scene640):
    u8, _, ref = scene640
    w, h, p = 640, 480, 640
    C, G = 500, 32
    assert len(ref.full) > C
    idx = ref.idx(C, G)
    assert not np.array_equal(idx, np.arange(C)) and not np.array_equal(idx, rb.retained(ref.full, C, fast=True))
    img = torch.from_numpy(np.ascontiguousarray(u8)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), retain_grid=G)
    got = fast_detect(ah, det, img, w, h, p, C)
    assert_points_equal(got, ref.full[idx])
    same_bytes(got, ref.full[idx])
    same_bytes(fast_detect(ah, det, img, w, h, p, len(ref.full) + 5), ref.full)          # no overflow: unchanged
    det.close()


def test_mixed_batch(ah, okz, torch, synth):
    w, h, B, C, G = 480, 270, 8, 200, 32                                       # (S: 52..444, and a flat image with none)
    p = ah.iAlignUp(w, 128)
    imgs = [synth.scene(w, h, 10 + i, nshapes=(150 if i % 2 == 0 else 25)) for i in range(B - 1)] + [np.full((h, w), 77, np.uint8)]
    refs = [Ref(okz, synth, u, p) for u in imgs]
    S = [len(r.full) for r in refs]
    assert sum(s > C for s in S) >= 3 and sum(0 < s <= C for s in S) >= 3 and S[-1] == 0, S
    d = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=C, batch=B, retain_grid=G)
    out = torch.zeros(B * C * ah.POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    num = torch.zeros(B, dtype=torch.int32, device="cuda")
    for _ in range(2):                                                        # (capture, then replay)
        out.zero_()
        ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d.data_ptr(), h * p, p, B, out.data_ptr(), num.data_ptr(), 1))
        ah.check(ah.lib.hak_sync(det.ctx))
        nums = num.cpu().numpy()
        host = out.cpu().numpy().view(ah.POINT_DTYPE).reshape(B, C)
        for i in range(B):
            assert nums[i] == min(S[i], C), (i, nums[i], S[i])
            if nums[i]:
                same_bytes(host[i, :nums[i]], refs[i].retain(C, G))
    det.close()


def test_switching_modes_on_one_context(ah, torch, synth, scene640, monkeypatch):
    """off -> grid -> strongest-N -> grid (another G) -> off at one clamp on one context whose calls replay captured graphs
    (HAK_GRAPH=2): each call gets its own mode's sequence; with S <= C the mode changes nothing"""
    monkeypatch.setenv("HAK_GRAPH", "2")
    u8, ref, _ = scene640
    w, h, p = 640, 480, 640
    S, C = len(ref.full), 300
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=S + 50)
    off = detect(ah, det, img, w, h, p, S + 50)
    same_bytes(off, ref.full)
    det.set_retain_grid(16)
    same_bytes(detect(ah, det, img, w, h, p, S + 50), off)
    det.set_retain_grid(0)
    data = ah.AkazeData()                                                     # one AkazeData: only the mode differs between calls
    ah.initAkazeData(data, C, True, True)
    steps = [(0, False, ref.full[:C]), (16, False, ref.retain(C, 16)), (0, True, rb.retain(ref.full, C)), (64, True, ref.retain(C, 64)),
             (16, False, ref.retain(C, 16)), (0, False, ref.full[:C])]
    assert len({s[2].tobytes() for s in steps}) == 4                          # four different answers
    for G, best, want in steps:
        det.set_retain_best(best)
        det.set_retain_grid(G)
        for _ in range(2):                                                    # captured (or found), then replayed
            same_bytes(detect(ah, det, img, w, h, p, C, data=data), want)
    ah.freeAkazeData(data)
    det.close()


def test_refused_cell_sizes(ah):
    det = ah.Akazer()
    det.init((PW, PH, ah.iAlignUp(PW, 128)))
    for G in (7, 129, -8, 1 << 20):
        assert ah.lib.hak_set_retain_grid(det.ctx, G) != 0
        assert b"cell size" in ah.lib.hak_last_error()
    for G in (8, 128, 0):
        ah.check(ah.lib.hak_set_retain_grid(det.ctx, G))
    det.close()


def test_pair_call_matches_the_retained_sets(ah, okz, torch, synth, golden, golden_refs):
    a, b = golden.lr_u8["left"], golden.lr_u8["right"]
    h, w = a.shape
    p = ah.iAlignUp(w, 128)
    caps, G = (700, 1100), 32
    imgs = [torch.from_numpy(synth.to_float(u, p)).cuda() for u in (a, b)]
    det = ah.Akazer()
    det.init((w, h, p), batch=2, retain_grid=G)
    d = [ah.AkazeData() for _ in range(2)]
    for k in range(2):
        ah.initAkazeData(d[k], caps[k], True, True)
    r1, r2 = golden_refs["left"].retain(caps[0], G), golden_refs["right"].retain(caps[1], G)
    want = okz.match(r1.copy(), r2.copy())
    for _ in range(2):
        det.detectAndComputePair(imgs[0].data_ptr(), imgs[1].data_ptr(), d[0], d[1], (w, h, p), True, True)
        assert d[0].num_pts == len(r1) and d[1].num_pts == len(r2)
        assert_points_equal(d[0].h_data[:d[0].num_pts], want, fields=ALL)
        assert_points_equal(d[1].h_data[:d[1].num_pts], r2)
    for x in d:
        ah.freeAkazeData(x)
    det.close()


def test_1080p(ah, okz, torch, synth):
    w, h, C, G = 1920, 1080, 1000, 32                                          # (2 040 cells: several selection blocks per image)
    p = ah.iAlignUp(w, 128)
    u8 = synth.scene(w, h, 1)
    ref = Ref(okz, synth, u8, p)
    assert len(ref.full) > 1500
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=C, retain_grid=G)
    got = detect(ah, det, img, w, h, p, C)
    want = ref.retain(C, G)
    assert_points_equal(got, want)
    same_bytes(got, want)
    det.close()


def test_demo_retain_grid(ah, okz, golden, golden_refs, tmp_path):
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    env = dict(os.environ)
    for k in ("HAK_HESS_STREAM", "HAK_FUSE_SF", "HAK_BASE_STREAM"):
        env.pop(k, None)
    r = subprocess.run([DEMO, "0", left, right, "2", "--dump", dump, "--retain-best", "500", "--retain-grid", "32"], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    (f1, f2), (q1, q2) = read_dump(dump, ah)[:2]
    r1, r2 = golden_refs["left"].retain(500, 32), golden_refs["right"].retain(500, 32)
    assert_points_equal(f1, okz.match(r1.copy(), r2.copy()), fields=ALL)
    assert_points_equal(f2, r2)
    s1, s2 = golden_refs["fast_left"].retain(500, 32), golden_refs["fast_right"].retain(500, 32)
    assert_points_equal(q1, okz.match(s1.copy(), s2.copy()), fields=ALL)
    assert_points_equal(q2, s2)

"""GPU suite: the strongest-N selection (hak_set_retain_best, kernels_select.hip).  Every case compares whole 104-byte records with
the numpy statement tests/retain_best_ref.py applied to the unclamped oracle list: synthetic 1080p scenes through
hak_detect_and_compute, the mode toggled on one context (graph-cache key), a mixed batch, a pair call with unequal capacities and
the match, the FAST path, planted response maps whose threshold falls inside a group of equal responses, a 4K / 5-octave and a
7680x4320 frame, and the demo's --retain-best flag."""
import os
import subprocess

import numpy as np
import pytest

import retain_best_ref as rb
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


def detect(ah, det, img, w, h, p, cap, desc=True, data=None):
    """one hak_detect_and_compute into an AkazeData of capacity cap (the call's clamp); `data`: reuse that one (same pointers:
    the call's graph key repeats)"""
    own = data is None
    if own:
        data = ah.AkazeData()
        ah.initAkazeData(data, cap, True, True)
    try:
        det.detectAndCompute(img.data_ptr(), data, (w, h, p), desc)
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


def oracle(okz, synth, u8, p, **kw):
    return okz.detect_and_compute(synth.to_float(u8, p), u8.shape[1], okz.default_params(**kw), max_pts=BIG).points


@pytest.mark.parametrize("seed", [1, 2])
def test_1080p_keeps_the_strongest(ah, okz, torch, synth, seed):
    w, h = 1920, 1080
    p = ah.iAlignUp(w, 128)
    u8 = synth.scene(w, h, seed)
    full = oracle(okz, synth, u8, p)
    assert len(full) > 1500
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), retain_best=True)
    for C in (300, 1000):
        got = detect(ah, det, img, w, h, p, C)
        want = rb.retain(full, C)
        assert len(got) == C
        assert_points_equal(got, want)
        same_bytes(got, want)                                                 # whole records (match fields -1 included)
        assert not np.array_equal(rb.retained(full, C), np.arange(C))        # (not the raster prefix)
    det.close()


def test_no_overflow_is_unchanged_and_toggling_uses_the_right_graph(ah, okz, torch, synth, monkeypatch):
    """mode on with S <= C: byte-identical to mode off; off -> on -> off at the same clamp on one context whose calls replay
    captured graphs (HAK_GRAPH=2): each call gets its own mode's sequence"""
    monkeypatch.setenv("HAK_GRAPH", "2")
    w, h = 1280, 720
    p = ah.iAlignUp(w, 128)
    u8 = synth.scene(w, h, 3)
    full = oracle(okz, synth, u8, p)
    S = len(full)
    assert S > 600
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=S + 50)
    off = detect(ah, det, img, w, h, p, S + 50)
    det.set_retain_best(True)
    on = detect(ah, det, img, w, h, p, S + 50)
    same_bytes(off, on)
    on = detect(ah, det, img, w, h, p, S)                                     # S == C: still everything
    same_bytes(off, on)
    C = 400
    data = ah.AkazeData()                                                     # one AkazeData: only the mode differs between calls
    ah.initAkazeData(data, C, True, True)
    det.set_retain_best(False)
    same_bytes(detect(ah, det, img, w, h, p, C, data=data), full[:C])        # (captured in the raster mode)
    det.set_retain_best(True)
    for _ in range(2):                                                        # captured, then replayed
        same_bytes(detect(ah, det, img, w, h, p, C, data=data), rb.retain(full, C))
    det.set_retain_best(False)
    same_bytes(detect(ah, det, img, w, h, p, C, data=data), full[:C])        # the raster graph again, not the other one
    det.set_retain_best(True)
    same_bytes(detect(ah, det, img, w, h, p, C, data=data), rb.retain(full, C))
    ah.freeAkazeData(data)
    det.close()


def test_mixed_batch(ah, okz, torch, synth):
    w, h, B, C = 960, 540, 8, 280                                              # (S: 231..348, and a flat image with none)
    p = ah.iAlignUp(w, 128)
    imgs = [synth.scene(w, h, 10 + i, nshapes=(None if i % 2 == 0 else 60)) for i in range(B - 1)] + [np.full((h, w), 77, np.uint8)]
    fulls = [oracle(okz, synth, u, p) for u in imgs]
    S = [len(f) for f in fulls]
    assert sum(s > C for s in S) >= 3 and sum(s <= C for s in S) >= 3, S
    stack = np.stack([synth.to_float(u, p) for u in imgs])
    d = torch.from_numpy(stack).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=C, batch=B, retain_best=True)
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
                assert_points_equal(host[i, :nums[i]], rb.retain(fulls[i], C))
    det.close()


@pytest.mark.parametrize("caps", [(700, 1100), (1200, 5000)])
def test_pair_call_matches_the_retained_sets(ah, okz, torch, synth, golden, caps):
    a, b = golden.lr_u8["left"], golden.lr_u8["right"]
    h, w = a.shape
    p = ah.iAlignUp(w, 128)
    g1, g2 = golden.lr["pts1"], golden.lr["pts2"]                            # the oracle's unclamped lists (3631 / 4834)
    imgs = [torch.from_numpy(synth.to_float(u, p)).cuda() for u in (a, b)]
    det = ah.Akazer()
    det.init((w, h, p), batch=2)
    det.set_retain_best(True)
    d = [ah.AkazeData() for _ in range(2)]
    for k in range(2):
        ah.initAkazeData(d[k], caps[k], True, True)
    r1, r2 = rb.retain(g1, caps[0]), rb.retain(g2, caps[1])
    want = okz.match(r1.copy(), r2.copy())
    for _ in range(2):
        det.detectAndComputePair(imgs[0].data_ptr(), imgs[1].data_ptr(), d[0], d[1], (w, h, p), True, True)
        assert d[0].num_pts == len(r1) and d[1].num_pts == len(r2)
        assert_points_equal(d[0].h_data[:d[0].num_pts], want, fields=ALL)
        assert_points_equal(d[1].h_data[:d[1].num_pts], r2)
    for x in d:
        ah.freeAkazeData(x)
    det.close()


def test_fast_path(ah, okz, torch, synth, golden):
    for u8, C in ((golden.lr_u8["left"], 1000), (synth.scene(1920, 1080, 1), 700)):
        h, w = u8.shape
        p = ah.iAlignUp(w, 128)
        full = okz.fast_detect_and_compute(u8, max_pts=BIG).points
        assert len(full) > C
        pad = np.zeros((h, p), np.uint8)
        pad[:, :w] = u8
        img = torch.from_numpy(pad).cuda()
        det = ah.Akazer()
        det.init((w, h, p))
        det.set_retain_best(True)
        got = fast_detect(ah, det, img, w, h, p, C)
        assert_points_equal(got, rb.retain(full, C, fast=True))
        same_bytes(fast_detect(ah, det, img, w, h, p, len(full)), full)      # no overflow: unchanged
        det.close()


# ------------------------------------------------------------------- planted response maps (hak_op_tail_seed / _finish)
PW, PH = 320, 240


def planted(kind, fast):
    """isolated candidates on an 8-px grid (layer 0: every one survives the NMS), responses by `kind`"""
    resp = np.zeros((PH, PW), np.int32 if fast else np.float32)
    layer = np.full((PH, PW), -1, np.int32)
    ys, xs = np.meshgrid(np.arange(40, PH - 40, 8), np.arange(40, PW - 40, 8), indexing="ij")
    n = ys.size
    rng = np.random.default_rng(7)
    if kind == "groups":
        vals = np.array([700, 500, 300], np.int32) if fast else np.array([0.5, 0.25, 0.125], np.float32)
        v = rng.choice(vals, n)
    elif kind == "equal":
        v = np.full(n, 400 if fast else 0.3, resp.dtype)
    else:                                                                     # signs: negative, -0.0 and positive, with ties
        v = rng.choice(np.array([-7, -1, 3, 9], np.int32) if fast else np.array([-0.5, -0.0, -1e-20, 0.25, 2.0], np.float32), n)
    resp[ys, xs] = v.reshape(ys.shape)
    layer[ys, xs] = 0
    return resp, layer, n


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("kind", ["groups", "equal", "signs"])
def test_planted_ties(ah, fast, kind):
    det = ah.Akazer()
    det.init((PW, PH, ah.iAlignUp(PW, 128)), max_pts=1000)
    resp, layer, n = planted(kind, fast)

    def run(C):
        det.tail_begin()
        det.tail_seed(resp, layer)
        return det.tail_finish(max_pts=C, refine=False, fast=fast)

    full, total = run(BIG >> 8)
    assert total == n == len(full)                                            # every planted candidate is a survivor
    assert (full["y"] * PW + full["x"]).tolist() == sorted((full["y"] * PW + full["x"]).tolist())
    det.set_retain_best(True)
    vals = np.sort(np.unique(full["response"]))[::-1]
    cnt = [(full["response"] == v).sum() for v in vals]
    # thresholds inside a group of equal responses: part of the top group, the top group and part of the next, the last one
    Cs = [1, cnt[0] // 2, cnt[0] + (cnt[1] // 3 if len(cnt) > 1 else 0), n - 1, n]
    for C in Cs:
        if C < 1:
            continue
        got, num = run(C)
        want = rb.retain(full, C, fast=fast)
        assert num == len(want) == min(C, n)
        same_bytes(got, want)
    det.close()


# ------------------------------------------------------------------------------------- large frames (several blocks per image)
@pytest.mark.parametrize("w,h,kw", [(3840, 2160, dict(noctaves=5)), (7680, 4320, {})], ids=["4k_5oct", "8k"])
def test_large_frames(ah, okz, torch, synth, w, h, kw):
    C = 2000
    p = ah.iAlignUp(w, 128)
    u8 = synth.scene(w, h, 4)
    full = oracle(okz, synth, u8, p, **kw)
    assert len(full) > 2 * C
    img = torch.from_numpy(synth.to_float(u8, p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), max_pts=C, retain_best=True, **kw)
    got = detect(ah, det, img, w, h, p, C)
    want = rb.retain(full, C)
    assert_points_equal(got, want)
    same_bytes(got, want)
    assert want["y"].max() > h / 2                                            # (the bottom half is represented)
    det.close()


def test_demo_retain_best(ah, okz, golden, tmp_path):
    left, right, dump = str(tmp_path / "left.pgm"), str(tmp_path / "right.pgm"), str(tmp_path / "points.bin")
    write_pgm(left, golden.lr_u8["left"])
    write_pgm(right, golden.lr_u8["right"])
    env = dict(os.environ)
    for k in ("HAK_HESS_STREAM", "HAK_FUSE_SF", "HAK_BASE_STREAM"):
        env.pop(k, None)
    r = subprocess.run([DEMO, "0", left, right, "2", "--dump", dump, "--retain-best", "500"], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    (f1, f2), (q1, q2) = read_dump(dump, ah)[:2]
    r1, r2 = rb.retain(golden.lr["pts1"], 500), rb.retain(golden.lr["pts2"], 500)
    assert_points_equal(f1, okz.match(r1.copy(), r2.copy()), fields=ALL)
    assert_points_equal(f2, r2)
    fast = np.load(os.path.join(golden.dir, "fast_oracle.npz"))
    s1, s2 = rb.retain(fast["left_pts"], 500, fast=True), rb.retain(fast["right_pts"], 500, fast=True)
    assert_points_equal(q1, okz.match(s1.copy(), s2.copy()), fields=ALL)
    assert_points_equal(q2, s2)

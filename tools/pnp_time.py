"""pnp_time.py: cost of the track linking and of the RANSAC absolute pose (hak_link_tracks_batch, hak_solve_pnp_batch,
hak_solve_pnp) next to the RANSAC homography on lists of the same size in the same process.  Batch calls are timed with HIP events
on the context's stream around windows of WINDOW back-to-back calls (a single call is too short a window); per call = window / WINDOW;
mean / min / max over the REPS windows.

  batched: 256 three-view scenes (akaze_hip.synth.three_view_scene: 1000 points, 0.3 px noise, 10 % wrong matches per list): the
           (I0, I1) lists with their planted points link to the (I1, I2) lists (about 900 correspondences each);
           hak_solve_pnp_batch on the linked lists (1024 hypotheses, 2 px); hak_find_homography_batch without refit on the first
           `count` records of the (I1, I2) match lists (1024 hypotheses, 3 px): the same list sizes
  single:  one 900-record list: host-side latency of the synchronous hak_solve_pnp, with and without a context
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind a PnP batch on the same context"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "cuda-akaze_amd"))
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

NPAIR, STRIDE, NPTS, REPS, WINDOW, ITER = 256, 1000, 1000, 10, 20, 1024


def stats(v):
    v = np.asarray(v)
    return f"mean {v.mean():.3f} / min {v.min():.3f} / max {v.max():.3f}"


A = np.zeros(NPAIR * STRIDE, ah.MATCH_PAIR_DTYPE)
B = np.zeros(NPAIR * STRIDE, ah.MATCH_PAIR_DTYPE)
X = np.zeros((NPAIR * STRIDE, 3), np.float32)
for k in range(NPAIR):
    sc = synth.three_view_scene(1000 + k, NPTS, 0.3, 0.1)
    A[k * STRIDE:k * STRIDE + NPTS], B[k * STRIDE:k * STRIDE + NPTS], X[k * STRIDE:k * STRIDE + NPTS] = sc[3], sc[4], sc[7]
K = ah.intrinsics(sc[0])
dA, dB = (torch.from_numpy(v.view(np.uint8).copy()).cuda() for v in (A, B))
dX = torch.from_numpy(X.reshape(-1)).cuda()
counts = torch.full((NPAIR,), NPTS, dtype=torch.int32, device="cuda")
corr = torch.zeros(NPAIR * STRIDE * 32, dtype=torch.uint8, device="cuda")
ncorr = torch.zeros(NPAIR, dtype=torch.int32, device="cuda")
poses = torch.zeros(NPAIR * 64, dtype=torch.uint8, device="cuda")
homs = torch.zeros(NPAIR * 52, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")

w, h, mp, NIMG = 1920, 1080, 10000, 256
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def link_batch():
    ah.check(ah.lib.hak_link_tracks_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), 1, None, dX.data_ptr(), dB.data_ptr(), STRIDE,
                                          counts.data_ptr(), 1, NPAIR, corr.data_ptr(), STRIDE, ncorr.data_ptr()))


def pnp_batch():
    ah.check(ah.lib.hak_solve_pnp_batch(det.ctx, corr.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, K.ctypes.data, ITER, 2.0, 0,
                                        poses.data_ptr(), masks.data_ptr()))


def hom_batch():
    ah.check(ah.lib.hak_find_homography_batch(det.ctx, dB.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, ITER, 3.0, 0, 0, homs.data_ptr(),
                                              masks.data_ptr()))


def windows(fn, reps=REPS, window=WINDOW, warm=3):
    """per-call ms of `reps` windows of `window` back-to-back calls between one event pair"""
    for _ in range(warm):
        fn()
    ah.check(ah.lib.hak_sync(det.ctx))
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(window):
            fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b) / window)
    return ms


l_ms = windows(link_batch)
nc = ncorr.cpu().numpy()
print(f"lists: {NPAIR} x {NPTS} matches per side (three_view_scene, 0.3 px noise, 10 % wrong matches per list), {ITER} hypotheses; "
      f"windows of {WINDOW} calls, {REPS} windows")
print(f"hak_link_tracks_batch, {NPAIR} pairs of lists: {stats(l_ms)} ms per call (correspondences/pair mean {nc.mean():.0f}, "
      f"min {nc.min()}, max {nc.max()})")
# the two estimators' timings alternate so that a drift of the machine shows in both (the link was timed once, above)
p_ms, g_ms = [], []
for _ in range(2):
    p_ms += windows(pnp_batch, REPS // 2)
    g_ms += windows(hom_batch, REPS // 2)
ps = poses.cpu().numpy().view(ah.ABS_POSE_DTYPE)
hs = homs.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
print(f"hak_solve_pnp_batch, the linked lists, 2 px, masks written: {stats(p_ms)} ms per call (inliers/list mean {ps['inliers'].mean():.0f}, "
      f"models {int((ps['hypothesis'] >= 0).sum())}/{NPAIR}, winning solutions {np.bincount(ps['solution'], minlength=4).tolist()})")
print(f"hak_find_homography_batch, refine=0, the (I1, I2) lists at the same counts, 3 px: {stats(g_ms)} ms per call "
      f"(inliers/list mean {hs['inliers'].mean():.0f})")
print(f"  ratio of the means, PnP / homography: {np.mean(p_ms) / np.mean(g_ms):.2f}, link / PnP: {np.mean(l_ms) / np.mean(p_ms):.3f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = corr[:900 * 32].clone()
mask1 = torch.zeros(900, dtype=torch.uint8, device="cuda")
r1 = np.zeros((), ah.ABS_POSE_DTYPE)
for ctx in (det.ctx, None):
    us = []
    for k in range(55):
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_solve_pnp(ctx, one.data_ptr(), 900, K.ctypes.data, ITER, 2.0, 0, mask1.data_ptr(), r1.ctypes.data))
        if k >= 5:
            us.append((time.perf_counter() - t0) * 1e6)
    print(f"hak_solve_pnp, 900 records, {ITER} hypotheses, ctx={'yes' if ctx else 'NULL'}: {stats(us)} us per synchronous call "
          f"(inliers {int(r1['inliers'])})")

# the detect path with and without a PnP batch in front of it on the same context
u1, u2 = synth.pair(w, h, 1)
two = torch.from_numpy(np.stack([synth.to_float(u1, p), synth.to_float(u2, p)])).cuda()
imgs = two.repeat(NIMG // 2, 1, 1).contiguous()
pts = torch.zeros(NIMG * mp * 104, dtype=torch.uint8, device="cuda")
num = torch.zeros(NIMG, dtype=torch.int32, device="cuda")


def detect():
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, imgs.data_ptr(), h * p, p, NIMG, pts.data_ptr(), num.data_ptr(), 1))


def timed_detect(before):
    ms = []
    for _ in range(5):
        if before:
            pnp_batch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        detect()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


detect()
ah.check(ah.lib.hak_sync(det.ctx))
for before in (False, True, False, True):
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a PnP batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

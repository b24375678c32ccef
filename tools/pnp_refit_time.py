"""pnp_refit_time.py: cost of the Gauss-Newton refit of the absolute pose (hak_refine_pnp_batch, hak_refine_pnp) next to the RANSAC
it follows (hak_solve_pnp_batch) and next to the fundamental matrix's refit (hak_refine_fundamental_batch) on lists of the same
size in the same process.  Batch calls are timed with HIP events on the context's stream around windows of WINDOW back-to-back calls
(a single call is too short a window); per call = window / WINDOW; median / min / max over the REPS windows.  A refit rewrites its
records in place, and a refitted record costs less to refit again (its first round is often the one rejected), so every timed
refit call is preceded by a device-to-device copy that restores the RANSAC records (16 KB); the copy alone is timed as well.

  batched: 256 three-view scenes (akaze_hip.synth.three_view_scene: 1000 points, 0.3 px noise, 10 % wrong matches per list), linked
           as in tools/pnp_time.py (about 905 correspondences per list); hak_solve_pnp_batch (1024 hypotheses, 2 px);
           hak_refine_pnp_batch at rounds 1 and 3 from those records (2 px); hak_find_fundamental_batch (256 hypotheses, 1 px) and
           hak_refine_fundamental_batch at rounds 1 and 3 on the first `count` records of the (I1, I2) match lists: the same sizes
  single:  one 900-record list: host-side latency of the synchronous hak_refine_pnp (3 rounds), with and without a context
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind a refit batch on the same context"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "cuda-akaze_amd"))
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

NPAIR, STRIDE, NPTS, REPS, WINDOW, ITER, FITER = 256, 1000, 1000, 10, 20, 1024, 256


def stats(v):
    v = np.asarray(v)
    return f"median {np.median(v):.3f} / min {v.min():.3f} / max {v.max():.3f}"


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
funds = torch.zeros(NPAIR * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")

w, h, mp, NIMG = 1920, 1080, 10000, 256
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def pnp_batch():
    ah.check(ah.lib.hak_solve_pnp_batch(det.ctx, corr.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, K.ctypes.data, ITER, 2.0, 0,
                                        poses.data_ptr(), masks.data_ptr()))


def restore(dst, src):
    with torch.cuda.stream(stream):
        dst.copy_(src, non_blocking=True)


def pnp_refit(rounds):
    restore(poses, poses0)
    ah.check(ah.lib.hak_refine_pnp_batch(det.ctx, corr.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, K.ctypes.data, 2.0, rounds,
                                         poses.data_ptr(), masks.data_ptr()))


def fund_refit(rounds):
    restore(funds, funds0)
    ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, dB.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, 1.0, rounds, funds.data_ptr(),
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


ah.check(ah.lib.hak_link_tracks_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), 1, None, dX.data_ptr(), dB.data_ptr(), STRIDE,
                                      counts.data_ptr(), 1, NPAIR, corr.data_ptr(), STRIDE, ncorr.data_ptr()))
pnp_batch()
ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, dB.data_ptr(), STRIDE, ncorr.data_ptr(), NPAIR, FITER, 1.0, 0, funds.data_ptr(), None))
ah.check(ah.lib.hak_sync(det.ctx))
poses0, funds0 = poses.clone(), funds.clone()
nc = ncorr.cpu().numpy()
ps0 = poses0.cpu().numpy().view(ah.ABS_POSE_DTYPE).copy()
fs0 = funds0.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE).copy()
print(f"lists: {NPAIR} x about {nc.mean():.0f} records (three_view_scene, {NPTS} points, 0.3 px noise, 10 % wrong matches per list; min "
      f"{nc.min()}, max {nc.max()}); windows of {WINDOW} calls, {REPS} windows; ms per call")
# the timings alternate so that a drift of the machine shows in all of them
t = {"pnp": [], "copy": [], "p1": [], "p3": [], "f1": [], "f3": []}
for _ in range(2):
    t["pnp"] += windows(pnp_batch, REPS // 2)
    t["copy"] += windows(lambda: restore(poses, poses0), REPS // 2)
    t["p1"] += windows(lambda: pnp_refit(1), REPS // 2)
    t["f1"] += windows(lambda: fund_refit(1), REPS // 2)
    t["p3"] += windows(lambda: pnp_refit(3), REPS // 2)
    t["f3"] += windows(lambda: fund_refit(3), REPS // 2)
ps3 = poses.cpu().numpy().view(ah.ABS_POSE_DTYPE).copy()               # (the last refit calls ran 3 rounds)
fs3 = funds.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE).copy()
print(f"hak_solve_pnp_batch, {ITER} hypotheses, 2 px, masks written: {stats(t['pnp'])} (inliers/list mean {ps0['inliers'].mean():.1f}, "
      f"models {int((ps0['hypothesis'] >= 0).sum())}/{NPAIR})")
print(f"the 16 KB record copy in front of every refit call below: {stats(t['copy'])}")
print(f"hak_refine_pnp_batch, rounds 1, 2 px, masks written: {stats(t['p1'])}")
print(f"hak_refine_pnp_batch, rounds 3, 2 px, masks written: {stats(t['p3'])} (inliers/list mean {ps0['inliers'].mean():.2f} -> "
      f"{ps3['inliers'].mean():.2f}, lists that gained {int((ps3['inliers'] > ps0['inliers']).sum())}, "
      f"refitted {int((ps3['solution'] == 4).sum())}/{NPAIR}, never fewer: {bool((ps3['inliers'] >= ps0['inliers']).all())})")
print(f"hak_refine_fundamental_batch, rounds 1, 1 px, the (I1, I2) lists at the same counts: {stats(t['f1'])}")
print(f"hak_refine_fundamental_batch, rounds 3: {stats(t['f3'])} (inliers/list mean {fs0['inliers'].mean():.1f} -> {fs3['inliers'].mean():.1f}, "
      f"refitted {int((fs3['root'] == 3).sum())}/{NPAIR})")
m = {k: float(np.median(v)) for k, v in t.items()}
print(f"  ratios of the medians less the copy: pose refit (3 rounds) / PnP RANSAC {(m['p3'] - m['copy']) / m['pnp']:.3f}; pose refit / "
      f"fundamental refit at 1 round {(m['p1'] - m['copy']) / (m['f1'] - m['copy']):.3f}, at 3 rounds "
      f"{(m['p3'] - m['copy']) / (m['f3'] - m['copy']):.3f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = corr[:900 * 32].clone()
mask1 = torch.zeros(900, dtype=torch.uint8, device="cuda")
for ctx in (det.ctx, None):
    us = []
    for k in range(55):
        r1 = np.array(ps0[0], ah.ABS_POSE_DTYPE).reshape(())
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_refine_pnp(ctx, one.data_ptr(), 900, K.ctypes.data, 2.0, 3, mask1.data_ptr(), r1.ctypes.data))
        if k >= 5:
            us.append((time.perf_counter() - t0) * 1e6)
    print(f"hak_refine_pnp, 900 records, 3 rounds, ctx={'yes' if ctx else 'NULL'}: {stats(us)} us per synchronous call "
          f"(inliers of the result {int(r1['inliers'])})")

# the detect path with and without a refit batch in front of it on the same context
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
            pnp_refit(3)
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
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a pose refit batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

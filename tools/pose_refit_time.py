"""pose_refit_time.py: cost of the calibrated Gauss-Newton refit of the relative pose (hak_refine_pose_batch, hak_refine_pose) next
to the decomposition it follows (hak_recover_pose_batch) and next to the absolute pose's refit (hak_refine_pnp_batch) on lists of
the same size in the same process.  Batch calls are timed with HIP events on the context's stream around windows of WINDOW
back-to-back calls (a single call is too short a window); per call = window / WINDOW; median / min / max over the REPS windows.  A
refit rewrites its records in place, and a refitted record costs less to refit again, so every timed refit call is preceded by a
device-to-device copy that restores the input records (16 KB); the copy alone is timed as well.

  batched: 256 two-view scenes (akaze_hip.synth.two_view_scene: 938 planted matches with 0.5 px noise and 402 wrong ones per list,
           1 340 records); hak_find_fundamental_batch (256 hypotheses, 1 px) -> hak_refine_fundamental_batch (3 rounds) ->
           hak_recover_pose_batch (1 px, depth < 50), timed; hak_refine_pose_batch at rounds 1 and 3 from those records (2 px, depth
           < 50, mask and points written); hak_refine_pnp_batch at rounds 1 and 3 (2 px) on 1 340 correspondences per list made of
           the pose's points and the matches' second-image coordinates, from the pose's (R, t)
  single:  one 1 470-record list: host-side latency of the synchronous hak_refine_pose (3 rounds), with and without a context
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

NPAIR, STRIDE, N_IN, N_OUT, REPS, WINDOW, FITER = 256, 1340, 938, 402, 10, 20, 256
THR, MD = 2.0, 50.0


def stats(v):
    v = np.asarray(v)
    return f"median {np.median(v):.3f} / min {v.min():.3f} / max {v.max():.3f}"


def pairs_of(recs):
    m = np.zeros(len(recs), ah.MATCH_PAIR_DTYPE)
    m["query"] = m["train"] = np.arange(len(recs))
    for k, f in enumerate(("x1", "y1", "x2", "y2")):
        m[f] = recs[:, k]
    return m


A = np.zeros(NPAIR * STRIDE, ah.MATCH_PAIR_DTYPE)
for k in range(NPAIR):
    sc = synth.two_view_scene(N_IN, N_OUT, 1000 + k, noise=0.5)
    A[k * STRIDE:(k + 1) * STRIDE] = pairs_of(sc[0])
K = ah.intrinsics(sc[3])
kp = K.ctypes.data
dA = torch.from_numpy(A.view(np.uint8).copy()).cuda()
counts = torch.full((NPAIR,), STRIDE, dtype=torch.int32, device="cuda")
funds = torch.zeros(NPAIR * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
poses = torch.zeros(NPAIR * 64, dtype=torch.uint8, device="cuda")
absp = torch.zeros(NPAIR * 64, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")
xyz = torch.zeros(NPAIR * STRIDE * 3, dtype=torch.float32, device="cuda")
amasks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")

w, h, mp, NIMG = 1920, 1080, 10000, 256
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def recover():
    ah.check(ah.lib.hak_recover_pose_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, funds.data_ptr(), kp, kp, 1.0, MD,
                                           poses.data_ptr(), masks.data_ptr(), xyz.data_ptr()))


def restore(dst, src):
    with torch.cuda.stream(stream):
        dst.copy_(src, non_blocking=True)


def pose_refit(rounds):
    restore(poses, poses0)
    ah.check(ah.lib.hak_refine_pose_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, kp, kp, THR, MD, rounds,
                                          poses.data_ptr(), masks.data_ptr(), xyz.data_ptr()))


def pnp_refit(rounds):
    restore(absp, absp0)
    ah.check(ah.lib.hak_refine_pnp_batch(det.ctx, corr.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, kp, THR, rounds, absp.data_ptr(),
                                         amasks.data_ptr()))


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


ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, FITER, 1.0, 0, funds.data_ptr(), None))
ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, dA.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1.0, 3, funds.data_ptr(), None))
recover()
ah.check(ah.lib.hak_sync(det.ctx))
poses0 = poses.clone()
ps0 = poses0.cpu().numpy().view(ah.POSE_DTYPE).copy()
# the correspondences of the PnP refit: the pose's points as seen in the second image, and the pose itself as an absolute pose
C = np.zeros(NPAIR * STRIDE, ah.CORR3D_DTYPE)
pts = xyz.cpu().numpy().reshape(-1, 3)
C["X"], C["Y"], C["Z"], C["u"], C["v"] = pts[:, 0], pts[:, 1], pts[:, 2], A["x2"], A["y2"]
corr = torch.from_numpy(C.view(np.uint8).copy()).cuda()
a0 = np.zeros(NPAIR, ah.ABS_POSE_DTYPE)
a0["R"], a0["t"], a0["n"] = ps0["R"], ps0["t"], STRIDE
a0["hypothesis"] = np.where(ps0["candidate"] >= 0, 0, -1)
absp0 = torch.from_numpy(a0.view(np.uint8).copy()).cuda()
print(f"lists: {NPAIR} x {STRIDE} records (two_view_scene, {N_IN} planted at 0.5 px noise, {N_OUT} wrong); windows of {WINDOW} calls, "
      f"{REPS} windows; ms per call")
# the timings alternate so that a drift of the machine shows in all of them
t = {"pose": [], "copy": [], "r1": [], "r3": [], "p1": [], "p3": []}
for _ in range(2):
    t["pose"] += windows(recover, REPS // 2)
    t["copy"] += windows(lambda: restore(poses, poses0), REPS // 2)
    t["r1"] += windows(lambda: pose_refit(1), REPS // 2)
    t["p1"] += windows(lambda: pnp_refit(1), REPS // 2)
    t["r3"] += windows(lambda: pose_refit(3), REPS // 2)
    t["p3"] += windows(lambda: pnp_refit(3), REPS // 2)
ps3 = poses.cpu().numpy().view(ah.POSE_DTYPE).copy()                    # (the last refit calls ran 3 rounds)
as3 = absp.cpu().numpy().view(ah.ABS_POSE_DTYPE).copy()
print(f"hak_recover_pose_batch, 1 px, depth < {MD:g}, mask and points written: {stats(t['pose'])} (in front/list mean "
      f"{ps0['in_front'].mean():.1f}, poses {int((ps0['candidate'] >= 0).sum())}/{NPAIR})")
print(f"the 16 KB record copy in front of every refit call below: {stats(t['copy'])}")
print(f"hak_refine_pose_batch, rounds 1, {THR:g} px, mask and points written: {stats(t['r1'])}")
print(f"hak_refine_pose_batch, rounds 3, {THR:g} px, mask and points written: {stats(t['r3'])} (in front/list mean "
      f"{ps0['in_front'].mean():.1f} at 1 px -> {ps3['in_front'].mean():.1f} at {THR:g} px, refitted "
      f"{int((ps3['candidate'] == 4).sum())}/{NPAIR})")
print(f"hak_refine_pnp_batch, rounds 1, {THR:g} px, masks written, lists of the same size: {stats(t['p1'])}")
print(f"hak_refine_pnp_batch, rounds 3: {stats(t['p3'])} (inliers/list mean {as3['inliers'].mean():.1f}, refitted "
      f"{int((as3['solution'] == 4).sum())}/{NPAIR})")
m = {k: float(np.median(v)) for k, v in t.items()}
print(f"  ratios of the medians less the copy: pose refit / pose recovery at 1 round {(m['r1'] - m['copy']) / m['pose']:.3f}, at 3 rounds "
      f"{(m['r3'] - m['copy']) / m['pose']:.3f}; pose refit / PnP refit at 1 round {(m['r1'] - m['copy']) / (m['p1'] - m['copy']):.3f}, "
      f"at 3 rounds {(m['r3'] - m['copy']) / (m['p3'] - m['copy']):.3f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
sc1 = synth.two_view_scene(1029, 441, 7, noise=0.5)
one = torch.from_numpy(pairs_of(sc1[0]).view(np.uint8).copy()).cuda()
N1 = 1470
rec1 = ah.recoverPose(one, ah.refineFundamental(one, ah.findFundamental(one, FITER, 1.0, 7)[0], 1.0, 3)[0], K, None, 1.0, MD)[0]
mask1 = torch.zeros(N1, dtype=torch.uint8, device="cuda")
xyz1 = torch.zeros(3 * N1, dtype=torch.float32, device="cuda")
for ctx in (det.ctx, None):
    us = []
    for k in range(55):
        r1 = np.array(rec1, ah.POSE_DTYPE).reshape(())
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_refine_pose(ctx, one.data_ptr(), N1, kp, kp, THR, MD, 3, mask1.data_ptr(), xyz1.data_ptr(), r1.ctypes.data))
        if k >= 5:
            us.append((time.perf_counter() - t0) * 1e6)
    print(f"hak_refine_pose, {N1} records, 3 rounds, ctx={'yes' if ctx else 'NULL'}: {stats(us)} us per synchronous call "
          f"(in front {int(rec1['in_front'])} -> {int(r1['in_front'])})")

# the detect path with and without a refit batch in front of it on the same context
u1, u2 = synth.pair(w, h, 1)
two = torch.from_numpy(np.stack([synth.to_float(u1, p), synth.to_float(u2, p)])).cuda()
imgs = two.repeat(NIMG // 2, 1, 1).contiguous()
dpts = torch.zeros(NIMG * mp * 104, dtype=torch.uint8, device="cuda")
num = torch.zeros(NIMG, dtype=torch.int32, device="cuda")


def detect():
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, imgs.data_ptr(), h * p, p, NIMG, dpts.data_ptr(), num.data_ptr(), 1))


def timed_detect(before):
    ms = []
    for _ in range(5):
        if before:
            pose_refit(3)
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

"""pose_time.py: cost of the pose recovery (hak_recover_pose_batch / hak_recover_pose) next to the RANSAC and the refit that feed
it, on the same lists in the same process, timed with HIP events on the context's stream; min / median / max over the repetitions.

  batched: the 256 lists of fundamental_refit_time.py (akaze_hip.synth.two_view_matches: 940 planted + 400 random records, 0.3 px
           noise): hak_find_fundamental_batch (1024 hypotheses, 1 px), hak_refine_fundamental_batch (rounds = 1) on its records,
           hak_recover_pose_batch on the refitted records (1 px, no depth limit; mask and points written)
  single:  one list of 1 470 records: host-side latency of the synchronous refit (rounds = 3) and of the pose call behind it
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind a pose batch on the same context"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "cuda-akaze_amd"))
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

NPAIR, STRIDE, N_IN, N_OUT, REPS = 256, 1500, 940, 400, 30
K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))                       # two_view_matches' camera
INF = float("inf")


def to_pairs(recs):
    m = np.zeros(len(recs), ah.MATCH_PAIR_DTYPE)
    for j, f in enumerate(("x1", "y1", "x2", "y2")):
        m[f] = recs[:, j]
    return m


def stats(v):
    v = np.sort(np.asarray(v))
    return f"min {v[0]:.3f} / median {np.median(v):.3f} / max {v[-1]:.3f}"


allp = np.zeros(NPAIR * STRIDE, ah.MATCH_PAIR_DTYPE)
for k in range(NPAIR):
    allp[k * STRIDE:k * STRIDE + N_IN + N_OUT] = to_pairs(synth.two_view_matches(N_IN, N_OUT, 1000 + k, noise=0.3)[0])
lists = torch.from_numpy(allp.view(np.uint8).copy()).cuda()
counts = torch.full((NPAIR,), N_IN + N_OUT, dtype=torch.int32, device="cuda")
out = torch.zeros(NPAIR * 52, dtype=torch.uint8, device="cuda")
poses = torch.zeros(NPAIR * 64, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")
xyz = torch.zeros(NPAIR * STRIDE * 3, dtype=torch.float32, device="cuda")

w, h, mp, NIMG = 1920, 1080, 10000, 256
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def fund_batch():
    ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1024, 1.0, 0,
                                               out.data_ptr(), masks.data_ptr()))


def refine_batch():
    """a refit batch on a fresh copy of the RANSAC records (the call rewrites them in place); the copy is inside the timing"""
    work.copy_(ransac, non_blocking=True)
    ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1.0, 1, work.data_ptr(),
                                                 masks.data_ptr()))


def pose_batch():
    ah.check(ah.lib.hak_recover_pose_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, work.data_ptr(), K.ctypes.data,
                                           K.ctypes.data, 1.0, INF, poses.data_ptr(), masks.data_ptr(), xyz.data_ptr()))


def events(fn, reps, warm=3):
    """one event pair per call: the list of per-call times in ms"""
    for _ in range(warm):
        fn()
    ah.check(ah.lib.hak_sync(det.ctx))
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


print(f"lists: {NPAIR} x {N_IN + N_OUT} records (two_view_matches, {N_IN} planted with 0.3 px noise + {N_OUT} random), 1024 hypotheses")
f_ms = events(fund_batch, REPS)
rec = out.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
print(f"hak_find_fundamental_batch, {NPAIR} pairs, 1 px: {stats(f_ms)} ms per call (inliers/pair mean {rec['inliers'].mean():.0f}, "
      f"models {int((rec['hypothesis'] >= 0).sum())}/{NPAIR})")
ransac, work = out.clone(), out.clone()
with torch.cuda.stream(stream):
    r_ms = events(refine_batch, REPS)
    ref = work.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
    print(f"hak_refine_fundamental_batch, same lists and records, rounds=1: {stats(r_ms)} ms per call (inliers/pair mean "
          f"{ref['inliers'].mean():.0f}; includes the 13 KB record copy)")
    p_ms = events(pose_batch, REPS)
    ps = poses.cpu().numpy().view(ah.POSE_DTYPE)
    print(f"hak_recover_pose_batch, same lists, the refitted records, mask and points written: {stats(p_ms)} ms per call "
          f"(in front/pair mean {ps['in_front'].mean():.0f} of {ps['inliers'].mean():.0f} inliers, poses "
          f"{int((ps['candidate'] >= 0).sum())}/{NPAIR}, winners {np.bincount(ps['candidate'][ps['candidate'] >= 0], minlength=4).tolist()})")
    print(f"  ratio of the medians, pose / refit: {np.median(p_ms) / np.median(r_ms):.2f}, pose / RANSAC: "
          f"{np.median(p_ms) / np.median(f_ms):.2f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = torch.from_numpy(to_pairs(synth.two_view_matches(1030, 440, 7, noise=0.3)[0]).view(np.uint8).copy()).cuda()
mask1 = torch.zeros(1470, dtype=torch.uint8, device="cuda")
xyz1 = torch.zeros(3 * 1470, dtype=torch.float32, device="cuda")
r0, p1 = np.zeros((), ah.FUNDAMENTAL_DTYPE), np.zeros((), ah.POSE_DTYPE)
ah.check(ah.lib.hak_find_fundamental(det.ctx, one.data_ptr(), 1470, 1024, 1.0, 0, mask1.data_ptr(), r0.ctypes.data))
for ctx in (det.ctx, None):
    us_r, us_p = [], []
    for k in range(55):
        r1 = r0.copy()
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_refine_fundamental(ctx, one.data_ptr(), 1470, 1.0, 3, mask1.data_ptr(), r1.ctypes.data))
        t1 = time.perf_counter()
        ah.check(ah.lib.hak_recover_pose(ctx, one.data_ptr(), 1470, r1["F"].ctypes.data_as(ah._fp), K.ctypes.data, K.ctypes.data, 1.0,
                                         INF, mask1.data_ptr(), xyz1.data_ptr(), p1.ctypes.data))
        if k >= 5:
            us_r.append((t1 - t0) * 1e6)
            us_p.append((time.perf_counter() - t1) * 1e6)
    print(f"hak_refine_fundamental, 1470 records, rounds=3, ctx={'yes' if ctx else 'NULL'}: {stats(us_r)} us per synchronous call "
          f"(inliers {int(r1['inliers'])})")
    print(f"hak_recover_pose, same list, ctx={'yes' if ctx else 'NULL'}: {stats(us_p)} us per synchronous call "
          f"(in front {int(p1['in_front'])} of {int(p1['inliers'])})")

# the detect path with and without a pose batch in front of it on the same context
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
            pose_batch()
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
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a pose batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

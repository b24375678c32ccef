"""triangulate_time.py: cost of the triangulation under two known views (hak_triangulate_batch / hak_triangulate) next to the pose
recovery (hak_recover_pose_batch / hak_recover_pose) on the same lists in the same process, timed with HIP events on the context's
stream; min / median / max over the repetitions.

  batched: the 256 lists of pose_time.py (akaze_hip.synth.two_view_matches: 940 planted + 400 random records, 0.3 px noise):
           hak_find_fundamental_batch (1024 hypotheses, 1 px) and hak_refine_fundamental_batch (rounds = 1) feed
           hak_recover_pose_batch (1 px, no depth limit; mask and points written); hak_triangulate_batch then re-triangulates
           every list under the identity and the pair's own hak_pose, read on the device (2 px, no depth limit, min_sin 0; mask
           and points written)
  single:  one list of 1 470 records: host-side latency of the synchronous pose call and of the synchronous triangulation under
           the pose it returned
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind a triangulation batch on the same context"""
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
fund = torch.zeros(NPAIR * 52, dtype=torch.uint8, device="cuda")
poses = torch.zeros(NPAIR * 64, dtype=torch.uint8, device="cuda")
tris = torch.zeros(NPAIR * 32, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")
xyz = torch.zeros(NPAIR * STRIDE * 3, dtype=torch.float32, device="cuda")
tmasks, txyz = torch.zeros_like(masks), torch.zeros_like(xyz)

w, h, mp, NIMG = 1920, 1080, 10000, 256
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def pose_batch():
    ah.check(ah.lib.hak_recover_pose_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, fund.data_ptr(), K.ctypes.data,
                                           K.ctypes.data, 1.0, INF, poses.data_ptr(), masks.data_ptr(), xyz.data_ptr()))


def tri_batch():
    ah.check(ah.lib.hak_triangulate_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), 1, NPAIR, None, ah.VIEW_IDENTITY, 0,
                                          poses.data_ptr(), ah.VIEW_RELATIVE, 1, K.ctypes.data, K.ctypes.data, 2.0, INF, 0.0,
                                          tris.data_ptr(), tmasks.data_ptr(), txyz.data_ptr()))


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


def burst(fn, calls=200):
    """`calls` calls back to back inside one event pair: ms per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(calls):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / calls


print(f"lists: {NPAIR} x {N_IN + N_OUT} records (two_view_matches, {N_IN} planted with 0.3 px noise + {N_OUT} random)")
ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1024, 1.0, 0, fund.data_ptr(), None))
ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1.0, 1, fund.data_ptr(), None))
with torch.cuda.stream(stream):
    p_ms = events(pose_batch, REPS)
    ps = poses.cpu().numpy().view(ah.POSE_DTYPE)
    print(f"hak_recover_pose_batch, {NPAIR} lists, refitted F, 1 px, mask and points written: {stats(p_ms)} ms per call "
          f"(in front/pair mean {ps['in_front'].mean():.0f} of {ps['inliers'].mean():.0f} inliers, poses "
          f"{int((ps['candidate'] >= 0).sum())}/{NPAIR})")
    t_ms = events(tri_batch, REPS)
    ts = tris.cpu().numpy().view(ah.TRIANGULATION_DTYPE)
    print(f"hak_triangulate_batch, same lists, identity and the pair's hak_pose, 2 px, mask and points written: {stats(t_ms)} ms per "
          f"call (kept/list mean {ts['kept'].mean():.0f}, rejected by parallax / depth / reprojection mean "
          f"{ts['rejected'][:, 0].mean():.0f} / {ts['rejected'][:, 1].mean():.0f} / {ts['rejected'][:, 2].mean():.0f}, models "
          f"{int(ts['model'].sum())}/{NPAIR})")
    print(f"  ratio of the medians, triangulation / pose: {np.median(t_ms) / np.median(p_ms):.2f}")
    # the two again in the other order, so that neither figure owes anything to what ran before it
    t2_ms, p2_ms = events(tri_batch, REPS), events(pose_batch, REPS)
    print(f"  again, triangulation first: triangulation {stats(t2_ms)} ms, pose {stats(p2_ms)} ms per call")
    # a call is one launch of tens of microseconds, near what an event pair resolves: 200 calls back to back inside one pair
    b_t, b_p = [burst(tri_batch) for _ in range(5)], [burst(pose_batch) for _ in range(5)]
    print(f"  200 calls per event pair, five times: triangulation {stats(b_t)} ms, pose {stats(b_p)} ms per call")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = torch.from_numpy(to_pairs(synth.two_view_matches(1030, 440, 7, noise=0.3)[0]).view(np.uint8).copy()).cuda()
mask1 = torch.zeros(1470, dtype=torch.uint8, device="cuda")
xyz1 = torch.zeros(3 * 1470, dtype=torch.float32, device="cuda")
r0, p1, t1r = np.zeros((), ah.FUNDAMENTAL_DTYPE), np.zeros((), ah.POSE_DTYPE), np.zeros((), ah.TRIANGULATION_DTYPE)
ah.check(ah.lib.hak_find_fundamental(det.ctx, one.data_ptr(), 1470, 1024, 1.0, 0, mask1.data_ptr(), r0.ctypes.data))
ah.check(ah.lib.hak_refine_fundamental(det.ctx, one.data_ptr(), 1470, 1.0, 3, mask1.data_ptr(), r0.ctypes.data))
for ctx in (det.ctx, None):
    us_p, us_t = [], []
    for k in range(55):
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_recover_pose(ctx, one.data_ptr(), 1470, r0["F"].ctypes.data_as(ah._fp), K.ctypes.data, K.ctypes.data, 1.0,
                                         INF, mask1.data_ptr(), xyz1.data_ptr(), p1.ctypes.data))
        view = np.concatenate([p1["R"], p1["t"]]).astype(np.float32)
        t1 = time.perf_counter()
        ah.check(ah.lib.hak_triangulate(ctx, one.data_ptr(), 1470, None, view.ctypes.data_as(ah._fp), K.ctypes.data, K.ctypes.data, 2.0,
                                        INF, 0.0, mask1.data_ptr(), xyz1.data_ptr(), t1r.ctypes.data))
        if k >= 5:
            us_p.append((t1 - t0) * 1e6)
            us_t.append((time.perf_counter() - t1) * 1e6)
    print(f"hak_recover_pose, 1470 records, ctx={'yes' if ctx else 'NULL'}: {stats(us_p)} us per synchronous call "
          f"(in front {int(p1['in_front'])} of {int(p1['inliers'])})")
    print(f"hak_triangulate, same list, under that pose, ctx={'yes' if ctx else 'NULL'}: {stats(us_t)} us per synchronous call "
          f"(kept {int(t1r['kept'])}, rejected {t1r['rejected'].tolist()})")

# the detect path with and without a triangulation batch in front of it on the same context
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
            tri_batch()
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
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a triangulation batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

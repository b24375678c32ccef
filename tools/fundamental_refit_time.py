"""fundamental_refit_time.py: cost of the rank-2 refit of the fundamental matrix (hak_refine_fundamental_batch /
hak_refine_fundamental) next to the RANSAC call that feeds it, on the same lists in the same process, timed with HIP events on the
context's stream; min / median / max over the repetitions.

  batched: 256 lists of synth size (akaze_hip.synth.two_view_matches: 940 planted + 400 random records, 0.3 px noise),
           hak_find_fundamental_batch (1024 hypotheses, 1 px), then hak_refine_fundamental_batch on its records, rounds = 1 and 3
  single:  one list of 1 470 records: host-side latency of the synchronous RANSAC call and of the refit behind it (rounds = 3)
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

NPAIR, STRIDE, N_IN, N_OUT, REPS = 256, 1500, 940, 400, 30


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
masks = torch.zeros(NPAIR * STRIDE, dtype=torch.uint8, device="cuda")

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


def refine_batch(rounds):
    """a refit batch on a fresh copy of the RANSAC records (the call rewrites them in place); the copy is inside the timing"""
    def run():
        work.copy_(ransac, non_blocking=True)
        ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1.0, rounds,
                                                     work.data_ptr(), masks.data_ptr()))
    return run


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
    for rounds in (1, 3):
        r_ms = events(refine_batch(rounds), REPS)
        ref = work.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
        print(f"hak_refine_fundamental_batch, same lists and records, rounds={rounds}: {stats(r_ms)} ms per call (inliers/pair mean "
              f"{ref['inliers'].mean():.0f}, refitted {int((ref['root'] == 3).sum())}/{NPAIR}; includes the 13 KB record copy)")
        print(f"  ratio of the medians, refit / RANSAC: {np.median(r_ms) / np.median(f_ms):.2f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = torch.from_numpy(to_pairs(synth.two_view_matches(1030, 440, 7, noise=0.3)[0]).view(np.uint8).copy()).cuda()
mask1 = torch.zeros(1470, dtype=torch.uint8, device="cuda")
r0 = np.zeros((), ah.FUNDAMENTAL_DTYPE)
for ctx in (det.ctx, None):
    us, us_f = [], []
    for k in range(55):
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_find_fundamental(ctx, one.data_ptr(), 1470, 1024, 1.0, 0, mask1.data_ptr(), r0.ctypes.data))
        t1 = time.perf_counter()
        r1 = r0.copy()
        ah.check(ah.lib.hak_refine_fundamental(ctx, one.data_ptr(), 1470, 1.0, 3, mask1.data_ptr(), r1.ctypes.data))
        if k >= 5:
            us_f.append((t1 - t0) * 1e6)
            us.append((time.perf_counter() - t1) * 1e6)
    print(f"hak_find_fundamental, 1470 records, ctx={'yes' if ctx else 'NULL'}: {stats(us_f)} us per synchronous call "
          f"(inliers {int(r0['inliers'])})")
    print(f"hak_refine_fundamental, same list, rounds=3, ctx={'yes' if ctx else 'NULL'}: {stats(us)} us per synchronous call "
          f"(inliers {int(r1['inliers'])})")

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
            with torch.cuda.stream(stream):
                refine_batch(3)()
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
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a refit batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

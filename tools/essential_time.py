"""essential_time.py: cost of the five-point RANSAC essential matrix (hak_find_essential_batch / hak_find_essential) next to the
seven-point fundamental matrix on the same lists in the same process, timed with HIP events on the context's stream; min / median /
max over the repetitions.

  batched: 256 lists of synth size (akaze_hip.synth.two_view_matches: 940 planted + 400 random records, 0.3 px noise):
           hak_find_essential_batch at 256, 512 and 1024 hypotheses and hak_find_fundamental_batch at 1024, all at 1 px
  single:  one list of 1 470 records, 1024 hypotheses: host-side latency of the synchronous call, with and without a context
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind an essential batch on the same context
  --kernels: only 20 essential batch calls at 1024 hypotheses, for one `rocprofv3 --kernel-trace --stats -- python
           tools/essential_time.py --kernels` run that splits the call into k_ess_models, k_ess_score and k_ess_finish"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "cuda-akaze_amd"), os.path.join(HERE, "..", "tests")]
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

NPAIR, STRIDE, N_IN, N_OUT, REPS = 256, 1500, 940, 400, 30
K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))                       # two_view_matches' camera


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

kernels_only = "--kernels" in sys.argv
w, h, mp, NIMG = 1920, 1080, 10000, (2 if kernels_only else 256)
p = ah.iAlignUp(w, 128)
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def ess_batch(iterations=1024):
    ah.check(ah.lib.hak_find_essential_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, K.ctypes.data, K.ctypes.data,
                                             iterations, 1.0, 0, out.data_ptr(), masks.data_ptr()))


def fund_batch():
    ah.check(ah.lib.hak_find_fundamental_batch(det.ctx, lists.data_ptr(), STRIDE, counts.data_ptr(), NPAIR, 1024, 1.0, 0,
                                               out.data_ptr(), masks.data_ptr()))


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


if kernels_only:
    for _ in range(20):
        ess_batch()
    ah.check(ah.lib.hak_sync(det.ctx))
    det.close()
    sys.exit(0)

print(f"lists: {NPAIR} x {N_IN + N_OUT} records (two_view_matches, {N_IN} planted with 0.3 px noise + {N_OUT} random), 1 px")
e_ms = {}
for it in (256, 512, 1024):
    e_ms[it] = events(lambda: ess_batch(it), REPS)
    rec = out.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
    print(f"hak_find_essential_batch, {NPAIR} pairs, {it} hypotheses: {stats(e_ms[it])} ms per call (inliers/pair mean "
          f"{rec['inliers'].mean():.0f}, models {int((rec['hypothesis'] >= 0).sum())}/{NPAIR})")
f_ms = events(fund_batch, REPS)
rec = out.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
print(f"hak_find_fundamental_batch, same lists, 1024 hypotheses: {stats(f_ms)} ms per call (inliers/pair mean {rec['inliers'].mean():.0f})")
for it in (256, 512, 1024):
    print(f"  ratio of the medians, essential at {it} / fundamental at 1024: {np.median(e_ms[it]) / np.median(f_ms):.2f}")

# one synchronous call
ah.check(ah.lib.hak_sync(det.ctx))
one = torch.from_numpy(to_pairs(synth.two_view_matches(1030, 440, 7, noise=0.3)[0]).view(np.uint8).copy()).cuda()
mask1 = torch.zeros(1470, dtype=torch.uint8, device="cuda")
r1 = np.zeros((), ah.FUNDAMENTAL_DTYPE)
for ctx in (det.ctx, None):
    us = []
    for k in range(55):
        t0 = time.perf_counter()
        ah.check(ah.lib.hak_find_essential(ctx, one.data_ptr(), 1470, K.ctypes.data, K.ctypes.data, 1024, 1.0, 0, mask1.data_ptr(),
                                           r1.ctypes.data))
        if k >= 5:
            us.append((time.perf_counter() - t0) * 1e6)
    print(f"hak_find_essential, 1470 records, 1024 hypotheses, ctx={'yes' if ctx else 'NULL'}: {stats(us)} us per synchronous call "
          f"(inliers {int(r1['inliers'])})")

# the detect path with and without an essential batch in front of it on the same context
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
            ess_batch()
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
    print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind an essential batch' if before else 'alone'}: "
          f"{stats(timed_detect(before))} ms per call")
det.close()

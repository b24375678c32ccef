"""homography_time.py: cost of the RANSAC homography (hak_find_homography_batch / hak_find_homography) on 2-NN lists of synth
1080p pairs, timed with HIP events on the context's stream.

  batched: 256 pairs (the lists of 8 detected pairs, repeated), 1024 hypotheses, 3 px, refine = 1
  single:  one list of the same pairs (and a planted list of 2000 matches), 1024 hypotheses: event time and the host-side
           latency of the synchronous call (launch + wait + record download)"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "cuda-akaze_amd"), os.path.join(HERE, "..", "tests")]
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

w, h, mp, NPAIR, NDET = 1920, 1080, 10000, 256, 8
p = ah.iAlignUp(w, 128)
imgs = []
for s in range(1, NDET + 1):
    imgs += list(synth.pair(w, h, s))
d = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=2 * NDET)
pts = torch.zeros(2 * NDET * mp * 104, dtype=torch.uint8, device="cuda")
num = torch.zeros(2 * NDET, dtype=torch.int32, device="cuda")
lst = torch.zeros(NDET * mp * 32, dtype=torch.uint8, device="cuda")
cnt = torch.zeros(NDET, dtype=torch.int32, device="cuda")
ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d.data_ptr(), h * p, p, 2 * NDET, pts.data_ptr(), num.data_ptr(), 1))
ah.check(ah.lib.hak_match_knn2_batch(det.ctx, pts.data_ptr(), num.data_ptr(), NDET, 4, 5, 1, 0, lst.data_ptr(), cnt.data_ptr()))
ah.check(ah.lib.hak_sync(det.ctx))
# 256 pairs: the 8 lists repeated (pair k = list k mod 8)
big = lst.view(NDET, mp * 32).repeat(NPAIR // NDET, 1).reshape(-1).contiguous()
bcnt = cnt.repeat(NPAIR // NDET).contiguous()
out = torch.zeros(NPAIR * ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
masks = torch.zeros(NPAIR * mp, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))


def batch_call(refine=1, iters=1024):
    ah.check(ah.lib.hak_find_homography_batch(det.ctx, big.data_ptr(), mp, bcnt.data_ptr(), NPAIR, iters, 3.0, 0, refine,
                                              out.data_ptr(), masks.data_ptr()))


def events(fn, reps):
    for _ in range(3):
        fn()
    ah.check(ah.lib.hak_sync(det.ctx))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


counts = cnt.cpu().numpy()
print(f"lists: {NDET} synth 1080p pairs, 2-NN ratio 4/5 + cross-check: {counts.min()}..{counts.max()} matches "
      f"(mean {counts.mean():.0f})")
for refine in (1, 0):
    ms = events(lambda: batch_call(refine), 20)
    rec = out.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
    print(f"batch {NPAIR} pairs x 1024 hypotheses, refine={refine}: {ms:.3f} ms per call "
          f"(inliers/pair mean {rec['inliers'].mean():.0f}, refined {int(rec['refined'].sum())}/{NPAIR})")
tests_per_call = float(counts.mean()) * 1024 * NPAIR
print(f"  = {tests_per_call / 1e9:.3f} G match tests per call")

# single pair
ah.check(ah.lib.hak_set_stream(det.ctx, None))
ah.check(ah.lib.hak_set_null_order(det.ctx, 1))
rec = np.zeros((), ah.HOMOGRAPHY_DTYPE)
k = int(np.argmax(counts))
one = lst.view(NDET, mp * 32)[k].contiguous()
mask1 = torch.zeros(mp, dtype=torch.uint8, device="cuda")
from test_homography_cpu import planted  # noqa: E402
recs, _, _ = planted(2000, 1, outlier_rate=0.4, w=1920, h=1080)
pl = np.zeros(2000, ah.MATCH_PAIR_DTYPE)
for j, f in enumerate(("x1", "y1", "x2", "y2")):
    pl[f] = recs[:, j]
dpl = torch.from_numpy(pl.view(np.uint8).copy()).cuda()
for name, buf, n in ((f"1080p list ({int(counts[k])} matches)", one, int(counts[k])), ("planted list (2000 matches)", dpl, 2000)):
    for ctx in (det.ctx, None):
        for _ in range(5):
            ah.check(ah.lib.hak_find_homography(ctx, buf.data_ptr(), n, 1024, 3.0, 0, 1, mask1.data_ptr(), rec.ctypes.data))
        t0 = time.perf_counter()
        for _ in range(50):
            ah.check(ah.lib.hak_find_homography(ctx, buf.data_ptr(), n, 1024, 3.0, 0, 1, mask1.data_ptr(), rec.ctypes.data))
        us = (time.perf_counter() - t0) / 50 * 1e6
        print(f"single {name}, ctx={'yes' if ctx else 'NULL'}: {us:.0f} us per synchronous call (inliers {int(rec['inliers'])}, "
              f"refined {int(rec['refined'])})")
det.close()

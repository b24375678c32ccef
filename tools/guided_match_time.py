"""guided_match_time.py: cost of guided matching (hak_match_guided_batch / hak_match_guided) next to the dense 2-NN match
(hak_match_knn2_batch / hak_match_knn2) on the same point sets, in one process.

  batched: 256 pairs -- the keypoints of 8 detected synth 1080p pairs, repeated (the sets profiles/homography_time.txt used) --
           radius 8, ratio 4/5, cross-check; H of every pair from hak_find_homography_batch on its 2-NN list.  Every call is timed
           on its own with HIP events on the context's stream, the two entry points alternating; median, min and max of the calls.
  single:  the first 1500 keypoints of both images of one pair: host-side latency of the synchronous call."""
import ctypes as C
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "cuda-akaze_amd")]
import numpy as np
import torch

import akaze_hip as ah
from akaze_hip import synth

w, h, mp, NPAIR, NDET, REPS = 1920, 1080, 10000, 256, 8, 30
RADIUS = 8.0
p = ah.iAlignUp(w, 128)
imgs = []
for s in range(1, NDET + 1):
    imgs += list(synth.pair(w, h, s))
d = torch.from_numpy(np.stack([synth.to_float(u, p) for u in imgs])).cuda()
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=2 * NDET)
pts8 = torch.zeros(2 * NDET * mp * 104, dtype=torch.uint8, device="cuda")
num8 = torch.zeros(2 * NDET, dtype=torch.int32, device="cuda")
ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d.data_ptr(), h * p, p, 2 * NDET, pts8.data_ptr(), num8.data_ptr(), 1))
ah.check(ah.lib.hak_sync(det.ctx))
det.close()
del d

# 256 pairs: the 8 pairs repeated (pair k = detected pair k mod 8), on a context whose batch holds them (the matcher does not care
# about the image geometry)
pts = pts8.view(NDET, 2 * mp * 104).repeat(NPAIR // NDET, 1).reshape(-1).contiguous()
num = num8.view(NDET, 2).repeat(NPAIR // NDET, 1).reshape(-1).contiguous()
big = ah.Akazer()
big.init((320, 240, ah.iAlignUp(320, 128)), max_pts=mp, batch=2 * NPAIR)
lst = torch.zeros(NPAIR * mp * 32, dtype=torch.uint8, device="cuda")
cnt = torch.zeros(NPAIR, dtype=torch.int32, device="cuda")
glst = torch.zeros(NPAIR * mp * 32, dtype=torch.uint8, device="cuda")
gcnt = torch.zeros(NPAIR, dtype=torch.int32, device="cuda")
hom = torch.zeros(NPAIR * ah.HOMOGRAPHY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(big.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(big.ctx, 0))
torch.cuda.synchronize()


def knn2():
    ah.check(ah.lib.hak_match_knn2_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, 4, 5, 1, 0, lst.data_ptr(), cnt.data_ptr()))


def guided():
    ah.check(ah.lib.hak_match_guided_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, hom.data_ptr(), RADIUS, 4, 5, 1, 0,
                                           glst.data_ptr(), gcnt.data_ptr()))


knn2()
ah.check(ah.lib.hak_find_homography_batch(big.ctx, lst.data_ptr(), mp, cnt.data_ptr(), NPAIR, 1024, 3.0, 0, 1, hom.data_ptr(), None))
for _ in range(3):
    guided()
    knn2()
ah.check(ah.lib.hak_sync(big.ctx))
times = {"knn2": [], "guided": []}
evs = []
for _ in range(REPS):
    for name, fn in (("knn2", knn2), ("guided", guided)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        evs.append((name, a, b))
ah.check(ah.lib.hak_sync(big.ctx))
for name, a, b in evs:
    times[name].append(a.elapsed_time(b))
n = num.cpu().numpy()
rec = hom.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)
c2, cg = cnt.cpu().numpy(), gcnt.cpu().numpy()
print(f"sets: {NDET} synth 1080p pairs repeated to {NPAIR}: {n.min()}..{n.max()} keypoints per image (mean {n.mean():.0f})")
print(f"2-NN ratio 4/5 + cross-check: {c2.mean():.0f} matches per pair, RANSAC inliers {rec['inliers'].mean():.0f}; "
      f"guided (radius {RADIUS:g}, ratio 4/5, cross-check): {cg.mean():.0f} matches per pair")
for name, label in (("knn2", "hak_match_knn2_batch  "), ("guided", "hak_match_guided_batch")):
    t = np.array(times[name])
    print(f"{label} {NPAIR} pairs: median {np.median(t):.3f} ms per call (min {t.min():.3f}, max {t.max():.3f}, {len(t)} calls)")

# single pair, about 1500 x 1500 points
ah.check(ah.lib.hak_set_stream(big.ctx, None))
ah.check(ah.lib.hak_set_null_order(big.ctx, 1))
k = int(np.argmax(n[:2 * NDET:2]))
n1, n2 = min(1500, int(n[2 * k])), min(1500, int(n[2 * k + 1]))
rows = pts8.view(2 * NDET, mp * 104)
p1, p2 = rows[2 * k].contiguous(), rows[2 * k + 1].contiguous()
out1 = torch.zeros(mp * 32, dtype=torch.uint8, device="cuda")
H = np.ascontiguousarray(rec[k]["H"], np.float32)
count = C.c_int(0)


def single_guided(ctx):
    ah.check(ah.lib.hak_match_guided(ctx, p1.data_ptr(), n1, p2.data_ptr(), n2, H.ctypes.data_as(C.POINTER(C.c_float)), RADIUS, 4, 5, 1, 0,
                                     None, out1.data_ptr(), C.byref(count), None))


def single_knn2(ctx):
    ah.check(ah.lib.hak_match_knn2(ctx, p1.data_ptr(), n1, p2.data_ptr(), n2, 4, 5, 1, 0, None, out1.data_ptr(), C.byref(count), None))


for label, fn in (("hak_match_knn2  ", single_knn2), ("hak_match_guided", single_guided)):
    for ctx in (big.ctx, None):
        for _ in range(5):
            fn(ctx)
        t = []
        for _ in range(50):
            t0 = time.perf_counter()
            fn(ctx)
            t.append((time.perf_counter() - t0) * 1e6)
        t = np.array(t)
        print(f"single {label} {n1} x {n2}, ctx={'yes' if ctx else 'NULL'}: median {np.median(t):.0f} us per synchronous call "
              f"(min {t.min():.0f}, max {t.max():.0f}; {count.value} matches)")
big.close()

"""epipolar_match_time.py: cost of epipolar guided matching (hak_match_epipolar_batch / hak_match_epipolar) next to the dense 2-NN
match (hak_match_knn2_batch / hak_match_knn2) and the homography-guided match (hak_match_guided_batch) on the same point sets, in
one process.

  batched: 256 pairs -- the keypoints of 8 detected synth 1080p pairs, repeated (the sets profiles/guided_match_time.txt used) --
           ratio 4/5, cross-check; epipolar radius 2 with F of every pair from hak_find_fundamental_batch on its 2-NN list, guided
           radius 8 with H from hak_find_homography_batch.  Every call is timed on its own with HIP events on the context's stream,
           the three entry points alternating; mean, min and max of the calls.
  single:  the first 1500 keypoints of both images of one pair: host-side latency of the synchronous call.
  Also printed, from numpy on the first pair: how many train points a query's band holds and how many lie within one cell side of
  its line (about what the walk lists and tests), against the n2 the dense match looks at."""
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
RADIUS = 8.0                     # homography-guided
ERADIUS = 2.0                    # epipolar
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
elst = torch.zeros(NPAIR * mp * 32, dtype=torch.uint8, device="cuda")
ecnt = torch.zeros(NPAIR, dtype=torch.int32, device="cuda")
fund = torch.zeros(NPAIR * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(big.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(big.ctx, 0))
torch.cuda.synchronize()


def knn2():
    ah.check(ah.lib.hak_match_knn2_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, 4, 5, 1, 0, lst.data_ptr(), cnt.data_ptr()))


def guided():
    ah.check(ah.lib.hak_match_guided_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, hom.data_ptr(), RADIUS, 4, 5, 1, 0,
                                           glst.data_ptr(), gcnt.data_ptr()))


def epipolar():
    ah.check(ah.lib.hak_match_epipolar_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, fund.data_ptr(), ERADIUS, 4, 5, 1, 0,
                                             elst.data_ptr(), ecnt.data_ptr()))


knn2()
ah.check(ah.lib.hak_find_fundamental_batch(big.ctx, lst.data_ptr(), mp, cnt.data_ptr(), NPAIR, 1024, 1.0, 0, fund.data_ptr(), None))
ah.check(ah.lib.hak_find_homography_batch(big.ctx, lst.data_ptr(), mp, cnt.data_ptr(), NPAIR, 1024, 3.0, 0, 1, hom.data_ptr(), None))
for _ in range(3):
    guided()
    epipolar()
    knn2()
ah.check(ah.lib.hak_sync(big.ctx))
times = {"knn2": [], "guided": [], "epipolar": []}
evs = []
for _ in range(REPS):
    for name, fn in (("knn2", knn2), ("guided", guided), ("epipolar", epipolar)):
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
frec = fund.cpu().numpy().view(ah.FUNDAMENTAL_DTYPE)
c2, cg, ce = cnt.cpu().numpy(), gcnt.cpu().numpy(), ecnt.cpu().numpy()
print(f"sets: {NDET} synth 1080p pairs repeated to {NPAIR}: {n.min()}..{n.max()} keypoints per image (mean {n.mean():.0f})")
print(f"2-NN ratio 4/5 + cross-check: {c2.mean():.0f} matches per pair, RANSAC inliers {rec['inliers'].mean():.0f}; "
      f"guided (radius {RADIUS:g}, ratio 4/5, cross-check): {cg.mean():.0f} matches per pair")
print(f"fundamental RANSAC (1024 x 1 px) inliers {frec['inliers'].mean():.0f}; epipolar (radius {ERADIUS:g}, ratio 4/5, cross-check): "
      f"{ce.mean():.0f} matches per pair")
for name, label in (("knn2", "hak_match_knn2_batch    "), ("guided", "hak_match_guided_batch  "), ("epipolar", "hak_match_epipolar_batch")):
    t = np.array(times[name])
    print(f"{label} {NPAIR} pairs: mean {t.mean():.3f} ms per call (min {t.min():.3f}, max {t.max():.3f}, {len(t)} calls)")

# what a query looks at, first pair: distance of every train point from every query's line (float64)
host = pts8.cpu().numpy().view(ah.POINT_DTYPE).reshape(2 * NDET, mp)
q0, t0 = host[0, :n[0]], host[1, :n[1]]
F0 = frec[0]["F"].astype(np.float64).reshape(3, 3)
ln = np.stack([q0["x"], q0["y"], np.ones(len(q0))], axis=1) @ F0.T
dist = np.abs(ln[:, :1] * t0["x"][None, :] + ln[:, 1:2] * t0["y"][None, :] + ln[:, 2:]) / np.hypot(ln[:, 0], ln[:, 1])[:, None]
side = max(ERADIUS * 1.0001 + 0.01, max(np.ptp(t0["x"]), np.ptp(t0["y"])) / 64)
print(f"first pair, {len(q0)} x {len(t0)}: {(dist < ERADIUS).sum(1).mean():.1f} train points per query inside the band, "
      f"{(dist < side).sum(1).mean():.0f} within one cell side ({side:.1f} px) of the line, {len(t0)} in the image")

# single pair, about 1500 x 1500 points
ah.check(ah.lib.hak_set_stream(big.ctx, None))
ah.check(ah.lib.hak_set_null_order(big.ctx, 1))
k = int(np.argmax(n[:2 * NDET:2]))
n1, n2 = min(1500, int(n[2 * k])), min(1500, int(n[2 * k + 1]))
rows = pts8.view(2 * NDET, mp * 104)
p1, p2 = rows[2 * k].contiguous(), rows[2 * k + 1].contiguous()
out1 = torch.zeros(mp * 32, dtype=torch.uint8, device="cuda")
F = np.ascontiguousarray(frec[k]["F"], np.float32)
count = C.c_int(0)


def single_epipolar(ctx):
    ah.check(ah.lib.hak_match_epipolar(ctx, p1.data_ptr(), n1, p2.data_ptr(), n2, F.ctypes.data_as(C.POINTER(C.c_float)), ERADIUS, 4, 5, 1,
                                       0, None, out1.data_ptr(), C.byref(count), None))


def single_knn2(ctx):
    ah.check(ah.lib.hak_match_knn2(ctx, p1.data_ptr(), n1, p2.data_ptr(), n2, 4, 5, 1, 0, None, out1.data_ptr(), C.byref(count), None))


for label, fn in (("hak_match_knn2    ", single_knn2), ("hak_match_epipolar", single_epipolar)):
    for ctx in (big.ctx, None):
        for _ in range(5):
            fn(ctx)
        t = []
        for _ in range(50):
            t0 = time.perf_counter()
            fn(ctx)
            t.append((time.perf_counter() - t0) * 1e6)
        t = np.array(t)
        print(f"single {label} {n1} x {n2}, ctx={'yes' if ctx else 'NULL'}: mean {t.mean():.0f} us per synchronous call "
              f"(min {t.min():.0f}, max {t.max():.0f}; {count.value} matches)")
big.close()

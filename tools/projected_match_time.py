"""projected_match_time.py: cost of projection-guided matching (hak_match_projected_batch / hak_match_projected) next to guided
matching (hak_match_guided_batch) and track linking (hak_link_tracks_batch) on the same point sets, in one process.

  batched: 256 pairs -- the keypoints of 8 detected synth 1080p pairs, repeated (the sets profiles/guided_match_time.txt used) --
           radius 8, ratio 4/5, cross-check.  H of every pair comes from hak_find_homography_batch on its 2-NN list.  The landmarks
           of a pair are ALL keypoints of its first image (an identity list A, D = the first image) at the points (px, py, 1), with
           (px, py) where H sends the keypoint, under the identity view and K = (1, 1, 0, 0): the projected call then searches the
           gates the guided call searches, and what differs is the code -- the landmark's record, mask-free eligibility, the 3-D
           projection, the descriptor through A[m].train, the hak_corr3d compaction.  The link call joins the pair's 2-NN list with
           the 2-NN list of the swapped pair.  Every call is timed on its own with HIP events on the context's stream, the three
           entry points alternating; median, min and max of the calls.
  single:  the first 1500 keypoints of both images of one pair: host-side latency of the synchronous call.
  detect:  a 256-image 1080p hak_detect_and_compute_batch on one context, alone and behind a projected batch of 128 lists (that
           context's pair capacity) on the same context."""
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

w, h, mp, NPAIR, NDET, REPS, NIMG = 1920, 1080, 10000, 256, 8, 30, 256
RADIUS = 8.0
K1 = ah.intrinsics((1.0, 1.0, 0.0, 0.0))
p = ah.iAlignUp(w, 128)


def stats(v):
    v = np.sort(np.asarray(v))
    return f"median {np.median(v):.3f} (min {v[0]:.3f}, max {v[-1]:.3f}, {len(v)} calls)"


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

# 256 pairs: the 8 pairs repeated (pair k = detected pair k mod 8), on a context whose batch holds them (the matchers do not care
# about the image geometry); `swp` holds every pair with its images exchanged, for list B of the link
rep = NPAIR // NDET
pts = pts8.view(NDET, 2 * mp * 104).repeat(rep, 1).reshape(-1).contiguous()
num = num8.view(NDET, 2).repeat(rep, 1).reshape(-1).contiguous()
swp = pts8.view(NDET, 2, mp * 104).flip(1).reshape(NDET, -1).repeat(rep, 1).reshape(-1).contiguous()
nsw = num8.view(NDET, 2).flip(1).repeat(rep, 1).reshape(-1).contiguous()
big = ah.Akazer()
big.init((320, 240, ah.iAlignUp(320, 128)), max_pts=mp, batch=2 * NPAIR)
zeros = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")
lst, cnt, lstB, cntB = zeros(NPAIR * mp * 32), zeros(NPAIR, torch.int32), zeros(NPAIR * mp * 32), zeros(NPAIR, torch.int32)
glst, gcnt = zeros(NPAIR * mp * 32), zeros(NPAIR, torch.int32)
plst, pcnt = zeros(NPAIR * mp * 32), zeros(NPAIR, torch.int32)
llst, lcnt = zeros(NPAIR * mp * 32), zeros(NPAIR, torch.int32)
hom = zeros(NPAIR * ah.HOMOGRAPHY_DTYPE.itemsize)
stream = torch.cuda.Stream()
ah.check(ah.lib.hak_set_stream(big.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(big.ctx, 0))
torch.cuda.synchronize()


def knn2(points=pts, counts=num, out=lst, out_counts=cnt):
    ah.check(ah.lib.hak_match_knn2_batch(big.ctx, points.data_ptr(), counts.data_ptr(), NPAIR, 4, 5, 1, 0, out.data_ptr(), out_counts.data_ptr()))


knn2()
knn2(swp, nsw, lstB, cntB)
ah.check(ah.lib.hak_find_homography_batch(big.ctx, lst.data_ptr(), mp, cnt.data_ptr(), NPAIR, 1024, 3.0, 0, 1, hom.data_ptr(), None))
ah.check(ah.lib.hak_sync(big.ctx))
n = num.cpu().numpy()
rec = hom.cpu().numpy().view(ah.HOMOGRAPHY_DTYPE)

# the landmarks: every keypoint of the first image at (px, py, 1), (px, py) = its position under the pair's H, in float32
host8 = pts8.cpu().numpy().view(ah.POINT_DTYPE).reshape(2 * NDET, mp)
A_host = np.zeros((NPAIR, mp), ah.MATCH_PAIR_DTYPE)
A_host["query"] = A_host["train"] = np.arange(mp)[None, :]
X_host = np.zeros((NPAIR, mp, 3), np.float32)
for k in range(NPAIR):
    q, H = host8[2 * (k % NDET)], rec[k]["H"].astype(np.float32)
    with np.errstate(all="ignore"):
        wz = (H[6] * q["x"] + H[7] * q["y"]) + H[8]
        X_host[k, :, 0] = ((H[0] * q["x"] + H[1] * q["y"]) + H[2]) / wz
        X_host[k, :, 1] = ((H[3] * q["x"] + H[4] * q["y"]) + H[5]) / wz
    X_host[k, :, 2] = 1.0
A = torch.from_numpy(A_host.view(np.uint8).reshape(-1)).cuda()
X = torch.from_numpy(X_host.reshape(-1)).cuda()


def guided():
    ah.check(ah.lib.hak_match_guided_batch(big.ctx, pts.data_ptr(), num.data_ptr(), NPAIR, hom.data_ptr(), RADIUS, 4, 5, 1, 0,
                                           glst.data_ptr(), gcnt.data_ptr()))


def projected(ctx=None, npairs=NPAIR):
    ah.check(ah.lib.hak_match_projected_batch(ctx or big.ctx, A.data_ptr(), mp, num.data_ptr(), 2, None, X.data_ptr(), pts.data_ptr(), 2 * mp,
                                              num.data_ptr(), 2, pts.data_ptr() + 104 * mp, 2 * mp, num.data_ptr() + 4, 2, npairs, None,
                                              ah.VIEW_IDENTITY, 0, K1.ctypes.data, RADIUS, 4, 5, 1, 0, plst.data_ptr(), mp, pcnt.data_ptr()))


def link():
    ah.check(ah.lib.hak_link_tracks_batch(big.ctx, lst.data_ptr(), mp, cnt.data_ptr(), 1, None, X.data_ptr(), lstB.data_ptr(), mp,
                                          cntB.data_ptr(), 1, NPAIR, llst.data_ptr(), mp, lcnt.data_ptr()))


calls = (("guided", guided), ("projected", projected), ("link", link))
for _ in range(3):
    for _, fn in calls:
        fn()
ah.check(ah.lib.hak_sync(big.ctx))
times = {name: [] for name, _ in calls}
evs = []
for _ in range(REPS):
    for name, fn in calls:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        evs.append((name, a, b))
ah.check(ah.lib.hak_sync(big.ctx))
for name, a, b in evs:
    times[name].append(a.elapsed_time(b))
c2, cg, cp, cl = cnt.cpu().numpy(), gcnt.cpu().numpy(), pcnt.cpu().numpy(), lcnt.cpu().numpy()
print(f"sets: {NDET} synth 1080p pairs repeated to {NPAIR}: {n.min()}..{n.max()} keypoints per image (mean {n.mean():.0f})")
print(f"2-NN ratio 4/5 + cross-check: {c2.mean():.0f} matches per pair, RANSAC inliers {rec['inliers'].mean():.0f}; guided (radius "
      f"{RADIUS:g}, ratio 4/5, cross-check): {cg.mean():.0f} matches per pair; projected, the same gates: {cp.mean():.0f} "
      f"correspondences per list (equal to the guided count in {int((cp == cg).sum())} of {NPAIR} lists); link of the 2-NN list with "
      f"the swapped pair's: {cl.mean():.0f} correspondences per pair")
for name, label in (("guided", "hak_match_guided_batch   "), ("projected", "hak_match_projected_batch"), ("link", "hak_link_tracks_batch    ")):
    print(f"{label} {NPAIR} lists: {stats(times[name])} ms per call")
print(f"  ratio of the medians, projected / guided: {np.median(times['projected']) / np.median(times['guided']):.3f}")

# single list, about 1500 x 1500 points
ah.check(ah.lib.hak_set_stream(big.ctx, None))
ah.check(ah.lib.hak_set_null_order(big.ctx, 1))
k = int(np.argmax(n[:2 * NDET:2]))
n1, n2 = min(1500, int(n[2 * k])), min(1500, int(n[2 * k + 1]))
rows = pts8.view(2 * NDET, mp * 104)
p1, p2 = rows[2 * k].contiguous(), rows[2 * k + 1].contiguous()
A1, X1 = A[:mp * 32].contiguous(), X.view(NPAIR, mp * 3)[k].contiguous()
out1 = zeros(mp * 32)
Hk = np.ascontiguousarray(rec[k]["H"], np.float32)
count = C.c_int(0)


def single_guided(ctx):
    ah.check(ah.lib.hak_match_guided(ctx, p1.data_ptr(), n1, p2.data_ptr(), n2, Hk.ctypes.data_as(C.POINTER(C.c_float)), RADIUS, 4, 5, 1, 0,
                                     None, out1.data_ptr(), C.byref(count), None))


def single_projected(ctx):
    ah.check(ah.lib.hak_match_projected(ctx, A1.data_ptr(), n1, None, X1.data_ptr(), p1.data_ptr(), n1, p2.data_ptr(), n2, None,
                                        K1.ctypes.data, RADIUS, 4, 5, 1, 0, out1.data_ptr(), C.byref(count), None))


for label, fn in (("hak_match_guided   ", single_guided), ("hak_match_projected", single_projected)):
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
              f"(min {t.min():.0f}, max {t.max():.0f}; {count.value} accepted)")
big.close()

# the detect path with and without a projected batch in front of it on the same context
det = ah.Akazer()
det.init((w, h, p), max_pts=mp, batch=NIMG)
ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
ah.check(ah.lib.hak_set_null_order(det.ctx, 0))
u1, u2 = imgs[0], imgs[1]
two = torch.from_numpy(np.stack([synth.to_float(u1, p), synth.to_float(u2, p)])).cuda()
frames = two.repeat(NIMG // 2, 1, 1).contiguous()
dpts = zeros(NIMG * mp * 104)
dnum = zeros(NIMG, torch.int32)


def detect():
    ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, frames.data_ptr(), h * p, p, NIMG, dpts.data_ptr(), dnum.data_ptr(), 1))


def timed_detect(before):
    ms = []
    for _ in range(5):
        if before:
            projected(det.ctx, NIMG // 2)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        detect()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


with torch.cuda.stream(stream):
    detect()
    ah.check(ah.lib.hak_sync(det.ctx))
    for before in (False, True, False, True):
        print(f"hak_detect_and_compute_batch, {NIMG} x 1080p, {'behind a projected batch of ' + str(NIMG // 2) + ' lists' if before else 'alone'}: "
              f"{stats(timed_detect(before))} ms per call")
det.close()

"""retain_best_time.py: cost of the strongest-N selection (hak_set_retain_best, kernels_select.hip).

  (a) bench.py's batch shape: 256 x 1080p synth images in one hak_detect_and_compute_batch sequence, max_pts 10000 (no image
      overflows): mode off vs on = the cost of the early-out
  (b) the same batch with max_pts 1000 (every image overflows): raster clamp (off) vs strongest 1000 (on)
  (c) one 4K / 5-octave image through hak_detect_and_compute with C = 2000: off vs on (host latency of the synchronous call)
  kernels: the select kernels' times from a separate `rocprofv3 --kernel-trace --stats` run of legs (a)-(c) with the mode on

Modes alternate inside one process (A B A B ...); every figure is the median over the rounds.  The orchestrator (no --leg) runs
each leg as a child process under its own `timeout` and writes the report (--out, default profiles/retain_best_time.txt)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def leg(trace):
    sys.path[:0] = [os.path.join(ROOT, "cuda-akaze_amd")]
    import numpy as np
    import torch

    import akaze_hip as ah
    from akaze_hip import synth

    rounds, reps = (1, 2) if trace else (7, 5)
    w, h, B = 1920, 1080, 256
    p = ah.iAlignUp(w, 128)
    distinct = [synth.scene(w, h, s) for s in range(1, 33)]
    one = torch.from_numpy(np.stack([synth.to_float(u, p) for u in distinct])).cuda()
    d = one.repeat(B // len(distinct), 1, 1).contiguous()                    # (the 32 distinct images, copied on the device)
    stream = torch.cuda.Stream()

    def batch_ab(mp, label):
        det = ah.Akazer()
        det.init((w, h, p), max_pts=mp, batch=B)
        ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
        ah.check(ah.lib.hak_set_null_order(det.ctx, 0))
        pts = torch.zeros(B * mp * ah.POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        num = torch.zeros(B, dtype=torch.int32, device="cuda")

        def run(on, n):
            ah.check(ah.lib.hak_set_retain_best(det.ctx, on))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(n):
                ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / n

        for on in (0, 1):                                                     # capture both graphs, warm up
            run(on, 2)
        t = {0: [], 1: []}
        counts = {}
        for _ in range(rounds):
            for on in (0, 1):
                t[on].append(run(on, reps))
                counts[on] = num.cpu().numpy().copy()
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"({label}) batch {B} x 1080p, max_pts {mp}: off {med[0]:.3f} ms, on {med[1]:.3f} ms per call, "
              f"on - off {1e3 * (med[1] - med[0]):+.1f} us ({100 * (med[1] / med[0] - 1):+.2f} %); "
              f"keypoints per image off {counts[0].mean():.1f}, on {counts[1].mean():.1f}; "
              f"spread off {min(t[0]):.3f}..{max(t[0]):.3f}, on {min(t[1]):.3f}..{max(t[1]):.3f} ms", flush=True)
        det.close()

    batch_ab(10000, "a")
    batch_ab(1000, "b")
    del d, one
    torch.cuda.empty_cache()

    # (c) one 4K / 5-octave image, C = 2000
    w, h, C = 3840, 2160, 2000
    p = ah.iAlignUp(w, 128)
    img = torch.from_numpy(synth.to_float(synth.scene(w, h, 4), p)).cuda()
    det = ah.Akazer()
    det.init((w, h, p), noctaves=5, max_pts=C)
    data = ah.AkazeData()
    ah.initAkazeData(data, C, True, True)

    def single(on, n):
        det.set_retain_best(bool(on))
        t0 = time.perf_counter()
        for _ in range(n):
            det.detectAndCompute(img.data_ptr(), data, (w, h, p), True)
        return (time.perf_counter() - t0) / n * 1e3

    for on in (0, 1):
        single(on, 2)
    t = {0: [], 1: []}
    for _ in range(rounds):
        for on in (0, 1):
            t[on].append(single(on, 2 * reps))
    med = {k: float(np.median(v)) for k, v in t.items()}
    big = ah.AkazeData()
    ah.initAkazeData(big, 1 << 18, True, True)
    det.set_retain_best(False)
    det.detectAndCompute(img.data_ptr(), big, (w, h, p), True)
    print(f"(c) one 4K / 5-octave image, C = {C} of {big.num_pts} survivors: off (raster prefix) {med[0]:.3f} ms, "
          f"on (strongest) {med[1]:.3f} ms per synchronous call, on - off {1e3 * (med[1] - med[0]):+.1f} us", flush=True)
    ah.freeAkazeData(big)
    ah.freeAkazeData(data)
    det.close()


def kernel_table(outdir):
    f = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        return ["(no kernel_stats.csv found)"]
    lines = [f"{'kernel':24s} {'calls':>6s} {'avg us':>9s} {'min us':>9s} {'max us':>9s} {'total ms':>9s}"]
    for r in csv.DictReader(open(f[0])):
        n = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if n.startswith("k_sel_") or n in ("k_nms_cand", "k_row_scan", "k_emit"):
            lines.append(f"{n:24s} {r['Calls']:>6s} {float(r['AverageNs']) / 1e3:9.1f} {float(r['MinNs']) / 1e3:9.1f} "
                         f"{float(r['MaxNs']) / 1e3:9.1f} {float(r['TotalDurationNs']) / 1e6:9.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("ab", "trace"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retain_best_time.txt"))
    args = ap.parse_args()
    if args.leg:
        leg(args.leg == "trace")
        return 0
    me = os.path.abspath(__file__)
    report = []
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, me, "--leg", "ab"], capture_output=True, text=True)
    report += r.stdout.strip().splitlines()
    if r.returncode != 0:
        report += [f"A/B leg failed: exit {r.returncode}", r.stderr.strip()[-2000:]]
        open(args.out, "w").write("\n".join(report) + "\n")
        print("\n".join(report))
        return 1
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                            "-d", td, "-o", "run", "--", sys.executable, me, "--leg", "trace"], capture_output=True, text=True, cwd=td)
        report += ["", "kernel times, rocprofv3 --kernel-trace --stats (mode on; legs (a)-(c) with 2 calls each, plus warm-up "
                   "and the mode-off calls):"]
        report += kernel_table(td) if r.returncode == 0 else [f"trace leg failed: exit {r.returncode}", r.stderr.strip()[-2000:]]
    open(args.out, "w").write("\n".join(report) + "\n")
    print("\n".join(report))
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

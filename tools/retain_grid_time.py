"""retain_grid_time.py: cost of the grid selection (hak_set_retain_grid, kernels_grid_select.hip) next to the strongest-N selection
(hak_set_retain_best, kernels_select.hip) -- the yardstick -- and to the mode-off sequence.

  (a) bench.py's batch shape: 256 x 1080p synth images in one hak_detect_and_compute_batch sequence, max_pts 10000 (no image
      overflows): off vs strongest-N vs grid G = 32 = the cost of the early-outs
  (b) the same batch with max_pts 1000 (every image overflows): raster clamp (off) vs strongest 1000 vs grid G = 32
  kernels: the selection kernels' times from a separate `rocprofv3 --kernel-trace --stats` run of both legs

Modes alternate inside one process (off best grid off best grid ...); every figure is the median over the rounds, the spread is
given next to it.  The orchestrator (no --leg) runs each leg as a child process under its own `timeout` and writes the report
(--out, default profiles/retain_grid_time.txt)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = 32
MODES = (("off", 0, 0), ("best", 1, 0), ("grid", 0, G))


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

    def batch_abc(mp, label):
        det = ah.Akazer()
        det.init((w, h, p), max_pts=mp, batch=B)
        ah.check(ah.lib.hak_set_stream(det.ctx, stream.cuda_stream))
        ah.check(ah.lib.hak_set_null_order(det.ctx, 0))
        pts = torch.zeros(B * mp * ah.POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        num = torch.zeros(B, dtype=torch.int32, device="cuda")

        def run(mode, n):
            ah.check(ah.lib.hak_set_retain_best(det.ctx, mode[1]))
            ah.check(ah.lib.hak_set_retain_grid(det.ctx, mode[2]))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(n):
                ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, d.data_ptr(), h * p, p, B, pts.data_ptr(), num.data_ptr(), 1))
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / n

        for m in MODES:                                                       # capture the three graphs, warm up
            run(m, 2)
        t = {m[0]: [] for m in MODES}
        counts = {}
        for _ in range(rounds):
            for m in MODES:
                t[m[0]].append(run(m, reps))
                counts[m[0]] = float(num.cpu().numpy().mean())
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"({label}) batch {B} x 1080p, max_pts {mp}, ms per call (median of {rounds} rounds of {reps} calls, min..max):", flush=True)
        for k in t:
            print(f"      {k:5s} {med[k]:8.3f}  ({min(t[k]):.3f}..{max(t[k]):.3f})  keypoints per image {counts[k]:.1f}", flush=True)
        cb, cg = med["best"] - med["off"], med["grid"] - med["off"]
        print(f"      best - off {1e3 * cb:+.1f} us, grid - off {1e3 * cg:+.1f} us, grid - best {1e3 * (cg - cb):+.1f} us"
              + (f", (grid - off) / (best - off) = {cg / cb:.2f}" if cb > 0 else ""), flush=True)
        det.close()

    batch_abc(10000, "a")
    batch_abc(1000, "b")


def kernel_table(outdir):
    f = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        return ["(no kernel_stats.csv found)"]
    lines = [f"{'kernel':24s} {'calls':>6s} {'avg us':>9s} {'min us':>9s} {'max us':>9s} {'total ms':>9s}"]
    for r in csv.DictReader(open(f[0])):
        n = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if n.startswith("k_sel_") or n.startswith("k_grid_") or n in ("k_nms_cand", "k_row_scan", "k_emit"):
            lines.append(f"{n:24s} {r['Calls']:>6s} {float(r['AverageNs']) / 1e3:9.1f} {float(r['MinNs']) / 1e3:9.1f} "
                         f"{float(r['MaxNs']) / 1e3:9.1f} {float(r['TotalDurationNs']) / 1e6:9.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("ab", "trace"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retain_grid_time.txt"))
    args = ap.parse_args()
    if args.leg:
        leg(args.leg == "trace")
        return 0
    me = os.path.abspath(__file__)
    report = []
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, me, "--leg", "ab"], capture_output=True, text=True)
    report += r.stdout.strip().splitlines()
    if r.returncode != 0:
        report += [f"A/B leg failed: exit {r.returncode}", r.stderr.strip()[-2000:]]
        open(args.out, "w").write("\n".join(report) + "\n")
        print("\n".join(report))
        return 1
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                            "-d", td, "-o", "run", "--", sys.executable, me, "--leg", "trace"], capture_output=True, text=True, cwd=td)
        report += ["", "kernel times, rocprofv3 --kernel-trace --stats (legs (a) and (b): per mode 2 warm-up calls and 2 timed calls of "
                   "256 images; half of each kernel's calls leave at once, in leg (a)):"]
        report += kernel_table(td) if r.returncode == 0 else [f"trace leg failed: exit {r.returncode}", r.stderr.strip()[-2000:]]
    open(args.out, "w").write("\n".join(report) + "\n")
    print("\n".join(report))
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

"""What paired contrasts cost: the cross kernel against the moments kernel on the same device-resident records, and
run_contrasts() against run_moments() on the same sweep.

    python scripts/bench_contrasts.py [--runs 8192] [--reps 3] [--kernel-reps 20] [--out FILE]

On the configs[3] grid (c4_grid(): 360 points x 9 miners) with pairs_vs_baseline (3 231 pairs):
  (k1) msim_cross_launch alone, by HIP events over resident records; logical bytes read = pairs x runs x 24
       (two 8-byte records and two 4-byte best heights per pair and run) over its time
  (k2) msim_moments_launch alone on the same buffers (no histogram); bytes read = points x runs x (8 M + 4)
  (w1) Sweep.run_contrasts wall time        (w2) Sweep.run_moments wall time
Every variant is warmed up at the timed shape, the kernels three times; the wall-clock variants are timed
alternately `--reps` times and end in a stream synchronise; medians and spreads are reported. One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=0, help="only the first N points of the grid (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench_contrasts.py needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    grid = msim.c4_grid()
    sw = msim.Sweep(grid[:args.points] if args.points else grid)
    points, m, runs = len(sw), sw.m, args.runs
    pairs = msim.pairs_vs_baseline(points, m)
    row = {"points": points, "miners": m, "runs_per_point": runs, "pairs": len(pairs),
           "lib": os.path.relpath(_lib.LIB_PATH, ROOT)}

    ws = torch.empty(sw.workspace_bytes(runs), dtype=torch.uint8, device=dev)
    sums = torch.zeros((points, m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((points, runs, m, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros((points, runs), dtype=torch.int32, device=dev)
    sw.launch(runs, 0, 1000, sums, ws, status, d_per_run=rec, d_best_height=bh)
    mom = torch.zeros((points, m, 20), dtype=torch.int64, device=dev)
    d_pairs = torch.from_numpy(np.asarray(pairs, dtype=np.uint32).view(np.int32)).to(dev)
    cross = torch.zeros((len(pairs), 12), dtype=torch.int64, device=dev)
    kernels = {
        "k1_cross": (lambda: sw.launch_cross(runs, rec, bh, d_pairs, len(pairs), cross), len(pairs) * runs * 24),
        "k2_moments": (lambda: sw.launch_moments(runs, rec, bh, mom), points * runs * (m * 8 + 4)),
    }
    for fn, _ in kernels.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in kernels}
    for _ in range(args.kernel_reps):  # alternating; each interval holds the launch's memset and the kernel
        for k, (fn, _) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for k, (_, nbytes) in kernels.items():
        med = statistics.median(ms[k])
        row[k] = {"median_ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "bytes_read": nbytes,
                  "read_TBs": nbytes / (med * 1e-3) / 1e12}
    row["unique_bytes"] = points * runs * (m * 8 + 4)
    del ws, rec, bh

    walls = {"w1_run_contrasts_s": lambda: msim.contrasts(sw.run_contrasts(runs, pairs, 0, 1000, 0)),
             "w2_run_moments_s": lambda: [msim.error_bars(r) for r in sw.run_moments(runs, 0, 1000, 0)]}
    times = {k: [] for k in walls}
    for fn in walls.values():
        fn()
    for _ in range(args.reps):
        for k, fn in walls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    for k, v in times.items():
        row[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

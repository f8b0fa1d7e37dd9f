"""What error bars cost: run_moments() against run() and against the only route there was before it,
run(per_run=True) plus a NumPy variance on the host.

    python scripts/bench_moments.py [--configs c2,c3,c4,c5] [--only a,b,c,d] [--reps 3] [--out FILE]

Per configuration (c2 and c3 at 32 768 runs, the configs[3] grid at 8 192 runs per point, c5 at 65 536 runs):
  (a) run() wall time
  (b) run(per_run=True) + NumPy variances of found, share and stale rate per miner
  (c) run_moments() with a 256-bin histogram + error_bars()
  (d) the moments kernel alone, by HIP events over device-resident records: its bytes read over its time
Every variant is warmed up once at the timed shape, then the variants are timed alternately `--reps` times;
the median and the spread (min, max) are reported. Host clocks around calls that end in a stream synchronise.
MSIM_LIB selects the library, so (a) and (b) can be taken on a build of another commit in the same GPU visit
(--only a,b). One JSON line per configuration."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_TBS = 6.3  # float4 copy, MI355X


def _numpy_errors(results):
    """What a user had to do: per-run shares and rates from the records, then variances."""
    import numpy as np

    out = []
    for r in results:
        f = r.found.astype(np.float64)
        L = r.best_height.astype(np.float64)[:, None]
        some = r.found > 0
        share = np.where(some, f / np.where(L > 0, L, 1.0), 0.0)
        rate = np.where(some, r.stale / np.where(some, f, 1.0), 0.0)
        n = f.shape[0]
        out.append([np.sqrt(x.var(axis=0, ddof=1) / n) for x in (f, share, rate)])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c4,c5")
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--runs-scale", type=float, default=1.0, help="scale every run count (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    import torch

    assert torch.cuda.is_available(), "bench_moments.py needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    have_moments = hasattr(msim.Simulation, "run_moments")
    plan = {
        "c2": (lambda: msim.Simulation(msim.PRESETS["c2"]()), 32768),
        "c3": (lambda: msim.Simulation(msim.PRESETS["c3"]()), 32768),
        "c4": (lambda: msim.Sweep(msim.c4_grid()), 8192),
        "c5": (lambda: msim.Simulation(msim.c5_network(), total_weight=msim.C5_TOTAL_WEIGHT), 65536),
    }
    sink = open(args.out, "a") if args.out else None
    for name in args.configs.split(","):
        make, runs = plan[name]
        runs = max(2, int(runs * args.runs_scale))
        obj = make()
        sweep = isinstance(obj, msim.Sweep)
        points = len(obj) if sweep else 1
        m = obj.m if sweep else len(obj.miners)
        as_list = (lambda r: r if sweep else [r])
        variants = {}
        if "a" in only:
            variants["a_run_s"] = lambda: obj.run(runs, 0, 1000, 0)
        if "b" in only:
            variants["b_per_run_numpy_s"] = lambda: _numpy_errors(as_list(obj.run(runs, 0, 1000, 0, per_run=True)))
        if "c" in only and have_moments:
            spec = msim.HistSpec.covering(0.0, 1.0, 256)
            variants["c_run_moments_s"] = lambda: [msim.error_bars(r) for r in
                                                   as_list(obj.run_moments(runs, 0, 1000, 0, hist=spec))]
        times = {k: [] for k in variants}
        for fn in variants.values():  # warm-up at the timed shape
            fn()
        for _ in range(args.reps):    # alternating
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        row = {"config": name, "runs_per_point": runs, "points": points, "miners": m, "reps": args.reps,
               "lib": _lib.LIB_PATH}
        for k, v in times.items():
            row[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        if "d" in only and have_moments:
            ws = torch.empty(obj.workspace_bytes(runs), dtype=torch.uint8, device=dev)
            lead = (points,) if sweep else ()
            sums = torch.zeros(lead + (m, 6), dtype=torch.int64, device=dev)
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            rec = torch.zeros(lead + (runs, m, 2), dtype=torch.int32, device=dev)
            bh = torch.zeros(lead + (runs,), dtype=torch.int32, device=dev)
            obj.launch(runs, 0, 1000, sums, ws, status, d_per_run=rec, d_best_height=bh)
            spec = msim.HistSpec.covering(0.0, 1.0, 256)
            mom = torch.zeros(lead + (m, 20), dtype=torch.int64, device=dev)
            hist = torch.zeros(lead + (m, 2, spec.bins + 2), dtype=torch.int64, device=dev)
            nbytes = points * runs * (m * 8 + 4)
            for label, hs, hb in (("d_kernel_hist256", spec, hist), ("d_kernel_nohist", None, None)):
                for _ in range(3):
                    obj.launch_moments(runs, rec, bh, mom, hs, hb)
                torch.cuda.synchronize()
                ms = []
                for _ in range(args.kernel_reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    obj.launch_moments(runs, rec, bh, mom, hs, hb)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                med = statistics.median(ms)
                # the interval holds the launch's memsets of the outputs and the kernel
                row[label] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "bytes_read": nbytes,
                              "read_TBs": nbytes / (med * 1e-3) / 1e12, "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS}
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        del obj
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

"""What miner classes cost: the fold kernel against the moments kernel it feeds, and run_classes() against the
per-miner run_moments() of another build.

    python scripts/bench_classes.py [--only a,b] [--reps 5] [--kernel-reps 20] [--parent-root DIR] [--out FILE]

Both on configs[4] (c5: 1 026 miners) at 65 536 runs:
  (a) msim_fold_launch alone, by HIP events over device-resident records, median of --kernel-reps, under three maps:
      classes_of(c5_network()) (3 classes), the identity (1 026 classes) and an adversarial one (16 classes, 1 011
      miners in one of them and the 15 others spread evenly among them). The yardstick is msim_moments_launch
      without a histogram on the same buffer: it reads the same bytes and does far more arithmetic. Bytes moved
      (records read + class records written + the map) over the time, against the float4 copy figure.
  (b) run_classes() with the 3 classes and a 256-bin histogram + error_bars(), against run_moments() with 256 bins
      + error_bars() of the tree --parent-root names (a checkout of the parent commit with its library built: the
      child process of that variant imports the package from there, so library and Python are both the parent's;
      MSIM_LIB still overrides the library). Each variant lives in one child process that is warmed up once at the
      timed shape; the children are then timed alternately --reps times, host clocks around calls that end in a stream synchronise.
      Reported: median and spread (min, max) per variant, and whether run_classes' median is within the parent's
      spread (max - min) of the parent's median.
One JSON line per part."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE_TBS = 6.3  # float4 copy, MI355X
RUNS = 65536


def adversarial_map(m: int, n_classes: int = 16):
    """n_classes - 1 single miners spread evenly over the network, every other miner in the last class."""
    cmap = [n_classes - 1] * m
    step = m // (n_classes - 1)
    for c in range(n_classes - 1):
        cmap[c * step + step // 2] = c
    return cmap


def _events(fn, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def part_a(args, runs):
    import numpy as np
    import torch

    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    dev = torch.device("cuda", 0)
    miners = msim.c5_network()
    m = len(miners)
    sim = msim.Simulation(miners, total_weight=msim.C5_TOTAL_WEIGHT)
    ws = torch.empty(sim.workspace_bytes(runs), dtype=torch.uint8, device=dev)
    sums = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((runs, m, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(runs, dtype=torch.int32, device=dev)
    sim.launch(runs, 0, 1000, sums, ws, status, d_per_run=rec, d_best_height=bh)
    torch.cuda.synchronize()
    assert int(status[1]) == 0
    mom = torch.zeros((m, 20), dtype=torch.int64, device=dev)
    row = {"part": "a", "config": "c5", "runs": runs, "miners": m, "kernel_reps": args.kernel_reps,
           "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS}
    ms = _events(lambda: sim.launch_moments(runs, rec, bh, mom), args.kernel_reps)
    nbytes = runs * (m * 8 + 4)
    yard = statistics.median(ms)
    row["moments_nohist"] = {"median_ms": yard, "min_ms": min(ms), "max_ms": max(ms), "bytes": nbytes,
                             "TBs": nbytes / (yard * 1e-3) / 1e12}
    maps = {"c5_classes": msim.classes_of(miners)[0], "identity": list(range(m)), "adversarial16": adversarial_map(m)}
    for name, cmap in maps.items():
        nc = max(cmap) + 1
        d_map = torch.from_numpy(np.asarray(cmap, dtype=np.uint32).view(np.int32)).to(dev)
        out = torch.empty((runs, nc, 2), dtype=torch.int32, device=dev)
        ms = _events(lambda: sim.launch_fold(runs, rec, d_map, nc, out), args.kernel_reps)
        # one spot check per map, so that a number is never reported for a wrong result
        torch.cuda.synchronize()
        r = rec[:64].cpu().numpy().view(np.uint32).astype(np.uint64)
        want = np.zeros((64, nc, 2), dtype=np.uint64)
        for k, c in enumerate(cmap):
            want[:, c] += r[:, k]
        assert np.array_equal(out[:64].cpu().numpy().view(np.uint32), want.astype(np.uint32)), name
        med = statistics.median(ms)
        nbytes = runs * (m + nc) * 8 + m * 4
        row["fold_" + name] = {"classes": nc, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "bytes": nbytes,
                               "TBs": nbytes / (med * 1e-3) / 1e12, "at_or_below_yardstick": med <= yard}
    return row


def child(which, runs, root):
    """One variant in its own process, on the package of `root`: warm up once, then time one call per line read
    from stdin."""
    sys.path.insert(0, root)
    import torch

    torch.cuda.set_device(0)
    import miningsimulation_amd as msim

    miners = msim.c5_network()
    sim = msim.Simulation(miners, total_weight=msim.C5_TOTAL_WEIGHT)
    spec = msim.HistSpec.covering(0.0, 1.0, 256)
    if which == "classes":
        cmap, _ = msim.classes_of(miners)
        fn = (lambda: msim.error_bars(sim.run_classes(runs, cmap, hist=spec, run_begin=0, seed_base=1000)))
    else:
        fn = (lambda: msim.error_bars(sim.run_moments(runs, 0, 1000, 0, hist=spec)))
    fn()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        print("t", repr(time.perf_counter() - t0), flush=True)


def part_b(args, runs):
    procs = {}
    for which, root in (("parent_run_moments_s", os.path.abspath(args.parent_root)), ("run_classes_s", ROOT)):
        procs[which] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--child", "classes" if which == "run_classes_s" else "moments",
             "--runs", str(runs), "--root", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    times = {k: [] for k in procs}
    try:
        def answer(p, k):  # the child's next protocol line ("ready" or "t <seconds>"); anything else is passed over
            while True:
                line = p.stdout.readline()
                assert line, f"{k}: the child process ended"
                if line.startswith(("ready", "t ")):
                    return line.split()

        for k, p in procs.items():
            assert answer(p, k) == ["ready"], k
        for _ in range(args.reps):  # alternating
            for k, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                times[k].append(float(answer(p, k)[1]))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    row = {"part": "b", "config": "c5", "runs": runs, "classes": 3, "bins": 256, "reps": args.reps,
           "parent_root": os.path.relpath(os.path.abspath(args.parent_root), ROOT)}
    for k, v in times.items():
        row[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    spread = row["parent_run_moments_s"]["max"] - row["parent_run_moments_s"]["min"]
    row["parent_spread_s"] = spread
    row["not_slower_than_parent_plus_spread"] = (row["run_classes_s"]["median"] <=
                                                 row["parent_run_moments_s"]["median"] + spread)
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (part b)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.runs, args.root)
        return
    sys.path.insert(0, ROOT)
    rows = []
    if "b" in args.only.split(","):  # first: its child processes are the only ones with the GPU open
        if not args.parent_root:
            ap.error("part b needs --parent-root")
        rows.append(part_b(args, args.runs))
    if "a" in args.only.split(","):
        import torch

        assert torch.cuda.is_available(), "bench_classes.py needs a GPU"
        torch.cuda.set_device(0)
        rows.append(part_a(args, args.runs))
    sink = open(args.out, "a") if args.out else None
    for row in rows:
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

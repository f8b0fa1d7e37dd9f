"""What exact quantiles cost: the rank selection kernels against the moments kernel over the same records, and
run_quantiles() against run(per_run=True) + numpy.partition of another build.

    python scripts/bench_quantiles.py [--only a,b] [--shapes c2,grid,c5] [--reps 5] [--kernel-reps 10]
                                      [--parent-root DIR] [--out FILE]

  (a) On configs[4] (c5: 1 026 miners) at 65 536 runs, by HIP events over device-resident records, median of
      --kernel-reps: begin + the eight count + step passes of three ranks (0.05, 0.5, 0.95), against
      msim_moments_launch without a histogram on the same buffer (it reads the same bytes once; the selection reads
      them at least eight times). Bytes read (8 x records and best heights) over the time, against the float4 copy
      figure. Then the all-equal single column at 65 536 runs (every key in one bin: same-address LDS atomics),
      against a random single column.
  (b) Per shape (c2 at 32 768 runs, the configs[3] grid at 360 x 8 192, c5 at 65 536), three variants, each in one
      child process that is warmed up once at the timed shape and then timed alternately --reps times (host clocks
      around calls that end in a stream synchronise):
        run          run() of the tree --parent-root names (a checkout of the parent commit with its library built)
        per_run      run(per_run=True) of that tree + numpy.partition at the same ranks of the four quantities
        quantiles    run_quantiles() of this tree
      Reported: median and spread (min, max) per variant, and the condition
        quantiles' median - run's median  <  per_run's median - run's median.
One JSON line per part and shape."""
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
QS = (0.05, 0.5, 0.95)
SHAPES = {"c2": 32768, "grid": 8192, "c5": 65536}


def _events(fn, reps):
    import torch

    for _ in range(2):
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


def _stat(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms)}
    if nbytes is not None:
        out.update(bytes=nbytes, TBs=nbytes / (med * 1e-3) / 1e12)
    return out


def _selection(sim, runs, rec, bh, ranks, columns=None):
    """A callable that runs begin + eight count + step passes, and the tensor its results land in."""
    import torch

    dev = rec.device
    m = columns or len(sim.miners)
    rws = torch.empty(sim.rank_workspace_bytes(len(ranks), columns), dtype=torch.uint8, device=dev)
    out = torch.zeros((m, 4, len(ranks), 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)

    def fn():
        sim.launch_rank_begin(ranks, rws, columns=columns)
        for p in range(8):
            sim.launch_rank_count(runs, rec, bh, p, rws, columns=columns)
            sim.launch_rank_step(p, rws, out, rst, columns=columns)

    return fn, out


def part_a(args):
    import numpy as np
    import torch

    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    runs = SHAPES["c5"]
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
    row = {"part": "a", "config": "c5", "runs": runs, "miners": m, "ranks": len(QS), "kernel_reps": args.kernel_reps,
           "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS}
    nbytes = runs * (m * 8 + 4)
    row["moments_nohist"] = _stat(_events(lambda: sim.launch_moments(runs, rec, bh, mom), args.kernel_reps), nbytes)
    ranks = [msim.quantile_rank(runs, q) for q in QS]
    fn, out = _selection(sim, runs, rec, bh, ranks)
    row["select_8_passes"] = _stat(_events(fn, args.kernel_reps), 8 * nbytes)
    row["select_over_moments"] = row["select_8_passes"]["median_ms"] / row["moments_nohist"]["median_ms"]
    # one spot check, so that a number is never reported for a wrong result: miner 0's found blocks
    torch.cuda.synchronize()
    f0 = np.sort(rec[:, 0, 0].cpu().numpy().view(np.uint32))
    got = out.cpu().numpy()[0, 0, :, 0]
    assert [int(x) for x in got] == [int(f0[r]) for r in ranks], (got, ranks)
    # one column, every key equal, against one random column
    one = msim.Simulation([msim.Miner(0, 100, 1000)])
    single = {}
    for name, col in (("all_equal", np.full((runs, 1, 2), 7, dtype=np.uint32)),
                      ("random", np.random.default_rng(1).integers(0, 50000, size=(runs, 1, 2), dtype=np.uint32))):
        r1 = torch.from_numpy(col.view(np.int32)).to(dev)
        b1 = torch.full((runs,), 60000, dtype=torch.int32, device=dev)
        fn, out = _selection(one, runs, r1, b1, ranks)
        single[name] = _stat(_events(fn, args.kernel_reps), 8 * runs * 12)
        torch.cuda.synchronize()
        srt = np.sort(col[:, 0, 0])
        assert [int(x) for x in out.cpu().numpy()[0, 0, :, 0]] == [int(srt[r]) for r in ranks], name
    row["single_column_65536"] = single
    return row


def _shape(msim, shape):
    """(object with run / run_quantiles, points) of a shape."""
    if shape == "c2":
        return msim.Simulation(msim.PRESETS["c2"]()), 1
    if shape == "c5":
        return msim.Simulation(msim.c5_network(), total_weight=msim.C5_TOTAL_WEIGHT), 1
    grid = msim.c4_grid()
    return msim.Sweep(grid), len(grid)


def child(which, shape, runs, root):
    """One variant in its own process, on the package of `root`: warm up once, then time one call per line read
    from stdin."""
    sys.path.insert(0, root)
    import math

    import numpy as np
    import torch

    torch.cuda.set_device(0)
    import miningsimulation_amd as msim

    job, points = _shape(msim, shape)
    ranks = [max(1, math.ceil(q * runs)) - 1 for q in QS]

    def per_run():
        res = job.run(runs, 0, 1000, 0, per_run=True)
        picked = []
        for r in (res if points > 1 else [res]):
            f, s, L = r.found.astype(np.float64), r.stale.astype(np.float64), r.best_height.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(L[:, None] > 0, f / L[:, None], 0.0)
                rate = np.where(f > 0, s / f, 0.0)
            picked.append([np.partition(x, ranks, axis=0)[ranks] for x in (r.found, r.stale, share, rate)])
        return picked

    fn = {"run": (lambda: job.run(runs, 0, 1000, 0)), "per_run": per_run,
          "quantiles": (lambda: job.run_quantiles(runs, qs=QS, run_begin=0, seed_base=1000))}[which]
    fn()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        print("t", repr(time.perf_counter() - t0), flush=True)


def part_b(args, shape):
    runs = SHAPES[shape]
    parent = os.path.abspath(args.parent_root)
    procs = {}
    for which, root in (("run", parent), ("per_run", parent), ("quantiles", ROOT)):
        procs[which] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--child", which, "--shape", shape, "--runs", str(runs), "--root",
             root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
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
    row = {"part": "b", "shape": shape, "runs_per_point": runs, "qs": list(QS), "reps": args.reps,
           "parent_root": os.path.relpath(parent, ROOT)}
    for k, v in times.items():
        row[k + "_s"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    a, b, c = (row[k + "_s"]["median"] for k in ("run", "per_run", "quantiles"))
    row["quantiles_minus_run_s"] = c - a
    row["per_run_minus_run_s"] = b - a
    row["condition_holds"] = (c - a) < (b - a)
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--shapes", default="c2,grid,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (part b)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--runs", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.shape, args.runs, args.root)
        return
    if args.reps < 3:
        ap.error("--reps is at least 3")
    sys.path.insert(0, ROOT)
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if "b" in args.only.split(","):  # first: its child processes are the only ones with the GPU open
        if not args.parent_root:
            ap.error("part b needs --parent-root")
        for shape in args.shapes.split(","):
            emit(part_b(args, shape))
    if "a" in args.only.split(","):
        import torch

        assert torch.cuda.is_available(), "bench_quantiles.py needs a GPU"
        torch.cuda.set_device(0)
        emit(part_a(args))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

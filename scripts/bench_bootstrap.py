"""What the bootstrap costs: its launches by HIP events, and run_bootstrap() against the parent's run_quantiles() and
the host route through per-run records.

    python scripts/bench_bootstrap.py [--only a,b] [--shapes c2,c5] [--reps 5] [--kernel-reps 10]
                                      [--parent-root DIR] [--variants quantiles,per_run,bootstrap] [--out FILE]

  (a) Per shape (c2 and c5 at 32 768 runs of a year), over device-resident records, by HIP events, median of
      --kernel-reps after two warm-up calls: one msim_boot_count_launch (pass 0, where every key matches, and pass 7
      after a real selection), one msim_boot_step_launch, one msim_boot_below_launch and the whole eight-pass selection
      (timed with its begin, which copies from host memory and is also timed alone and subtracted) for own_bootstrap
      of every miner's share at q = 0.05 with 200 replicates; next to them msim_rank_launch (begin + 8 x (count + step)) for ONE rank on the same records, and
      200 x that time: the naive cost of one selection per replicate, which the shared key and the replicate tile
      are to beat.
  (b) Per shape, three variants, each in a child process that is warmed up once at the timed shape and then timed
      alternately --reps times (host clocks around calls that end synchronised), median with min and max:
        quantiles    run_quantiles(qs=(0.05,)) of the tree --parent-root names (a built checkout of the parent commit)
        per_run      the parent tree's run(per_run=True) plus a numpy Poisson bootstrap of the same statistic on the
                     host: 200 replicates of every miner's q = 0.05 share and its expected shortfall
        bootstrap    this tree's run_bootstrap(qs=(0.05,), replicates=200)
      The condition is (bootstrap - quantiles) < (per_run - quantiles).
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
RUNS = 32768
Q = 0.05
REPLICATES = 200
BOOT_SEED = 12345


def _sim(msim, shape):
    if shape == "c5":
        return msim.Simulation(msim.c5_network(), total_weight=msim.C5_TOTAL_WEIGHT)
    return msim.Simulation(msim.PRESETS[shape]())


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def part_a(args, shape):
    import numpy as np
    import torch

    import miningsimulation_amd as msim
    from miningsimulation_amd import bootstrap as bs

    dev = torch.device("cuda", 0)
    sim = _sim(msim, shape)
    m, B = len(sim.miners), REPLICATES
    ws = torch.empty(sim.workspace_bytes(RUNS), dtype=torch.uint8, device=dev)
    sums = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((RUNS, m, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(RUNS, dtype=torch.int32, device=dev)
    sim.launch(RUNS, 0, 1000, sums, ws, status, d_per_run=rec, d_best_height=bh)
    torch.cuda.synchronize()
    assert int(status[1]) == 0
    del ws
    items = msim.own_bootstrap(1, m, "share", 0)
    d_W = torch.zeros(B, dtype=torch.int64, device=dev)
    row = {"part": "a", "shape": shape, "runs": RUNS, "items": m, "replicates": B, "kernel_reps": args.kernel_reps}
    row["weights"] = _events(lambda: msim.launch_boot_weights(BOOT_SEED, 0, RUNS, B, d_W), args.kernel_reps)
    d_W.zero_()
    msim.launch_boot_weights(BOOT_SEED, 0, RUNS, B, d_W)
    W = d_W.cpu().tolist()
    ranks = msim.boot_ranks(W, (Q,))
    bws = torch.empty(bs.boot_workspace_bytes(m, B), dtype=torch.uint8, device=dev)
    rows = torch.zeros((m, B, 5), dtype=torch.int64, device=dev)
    bst = torch.zeros(1, dtype=torch.int32, device=dev)

    scratch_st = torch.zeros(1, dtype=torch.int32, device=dev)  # a timed step on cleared counts flags every row

    def passes(upto=8, st=scratch_st):
        for p in range(upto):
            sim.launch_boot_count(RUNS, rec, bh, BOOT_SEED, 0, m, B, p, bws)
            sim.launch_boot_step(m, B, p, bws, rows, st)

    def selection():  # begin each time: a finished workspace would match almost no key in the later passes
        sim.launch_boot_begin(items, B, ranks, 1, bws)
        passes()

    row["begin"] = _events(lambda: sim.launch_boot_begin(items, B, ranks, 1, bws), args.kernel_reps)
    row["begin_and_8_passes"] = _events(selection, args.kernel_reps)
    row["selection_8_passes_ms"] = row["begin_and_8_passes"]["median_ms"] - row["begin"]["median_ms"]
    # pass 0 alone (every key matches); the step after it narrows, so begin again before each timed count
    def count0():
        sim.launch_boot_count(RUNS, rec, bh, BOOT_SEED, 0, m, B, 0, bws)

    sim.launch_boot_begin(items, B, ranks, 1, bws)
    row["count_pass0"] = _events(count0, args.kernel_reps)  # the counts pile up; no step reads them
    sim.launch_boot_begin(items, B, ranks, 1, bws)
    passes(7)

    def count7():
        sim.launch_boot_count(RUNS, rec, bh, BOOT_SEED, 0, m, B, 7, bws)

    row["count_pass7"] = _events(count7, args.kernel_reps)
    sim.launch_boot_begin(items, B, ranks, 1, bws)
    passes(7)
    sim.launch_boot_count(RUNS, rec, bh, BOOT_SEED, 0, m, B, 7, bws)
    row["step"] = _events(lambda: sim.launch_boot_step(m, B, 7, bws, rows, scratch_st), args.kernel_reps)
    sim.launch_boot_begin(items, B, ranks, 1, bws)
    passes(st=bst)
    torch.cuda.synchronize()
    first = rows.cpu().numpy().copy()
    row["below"] = _events(lambda: sim.launch_boot_below(RUNS, rec, bh, BOOT_SEED, 0, m, B, bws, rows), args.kernel_reps)
    # one rank through the rank kernels on the same records, and a spot check: replicate 0 is that order statistic
    rank0 = [msim.quantile_rank(RUNS, Q)]
    rws = torch.empty(sim.rank_workspace_bytes(1), dtype=torch.uint8, device=dev)
    out = torch.zeros((m, 4, 1, 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)

    def one_rank():
        sim.launch_rank_begin(rank0, rws)
        for p in range(8):
            sim.launch_rank_count(RUNS, rec, bh, p, rws)
            sim.launch_rank_step(p, rws, out, rst)

    row["rank_one_selection"] = _events(one_rank, args.kernel_reps)
    torch.cuda.synchronize()
    assert first[:, 0, :3].tolist() == out.cpu().numpy()[:, 2, 0, :].tolist() and int(bst[0]) == 0 and int(rst[0]) == 0
    row["naive_B_selections_ms"] = B * row["rank_one_selection"]["median_ms"]
    row["selection_over_naive"] = row["selection_8_passes_ms"] / row["naive_B_selections_ms"]
    return row


def child(which, shape, root):
    """One variant in its own process, on the package of `root`: warm up once, then time one call per line read
    from stdin."""
    sys.path.insert(0, root)
    import math

    import numpy as np
    import torch

    torch.cuda.set_device(0)
    import miningsimulation_amd as msim

    sim = _sim(msim, shape)

    def per_run():
        res = sim.run(RUNS, 0, 1000, 0, per_run=True)
        f, L = res.found.astype(np.float64), res.best_height.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(L[:, None] > 0, f / L[:, None], 0.0)
        order = np.argsort(share, axis=0, kind="stable")
        srt = np.take_along_axis(share, order, axis=0)
        rng = np.random.default_rng(BOOT_SEED)
        cols = np.arange(share.shape[1])
        vals, falls = [], []
        for _ in range(REPLICATES):
            w = rng.poisson(1.0, RUNS)[order].astype(np.float64)  # every run's weight, in each column's sorted order
            cum = np.cumsum(w, axis=0)
            k = np.maximum(1, np.ceil(Q * cum[-1]))
            at = (cum >= k).argmax(axis=0)
            v = srt[at, cols]
            part = np.cumsum(w * srt, axis=0)
            upto = part[at, cols] - (cum[at, cols] - k) * v  # the k smallest, the last tie taken partly
            vals.append(v)
            falls.append(upto / k)
        return np.std(vals, axis=0, ddof=1), np.std(falls, axis=0, ddof=1)

    fn = {"quantiles": (lambda: sim.run_quantiles(RUNS, qs=(Q,), run_begin=0, seed_base=1000)), "per_run": per_run,
          "bootstrap": (lambda: sim.run_bootstrap(RUNS, qs=(Q,), replicates=REPLICATES, boot_seed=BOOT_SEED, run_begin=0,
                                                  seed_base=1000))}[which]
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
    parent = os.path.abspath(args.parent_root)
    procs = {}
    for which, root in (("quantiles", parent), ("per_run", parent), ("bootstrap", ROOT)):
        if which not in args.variants.split(","):
            continue
        procs[which] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--child", which, "--shape", shape, "--root", root],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
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
            print(f"{shape} {k}: warmed up", file=sys.stderr, flush=True)
        for _ in range(args.reps):  # alternating
            for k, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                times[k].append(float(answer(p, k)[1]))
                print(f"{shape} {k}: {times[k][-1]:.4f} s", file=sys.stderr, flush=True)  # the host route takes minutes
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    row = {"part": "b", "shape": shape, "runs": RUNS, "q": Q, "replicates": REPLICATES, "reps": args.reps,
           "parent_root": os.path.relpath(parent, ROOT)}
    for k, v in times.items():
        row[k + "_s"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if len(times) < 3:  # a subset of the variants: the times only
        return row
    a, b, c = (row[k + "_s"]["median"] for k in ("quantiles", "per_run", "bootstrap"))
    row["bootstrap_minus_quantiles_s"] = c - a
    row["per_run_minus_quantiles_s"] = b - a
    row["condition_holds"] = (c - a) < (b - a)
    # the only margin asked: the spreads must not bridge the gap
    row["holds_beyond_spread"] = (row["bootstrap_s"]["max"] - row["quantiles_s"]["min"]) < \
                                 (row["per_run_s"]["min"] - row["quantiles_s"]["max"])
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--shapes", default="c2,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (part b)")
    ap.add_argument("--variants", default="quantiles,per_run,bootstrap",
                    help="part b: which variants to time (the host route takes minutes on c5)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.shape, args.root)
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

        assert torch.cuda.is_available(), "bench_bootstrap.py needs a GPU"
        torch.cuda.set_device(0)
        for shape in args.shapes.split(","):
            emit(part_a(args, shape))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

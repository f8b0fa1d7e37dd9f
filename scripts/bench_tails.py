"""What tail statistics cost: the tail kernel against the cross kernel over the same records, and run_tails() against
run_quantiles() with the same ranks.

    python scripts/bench_tails.py [--only a,b] [--shapes c2,c5] [--reps 5] [--kernel-reps 10] [--out FILE]

  (a) On configs[4] (c5: 1 026 miners) at 32 768 runs, by HIP events over device-resident records, median of
      --kernel-reps after two warm-up calls: msim_tail_launch with the 1 026 own-tail items at q = 0.05 (every
      column's own share; thresholds from msim_rank_launch on the same records) against msim_cross_launch with the
      1 026 self-pairs, the nearest existing yardstick (same grid shape, two to four divisions per run), and
      msim_moments_launch without a histogram. The tail launch is also timed at q = 0.5 and q = 1 (every run
      accepted: the full moments work per item).
  (b) Per shape (c2 and c5 at 32 768 runs of a year), run_quantiles(qs=(0.05,)) and run_tails(q=0.05) of this tree,
      warmed up once at the timed shape and then timed alternately --reps times by host clocks around the calls
      (both end in a stream synchronise). run_quantiles is the parent's code path unchanged (the driver's tail job
      is null), so the difference is what the tail stage adds: one msim_moments_launch per chunk, the items'
      upload, one msim_tail_launch per resident buffer and the copies back.
One JSON line per part and shape."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 32768


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


def part_a(args):
    import numpy as np
    import torch

    import miningsimulation_amd as msim
    from miningsimulation_amd import tails

    dev = torch.device("cuda", 0)
    miners = msim.c5_network()
    m = len(miners)
    sim = msim.Simulation(miners, total_weight=msim.C5_TOTAL_WEIGHT)
    ws = torch.empty(sim.workspace_bytes(RUNS), dtype=torch.uint8, device=dev)
    sums = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((RUNS, m, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(RUNS, dtype=torch.int32, device=dev)
    sim.launch(RUNS, 0, 1000, sums, ws, status, d_per_run=rec, d_best_height=bh)
    torch.cuda.synchronize()
    assert int(status[1]) == 0
    qs = (0.05, 0.5, 1.0)
    ranks = [msim.quantile_rank(RUNS, q) for q in qs]
    rws = torch.empty(sim.rank_workspace_bytes(len(ranks)), dtype=torch.uint8, device=dev)
    out = torch.zeros((m, 4, len(ranks), 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)
    sim.launch_rank_begin(ranks, rws)
    for p in range(8):
        sim.launch_rank_count(RUNS, rec, bh, p, rws)
        sim.launch_rank_step(p, rws, out, rst)
    torch.cuda.synchronize()
    order = msim.order_stats_from_words(out.cpu().numpy(), 1, m, len(ranks))
    row = {"part": "a", "config": "c5", "runs": RUNS, "items": m, "kernel_reps": args.kernel_reps}
    d_tails = torch.zeros((m, tails.TAIL_WORDS), dtype=torch.int64, device=dev)
    for j, q in enumerate(qs):
        items = tails.items_from_specs(msim.own_tails(1, m, "share", j), order)
        d_items = torch.from_numpy(msim.items_words(items).view(np.int32)).to(dev)
        row[f"tail_q{q:g}"] = _events(lambda: sim.launch_tails(RUNS, rec, bh, d_items, m, d_tails), args.kernel_reps)
        torch.cuda.synchronize()
        # a spot check, so that a number is never reported for a wrong result: the counts are the selection's
        got = d_tails.cpu().numpy()[:, :2].tolist()
        assert got == [[order[0][k][2][j].below, order[0][k][2][j].equal] for k in range(m)], q
    pairs = torch.from_numpy(np.array([[0, k, 0, k] for k in range(m)], dtype=np.uint32).view(np.int32)).to(dev)
    d_cross = torch.zeros((m, 12), dtype=torch.int64, device=dev)
    row["cross_self_pairs"] = _events(lambda: sim.launch_cross(RUNS, rec, bh, pairs, m, d_cross), args.kernel_reps)
    mom = torch.zeros((m, 20), dtype=torch.int64, device=dev)
    row["moments_nohist"] = _events(lambda: sim.launch_moments(RUNS, rec, bh, mom), args.kernel_reps)
    row["tail_q0.05_over_cross"] = row["tail_q0.05"]["median_ms"] / row["cross_self_pairs"]["median_ms"]
    return row


def part_b(args, shape):
    import torch

    import miningsimulation_amd as msim

    sim = (msim.Simulation(msim.c5_network(), total_weight=msim.C5_TOTAL_WEIGHT) if shape == "c5"
           else msim.Simulation(msim.PRESETS[shape]()))
    fns = {"quantiles": (lambda: sim.run_quantiles(RUNS, qs=(0.05,), run_begin=0, seed_base=1000)),
           "tails": (lambda: sim.run_tails(RUNS, q=0.05, run_begin=0, seed_base=1000))}
    times = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    for _ in range(args.reps):  # alternating
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    row = {"part": "b", "shape": shape, "runs": RUNS, "q": 0.05, "reps": args.reps}
    for k, v in times.items():
        row[k + "_s"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    row["tails_minus_quantiles_s"] = row["tails_s"]["median"] - row["quantiles_s"]["median"]
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--shapes", default="c2,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps is at least 3")
    sys.path.insert(0, ROOT)
    import torch

    assert torch.cuda.is_available(), "bench_tails.py needs a GPU"
    torch.cuda.set_device(0)
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if "a" in args.only.split(","):
        emit(part_a(args))
    if "b" in args.only.split(","):
        for shape in args.shapes.split(","):
            emit(part_b(args, shape))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

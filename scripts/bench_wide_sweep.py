"""What a propagation sweep of a large network costs in the shared-draw form (one W1 pass per draw group,
DESIGN.md §3.4b) against the plain large-network pipeline, on c5_network() at P uniform delays.

    python scripts/bench_wide_sweep.py --points 8 [--runs 32768] [--months 12] [--reps 3] [--out FILE]

P = 3 is 10 s, 1 s, 100 ms; any other P is log-spaced from 100 ms to 10 s (the lists of bench_honest_sweep.py).
Timed, by HIP events around the launch on one stream:
  (s) Sweep.launch of the shared-draw sweep                                    the code under test
  (a) Sweep.launch of the same points with flags 0: one wide launch per point  reported (new code too)
  (b) P Simulation.launch steps, one per point, one after another              the yardstick
Every variant is warmed up once at the timed shape, then the variants are timed alternately `--reps` times; medians
and spreads are reported, with the run-years per second of each. `--only s` (or a, b, or a list) times only those
variants, e.g. for a kernel trace of the shared form alone. One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)



def delays(p: int):
    if p == 3:
        return [10_000, 1_000, 100]
    if p == 1:
        return [10_000]
    return [int(round(100 * 100 ** (i / (p - 1)))) for i in range(p - 1, -1, -1)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--runs", type=int, default=32768)
    ap.add_argument("--months", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="s,a,b")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    assert torch.cuda.is_available(), "bench_wide_sweep.py needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    duration = msim.SIM_DURATION_MS * args.months // 12
    ds = delays(args.points)
    P, runs, W = len(ds), args.runs, msim.C5_TOTAL_WEIGHT
    m = len(msim.c5_network())
    only = set(args.only.split(","))
    row = {"points": P, "delays_ms": ds, "runs_per_point": runs, "months": args.months, "miners": m,
           "lib": os.path.relpath(_lib.LIB_PATH, ROOT)}
    sums = torch.zeros((P, m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    variants, keep, check = {}, [], {}

    if "s" in only:
        sw = msim.propagation_sweep(msim.c5_network(), ds, duration, total_weight=W)
        row["plan"] = sw.plan(runs)
        assert row["plan"]["engine"] == 2 and row["plan"]["draw_groups"] == 1, row["plan"]
        ws = torch.empty(sw.workspace_bytes(runs), dtype=torch.uint8, device=dev)
        s_sums = torch.zeros_like(sums)
        keep += [sw, ws]
        variants["shared"] = lambda: sw.launch(runs, 0, 1000, s_sums, ws, status)
        check["shared"] = s_sums
    if "a" in only:
        sa = msim.Sweep([msim.c5_network(d) for d in ds], duration, total_weight=W)
        assert sa.plan(runs)["engine"] == 2 and sa.plan(runs)["draw_groups"] == P
        wa = torch.empty(sa.workspace_bytes(runs), dtype=torch.uint8, device=dev)
        a_sums = torch.zeros_like(sums)
        keep += [sa, wa]
        variants["per_point"] = lambda: sa.launch(runs, 0, 1000, a_sums, wa, status)
        check["per_point"] = a_sums
    if "b" in only:
        sims = [msim.Simulation(msim.c5_network(d), duration, total_weight=W) for d in ds]
        wb = torch.empty(max(s.workspace_bytes(runs) for s in sims), dtype=torch.uint8, device=dev)
        b_sums = torch.zeros_like(sums)
        keep += [sims, wb]

        def serial():
            for p, s in enumerate(sims):
                s.launch(runs, 0, 1000, b_sums[p], wb, status)

        variants["serial"] = serial
        check["serial"] = b_sums

    for fn in variants.values():  # warm-up at the timed shape (tables uploaded, kernels loaded)
        fn()
    torch.cuda.synchronize()
    assert status.cpu().tolist()[1] == 0, "a run failed"
    ref = None
    for k, t in check.items():  # every variant computes the same sums
        if ref is None:
            ref = t.cpu()
        else:
            assert torch.equal(ref, t.cpu()), f"{k}: sums differ"
    ms = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    run_years = P * runs * args.months / 12
    for k, v in ms.items():
        med = statistics.median(v)
        row[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "run_years_per_s": run_years / (med * 1e-3)}
    if "shared" in row and "serial" in row:
        row["serial_over_shared"] = row["serial"]["median_ms"] / row["shared"]["median_ms"]
    if "shared" in row and "per_point" in row:
        row["per_point_over_shared"] = row["per_point"]["median_ms"] / row["shared"]["median_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

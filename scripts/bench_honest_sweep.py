"""What a propagation sweep costs in the shared-draw form (Sweep(..., shared_draws=True): one draw pass per draw
group) against its two yardsticks, on one network at P uniform delays.

    python scripts/bench_honest_sweep.py --points 8 [--runs 32768] [--months 12] [--reps 3] [--out FILE]

The network is setup_miners(); P = 3 is the README's example (10 s, 1 s, 100 ms), any other P is log-spaced from
100 ms to 10 s. Timed, by HIP events around the launch on one stream:
  (s) Sweep.launch of the shared-draw sweep                                    the code under test
  (a) Sweep.launch of the same points without the flag: the per-lane kernel    yardstick (a)
  (b) P Simulation.launch steps, one per point, one after another              yardstick (b)
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

    assert torch.cuda.is_available(), "bench_honest_sweep.py needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    duration = msim.SIM_DURATION_MS * args.months // 12
    ds = delays(args.points)
    P, runs = len(ds), args.runs
    base = msim.setup_miners()
    m = len(base)
    only = set(args.only.split(","))
    row = {"points": P, "delays_ms": ds, "runs_per_point": runs, "months": args.months, "miners": m,
           "lib": os.path.relpath(_lib.LIB_PATH, ROOT)}
    sums = torch.zeros((P, m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    variants, keep, check = {}, [], {}

    if "s" in only:
        sw = msim.propagation_sweep(base, ds, duration)
        row["plan"] = sw.plan(runs)
        assert row["plan"]["engine"] == 1, row["plan"]
        ws = torch.empty(sw.workspace_bytes(runs), dtype=torch.uint8, device=dev)
        s_sums = torch.zeros_like(sums)
        keep += [sw, ws]
        variants["shared"] = lambda: sw.launch(runs, 0, 1000, s_sums, ws, status)
        check["shared"] = s_sums
    if "a" in only:
        sa = msim.Sweep([msim.setup_miners(d) for d in ds], duration)
        assert sa.plan(runs)["engine"] == 0
        wa = torch.empty(sa.workspace_bytes(runs), dtype=torch.uint8, device=dev)
        a_sums = torch.zeros_like(sums)
        keep += [sa, wa]
        variants["per_lane"] = lambda: sa.launch(runs, 0, 1000, a_sums, wa, status)
        check["per_lane"] = a_sums
    if "b" in only:
        sims = [msim.Simulation(msim.setup_miners(d), duration) for d in ds]
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
    if "shared" in row and "per_lane" in row:
        row["per_lane_over_shared"] = row["per_lane"]["median_ms"] / row["shared"]["median_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

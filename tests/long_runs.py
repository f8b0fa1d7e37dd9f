"""Runs longer than a year: the cases of tests/test_long_runs_host.py and tests/test_gpu_long_runs.py, and the generator
of their expected values, tests/golden/long_runs.json.

Every other test simulates at most one year (about 52 600 blocks). Several engines keep per-run state in 16-bit
fields: the honest pipeline's per-segment owner counts (msim_pipeline.h CNT_WORDS, u16 pairs), the settled form's
pend[] / stp[] behind the guards of msim_selm.h. The cases here cross those widths: a miner that owns more than 65 535
blocks of a run, a segment of the longest length the planner lays out, a selfish run whose best height passes 0xFF00
with almost no hand-over to the engine, and one whose honest chain passes 0xFFF0.

Run as a script, the module records the oracle's (oracle/msim_oracle.c through pyoracle.run_batch: never code under
test) per-run found, stale and best height of every case:

    python tests/long_runs.py            # rewrites tests/golden/long_runs.json

The oracle is quadratic in the length of a withheld chain (a 60 %-selfish run of 3.5 years takes tens of seconds), so
the tests read the file; tests/test_long_runs_reference.py recomputes two cheap cases against it. The best height is
the sum of a run's found counters (every case has distinct miner ids: each block of the best chain is found by one
miner); the recorder checks that against the oracle's own share = found / best height."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "long_runs.json")

Y = 31_556_952_000
BASE = 1000
H9 = [30, 29, 12, 11, 8, 5, 3, 1, 1]            # configs[0] / configs[1]
C3 = [40, 19, 12, 11, 8, 5, 3, 1, 1]            # configs[2]: miner 0 selfish
C5 = [30720, 29696] + [41] * 1024               # configs[4], W = 102 400
POOLS = [70000, 30000] + [75] * 32              # two pools and 32 small miners, W = 102 400
PIPE_MAX_SEG = 65_535 // 32 * 32                # msim_pipeline.h: the longest segment the planner lays out
# honest_100's duration: the longest whose run of pipe_need(D) blocks the planner, at one wave slot (MSIM_K1_SLOTS=1,
# two launches in flight) and 257 runs, cuts into TWO segments, which are then PIPE_MAX_SEG blocks long (found by scanning msim_pipeline_info on the CPU;
# tests/test_long_runs_host.py asserts the plan)
HONEST_100_MS = 76_848_000_000


def _case(weights, delay, duration, runs, selfish=None, W=100):
    return {"weights": list(weights), "delays": [delay] * len(weights), "selfish": [k == selfish for k in range(len(weights))],
            "W": W, "duration": int(duration), "runs": runs, "base": BASE}


CASES = {
    "honest_100": _case([100], 0, HONEST_100_MS, 257),
    "honest_100_parent": _case([100], 0, Y * 14 // 10, 257),
    "honest_70_30": _case([70, 30], 100, 2 * Y, 257),
    "honest_h9_10s": _case(H9, 10_000, Y * 9 // 2, 64),  # 4.5 years: the 30 % miner passes 65 535 blocks
    "honest_70_30_10s": _case([70, 30], 10_000, 2 * Y, 64),  # the other point of the shared-draw sweep
    "selfish_flush": _case([40, 35, 25], 1, Y * 5 // 2, 64, selfish=0),
    "selfish_majority": _case([60, 25, 15], 100, Y * 7 // 2, 8, selfish=0),
    "selfish_c3_long": _case(C3, 1000, 2 * Y, 64, selfish=0),
    # at 10 s and 4 years the candidates of a run outgrow W3's LDS (msim_api.hip: wide_w3_lds past 160 KiB), so the
    # library runs wide_pools on the general engine, minutes for one lane: the host body of the large-network pipeline
    # runs it, the device runs the same network at 5 s, the largest of 10 / 5 / 3 / 2 / 1 s that W1-W3 serve
    "wide_pools": _case(POOLS, 10_000, 4 * Y, 32, W=102_400),
    "wide_pools_5s": _case(POOLS, 5_000, 4 * Y, 32, W=102_400),
    "wide_c5": _case(C5, 1000, Y * 14 // 10, 32, W=102_400),
}
HONEST = ("honest_100", "honest_100_parent", "honest_70_30", "honest_h9_10s")  # run alone on the pipeline
SELFISH = ("selfish_flush", "selfish_majority", "selfish_c3_long")
WIDE = ("wide_pools", "wide_pools_5s", "wide_c5")
WIDE_ON_DEVICE = ("wide_pools_5s", "wide_c5")  # the large-network pipeline serves them on the device
CHEAP = ("honest_70_30", "selfish_c3_long")  # recomputed by tests/test_long_runs_reference.py


def oracle_counters(pyoracle, c, runs=None, threads=16):
    """(found [n, M], stale [n, M], best height [n]) of a case's first `runs` runs, from the oracle."""
    n = c["runs"] if runs is None else runs
    f, s, share, _ = pyoracle.run_batch(c["weights"], c["delays"], c["selfish"], c["duration"], n, 0, c["base"],
                                        threads=threads, total_weight=c["W"])
    L = f.sum(axis=1)
    some = f > 0
    assert np.array_equal(share[some], (f / np.maximum(L, 1)[:, None])[some]), "best height is not the sum of found"
    return f, s, L


_EXPECTED = {}


def expected(name, runs=None):
    """The recorded (found [n, M], stale [n, M], best height [n]) of a case as read-only int64 arrays; with `runs`,
    of its first runs."""
    if not _EXPECTED:
        with open(GOLDEN) as fh:
            doc = json.load(fh)
        for k, c in CASES.items():
            rec = doc["cases"][k]
            assert rec["case"] == c, f"{k}: tests/golden/long_runs.json was recorded for another case; record it again"
            f = np.array(rec["found"], dtype=np.int64).reshape(c["runs"], len(c["weights"]))
            s = np.array(rec["stale"], dtype=np.int64).reshape(c["runs"], len(c["weights"]))
            L = np.array(rec["best_height"], dtype=np.int64)
            for a in (f, s, L):
                a.setflags(write=False)
            _EXPECTED[k] = (f, s, L)
    f, s, L = _EXPECTED[name]
    return (f, s, L) if runs is None else (f[:runs], s[:runs], L[:runs])


def miners(msim, c, delay=None):
    """The case's network as msim.Miner objects (delay: every miner's propagation instead of the case's)."""
    return [msim.Miner(k, c["weights"][k], c["delays"][k] if delay is None else delay, c["selfish"][k])
            for k in range(len(c["weights"]))]


def record():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import pyoracle

    doc = {"cases": {}}
    for name, c in CASES.items():
        f, s, L = oracle_counters(pyoracle, c)
        doc["cases"][name] = {"case": c, "found": f.ravel().tolist(), "stale": s.ravel().tolist(),
                              "best_height": L.tolist()}
        print(f"{name}: best height {int(L.min())}..{int(L.max())}, largest found {int(f.max())}", flush=True)
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    record()

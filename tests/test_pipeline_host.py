"""The event-skipping pipeline (miningsimulation_amd/csrc/msim_pipeline.h) executed on the host from the
SAME lane bodies the gfx950 kernels run (tests/native/pipeline_host.cpp, test-only), against the oracle.

It checks the decomposition itself — jump-ahead states vs sequential stepping, fast/slow blocks, episodes
from quiet states, the end-of-run search and the last-block correction — bit-exactly on CPU-only hosts;
tests/test_gpu_parity.py checks the device build of the same code against the same oracle."""
import random
import subprocess

import numpy as np
import pytest

import pipeline_host_lib

D = 31_556_952_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def pipe(native_tests):
    return pipeline_host_lib.load(native_tests["pipeline_host"])


def _check(pipe, oracle, percs, props, duration, n, base=1000, begin=0, cap=0, need_all_ok=True, slots=8192, **over):
    f, s, ok, ne = pipe(percs, props, duration, n, base, begin, cap, slots, **over)
    of, os_, _, _ = oracle.run_batch(percs, props, [0] * len(percs), duration, n, begin, base, threads=8)
    if need_all_ok:
        assert ok.all(), f"{(~ok).sum()} runs flagged for retry"
    assert np.array_equal(f[ok], of[ok]), (percs, props, duration)
    assert np.array_equal(s[ok], os_[ok]), (percs, props, duration)
    return ok, ne


@pytest.mark.parametrize("prop", [0, 1, 100, 1000, 10_000, 30_000])
def test_presets_full_year(pipe, oracle, prop):
    _check(pipe, oracle, H, [prop] * 9, D, 12)


@pytest.mark.parametrize("slots", [1, 64, 5000, 10**6])
def test_worker_geometries(pipe, oracle, slots):
    """Segment lengths from one worker per run (no jump) to the shortest allowed workers."""
    _check(pipe, oracle, H, [1000] * 9, D, 8, slots=slots)


def _rand_percs(m, rng):
    cuts = sorted(rng.sample(range(1, 100), m - 1)) if m > 1 else []
    b = [0] + cuts + [100]
    return [b[i + 1] - b[i] for i in range(m)]


@pytest.mark.parametrize("seed", range(4))
def test_random_networks(pipe, oracle, seed):
    """Heterogeneous propagation (incl. 0 ms), zero-percent miners, 1..15 miners, random run ranges."""
    rng = random.Random(77 + seed)
    for _ in range(6):
        m = rng.randint(1, 15)
        percs = _rand_percs(m, rng)
        if m > 2 and rng.random() < 0.3:
            percs[rng.randrange(m)] += percs[0]
            percs[0] = 0
        props = [rng.choice([0, 1, 7, 250, 2000, 12_000, 45_000]) for _ in range(m)]
        dur = rng.choice([D, D // 3, 86_400_000 * 30])
        _check(pipe, oracle, percs, props, dur, 4, base=rng.randrange(2**32), begin=rng.randrange(10**9))


@pytest.mark.parametrize("dur", [0, 1, 599_999, 600_000, 3_600_000, 25_000_000, 250_000_000])
def test_short_durations(pipe, oracle, dur):
    """Runs that end before the first block, inside the first segment, or after a handful of blocks."""
    _check(pipe, oracle, H, [10_000] * 9, dur, 64)


def test_capacity_overflow_is_flagged(pipe, oracle):
    """With one slot per segment, runs with more slow blocks must be flagged, never mis-counted."""
    ok, _ = _check(pipe, oracle, H, [10_000] * 9, D, 8, cap=1, need_all_ok=False)
    assert not ok.all()


# ------------------------------------------------------------------ lowered capacities (tests/test_gpu_pipe_overflow.py
# sets the same values on the device through MSIM_PIPE_TEST_*). 257 runs of 10^9 ms at seed base 1000; flagged runs
# are a subset of the runs and every unflagged run is exact (_check compares f[ok] with the oracle run by run).
N_OVER = 257
D9 = 10**9
RHO_10S = 1.0 - np.exp(-10_001 / 599_999.5)  # P(a block of a 10 s network is not fast)
W_M = {1: [100], 2: [70, 30], 15: [20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1]}


def test_explicit_geometry_is_the_layouts(pipe, oracle):
    """nseg and seg given explicitly (the device's, from msim_pipeline_info) give the run the helper's own choice
    gives: 4 workers of 544 blocks for 10^9 ms at any slot count of 32 or more."""
    a = pipe(H, [10_000] * 9, D9, 64, cap=13, detail=True)
    b = pipe(H, [10_000] * 9, D9, 64, cap=13, nseg=4, seg=544, detail=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _check(pipe, oracle, H, [10_000] * 9, D9, 64, nseg=2, seg=1056)
    _check(pipe, oracle, H, [10_000] * 9, D9, 64, nseg=1, seg=2080)


@pytest.mark.parametrize("cap,flagged", [(1, 257), (8, 247), (12, 104), (13, 74), (14, 51), (16, 9)])
def test_slot_capacity_overflow_counts(pipe, oracle, cap, flagged):
    """13 and 16 are ceil(lam + 1.3 sqrt(lam)) and ceil(lam + 2.3 sqrt(lam)) at lam = rho * 544 = 8.99. The counts are
    the host's at 4 workers of 544 blocks (the flagged set is a function of the draws and the geometry alone)."""
    assert pipeline_host_lib.sigma_cap(RHO_10S * 544, 1.3) == 13 and pipeline_host_lib.sigma_cap(RHO_10S * 544, 2.3) == 16
    ok, _ = _check(pipe, oracle, H, [10_000] * 9, D9, N_OVER, cap=cap, need_all_ok=False, nseg=4, seg=544)
    assert int((~ok).sum()) == flagged


def test_list_capacity_overflow(pipe, oracle):
    """lcap 1 flags every run that lists a block; half the list count flags the runs appended past it (the host
    appends run by run, so the later runs; the device's order differs, its results may not)."""
    f, s, ok0, ne, listed, _ = pipe(H, [10_000] * 9, D9, N_OVER, detail=True)
    assert ok0.all() and ne == 9454
    ok, ne1 = _check(pipe, oracle, H, [10_000] * 9, D9, N_OVER, lcap=1, need_all_ok=False)
    assert ne1 == ne, "the list count keeps growing past lcap"
    assert np.array_equal(~ok[1:], listed[1:] > 0) and (listed > 0).all() and not ok[0]
    ok, _ = _check(pipe, oracle, H, [10_000] * 9, D9, N_OVER, lcap=ne // 2, need_all_ok=False)
    assert 0 < (~ok).sum() < N_OVER and ok[:100].all() and not ok[-100:].any()


@pytest.mark.parametrize("percs,duration,flagged,one_read", [
    ([100], 5 * D9, 98, "all"), ([70, 30], 5 * D9, 31, "all"),
    ([100], D9, 24, "all"), ([70, 30], D9, 7, "all"),
    ([100], D9 // 10, 2, "none"), ([70, 30], D9 // 10, 1, "none")])
def test_lean_k2_errors_are_flagged(pipe, oracle, percs, duration, flagged, one_read):
    """45 s delays on K2's lean state machine (2 in-flight blocks): an episode that outgrows it sets REC_ERR and K3
    flags the run, on its one-read path (more than 32 listed blocks up to the end of the run: every run at 5*10^9 and
    at 10^9 ms, which list 93 or more) and on its batched path (the flagged runs at 10^8 ms). The network's own mid
    machine flags nothing."""
    props = [45_000] * len(percs)
    ok, _ = _check(pipe, oracle, percs, props, duration, N_OVER)
    assert ok.all()
    f, s, ok, ne, listed, onepath = pipe(percs, props, duration, N_OVER, kind=0, detail=True)
    _check(pipe, oracle, percs, props, duration, N_OVER, kind=0, need_all_ok=False)
    assert int((~ok).sum()) == flagged
    assert np.array_equal(onepath, listed > 32)
    assert onepath.all() if one_read == "all" else not onepath[~ok].any()


@pytest.mark.parametrize("m", [1, 2, 15])
def test_overflows_at_other_miner_counts(pipe, oracle, m):
    props = [10_000] * m
    ok, ne = _check(pipe, oracle, W_M[m], props, D9, N_OVER, cap=13, need_all_ok=False, nseg=4, seg=544)
    assert int((~ok).sum()) == 74  # uniform delays: the listing depends on the intervals alone
    ok, _ = _check(pipe, oracle, W_M[m], props, D9, N_OVER, lcap=ne // 2, need_all_ok=False)
    assert 0 < (~ok).sum() < N_OVER


def test_lane_bodies_at_lowered_capacities_under_sanitizers():
    """build/pipe_overflow_check: K1's, S1's, K2's and K3's lane bodies with every buffer at exactly the lowered cap,
    lcap and point capacities, under ASan + UBSan."""
    r = subprocess.run([pipeline_host_lib.ensure_check()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")

"""Runs longer than a year on the CPU: the host builds of every engine's lane bodies against the recorded oracle
counters of tests/long_runs.py, and the planner's segment bound over a grid of durations, run counts, wave slots and
launches in flight (host-only entry points: no device is touched).

The honest pipeline packs a segment's per-owner counts as u16 pairs (msim_pipeline.h CNT_WORDS), so a segment holds
at most 65 535 blocks; msim_pipeline.h pipe_workers keeps every plan at or below PIPE_MAX_SEG = 65 504. The pipeline
cases run the host bodies at the geometry msim_pipeline_info gives under MSIM_K1_SLOTS=1 (the fewest workers the
planner allows): planned as one segment of 75 872 blocks, `honest_100_parent` loses 65 536 blocks of its only miner
and flags nothing.

The preconditions (a miner past 65 535 blocks, a segment at the bound, best heights past the settled form's guards)
are asserted from the expected values, so no case passes without crossing the width it is here for."""
import ctypes
import math

import numpy as np
import pytest

import host_plans
import long_runs
import pipeline_host_lib
from long_runs import CASES, Y

U16 = 65_535


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import miningsimulation_amd as m

    return m


def pipe_need(duration_ms):
    """msim_pipeline.h pipe_need: the blocks pre-generated per run."""
    mu = duration_ms / 599_999.5
    return mu + 8.0 * math.sqrt(max(mu, 1.0)) + 64.0


def slots_1_plan(msim, name, runs=None, duration=None):
    """msim_pipeline_info of a case planned for ONE wave slot, the fewest and longest segments the planner lays out:
    MSIM_K1_SLOTS=1 with two launches in flight (one launch in flight plans three rounds of the slots, i.e. three)."""
    c = CASES[name]
    with host_plans._env({"MSIM_K1_SLOTS": "1"}):
        sim = msim.Simulation(long_runs.miners(msim, c), duration or c["duration"], c["W"])
        sim.set_concurrent_launches(2)
        return sim.pipeline_info(runs or c["runs"])


# ------------------------------------------------------------------ preconditions, from the expected values
@pytest.mark.parametrize("name", long_runs.HONEST)
def test_honest_cases_pass_the_u16_width(name):
    f, _, _ = long_runs.expected(name)
    assert f.max(axis=1).min() > U16, "every run must give one miner more than 65 535 blocks"


def test_honest_100_fills_the_longest_segment(msim):
    """The only miner owns every block, so a full segment's count is segment_blocks itself: the planner's bound, and
    two such segments (the run ends in the second)."""
    info = slots_1_plan(msim, "honest_100")
    assert info["uses_pipeline"] == 1 and info["segments"] == 2, info
    assert info["segment_blocks"] == long_runs.PIPE_MAX_SEG and U16 - info["segment_blocks"] < 32
    f, _, _ = long_runs.expected("honest_100")
    assert f.min() > info["segment_blocks"], "every run fills its first segment"
    # 1 000 s more needs a third segment: this is the longest two-segment run
    nxt = slots_1_plan(msim, "honest_100", duration=CASES["honest_100"]["duration"] + 1_000_000)
    assert nxt["segments"] == 3 and nxt["segment_blocks"] < info["segment_blocks"], nxt


def test_selfish_cases_pass_the_settled_forms_guards():
    _, _, L = long_runs.expected("selfish_flush")
    assert L.min() >= 70_000  # 0xFF00 plus the hand-overs (about 0.2 a year at 1 ms)
    f, _, _ = long_runs.expected("selfish_majority")
    assert f[:, 1:].sum(axis=1).min() >= 0xFFF0 and f[:, 0].max() < 1000


def test_wide_pools_pass_the_u16_width():
    for name in ("wide_pools", "wide_pools_5s"):
        f, _, _ = long_runs.expected(name)
        assert f[:, 0].min() > U16


# ------------------------------------------------------------------ host bodies against the expected values
@pytest.fixture(scope="module")
def pipe(native_tests):
    return pipeline_host_lib.load(native_tests["pipeline_host"])


@pytest.mark.parametrize("name", long_runs.HONEST)
def test_pipeline_host(msim, pipe, name):
    """K1's, K2's and K3's lane bodies at the plan of one wave slot."""
    c = CASES[name]
    info = slots_1_plan(msim, name)
    assert info["uses_pipeline"] == 1 and info["segment_blocks"] <= U16, info
    f, s, ok, _ = pipe(c["weights"], c["delays"], c["duration"], c["runs"], c["base"], nseg=info["segments"],
                       seg=info["segment_blocks"])
    ef, es, _ = long_runs.expected(name)
    assert ok.all(), f"{int((~ok).sum())} runs flagged"
    assert np.array_equal(f, ef), (info, f[0].tolist(), ef[0].tolist())
    assert np.array_equal(s, es)


def _per_run(lib_fn, c, runs, *extra):
    m = len(c["weights"])
    F, S, L, E = [], [], [], []
    for r in range(runs):
        f, s = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        bh, err = ctypes.c_uint32(), ctypes.c_uint32()
        rc = lib_fn(f, s, bh, err, c["base"] + 2 * r, c["base"] + 2 * r + 1, *extra)
        assert rc == 0
        F.append(list(f)), S.append(list(s)), L.append(bh.value), E.append(err.value)
    return np.array(F, dtype=np.int64), np.array(S, dtype=np.int64), np.array(L, dtype=np.int64), np.array(E)


def _arrays(c):
    m = len(c["weights"])
    return ((ctypes.c_uint64 * m)(*c["weights"]), (ctypes.c_int64 * m)(*c["delays"]),
            (ctypes.c_uint8 * m)(*[1 if x else 0 for x in c["selfish"]]), m)


@pytest.mark.parametrize("caps", [10, 1], ids=["mixed", "engine"])
@pytest.mark.parametrize("name", long_runs.SELFISH)
def test_sel_host(native_tests, name, caps):
    """The settled form with the engine at the device's capacities (E1's schedule for one lane), and the engine alone
    at the retry kernel's."""
    lib = ctypes.CDLL(native_tests["sel_host"])
    lib.sel_set_fold_every.argtypes = [ctypes.c_uint32]
    lib.sel_set_fold_every(0)
    c = CASES[name]
    w, p, sf, m = _arrays(c)
    fn = lambda f, s, bh, err, si, sp: lib.sel_run(w, p, sf, m, ctypes.c_uint64(c["W"]), ctypes.c_int64(c["duration"]),
                                                    ctypes.c_uint32(si), ctypes.c_uint32(sp), caps, f, s,
                                                    ctypes.byref(bh), ctypes.byref(err))
    f, s, L, err = _per_run(fn, c, c["runs"])
    ef, es, eL = long_runs.expected(name)
    assert not err.any(), err.tolist()
    assert np.array_equal(f, ef) and np.array_equal(s, es) and np.array_equal(L, eL)


def test_general_engine_refuses_a_window_past_32_bits(msim):
    """msim_config_create, host only: a selfish network on the general engine needs a last window of every block a run
    can have. Three miners pass 96 GiB of chains per lane at about 54 000 years; two miners would pass it exactly
    where the window's block count passes 2^32 (12 B a block, 96 GiB / 24 B): MSIM_E_MINERS for both, never a window
    that wrapped to a small one."""
    from miningsimulation_amd import _lib

    with host_plans._env({"MSIM_FORCE_GENERAL": "1"}):
        ok = msim.Simulation([msim.Miner(0, 70, 100, True), msim.Miner(1, 30, 100)], 4 * Y)
        assert ok.pipeline_info(8)["uses_pipeline"] == 4
        for weights, duration in (([60, 25, 15], 2 * 10**15), ([70, 30], 26 * 10**14), ([70, 30], 10**16)):
            with pytest.raises(msim.MsimError) as e:
                msim.Simulation([msim.Miner(k, w, 100, k == 0) for k, w in enumerate(weights)], duration)
            assert e.value.code == _lib.MSIM_E_MINERS, (weights, duration)


@pytest.mark.parametrize("name", long_runs.HONEST + ("selfish_flush", "selfish_c3_long"))
def test_model_host(native_tests, name):
    """The per-lane kernel's state machine (msim_model.h), 16 runs of each case."""
    lib = ctypes.CDLL(native_tests["model_host"])
    c = CASES[name]
    w, p, sf, m = _arrays(c)
    fn = lambda f, s, bh, err, si, sp: lib.model_run(w, p, sf, m, ctypes.c_int64(c["duration"]), ctypes.c_uint32(si),
                                                      ctypes.c_uint32(sp), 0, f, s, ctypes.byref(bh), ctypes.byref(err))
    runs = min(c["runs"], 16)
    f, s, L, err = _per_run(fn, c, runs)
    ef, es, eL = long_runs.expected(name, runs)
    assert not err.any(), err.tolist()
    assert np.array_equal(f, ef) and np.array_equal(s, es) and np.array_equal(L, eL)


def test_model_host_400_years(native_tests, oracle, msim):
    """Past about 318 years the pipeline's 256 segments no longer cover a run and it stays on the per-lane kernel: one
    run of [70, 30] at 100 ms for 400 years (21 million blocks) on its state machine, against the oracle."""
    w, d, D = [70, 30], [100, 100], 400 * Y
    with host_plans._env():
        assert msim.Simulation([msim.Miner(0, 70, 100), msim.Miner(1, 30, 100)], D).pipeline_info(257)["uses_pipeline"] == 0
    rc, want, best = oracle.run(w, d, [False, False], D, 1000, 1001)
    assert rc == 0 and want[:, 0].max() > 10**7
    lib = ctypes.CDLL(native_tests["model_host"])
    f, s = (ctypes.c_uint32 * 2)(), (ctypes.c_uint32 * 2)()
    bh, err = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.model_run((ctypes.c_uint64 * 2)(*w), (ctypes.c_int64 * 2)(*d), (ctypes.c_uint8 * 2)(), 2, ctypes.c_int64(D),
                         ctypes.c_uint32(1000), ctypes.c_uint32(1001), 0, f, s, ctypes.byref(bh), ctypes.byref(err)) == 0
    assert err.value == 0 and [list(f), list(s)] == want.T.tolist() and bh.value == best


@pytest.mark.parametrize("name", long_runs.WIDE + ("honest_70_30",))
def test_wide_host(native_tests, name):
    """W1's draws and W2's episodes on the host (tests/native/wide_host.cpp); honest_70_30 as MSIM_FORCE_WIDE runs it."""
    lib = ctypes.CDLL(native_tests["wide_host"])
    c = CASES[name]
    w, p, _, m = _arrays(c)
    n = min(c["runs"], 32)
    f, s, e = (ctypes.c_uint32 * (n * m))(), (ctypes.c_uint32 * (n * m))(), (ctypes.c_uint32 * n)()
    ne = ctypes.c_uint32()
    rc = lib.wide_host_run(w, p, ctypes.c_uint32(m), ctypes.c_uint64(c["W"]), ctypes.c_int64(c["duration"]),
                           ctypes.c_uint32(c["base"]), ctypes.c_uint64(0), ctypes.c_uint32(n), f, s, e, ctypes.byref(ne))
    assert rc == 0 and not any(e), list(e)
    ef, es, _ = long_runs.expected(name, n)
    assert np.array_equal(np.array(f, dtype=np.int64).reshape(n, m), ef)
    assert np.array_equal(np.array(s, dtype=np.int64).reshape(n, m), es)


# ------------------------------------------------------------------ the planner's bound over the grid
YEARS = (0.5, 1, 1.4, 2, 3, 5, 10, 20, 50, 100, 400)
RUNS = (1, 257, 8_192, 32_768, 65_536, 1 << 20, 1 << 22)
SLOTS = (1, 64, 512, 2_048, 4_096, 8_192)
LAUNCHES = (1, 2, 4)
NETWORKS = {"one": ([100], 0), "two": ([70, 30], 100), "c2": (long_runs.H9, 100)}
SWEEP_DELAYS = (10_000, 100)


@pytest.mark.parametrize("net", list(NETWORKS))
def test_no_plan_has_a_segment_past_u16(msim, net):
    """Wherever msim_pipeline_info says the honest pipeline serves the run, segment_blocks <= 65 535 and
    blocks_per_run >= pipe_need; a duration the pipeline cannot serve comes back as the per-lane kernel (or an error
    of msim_config_create), never as a plan past the bound. The same for a shared-draw propagation sweep: its plan
    names no segment, so the group's envelope network (uniform delays: the slowest point) is asked for the plan of
    the sweep's own slice at the same wave slots."""
    weights, delay = NETWORKS[net]
    seen = {"pipeline": 0, "other": 0, "longest": 0, "sweeps": 0}
    for years in YEARS:
        D = int(years * Y)
        mk = lambda d: [msim.Miner(k, weights[k], d) for k in range(len(weights))]
        with host_plans._env():
            sims = {}
            for jobs in LAUNCHES:
                sims[jobs] = msim.Simulation(mk(delay), D)
                sims[jobs].set_concurrent_launches(jobs)
            sweep = msim.propagation_sweep(mk(0), SWEEP_DELAYS, D)
            env_sim = msim.Simulation(mk(max(SWEEP_DELAYS)), D)
        for slots in SLOTS:
            with host_plans._env({"MSIM_K1_SLOTS": str(slots)}):
                for n in RUNS:
                    for jobs in LAUNCHES:
                        info = sims[jobs].pipeline_info(n)
                        what = (net, years, n, slots, jobs, info)
                        assert info["uses_pipeline"] in (0, 1), what
                        if info["uses_pipeline"] == 1:
                            assert info["segment_blocks"] <= U16 and info["segment_blocks"] % 32 == 0, what
                            assert info["blocks_per_run"] == info["segments"] * info["segment_blocks"], what
                            assert info["blocks_per_run"] >= pipe_need(D) and info["segments"] <= 256, what
                            seen["pipeline"] += 1
                            seen["longest"] = max(seen["longest"], info["segment_blocks"])
                        else:
                            assert years == 400, what  # 256 workers of 65 504 blocks cover about 318 years
                            seen["other"] += 1
                    plan = sweep.plan(n)
                    if plan["engine"] == 1:
                        info = env_sim.pipeline_info(plan["slice_runs"])
                        what = (net, years, n, slots, plan, info)
                        assert info["uses_pipeline"] == 1 and info["slice_runs"] == plan["slice_runs"], what
                        assert info["segment_blocks"] <= U16 and info["blocks_per_run"] >= pipe_need(D), what
                        seen["sweeps"] += 1
                    else:
                        assert plan["engine"] == 0 and years == 400, (net, years, n, slots, plan)
    per = len(RUNS) * len(SLOTS) * len(LAUNCHES)
    assert seen["pipeline"] == 10 * per and seen["other"] == per and seen["sweeps"] == 10 * len(RUNS) * len(SLOTS), seen
    # the bound binds inside the grid (honest_100's plan is the one exactly at it)
    assert 65_000 <= seen["longest"] <= long_runs.PIPE_MAX_SEG, seen


def test_plans_the_issue_names(msim):
    """The natural plans that laid out segments past 65 535 blocks: a 2-miner network at 12 288, 4 096 and 2 048 wave
    slots (one, two and four launches in flight on a device of 4 096 K1 wave slots)."""
    for slots, jobs, years, n in ((4096, 1, 20, 65_536), (4096, 2, 10, 32_768), (4096, 2, 20, 32_768), (4096, 4, 3, 65_536)):
        with host_plans._env({"MSIM_K1_SLOTS": str(slots)}):
            sim = msim.Simulation([msim.Miner(0, 70, 100), msim.Miner(1, 30, 100)], years * Y)
            sim.set_concurrent_launches(jobs)
            info = sim.pipeline_info(n)
        assert info["uses_pipeline"] == 1 and info["segment_blocks"] <= U16, (slots, jobs, years, n, info)

"""Sweeps on the large-network pipeline (miningsimulation_amd/csrc/msim_widesplit.h) on CPU-only hosts.

The lane bodies the gfx950 kernels run (wide_pick, draw_interval, the split's selection wsplit_select, wide_episode;
tests/native/wide_sweep_body.h, test-only) are executed on the host the way W1, WS, W2 and W3 compose them and compared
run by run with the oracle; every point's selection is compared block for block with the listing on the point's own
thresholds (the harness returns an error otherwise); capacities are passed in to force both overflow rules. The C
ABI's host-only entry points are checked without a device, and a stand-alone program runs the same lane bodies under
AddressSanitizer and UBSan as a child process. tests/test_gpu_wide_sweep.py checks the device build of the same code."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import wide_sweep_native

Y = 31_556_952_000
DAY = 86_400_000
DELAYS = [0, 1, 7, 250, 2_000, 12_000, 45_000, 60_000]


def _weights(m, rng):
    w = [rng.choice([0, 1, 2, 5, 40, 300]) for _ in range(m)]
    w[rng.randrange(m)] += 500
    return w


def _check(oracle, w, props, duration, n, base=1000, begin=0, **kw):
    W = sum(w)
    f, s, ok, cnt = wide_sweep_native.run_group(w, props, W, duration, n, base, begin, **kw)
    for p, pp in enumerate(props):
        of, os_, _, _ = oracle.run_batch(w, list(pp), [0] * len(w), duration, n, begin, base, threads=8, total_weight=W)
        good = ok[p] == 1
        assert np.array_equal(f[p][good], of[good]), (p, props, duration)
        assert np.array_equal(s[p][good], os_[good]), (p, props, duration)
    return ok, cnt


@pytest.mark.parametrize("m", [3, 17, 300])
def test_uniform_delays(oracle, m):
    w = _weights(m, random.Random(m))
    ok, cnt = _check(oracle, w, [[d] * m for d in (60_000, 10_000, 1_000, 100, 1, 0)], 30 * DAY, 6)
    assert (ok == 1).all()
    assert (cnt[0] == cnt[1]).all() and (cnt[1] >= cnt[2]).all() and (cnt[2] >= cnt[6]).all() and cnt[1].min() > 0


@pytest.mark.parametrize("seed", range(4))
def test_random_heterogeneous_groups(oracle, seed):
    """3 / 17 / 300 miners with zero weights, 2 to 6 points, delays of 0 ms to 60 s per miner."""
    rng = random.Random(900 + seed)
    for m in (3, 17, 300):
        np_ = rng.randint(2, 6)
        w = _weights(m, rng)
        props = [[rng.choice(DELAYS) for _ in range(m)] for _ in range(np_)]
        ok, _ = _check(oracle, w, props, rng.choice([3 * DAY, 20 * DAY, 60 * DAY]), 4, base=rng.randrange(2**32),
                       begin=rng.randrange(10**9))
        assert (ok == 1).all()


def test_envelope_is_none_of_the_points(oracle):
    rng = random.Random(5)
    w = _weights(17, rng)
    a = [10_000] + [100] * 16
    b = [100] + [10_000] * 16
    c = [1000 * (k % 9) for k in range(17)]
    env = [max(x) for x in zip(a, b, c)]
    assert env not in (a, b, c)
    ok, cnt = _check(oracle, w, [a, b, c], 60 * DAY, 8)
    assert (ok == 1).all() and (cnt[0] > cnt[1:].max(axis=0)).any()


@pytest.mark.parametrize("dur", [0, 1, 600_000, 3 * DAY, 10**9])
def test_durations(oracle, dur):
    rng = random.Random(dur % 97)
    w = _weights(17, rng)
    ok, _ = _check(oracle, w, [[60_000] * 17, [10_000] * 17, [0] * 17], dur, 16)
    assert (ok == 1).all()


def test_envelope_capacity_fails_the_run_at_every_point(oracle):
    w = _weights(17, random.Random(1))
    props = [[30_000] * 17, [100] * 17]
    _, cnt = wide_sweep_native.run_group(w, props, sum(w), 30 * DAY, 8)[2:]
    cap = int(np.sort(cnt[0])[3])
    ok, _ = _check(oracle, w, props, 30 * DAY, 8, rcap_env=cap)
    assert np.array_equal(ok[0], (cnt[0] <= cap).astype(np.int64)) and np.array_equal(ok[0], ok[1])
    assert (ok[0] == 0).any() and (ok[0] == 1).any()


def test_point_capacity_fails_that_point_only(oracle):
    w = _weights(17, random.Random(2))
    props = [[30_000] * 17, [20_000] * 17, [100] * 17]
    _, cnt = wide_sweep_native.run_group(w, props, sum(w), 30 * DAY, 8)[2:]
    cap = int(np.sort(cnt[2])[3])
    ok, _ = _check(oracle, w, props, 30 * DAY, 8, rcap_pt=[0, cap, 0])
    assert (ok[0] == 1).all() and (ok[2] == 1).all()
    assert np.array_equal(ok[1], (cnt[2] <= cap).astype(np.int64)) and (ok[1] == 0).any() and (ok[1] == 1).any()


def test_lane_bodies_under_sanitizers():
    """build/wide_sweep_check: listing, selection, episodes and combine, overflow cases included, under ASan + UBSan."""
    exe = wide_sweep_native.ensure()["check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


# ------------------------------------------------------------------ the C ABI, host only (no device)
def _c5(msim, delays):
    net = msim.c5_network()
    return [[msim.Miner(mn.id, mn.perc, d) for mn in net] for d in delays]


def _net(msim, w, props):
    return [msim.Miner(k, w[k], props[k]) for k in range(len(w))]


def test_one_group(msim_lib_path):
    import miningsimulation_amd as msim

    sw = msim.propagation_sweep(msim.c5_network(), (10_000, 1_000, 100), total_weight=msim.C5_TOTAL_WEIGHT)
    plan = sw.plan(1024)
    assert plan["engine"] == 2 and plan["draw_groups"] == 1 and plan["largest_group"] == 3
    assert plan["slice_runs"] == 1024 and plan["workspace_bytes"] == sw.workspace_bytes(1024) > 0
    assert [sw.group_of(p) for p in range(4)] == [0, 0, 0, -1]
    assert sw.workspace_bytes(4096) >= sw.workspace_bytes(1024) >= sw.workspace_bytes(16)


def test_flags_0_every_point_its_own_group(msim_lib_path):
    import miningsimulation_amd as msim

    sw = msim.Sweep(_c5(msim, (10_000, 1_000, 100)), total_weight=msim.C5_TOTAL_WEIGHT)
    plan = sw.plan(1024)
    assert plan["engine"] == 2 and plan["draw_groups"] == 3 and plan["largest_group"] == 1
    assert [sw.group_of(p) for p in range(3)] == [-1, -1, -1]
    one = msim.Simulation(_c5(msim, (10_000,))[0], total_weight=msim.C5_TOTAL_WEIGHT)
    assert plan["workspace_bytes"] == one.workspace_bytes(1024) > 0  # the largest point's plain launch
    assert sw.workspace_bytes(4096) >= sw.workspace_bytes(1024)


def test_two_groups_and_a_singleton(msim_lib_path):
    import miningsimulation_amd as msim

    tail = [7, 1, 1, 2, 5, 3, 0, 6, 4, 9, 8, 2, 1, 6, 5]
    wc, wb, ws = [41, 0] + tail, [20, 21] + tail, [19, 22] + tail  # three weight lists, W = 101
    wd, W = wb, 101
    pts = [_net(msim, wc, [10_000] * 17), _net(msim, wb, [1_000] * 17), _net(msim, wc, [100] * 17),
           _net(msim, ws, [2_000] * 17), _net(msim, wd, [50] * 17)]
    sw = msim.Sweep(pts, 10**9, shared_draws=True, total_weight=W)
    plan = sw.plan(67)
    assert plan["engine"] == 2 and plan["draw_groups"] == 3 and plan["largest_group"] == 2
    assert [sw.group_of(p) for p in range(5)] == [0, 1, 0, 2, 1]


def test_groups_split_by_duration_and_total_weight(msim_lib_path):
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    w = [3, 0, 7, 10]
    sims = [msim.Simulation(_net(msim, w, [1000] * 4), 10**9, total_weight=20),
            msim.Simulation(_net(msim, w, [100] * 4), 10**8, total_weight=20),
            msim.Simulation(_net(msim, w, [10] * 4), 10**9, total_weight=20)]
    hs = (ctypes.c_void_p * 3)(*[s.handle.value for s in sims])
    h = ctypes.c_void_p()
    assert _lib.lib.msim_sweep_create_ex(hs, 3, 1, ctypes.byref(h)) == _lib.MSIM_OK
    assert [_lib.lib.msim_sweep_group_of(h, p) for p in range(3)] == [0, 1, 0]
    _lib.lib.msim_sweep_destroy(h)


def test_envelope_the_pipeline_does_not_take_is_split(msim_lib_path):
    """c5 weights for a year: point A (the pools at 25 s) and point B (the small miners at 36 s) each keep their
    candidate capacity under what W3's LDS holds (about 1 960 at 1 026 miners); their envelope does not, so B, the
    point with the largest delay, leaves the group."""
    import miningsimulation_amd as msim

    net = msim.c5_network()
    a = [msim.Miner(mn.id, mn.perc, 25_000 if mn.id < 2 else 0) for mn in net]
    b = [msim.Miner(mn.id, mn.perc, 0 if mn.id < 2 else 36_000) for mn in net]
    c = [msim.Miner(mn.id, mn.perc, 100) for mn in net]
    for p in (a, b):
        assert msim.Simulation(p, total_weight=msim.C5_TOTAL_WEIGHT).pipeline_info(16)["uses_pipeline"] == 2
    env = [msim.Miner(mn.id, mn.perc, 25_000 if mn.id < 2 else 36_000) for mn in net]
    assert msim.Simulation(env, total_weight=msim.C5_TOTAL_WEIGHT).pipeline_info(16)["uses_pipeline"] == 4
    sw = msim.Sweep([a, b], shared_draws=True, total_weight=msim.C5_TOTAL_WEIGHT)
    assert sw.plan(16)["engine"] == 2 and sw.plan(16)["draw_groups"] == 2 and sw.plan(16)["largest_group"] == 1
    assert [sw.group_of(p) for p in range(2)] == [0, 1]
    sw = msim.Sweep([a, b, c], shared_draws=True, total_weight=msim.C5_TOTAL_WEIGHT)
    assert sw.plan(16)["draw_groups"] == 2 and sw.plan(16)["largest_group"] == 2
    assert [sw.group_of(p) for p in range(3)] == [0, 1, 0]


def test_mixed_narrow_and_wide_is_invalid(msim_lib_path, monkeypatch):
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    narrow = msim.Simulation(msim.setup_miners(1000))
    monkeypatch.setenv("MSIM_FORCE_WIDE", "1")
    wide = msim.Simulation(msim.setup_miners(100))
    monkeypatch.delenv("MSIM_FORCE_WIDE")
    assert wide.wide and not narrow.wide
    hs = (ctypes.c_void_p * 2)(narrow.handle.value, wide.handle.value)
    for flags in (0, 1):
        h = ctypes.c_void_p()
        assert _lib.lib.msim_sweep_create_ex(hs, 2, flags, ctypes.byref(h)) == _lib.MSIM_E_INVALID
    # points forced wide when they were created form a wide sweep whatever the switch says now
    hs = (ctypes.c_void_p * 2)(wide.handle.value, wide.handle.value)
    h = ctypes.c_void_p()
    assert _lib.lib.msim_sweep_create_ex(hs, 2, 1, ctypes.byref(h)) == _lib.MSIM_OK
    pl = _lib.MsimSweepPlan()
    assert _lib.lib.msim_sweep_info(h, 64, ctypes.byref(pl)) == _lib.MSIM_OK
    assert pl.engine == 2 and pl.draw_groups == 1 and pl.largest_group == 2
    _lib.lib.msim_sweep_destroy(h)


def test_a_general_point_still_gives_engine_4(msim_lib_path):
    import miningsimulation_amd as msim

    net = msim.c5_network()
    slow = [msim.Miner(mn.id, mn.perc, 60_000) for mn in net]  # fork rate past W3's LDS: the general engine
    assert msim.Simulation(slow, Y, total_weight=msim.C5_TOTAL_WEIGHT).pipeline_info(16)["uses_pipeline"] == 4
    sw = msim.Sweep([net, slow], Y, shared_draws=True, total_weight=msim.C5_TOTAL_WEIGHT)
    assert sw.plan(16)["engine"] == 4 and sw.group_of(0) == -1

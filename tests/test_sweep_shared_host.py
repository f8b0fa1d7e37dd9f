"""The shared-draw form of honest sweeps (miningsimulation_amd/csrc/msim_sweepsplit.h) on CPU-only hosts.

The lane bodies the gfx950 kernels run (the envelope's draw_segment, split_segment, episode_entry with the index
list, combine_run per point; tests/native/sweep_shared_body.h, test-only) are executed on the host and compared run
by run with the oracle; the split's listing of every (run, segment) is compared with the listing draw_segment
produces on the point's own tables; capacities are passed in to force each overflow rule. The C ABI's host-only
entry points (msim_sweep_create_ex, msim_sweep_group_of, msim_sweep_info) are checked without a device, and a
stand-alone program runs the same lane bodies under AddressSanitizer and UBSan as a child process.
tests/test_gpu_sweep_shared.py checks the device build of the same code."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import sweep_shared_native

Y = 31_556_952_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def shared():
    lib = ctypes.CDLL(sweep_shared_native.ensure()["lib"])

    def run(percs, props, duration, n, base=1000, begin=0, env_cap=0, env_lcap=0, pt_cap=None, pt_lcap=None,
            max_group=0, slots=8192):
        m, np_ = len(percs), len(props)
        flat = [d for pt in props for d in pt]
        f = (ctypes.c_uint32 * (np_ * n * m))()
        s = (ctypes.c_uint32 * (np_ * n * m))()
        ok = (ctypes.c_uint8 * (np_ * n))()
        lst = (ctypes.c_uint8 * np_)()
        ne = ctypes.c_uint32()
        u32s = lambda v: (ctypes.c_uint32 * np_)(*(v or [0] * np_))
        rc = lib.sweep_shared_run((ctypes.c_uint64 * m)(*percs), (ctypes.c_int64 * len(flat))(*flat), m,
                                  ctypes.c_uint32(np_), ctypes.c_int64(duration), ctypes.c_uint32(base),
                                  ctypes.c_uint64(begin), ctypes.c_uint32(n), ctypes.c_uint32(slots),
                                  ctypes.c_uint32(env_cap), ctypes.c_uint32(env_lcap), u32s(pt_cap), u32s(pt_lcap),
                                  ctypes.c_uint32(max_group), f, s, ok, lst, ctypes.byref(ne))
        assert rc == 0, rc
        return (np.array(f, dtype=np.int64).reshape(np_, n, m), np.array(s, dtype=np.int64).reshape(np_, n, m),
                np.array(ok, dtype=np.int64).reshape(np_, n), list(lst), ne.value)

    return run


def _check(shared, oracle, percs, props, duration, n, base=1000, begin=0, **kw):
    """Every point's counters equal the oracle's (flagged runs through the retry machine), every listing equals
    the point's own. Returns the ok flags [points][runs] (1: combined by the pipeline, 0: retried)."""
    f, s, ok, lst, ne = shared(percs, props, duration, n, base, begin, **kw)
    assert all(lst), (lst, percs, props, duration)
    assert (ok != 2).all(), "the retry machine failed"
    for p, pp in enumerate(props):
        of, os_, _, _ = oracle.run_batch(percs, list(pp), [0] * len(percs), duration, n, begin, base, threads=8)
        assert np.array_equal(f[p], of), (p, percs, props, duration)
        assert np.array_equal(s[p], os_), (p, percs, props, duration)
    return ok


def _rand_percs(m, rng):
    cuts = sorted(rng.sample(range(1, 100), m - 1)) if m > 1 else []
    b = [0] + cuts + [100]
    return [b[i + 1] - b[i] for i in range(m)]


@pytest.mark.parametrize("m", [1, 2, 9, 15])
def test_uniform_delays(shared, oracle, m):
    rng = random.Random(m)
    percs = H if m == 9 else _rand_percs(m, rng)
    ok = _check(shared, oracle, percs, [[d] * m for d in (60_000, 10_000, 1_000, 100, 1, 0)], Y // 6, 6)
    assert (ok == 1).all()


@pytest.mark.parametrize("seed", range(4))
def test_random_heterogeneous_groups(shared, oracle, seed):
    """1 to 15 miners, 2 to 6 points, delays of 0 ms to 60 s per miner: the envelope is (almost always) none of the
    points. Groups of more than two points also run in split passes of two."""
    rng = random.Random(500 + seed)
    for _ in range(4):
        m = rng.randint(1, 15)
        np_ = rng.randint(2, 6)
        percs = _rand_percs(m, rng)
        props = [[rng.choice([0, 1, 7, 250, 2_000, 12_000, 45_000, 60_000]) for _ in range(m)] for _ in range(np_)]
        dur = rng.choice([Y // 4, Y // 12, 86_400_000 * 10])
        _check(shared, oracle, percs, props, dur, 4, base=rng.randrange(2**32), begin=rng.randrange(10**9),
               max_group=rng.choice([0, 2]))


def test_envelope_is_none_of_the_points(shared, oracle):
    a = [10_000] + [100] * 8
    b = [100] + [10_000] * 8
    c = [1000 * k for k in range(9)]
    ok = _check(shared, oracle, H, [a, b, c], Y // 3, 8)
    assert (ok == 1).all()


@pytest.mark.parametrize("dur", [0, 1, 600_000, 10**9])
def test_durations(shared, oracle, dur):
    _check(shared, oracle, H, [[60_000] * 9, [10_000] * 9, [0] * 9], dur, 32)


def test_envelope_cap_flags_every_point(shared, oracle):
    ok = _check(shared, oracle, H, [[10_000] * 9, [100] * 9], Y, 8, env_cap=1)
    assert (ok[0] == 0).any() and np.array_equal(ok[0], ok[1])


def test_envelope_list_capacity_flags_every_point(shared, oracle):
    ok = _check(shared, oracle, H, [[10_000] * 9, [100] * 9], Y, 8, env_lcap=5)
    assert (ok[0] == 0).any() and np.array_equal(ok[0], ok[1])


def test_point_cap_flags_that_point_only(shared, oracle):
    ok = _check(shared, oracle, H, [[10_000] * 9, [9_000] * 9, [100] * 9], Y, 8, pt_cap=[0, 1, 0])
    assert (ok[1] == 0).any() and (ok[0] == 1).all() and (ok[2] == 1).all()


def test_point_list_capacity_flags_that_point_only(shared, oracle):
    ok = _check(shared, oracle, H, [[10_000] * 9, [9_000] * 9, [100] * 9], Y, 8, pt_lcap=[0, 5, 0])
    assert (ok[1] == 0).any() and (ok[0] == 1).all() and (ok[2] == 1).all()


def test_lane_bodies_under_sanitizers():
    """build/sweep_shared_check: split, episode and combine lane bodies, overflow cases included, under ASan + UBSan."""
    exe = sweep_shared_native.ensure()["check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


# ------------------------------------------------------------------ the C ABI, host only (no device)
def _net(msim, percs, props, selfish=None):
    return [msim.Miner(k, percs[k], props[k], bool(selfish and selfish[k])) for k in range(len(percs))]


def test_create_ex_rejects_unknown_flags(msim_lib_path):
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    sim = msim.Simulation(msim.setup_miners())
    hs = (ctypes.c_void_p * 1)(sim.handle.value)
    for flags, want in ((0, _lib.MSIM_OK), (1, _lib.MSIM_OK), (2, _lib.MSIM_E_INVALID), (3, _lib.MSIM_E_INVALID),
                        (0x80000000, _lib.MSIM_E_INVALID)):
        h = ctypes.c_void_p()
        assert _lib.lib.msim_sweep_create_ex(hs, 1, flags, ctypes.byref(h)) == want, flags
        if want == _lib.MSIM_OK:
            _lib.lib.msim_sweep_destroy(h)


def test_groups_by_weights_and_duration(msim_lib_path):
    import miningsimulation_amd as msim

    w2 = [20, 20, 20, 10, 10, 10, 5, 4, 1]
    pts = [_net(msim, H, [1000] * 9), _net(msim, w2, [100] * 9), _net(msim, H, [100] * 9), _net(msim, w2, [5000] * 9),
           _net(msim, H, [10] * 9)]
    sw = msim.Sweep(pts, 10**9, shared_draws=True)
    assert [sw.group_of(p) for p in range(5)] == [0, 1, 0, 1, 0] and sw.group_of(5) == -1
    plan = sw.plan(257)
    assert plan["engine"] == 1 and plan["draw_groups"] == 2 and plan["largest_group"] == 3
    assert plan["slice_runs"] == 512 and plan["workspace_bytes"] == sw.workspace_bytes(257) > 0
    # one duration per Sweep in Python; two durations through the C entry point
    from miningsimulation_amd import _lib

    sims = [msim.Simulation(pts[0], 10**9), msim.Simulation(pts[2], 10**8), msim.Simulation(pts[4], 10**9)]
    hs = (ctypes.c_void_p * 3)(*[s.handle.value for s in sims])
    h = ctypes.c_void_p()
    assert _lib.lib.msim_sweep_create_ex(hs, 3, 1, ctypes.byref(h)) == _lib.MSIM_OK
    assert [_lib.lib.msim_sweep_group_of(h, p) for p in range(3)] == [0, 1, 0]
    _lib.lib.msim_sweep_destroy(h)


def test_no_group_without_the_shared_form(msim_lib_path):
    import miningsimulation_amd as msim

    honest = [msim.setup_miners(p) for p in (10_000, 1_000, 100)]
    cases = {"flags 0": (honest, False, 0),
             "a selfish point": ([msim.setup_miners(1000), msim.setup_miners(1000, 30)], True, 3),
             "a 600 s point": ([msim.setup_miners(1000), msim.setup_miners(600_000)], True, 0)}
    for what, (pts, flag, engine) in cases.items():
        sw = msim.Sweep(pts, shared_draws=flag)
        assert [sw.group_of(p) for p in range(len(pts))] == [-1] * len(pts), what
        plan = sw.plan(1024)
        assert plan["engine"] == engine and plan["draw_groups"] == 0 and plan["largest_group"] == 0, what
        assert plan == msim.Sweep(pts).plan(1024) and sw.workspace_bytes(1024) == msim.Sweep(pts).workspace_bytes(1024), what
    assert msim.Sweep(honest, shared_draws=True).plan(1024)["engine"] == 1


def test_envelope_past_the_fork_rate_limit_is_split(msim_lib_path):
    """Each point alone has rho = 0.5 (1 - exp(-60001 / 599999.5)) = 0.048 <= 0.08; their envelope (both miners at
    60 s) has 0.095: the group loses a 60 s point to a group of its own."""
    import miningsimulation_amd as msim

    a = _net(msim, [50, 50], [60_000, 0])
    b = _net(msim, [50, 50], [0, 60_000])
    c = _net(msim, [50, 50], [100, 100])
    sw = msim.Sweep([a, b, c], shared_draws=True)
    assert sw.plan(1024)["engine"] == 1 and sw.plan(1024)["draw_groups"] == 2
    assert [sw.group_of(p) for p in range(3)] == [1, 0, 0]
    sw2 = msim.propagation_sweep(msim.setup_miners(), [10_000, 1_000, 100])
    assert sw2.plan(1024)["draw_groups"] == 1 and [sw2.group_of(p) for p in range(3)] == [0, 0, 0]
    assert [m.propagation_ms for m in sw2.sims[2].miners] == [100] * 9

"""The shared-draw form of honest sweeps on the device (msim_sweep_create_ex with MSIM_SWEEP_SHARED_DRAWS;
miningsimulation_amd/csrc/msim_sweepsplit.h): one draw pass per draw group on the envelope network, the split
kernel S1, then the episode and combine kernels per point.

Every comparison is exact: found, stale and best height of every run against the oracle, and sums byte for byte
against Simulation(points[p]).run (the plain pipeline) or against the flags-0 sweep (the per-lane kernel) at the
same seeds. Unless stated, runs last 10^9 ms (about 1 667 blocks: several draw segments) and a point has 257 runs
(one full workgroup plus one lane). The oracle's counters are computed once per network and shared."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 10**9
N = 257
BASE = 1000
W = {1: [100], 2: [70, 30], 9: [30, 29, 12, 11, 8, 5, 3, 1, 1],
     15: [20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1]}
W9B = [20, 20, 20, 10, 10, 10, 5, 4, 1]


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


_REF = {}


def _oracle(oracle, percs, props, duration, n, begin=0):
    k = (tuple(percs), tuple(props), duration, n, begin)
    if k not in _REF:
        f, s, _, _ = oracle.run_batch(list(percs), list(props), [False] * len(percs), duration, n, begin, BASE, threads=16)
        f.setflags(write=False)
        s.setflags(write=False)
        _REF[k] = (f, s)
    return _REF[k]


def _net(msim, percs, props):
    return [msim.Miner(k, percs[k], props[k]) for k in range(len(percs))]


def _sum_bytes(res):
    return b"".join(bytes(x) for x in res.sums)


def _shared(msim, points, duration=D):
    sw = msim.Sweep(points, duration, shared_draws=True)
    assert sw.plan(N)["engine"] == 1, sw.plan(N)
    return sw


def _check_points(msim, oracle, sw, points, duration, n, begin=0, singles=True):
    out = sw.run(n, run_begin=begin, seed_base=BASE, per_run=True)
    for p, (res, pt) in enumerate(zip(out, points)):
        f, s = _oracle(oracle, [m.perc for m in pt], [m.propagation_ms for m in pt], duration, n, begin)
        assert np.array_equal(res.found.astype(np.int64), f), (p, np.argwhere(res.found != f)[:5])
        assert np.array_equal(res.stale.astype(np.int64), s), (p, np.argwhere(res.stale != s)[:5])
        assert np.array_equal(res.best_height.astype(np.int64), f.sum(axis=1)), p
        if singles:
            one = msim.Simulation(pt, duration).run(n, run_begin=begin, seed_base=BASE)
            assert _sum_bytes(res) == _sum_bytes(one), p
    return out


@pytest.mark.parametrize("m", [1, 2, 9, 15])
def test_uniform_delays_per_run_vs_oracle(msim, oracle, m):
    points = [_net(msim, W[m], [d] * m) for d in (10_000, 1_000, 100, 0)]
    sw = _shared(msim, points)
    assert sw.plan(N)["draw_groups"] == 1 and sw.plan(N)["largest_group"] == 4
    _check_points(msim, oracle, sw, points, D, N)


def test_heterogeneous_group(msim, oracle):
    """The envelope (every miner at 10 s, or at max(10 s, 1000 k)) is none of the points."""
    a = _net(msim, W[9], [10_000] + [100] * 8)
    b = _net(msim, W[9], [100] + [10_000] * 8)
    c = _net(msim, W[9], [1000 * k for k in range(9)])
    sw = _shared(msim, [a, b, c])
    assert [sw.group_of(p) for p in range(3)] == [0, 0, 0]
    _check_points(msim, oracle, sw, [a, b, c], D, N)


def test_two_groups_and_a_singleton(msim, oracle):
    points = [_net(msim, W[9], [10_000] * 9), _net(msim, W9B, [1_000] * 9), _net(msim, W[9], [100] * 9),
              _net(msim, [60, 10, 5, 5, 5, 5, 5, 4, 1], [2_000] * 9), _net(msim, W9B, [50] * 9)]
    sw = _shared(msim, points)
    assert sw.plan(N)["draw_groups"] == 3 and sw.plan(N)["largest_group"] == 2
    assert [sw.group_of(p) for p in range(5)] == [0, 1, 0, 2, 1]
    _check_points(msim, oracle, sw, points, D, N)


@pytest.mark.parametrize("kind", ["selfish", "600s"])
def test_fallback_is_todays_engine(msim, kind):
    if kind == "selfish":
        points = [msim.setup_miners(1000), msim.setup_miners(1000, 30), msim.setup_miners(100)]
        engine = 3
    else:
        points = [_net(msim, W[9], [1000] * 9), _net(msim, W[9], [600_000] * 9)]
        engine = 0
    on, off = msim.Sweep(points, D, shared_draws=True), msim.Sweep(points, D)
    assert on.plan(N) == off.plan(N) and on.plan(N)["engine"] == engine and on.group_of(0) == -1
    assert on.workspace_bytes(N) == off.workspace_bytes(N)
    import torch

    outs = []
    for sw in (on, off):
        m, P = sw.m, len(points)
        sums = torch.empty((P, m, 6), dtype=torch.int64, device="cuda")
        rec = torch.empty((P, N, m, 2), dtype=torch.int32, device="cuda")
        bh = torch.empty((P, N), dtype=torch.int32, device="cuda")
        st = torch.empty(2, dtype=torch.int32, device="cuda")
        ws = torch.zeros(sw.workspace_bytes(N), dtype=torch.uint8, device="cuda")
        sw.launch(N, 0, BASE, sums, ws, st, rec, bh)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().tobytes() for t in (sums, rec, bh, st)])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257])
def test_run_counts(msim, oracle, n):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    _check_points(msim, oracle, _shared(msim, points), points, D, n, begin=5)


@pytest.mark.parametrize("duration", [1, 600_000])
def test_short_durations(msim, oracle, duration):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    _check_points(msim, oracle, _shared(msim, points, duration), points, duration, N)


def test_slices(msim, oracle, monkeypatch):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points)
    whole = sw.run(600, seed_base=BASE, per_run=True)
    monkeypatch.setenv("MSIM_MAX_SLICE_RUNS", "256")
    assert sw.plan(600)["slice_runs"] == 256
    cut = _check_points(msim, oracle, sw, points, D, 600, singles=False)
    for a, b in zip(whole, cut):
        assert _sum_bytes(a) == _sum_bytes(b)
        assert np.array_equal(a.found, b.found) and np.array_equal(a.stale, b.stale)
        assert np.array_equal(a.best_height, b.best_height)


def _launch(sw, n, ws, fill):
    import torch

    m, P = sw.m, len(sw)
    sums = torch.full((P, m, 6), fill, dtype=torch.int64, device="cuda")
    rec = torch.full((P, n, m, 2), fill, dtype=torch.int32, device="cuda")
    bh = torch.full((P, n), fill, dtype=torch.int32, device="cuda")
    st = torch.full((2,), fill, dtype=torch.int32, device="cuda")
    sw.launch(n, 0, BASE, sums, ws, st, rec, bh)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (sums, rec, bh, st)]


def test_forced_retry(msim, oracle, monkeypatch):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points)
    monkeypatch.setenv("MSIM_PIPE_FORCE_RETRY", "1")
    import torch

    ws = torch.zeros(sw.workspace_bytes(N), dtype=torch.uint8, device="cuda")
    sums, rec, bh, st = _launch(sw, N, ws, 0)
    assert st.tolist() == [len(points) * N, 0]
    for p, pt in enumerate(points):
        f, s = _oracle(oracle, W[9], [m.propagation_ms for m in pt], D, N)
        assert np.array_equal(rec[p, :, :, 0].astype(np.int64), f) and np.array_equal(rec[p, :, :, 1].astype(np.int64), s)
        assert np.array_equal(bh[p].astype(np.int64), f.sum(axis=1))
        assert np.array_equal(sums[p, :, 0], f.sum(axis=0)) and np.array_equal(sums[p, :, 1], s.sum(axis=0))


def test_group_bound(msim, oracle, monkeypatch):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 3_000, 1_000, 300, 100)]
    sw = _shared(msim, points)
    whole = sw.run(N, seed_base=BASE, per_run=True)
    monkeypatch.setenv("MSIM_SWEEP_SHARED_MAX_GROUP", "2")
    assert sw.plan(N)["draw_groups"] == 1 and sw.plan(N)["largest_group"] == 5
    cut = _check_points(msim, oracle, sw, points, D, N, singles=False)
    for a, b in zip(whole, cut):
        assert _sum_bytes(a) == _sum_bytes(b)
        assert np.array_equal(a.found, b.found) and np.array_equal(a.stale, b.stale)


def test_dirty_workspace(msim):
    import torch

    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points)
    nb = sw.workspace_bytes(N)
    clean = _launch(sw, N, torch.zeros(nb, dtype=torch.uint8, device="cuda"), 0)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    dirty = _launch(sw, N, ws, -1)
    again = _launch(sw, N, ws, -1)  # the same workspace, now holding the first launch's lists and records
    for a, b, c in zip(clean, dirty, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert clean[3].tolist() == [0, 0]


def _raw_contrasts(msim, sw, n, pairs):
    """msim_sweep_run_contrasts' outputs as the library wrote them: sums, moments and cross words."""
    import ctypes

    from miningsimulation_amd import _lib
    from miningsimulation_amd.contrasts import Pair, pairs_struct

    nm = len(sw) * sw.m
    pairs = [Pair(*q) for q in pairs]
    arr = pairs_struct(pairs, len(sw), sw.m)
    stats, sums, mom = (_lib.MsimStats * nm)(), (_lib.MsimSums * nm)(), (_lib.MsimMoments * nm)()
    cross = (_lib.MsimCross * len(pairs))()
    _lib.check(_lib.lib.msim_sweep_run_contrasts(sw._h, 0, n, BASE, 0, arr, len(pairs), stats, sums, mom, cross),
               "msim_sweep_run_contrasts")
    return bytes(sums), bytes(mom), bytes(cross)


def test_contrasts_word_for_word(msim):
    points = [_net(msim, W[9], [d] * 9) for d in (10_000, 1_000, 100)]
    pairs = msim.pairs_vs_baseline(3, 9)
    a = _raw_contrasts(msim, _shared(msim, points), N, pairs)
    b = _raw_contrasts(msim, msim.Sweep(points, D), N, pairs)
    assert a[0] == b[0], "sums"
    assert a[1] == b[1], "moments"
    assert a[2] == b[2], "cross sums"
    assert any(a[2])


def test_host_driver(msim, tmp_path):
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    spec = {"runs": 64, "seed_base": BASE, "duration_ms": D,
            "points": [{"miners": [{"id": k, "perc": W[9][k], "propagation_ms": d} for k in range(9)]}
                       for d in (10_000, 1_000, 100)]}
    path = tmp_path / "sweep.json"
    path.write_text(json.dumps(spec))
    outs = [subprocess.run([exe, "--sweep", str(path), *extra], check=True, capture_output=True, text=True,
                           timeout=120).stdout for extra in ([], ["--shared-draws"])]
    assert outs[0] == outs[1] and "Point 3 of 3" in outs[0]

"""Exact quantiles without a GPU: msim_rank.h's sequential host selection (the lines the gfx950 kernels run) against
tests/rank_reference.py, the stand-alone sanitizer build, quantile_rank against hist_quantile's k, the ABI's argument
checks, the workspace layout, and the sharded path under gloo with stand-in launches."""
import ctypes
import fcntl
import math
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import rank_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "librank_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "rank_check")


def _built():
    """build/librank_host.so and build/rank_check, built here when missing or older than their sources."""
    import __graft_entry__ as ge

    srcs = [os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_rank.h"),
            os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_moments.h"),
            os.path.join(ROOT, "include", "msim.h"),
            os.path.join(ROOT, "tests", "native", "rank_host.cpp"),
            os.path.join(ROOT, "tests", "native", "rank_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".rank_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_rank_tests()
    return HOST_LIB


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_select(found, stale, best_height, ranks):
    """(order[column][quantity][j] triples, number of rows with a rank that is not below the run count) from
    librank_host.so; the entries of such rows stay at the 0xFF fill."""
    h = ctypes.CDLL(_built())
    h.rank_host_select.restype = ctypes.c_longlong
    rec = rr.records(found, stale)
    n, m = found.shape
    bh = np.ascontiguousarray(best_height, dtype=np.uint32)
    rk = np.asarray(ranks, dtype=np.uint64)
    out = np.full((m, 4, len(ranks), 3), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    bad = h.rank_host_select(_vp(rec), _vp(bh), ctypes.c_uint64(n), ctypes.c_uint32(m), _vp(rk),
                             ctypes.c_uint32(len(ranks)), _vp(out))
    assert bad >= 0
    return out.tolist(), bad


def test_struct_and_constants(msim_lib_path):
    from miningsimulation_amd import _lib, quantiles

    assert ctypes.sizeof(_lib.MsimOrderStat) == 24
    assert (quantiles.MAX_RANKS, quantiles.RANK_PASSES) == (32, 8)
    with open(os.path.join(ROOT, "include", "msim.h")) as f:
        src = f.read()
    assert "#define MSIM_MAX_RANKS 32u" in src and "#define MSIM_RANK_PASSES 8u" in src
    assert "MSIM_RANK_TEST_WG_RUNS" in src


def test_cases_hold_every_extreme():
    f, s, L = rr.synthetic(257, 9)
    k4 = rr.keys(f, s, L)
    assert (k4[:, :, 0] == 0).all()                                   # all zero
    assert (f[:, 1] == 6).all() and (k4[3, :, 1] == k4[3, 0, 1]).all()  # all equal
    assert (k4[2, :, 2] == 1 << 32).any() and (k4[2, L == 0, 2] == 0).all()
    assert int(k4[3, :, 3].max()) == 2**64 - 2**32
    assert (L == 0).any() and (f[L == 0, 4] == 5).all() and (k4[2, L == 0, 4] == 0).all()
    assert set((f[:, 5] ^ f[0, 5]).tolist()) == {0, 1}               # the lowest byte only
    assert set((f[:, 6] ^ f[0, 6]).tolist()) == {0, 3 << 24}         # the highest non-zero byte only
    assert set((s[:, 6] ^ s[0, 6]).tolist()) == {0, 0xC0000000}
    assert (np.diff(f[:, 7].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("n_runs,m", [(1, 1), (2, 2), (65, 9), (257, 17)])
def test_host_selection_equals_reference(n_runs, m):
    f, s, L = rr.synthetic(n_runs, m, shift=3 if m < 9 else 0, seed=n_runs)
    for nr, ranks in rr.rank_lists(n_runs).items():
        got, bad = host_select(f, s, L, ranks)
        assert bad == 0
        miss = rr.diff(got, rr.select(f, s, L, ranks))
        assert not miss, (nr, miss[:8])
        for col in got:
            for row in col:
                for (v, below, equal), r in zip(row, ranks):
                    assert below <= r < below + equal
    # all equal: equal == N on found, stale and rate
    if m >= 9:
        got, _ = host_select(f, s, L, [n_runs // 2])
        assert [got[1][q][0] for q in (0, 1)] == [[6, 0, n_runs], [2, 0, n_runs]] and got[1][3][0][1:] == [0, n_runs]


def test_host_selection_flags_a_rank_past_the_runs():
    f, s, L = rr.synthetic(13, 9)
    ranks = [6, 13, 0, 2**64 - 1]
    got, bad = host_select(f, s, L, ranks)
    assert bad == 2 * 9 * 4
    assert not rr.diff(got, rr.select(f, s, L, ranks))
    assert all(got[k][q][j] == [2**64 - 1] * 3 for k in range(9) for q in range(4) for j in (1, 3))  # untouched


def test_rank_check_under_sanitizers():
    """The key, match, digit and narrowing functions and the host selection, built stand-alone with ASan + UBSan,
    on the extreme records: a child process on the CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rank_check: ok" in r.stdout


def test_quantile_rank_is_hist_quantiles_k(msim_lib_path):
    """quantile_rank(n, q) + 1 is the k hist_quantile reaches: with one value per bin, the bin it returns is bin k."""
    from miningsimulation_amd import HistSpec, hist_quantile, quantile_rank

    for n in range(1, 51):
        spec = HistSpec(n, share_shift=4)             # n bins of 16 units: edges(b) = (16 (b - 1), 16 b) / 2^32
        counts = [0] + [1] * n + [0]
        for q in (0.0, 1e-9, 0.05, 0.5, 0.95, 1.0):
            k = quantile_rank(n, q) + 1
            assert 1 <= k <= n
            assert hist_quantile(counts, spec, q) == spec.edges(k), (n, q, k)
            assert k == max(1, math.ceil(q * n))
    with pytest.raises(ValueError):
        quantile_rank(0, 0.5)
    with pytest.raises(ValueError):
        quantile_rank(10, 1.5)


def test_quantile_ci_ranks(msim_lib_path):
    from miningsimulation_amd import quantile_ci_ranks, quantile_rank

    for n in (1, 2, 10, 257, 32768):
        for q in (0.0, 0.05, 0.5, 0.95, 1.0):
            lo, hi = quantile_ci_ranks(n, q)
            assert 0 <= lo <= hi <= n - 1
            assert lo <= quantile_rank(n, q) <= hi
            assert quantile_ci_ranks(n, q, z=0.0) == (quantile_rank(n, q),) * 2
    assert quantile_ci_ranks(100, 0.5) == (40, 59)     # 50 -+ 1.96 * 5 = 40.2, 59.8: order statistics 41 and 60
    # 1638.4 -+ 1.96 * sqrt(1556.48) = 1561.07.., 1715.72..: order statistics 1562 and 1716
    assert quantile_ci_ranks(32768, 0.05) == (1561, 1715)


def test_order_stats_from_words(msim_lib_path):
    from miningsimulation_amd import OrderStat, order_stats_from_words

    words = np.arange(2 * 3 * 4 * 2 * 3, dtype=np.uint64)
    words[0] = 2**64 - 2**32
    order = order_stats_from_words(words.view(np.int64), 2, 3, 2)
    assert order[0][0][0][0] == OrderStat(2**64 - 2**32, 1, 2) and isinstance(order[0][0][0][0].value, int)
    assert order[1][2][3][1] == OrderStat(141, 142, 143)
    assert order_stats_from_words(words.tolist(), 2, 3, 2) == order
    with pytest.raises(ValueError):
        order_stats_from_words(words[:-1], 2, 3, 2)


def test_report_quantiles_format(msim_lib_path):
    from miningsimulation_amd import OrderStat, QuantileResult, report_quantiles, setup_miners

    miners = setup_miners(1000)[:2]
    col = (lambda a, b: [[OrderStat(a, 0, 1), OrderStat(b, 1, 1)], [OrderStat(1, 0, 1), OrderStat(3, 1, 1)],
                         [OrderStat(1 << 30, 0, 1), OrderStat(3 << 30, 1, 1)], [OrderStat(0, 0, 1), OrderStat(1 << 29, 1, 1)]])
    res = QuantileResult(points=[None], ranks=[0, 1], qs=[0.05, 0.95], order=[[col(10, 20), col(1, 2)]], n_runs=2)
    lines = report_quantiles(miners, res).splitlines()
    assert lines[0] == ("  - Miner 0 (30% of network hashrate) blocks found: q0.05 = 10, q0.95 = 20; share of blocks: "
                        "q0.05 = 25%, q0.95 = 75%; stale rate: q0.05 = 0%, q0.95 = 12.5%.")
    assert lines[1].startswith("  - Miner 1 (29% of network hashrate) blocks found: q0.05 = 1, q0.95 = 2;")
    assert res.value(0, "share", 1) == 0.75 and res.values[0][1][0] == [1.0, 2.0]
    res.qs = None
    assert "rank 0 = 10, rank 1 = 20" in report_quantiles(miners, res)
    lines = report_quantiles(miners, res, members=[[0], [1]]).splitlines()
    assert lines[1].startswith("  - Class 1 (1 miners, 49.1525% of network hashrate) blocks found: rank 0 = 1,")


# ---------------------------------------------------------------- the ABI's argument checks (no GPU call is reached)
def test_workspace_and_counts_view(msim_lib_path):
    from miningsimulation_amd import _lib

    h = ctypes.CDLL(_built())
    lib = _lib.lib
    u64 = ctypes.c_uint64
    for m, points, nr in ((1, 1, 1), (9, 3, 3), (1026, 1, 32), (257, 65535, 1)):
        b, at, words = u64(), u64(), u64()
        h.rank_host_layout(ctypes.c_uint32(m), ctypes.c_uint32(points), ctypes.c_uint32(nr), ctypes.byref(b),
                           ctypes.byref(at), ctypes.byref(words))
        assert lib.msim_rank_workspace_bytes(m, points, nr) == b.value
        off, w = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.msim_rank_counts_view(m, points, nr, ctypes.byref(off), ctypes.byref(w)) == _lib.MSIM_OK
        assert (off.value, w.value) == (at.value, words.value)
        assert w.value == points * m * 4 * nr * 256 and off.value % 256 == 0 and off.value + 8 * w.value == b.value
    off, w = ctypes.c_size_t(7), ctypes.c_size_t(7)
    for m, points, nr in ((0, 1, 1), (1, 0, 1), (1, 65536, 1), (1, 1, 0), (1, 1, 33)):
        assert lib.msim_rank_workspace_bytes(m, points, nr) == 0
        assert lib.msim_rank_counts_view(m, points, nr, ctypes.byref(off), ctypes.byref(w)) == _lib.MSIM_E_INVALID
    assert lib.msim_rank_counts_view(1, 1, 1, None, ctypes.byref(w)) == _lib.MSIM_E_INVALID
    assert lib.msim_rank_counts_view(1, 1, 1, ctypes.byref(off), None) == _lib.MSIM_E_INVALID
    assert (off.value, w.value) == (7, 7)


def test_ranks_check(msim_lib_path):
    from miningsimulation_amd import _lib
    from miningsimulation_amd.quantiles import ranks_array

    lib = _lib.lib
    arr = (lambda *r: (ctypes.c_uint64 * len(r))(*r))
    assert lib.msim_ranks_check(10, arr(0, 9, 5, 5), 4) == _lib.MSIM_OK
    assert lib.msim_ranks_check(10, arr(0, 10), 2) == _lib.MSIM_E_INVALID
    assert lib.msim_ranks_check(10, arr(0), 0) == _lib.MSIM_E_INVALID
    assert lib.msim_ranks_check(10, None, 1) == _lib.MSIM_E_INVALID
    assert lib.msim_ranks_check(100, arr(*range(33)), 33) == _lib.MSIM_E_INVALID
    assert lib.msim_ranks_check(0, arr(0), 1) == _lib.MSIM_E_INVALID
    assert lib.msim_ranks_check(2**64 - 1, arr(2**64 - 2), 1) == _lib.MSIM_OK
    for bad in ([], list(range(33)), [-1], [2**64]):
        with pytest.raises(ValueError):
            ranks_array(bad)
    with pytest.raises(ValueError):
        ranks_array([3], n_runs=3)


def test_launches_reject_bad_arguments(msim_lib_path):
    """Every refusal comes before any HIP call, so it can be checked on a host without a device; the pointers are
    never dereferenced."""
    from miningsimulation_amd import _lib

    lib = _lib.lib
    E = _lib.MSIM_E_INVALID
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused
    ranks = (ctypes.c_uint64 * 3)(0, 1, 2)
    big = lib.msim_rank_workspace_bytes(9, 1, 3)
    ok = dict(m=9, points=1, runs=100, rec=p, bh=p, ranks=ranks, nr=3, out=p, status=p, ws=p, wsb=big, p=0)
    changes = (dict(m=0), dict(points=0), dict(points=65536), dict(nr=0), dict(nr=33), dict(ranks=None), dict(ws=None),
               dict(wsb=big - 1))
    for ch in changes:
        a = dict(ok, **ch)
        assert lib.msim_rank_begin_launch(a["m"], a["points"], a["ranks"], a["nr"], a["ws"], a["wsb"], None) == E, ch
    small = lib.msim_rank_workspace_bytes(9, 1, 1)
    for ch in (dict(m=0), dict(points=0), dict(points=65536), dict(runs=0), dict(runs=1 << 32), dict(rec=None),
               dict(bh=None), dict(p=8), dict(ws=None), dict(wsb=small - 1)):
        a = dict(ok, **ch)
        assert lib.msim_rank_count_launch(a["m"], a["points"], a["runs"], a["rec"], a["bh"], a["p"], a["ws"], a["wsb"],
                                          None) == E, ch
    for ch in (dict(m=0), dict(points=0), dict(points=65536), dict(p=8), dict(ws=None), dict(wsb=small - 1),
               dict(status=None), dict(p=7, out=None)):
        a = dict(ok, **ch)
        assert lib.msim_rank_step_launch(a["m"], a["points"], a["p"], a["ws"], a["wsb"], a["out"], a["status"], None) == E, ch
    for ch in changes + (dict(runs=0), dict(runs=1 << 32), dict(rec=None), dict(bh=None), dict(out=None),
                         dict(status=None)):
        a = dict(ok, **ch)
        assert lib.msim_rank_launch(a["m"], a["points"], a["runs"], a["rec"], a["bh"], a["ranks"], a["nr"], a["out"],
                                    a["status"], a["ws"], a["wsb"], None) == E, ch


def test_run_order_stats_rejects_bad_arguments(msim_lib_path):
    from miningsimulation_amd import Simulation, _lib, setup_miners

    sim = Simulation(setup_miners())
    lib = _lib.lib
    stats, sums = (_lib.MsimStats * 9)(), (_lib.MsimSums * 9)()
    out = (_lib.MsimOrderStat * (9 * 4 * 2))()
    ranks = (ctypes.c_uint64 * 2)(0, 15)
    cmap = (ctypes.c_uint32 * 9)()
    call = (lambda h, n, cm, nc, rk, nr, st, o: lib.msim_run_order_stats(h, 0, n, 1000, 0, cm, nc, rk, nr, st, sums, o))
    E = _lib.MSIM_E_INVALID
    assert call(None, 16, None, 0, ranks, 2, stats, out) == E
    assert call(sim.handle, 0, None, 0, ranks, 2, stats, out) == E
    assert call(sim.handle, 15, None, 0, ranks, 2, stats, out) == E          # rank 15 of 15 runs
    assert call(sim.handle, 16, None, 0, None, 2, stats, out) == E
    assert call(sim.handle, 16, None, 0, ranks, 0, stats, out) == E
    assert call(sim.handle, 16, None, 0, ranks, 2, None, out) == E
    assert call(sim.handle, 16, None, 0, ranks, 2, stats, None) == E
    assert call(sim.handle, 16, cmap, 0, ranks, 2, stats, out) == E          # a map without a class count
    assert call(sim.handle, 16, None, 1, ranks, 2, stats, out) == E
    assert call(sim.handle, 16, cmap, 10, ranks, 2, stats, out) == E
    assert lib.msim_sweep_run_order_stats(None, 0, 16, 1000, 0, None, 0, ranks, 2, stats, sums, out) == E
    with pytest.raises(ValueError):
        sim.run_quantiles(16, ranks=[16])
    with pytest.raises(ValueError):
        sim.run_quantiles(16, qs=[1.5])
    with pytest.raises(ValueError):
        sim.run_quantiles(16, class_of=[0] * 8 + [2], n_classes=2)


# ---------------------------------------------------------------- the primitives on the host, and the sharded path
def _host_fns():
    h = ctypes.CDLL(_built())
    for fn in (h.rank_host_begin, h.rank_host_count, h.rank_host_step):
        fn.restype = ctypes.c_int
    return h


def _host_passes(buffers, m, ranks):
    """begin, then eight passes of one count per buffer and one step, on a host workspace in the library's layout."""
    from miningsimulation_amd import _lib

    h = _host_fns()
    ws = np.full(_lib.lib.msim_rank_workspace_bytes(m, 1, len(ranks)) // 8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rk = np.asarray(ranks, dtype=np.uint64)
    out = np.zeros((m, 4, len(ranks), 3), dtype=np.uint64)
    status = np.zeros(1, dtype=np.uint32)
    assert h.rank_host_begin(ctypes.c_uint32(m), _vp(rk), ctypes.c_uint32(len(ranks)), _vp(ws)) == 0
    for p in range(8):
        for f, s, L in buffers:
            rec, bh = rr.records(f, s), np.ascontiguousarray(L, dtype=np.uint32)
            assert h.rank_host_count(_vp(rec), _vp(bh), ctypes.c_uint64(len(L)), ctypes.c_uint32(m), ctypes.c_uint32(p),
                                     _vp(ws)) == 0
        assert h.rank_host_step(ctypes.c_uint32(m), ctypes.c_uint32(p), _vp(ws), _vp(out), _vp(status)) == 0
    return out.tolist(), int(status[0])


def test_host_primitives_two_buffers(msim_lib_path):
    """100 + 157 runs through begin / count x 2 / step equal the selection over the 257 runs, from a workspace that
    held 0xFF everywhere."""
    f, s, L = rr.synthetic(257, 9)
    ranks = rr.rank_lists(257)[5]
    got, status = _host_passes([(f[:100], s[:100], L[:100]), (f[100:], s[100:], L[100:])], 9, ranks)
    assert status == 0 and not rr.diff(got, rr.select(f, s, L, ranks))
    got, status = _host_passes([(f, s, L)], 9, ranks + [257])
    assert status == 8 * 9 * 4 and not rr.diff(got, rr.select(f, s, L, ranks + [257]))


N_TOTAL, M_SH, CHUNK = 29, 4, 6
QS = (0.05, 0.5, 0.95, 1.0)


class _FakeSim:
    """Stands in for Simulation on a CPU rank: launch fills the records of runs [begin, begin + n) of one fixed
    synthetic data set (and their first sums), the rank launches are librank_host.so's primitives on the workspace."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = rr.synthetic(N_TOTAL, M_SH, shift=5, seed=7)
        self.h = _host_fns()
        self.counts = []

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        import moments_reference as ref

        assert ws is None and 0 < n <= CHUNK
        f, s, L = self.f[begin:begin + n], self.s[begin:begin + n], self.L[begin:begin + n]
        d_per_run[:n] = torch.from_numpy(rr.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        st, rt = ref.terms(f, s, L)
        tot = (lambda a: [int(x) for x in a.astype(object).sum(axis=0)])
        lo = np.uint64(0xFFFFFFFF)  # limbs summed on their own, as the engines do: additive over any partition
        rows = [list(r) for r in zip(tot(f), tot(s), tot(st >> np.uint64(32)), tot(st & lo), tot(rt >> np.uint64(32)),
                                     tot(rt & lo))]
        sums.copy_(torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)))
        status.zero_()

    def launch_rank_begin(self, ranks, d_ws, stream=None):
        rk = np.asarray(ranks, dtype=np.uint64)
        assert self.h.rank_host_begin(ctypes.c_uint32(M_SH), _vp(rk), ctypes.c_uint32(len(ranks)),
                                      ctypes.c_void_p(d_ws.data_ptr())) == 0

    def launch_rank_count(self, n, d_per_run, d_best_height, pass_, d_ws, stream=None):
        self.counts.append((pass_, n))
        assert self.h.rank_host_count(ctypes.c_void_p(d_per_run.data_ptr()), ctypes.c_void_p(d_best_height.data_ptr()),
                                      ctypes.c_uint64(n), ctypes.c_uint32(M_SH), ctypes.c_uint32(pass_),
                                      ctypes.c_void_p(d_ws.data_ptr())) == 0

    def launch_rank_step(self, pass_, d_ws, d_out, d_status, stream=None):
        assert self.h.rank_host_step(ctypes.c_uint32(M_SH), ctypes.c_uint32(pass_), ctypes.c_void_p(d_ws.data_ptr()),
                                     ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(d_status.data_ptr())) == 0


def _run_fake():
    import torch

    from miningsimulation_amd.distributed import run_sharded_quantiles

    sim = _FakeSim()
    res = run_sharded_quantiles(sim, N_TOTAL, 1000, qs=QS, launch=sim.launch, launch_rank_begin=sim.launch_rank_begin,
                                launch_rank_count=sim.launch_rank_count, launch_rank_step=sim.launch_rank_step,
                                device=torch.device("cpu"), max_chunk=CHUNK)
    sums = [[getattr(x, f) for f, _ in x._fields_] for x in res.points[0].sums]
    out = {"order": [[[list(o) for o in row] for row in col] for col in res.order[0]], "ranks": res.ranks,
           "qs": res.qs, "sums": sums, "n_runs": res.n_runs, "share": [s.blocks_share for s in res.points[0].stats_total]}
    return out, sim.counts


def _worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce

    def counted(t, *a, **kw):
        calls.append(t.numel())
        return real(t, *a, **kw)

    dist.all_reduce = counted
    try:
        res, counts = _run_fake()
    finally:
        dist.all_reduce = real
    out_q.put((rank, res, counts, calls))
    dist.destroy_process_group()


def test_gloo_world2_run_sharded_quantiles_matches_world1(msim_lib_path):
    from miningsimulation_amd import quantile_rank

    _built()
    want, counts = _run_fake()  # no process group: world 1
    f, s, L = rr.synthetic(N_TOTAL, M_SH, shift=5, seed=7)
    assert want["ranks"] == [quantile_rank(N_TOTAL, q) for q in QS] == [1, 14, 27, 28]
    assert not rr.diff(want["order"], rr.select(f, s, L, want["ranks"]))
    assert [int(r[0]) for r in want["sums"]] == f.astype(np.int64).sum(axis=0).tolist()
    assert counts == [(p, n) for p in range(8) for n in (6, 6, 6, 6, 5)]  # five resident buffers, every pass

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    words = M_SH * 4 * len(QS) * 256
    for rank, res, counts, calls in got:
        assert res == want, rank
        # eight all-reduces of the counts view; the sums and status words ride behind the first
        assert calls == [words + 6 * M_SH + 2] + [words] * 7, (rank, calls)
        assert counts == [(p, n) for p in range(8) for n in ((6, 6, 3) if rank == 0 else (6, 6, 2))]

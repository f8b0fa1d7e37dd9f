"""The bootstrap kernels (msim_boot.hip) and the entry points over them, on the device.

Synthetic records through the launches, compared word by word with tests/boot_reference.py at run, item and replicate
counts around the kernels' tile (32 replicates), lane and workgroup boundaries; then the end-to-end cases against the
oracle's per-run counters, where replicate 0 must also reproduce run_quantiles' order statistic and run_tails'
expected shortfall. Every comparison is exact."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import boot_reference as br
import classes_reference as cls
import rank_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
BOOT_SEED = 0x5EEDB007
DAY = 86_400_000
YEAR_MS = 31_556_952_000
SHORT_MS = 10**9
E2E_BEGIN = 7000
QS = (1e-9, 0.05, 0.5, 1.0)
U64 = 2**64 - 1


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C").view(np.int32)).to(torch.device("cuda", 0))  # a writable copy


def synthetic_points(p, n, m, seed=0):
    pts = [rr.synthetic(n, m, shift=(3 * k + seed) % 9 if m < 9 else k, seed=seed + k) for k in range(p)]
    return (np.stack([x[0] for x in pts]), np.stack([x[1] for x in pts]), np.stack([x[2] for x in pts]))


def pick_items(p, m, count):
    """`count` items spread over every (point, column, quantity), the quantile index cycling over QS."""
    pool = [(pt, k, q, (pt + k + q) % len(QS)) for pt in range(p) for k in range(m) for q in range(4)]
    step = max(1, len(pool) // count) | 1
    picked = pool[::step][:count]
    return picked + pool[:count - len(picked)]


def gpu_select(f, s, L, items, B, seed=BOOT_SEED, run_begin=0, cuts=(), fill=-1, qs=QS):
    """W and rows[i][b] through the launches: weights per buffer, begin, eight count-per-buffer and step rounds, the
    below pass per buffer. `cuts` splits the runs into several record buffers; the workspace, W's scratch and the
    rows start filled with `fill` (0xFF bytes by default)."""
    import torch

    from miningsimulation_amd import bootstrap as bs

    p, n, m = f.shape
    dev = torch.device("cuda", 0)
    edges = [0, *cuts, n]
    bufs = [(a, b - a, _dev(rr.records(f[:, a:b], s[:, a:b])), _dev(L[:, a:b])) for a, b in zip(edges, edges[1:])]
    d_W = torch.zeros(B, dtype=torch.int64, device=dev)
    for a, cnt, _, _ in bufs:
        bs.launch_boot_weights(seed, run_begin + a, cnt, B, d_W)
    W = d_W.cpu().numpy().view(np.uint64).tolist()
    ws = torch.full((bs.boot_workspace_bytes(len(items), B) // 8,), fill, dtype=torch.int64, device=dev)
    rows = torch.full((len(items), B, 5), fill, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bs._launch_boot_begin(m, p, items, B, bs.boot_ranks(W, qs), len(qs), ws, None)
    for pass_ in range(8):
        for a, cnt, d_rec, d_bh in bufs:
            bs._launch_boot_count(m, p, seed, run_begin + a, cnt, d_rec, d_bh, len(items), B, pass_, ws, None)
        bs._launch_boot_step(len(items), B, pass_, ws, rows if pass_ == 7 else None, status, None)
    for a, cnt, d_rec, d_bh in bufs:
        bs._launch_boot_below(m, p, seed, run_begin + a, cnt, d_rec, d_bh, len(items), B, ws, rows, None)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    off, words = bs.boot_counts_view(len(items), B)
    assert (ws[off // 8:off // 8 + words] == 0).all(), "the last step leaves the counts zero"
    return W, rows.cpu().numpy().view(np.uint64).tolist()


def reference(f, s, L, items, B, seed=BOOT_SEED, run_begin=0, qs=QS):
    return br.bootstrap([br.point_keys(f[k], s[k], L[k]) for k in range(f.shape[0])], items, qs, B, seed, run_begin)


def _check(got, want, what):
    assert got[0] == want[0], (what, "W")
    bad = br.diff_rows(got[1], want[1])
    assert not bad, (what, bad[:8])


# runs x items x replicates x points: every run count 1, 3, 255, 256, 257, 513, item count 1, 4, 37 and replicate count
# 1, 2, 31, 32, 33, 65, 257 (around the tile of 32) occurs, with one and with three points
SHAPES = [(1, 1, 1, 1), (1, 4, 65, 1), (3, 4, 33, 3), (3, 37, 2, 1), (255, 4, 31, 3), (256, 1, 32, 1), (256, 4, 33, 1),
          (257, 37, 65, 3), (257, 4, 257, 1), (513, 4, 257, 1), (513, 37, 2, 3), (513, 1, 31, 1)]


@pytest.mark.parametrize("n,count,B,p", SHAPES)
def test_gpu_boot_synthetic(msim, n, count, B, p):
    f, s, L = synthetic_points(p, n, 9, seed=n)
    items = pick_items(p, 9, count)
    got = gpu_select(f, s, L, items, B)
    _check(got, reference(f, s, L, items, B), (n, count, B, p))
    assert got[0][0] == n
    if n <= 3 and B >= 33:
        empty = [b for b in range(B) if got[0][b] == 0]
        assert empty and all(got[1][i][b] == [0] * 5 for i in range(count) for b in empty)


def test_gpu_boot_1026_columns(msim):
    """Column indices up to 1 025 at 65 runs and 3 points, and a run_begin past 2^32."""
    f, s, L = synthetic_points(3, 65, 1026, seed=5)
    items = [(pt, k, q, q) for pt in range(3) for k, q in ((0, 0), (1, 1), (511, 2), (1024, 3), (1025, 2), (1025, 3))]
    _check(gpu_select(f, s, L, items, 33), reference(f, s, L, items, 33), "1026 columns")
    rb = 2**40 + 7
    _check(gpu_select(f, s, L, items, 33, run_begin=rb), reference(f, s, L, items, 33, run_begin=rb), "run_begin")


def test_gpu_boot_several_workgroups(msim, monkeypatch):
    """MSIM_BOOT_TEST_WG_RUNS=64: 513 runs are nine workgroups along the runs; then one run per workgroup."""
    f, s, L = synthetic_points(3, 513, 9, seed=1)
    items = pick_items(3, 9, 37)
    whole = gpu_select(f, s, L, items, 65)
    monkeypatch.setenv("MSIM_BOOT_TEST_WG_RUNS", "64")
    parts = gpu_select(f, s, L, items, 65)
    assert parts == whole
    _check(parts, reference(f, s, L, items, 65), "nine workgroups")
    monkeypatch.setenv("MSIM_BOOT_TEST_WG_RUNS", "1")
    few = pick_items(1, 9, 4)
    _check(gpu_select(f[:1, :65], s[:1, :65], L[:1, :65], few, 33), reference(f[:1, :65], s[:1, :65], L[:1, :65], few, 33),
           "one run per workgroup")


def test_gpu_boot_two_buffers_and_fills(msim):
    """100 + 157 runs through two record buffers equal the 257 runs in one; a zero fill and the 0xFF fill of the
    workspace and the rows give the same words; three buffers at 3 runs keep the empty replicates."""
    f, s, L = synthetic_points(3, 257, 9, seed=2)
    items = pick_items(3, 9, 37)
    one = gpu_select(f, s, L, items, 33)
    assert gpu_select(f, s, L, items, 33, cuts=(100,)) == one
    assert gpu_select(f, s, L, items, 33, fill=0) == one
    _check(one, reference(f, s, L, items, 33), "two buffers")
    few = pick_items(1, 9, 4)
    tiny = gpu_select(f[:1, :3], s[:1, :3], L[:1, :3], few, 65, cuts=(1, 2))
    _check(tiny, reference(f[:1, :3], s[:1, :3], L[:1, :3], few, 65), "three buffers of one run")
    assert any(w == 0 for w in tiny[0])


def test_gpu_boot_extreme_and_all_equal_columns(msim):
    """found 0 / 2^32 - 1, a rate key of 2^64 - 2^32, and the all-equal column: below = 0, equal = W_b."""
    f, s, L = br.extreme_columns(257)
    f, s, L = f[None], s[None], L[None]
    items = [(0, k, q, j) for k in range(3) for q in range(4) for j in (1, 3)]
    W, rows = gpu_select(f, s, L, items, 65)
    _check((W, rows), reference(f, s, L, items, 65), "extremes")
    for i, it in enumerate(items):
        if it[1] == 0:
            assert all(rows[i][b][1] == 0 and rows[i][b][2] == W[b] and rows[i][b][3:] == [0, 0] for b in range(65))
    assert rows[items.index((0, 2, 3, 3))][0][0] == 2**64 - 2**32
    assert rows[items.index((0, 1, 0, 3))][0][0] == 2**32 - 1


def test_gpu_boot_unprepared_workspace_is_a_noop(msim):
    """A count, a step and a below on a workspace no begin prepared (0xFF, zero, or begun for another shape) write
    nothing."""
    import torch

    from miningsimulation_amd import bootstrap as bs

    f, s, L = synthetic_points(1, 65, 9)
    items = pick_items(1, 9, 4)
    dev = torch.device("cuda", 0)
    d_rec, d_bh = _dev(rr.records(f, s)), _dev(L)
    n_words = bs.boot_workspace_bytes(4, 33) // 8
    for fill in (-1, 0):
        ws = torch.full((n_words,), fill, dtype=torch.int64, device=dev)
        rows = torch.full((4, 33, 5), -1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        bs._launch_boot_count(9, 1, BOOT_SEED, 0, 65, d_rec, d_bh, 4, 33, 0, ws, None)
        bs._launch_boot_step(4, 33, 7, ws, rows, status, None)
        bs._launch_boot_below(9, 1, BOOT_SEED, 0, 65, d_rec, d_bh, 4, 33, ws, rows, None)
        torch.cuda.synchronize()
        assert (ws == fill).all() and (rows == -1).all() and int(status.item()) == 0
    # begun for 4 items x 33 replicates of 9 columns: launches that name another shape leave it alone
    ws = torch.full((bs.boot_workspace_bytes(8, 65) // 8,), -1, dtype=torch.int64, device=dev)
    bs._launch_boot_begin(9, 1, items, 33, bs.boot_ranks([65] * 33, QS), len(QS), ws, None)
    before = ws.clone()
    rows = torch.full((8, 65, 5), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bs._launch_boot_count(9, 1, BOOT_SEED, 0, 65, d_rec, d_bh, 4, 32, 0, ws, None)
    bs._launch_boot_count(9, 1, BOOT_SEED, 0, 65, d_rec, d_bh, 8, 33, 0, ws, None)
    bs._launch_boot_step(4, 65, 7, ws, rows, status, None)
    bs._launch_boot_below(9, 1, BOOT_SEED, 0, 65, d_rec, d_bh, 3, 33, ws, rows, None)
    torch.cuda.synchronize()
    assert torch.equal(ws, before) and (rows == -1).all()


def test_gpu_boot_refused_launches_write_nothing(msim):
    import torch

    from miningsimulation_amd import _lib
    from miningsimulation_amd import bootstrap as bs

    lib, E = _lib.lib, _lib.MSIM_E_INVALID
    p_ = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None)
    f, s, L = synthetic_points(1, 65, 9)
    dev = torch.device("cuda", 0)
    d_rec, d_bh = _dev(rr.records(f, s)), _dev(L)
    nb = bs.boot_workspace_bytes(4, 33)
    ws = torch.full((nb // 8,), -1, dtype=torch.int64, device=dev)
    rows = torch.full((4, 33, 5), -1, dtype=torch.int64, device=dev)
    W = torch.full((33,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    items = (_lib.MsimBootItem * 4)(*[_lib.MsimBootItem(*it) for it in pick_items(1, 9, 4)])
    ranks = (ctypes.c_uint64 * (4 * 33))(*([0] * 132))
    for runs, B, w in ((0, 33, W), (1 << 32, 33, W), (65, 0, W), (65, 4097, W), (65, 33, None)):
        assert lib.msim_boot_weights_launch(1, 0, runs, B, p_(w), None) == E
    ok = dict(m=9, np_=1, items=items, ni=4, B=33, ranks=ranks, nq=4, ws=ws, wsb=nb)
    for ch in (dict(m=0), dict(np_=0), dict(items=None), dict(ni=0), dict(B=0), dict(B=4097), dict(ranks=None), dict(nq=0),
               dict(nq=33), dict(ws=None), dict(wsb=nb - 1), dict(m=6)):  # m = 6: an item names column 6
        a = dict(ok, **ch)
        assert lib.msim_boot_begin_launch(a["m"], a["np_"], a["items"], a["ni"], a["B"], a["ranks"], a["nq"], p_(a["ws"]),
                                          a["wsb"], None) == E, ch
    ok = dict(m=9, np_=1, runs=65, rec=d_rec, bh=d_bh, ni=4, B=33, p=0, ws=ws, wsb=nb, rows=rows)
    for ch in (dict(m=0), dict(np_=0), dict(runs=0), dict(runs=1 << 32), dict(rec=None), dict(bh=None), dict(ni=0),
               dict(B=0), dict(p=8), dict(ws=None), dict(wsb=nb - 1), dict(rows=None)):
        a = dict(ok, **ch)
        if "rows" not in ch:
            assert lib.msim_boot_count_launch(a["m"], a["np_"], 1, 0, a["runs"], p_(a["rec"]), p_(a["bh"]), a["ni"], a["B"],
                                              a["p"], p_(a["ws"]), a["wsb"], None) == E, ch
        if "p" not in ch:
            assert lib.msim_boot_below_launch(a["m"], a["np_"], 1, 0, a["runs"], p_(a["rec"]), p_(a["bh"]), a["ni"], a["B"],
                                              p_(a["ws"]), a["wsb"], p_(a["rows"]), None) == E, ch
    for ni, B, ps, w, wsb, out, st in ((0, 33, 0, ws, nb, rows, status), (4, 0, 0, ws, nb, rows, status),
                                       (4, 33, 8, ws, nb, rows, status), (4, 33, 0, None, nb, rows, status),
                                       (4, 33, 0, ws, nb - 1, rows, status), (4, 33, 7, ws, nb, None, status),
                                       (4, 33, 0, ws, nb, rows, None)):
        assert lib.msim_boot_step_launch(ni, B, ps, p_(w), wsb, p_(out), p_(st), None) == E
    torch.cuda.synchronize()
    assert (ws == -1).all() and (rows == -1).all() and (W == -1).all() and int(status.item()) == 0
    with pytest.raises(ValueError):
        bs._launch_boot_count(9, 1, 1, 0, 66, d_rec, d_bh, 4, 33, 0, ws, None)
    with pytest.raises(ValueError):
        bs._launch_boot_step(4, 33, 7, ws, rows[:3], status, None)


# ---------------------------------------------------------------- end to end against the oracle
_ORACLE = {}
E2E_QS = (0.05, 0.5)
E2E_B = 33


def _oracle(oracle, key, miners, n_runs, duration, total_weight=100, begin=E2E_BEGIN):
    if key not in _ORACLE:
        f, s, _, _ = oracle.run_batch([m.perc for m in miners], [m.propagation_ms for m in miners],
                                      [m.is_selfish for m in miners], duration, n_runs, begin, SEED, threads=16,
                                      total_weight=total_weight)
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[key] = (f, s, f.sum(axis=1))
    return _ORACLE[key]


def _items(msim, points, cols):
    """Every column's share at q = 0.05 and its found count at the median."""
    return msim.own_bootstrap(points, cols, "share", 0) + msim.own_bootstrap(points, cols, "found", 1)


def _check_result(res, sets, what, quant, tails):
    """A BootstrapResult against the reference over `sets` = [(f, s, L)] per point, and its replicate 0 against the
    run_quantiles and run_tails results of the same runs."""
    f, s, L = (np.stack([x[i] for x in sets]) for i in range(3))
    n = f.shape[1]
    W, rows = reference(f, s, L, [tuple(it) for it in res.items], res.replicates, seed=res.boot_seed, run_begin=E2E_BEGIN,
                        qs=E2E_QS)
    assert res.W == W and res.W[0] == n == res.n_runs, what
    bad = br.diff_rows(res.rows.tolist(), rows)
    assert not bad, (what, bad[:8])
    assert res.order == quant.order and res.ranks == quant.ranks, what
    for i, it in enumerate(res.items):
        o = quant.order[it.point][it.column][it.quantity][it.q_index]
        assert res.row(i, 0)[:3] == tuple(o), (what, it)
        assert res.shortfalls(i) == [br.shortfall(tuple(r), W[b], E2E_QS[it.q_index]) for b, r in enumerate(rows[i])]
        if it.quantity == 2 and it.q_index == 0:  # run_tails' default specs: every column's own share at q = 0.05
            assert res.shortfalls(i)[0] == tails.expected_shortfall(it.column, it.point), (what, it)
    assert [pt.stats_total for pt in res.points] == [pt.stats_total for pt in quant.points], what


def _run_all(target, n, items, **kw):
    res = target.run_bootstrap(n, items=items, qs=E2E_QS, replicates=E2E_B, boot_seed=BOOT_SEED, run_begin=E2E_BEGIN,
                               seed_base=SEED, **kw)
    quant = target.run_quantiles(n, qs=E2E_QS, run_begin=E2E_BEGIN, seed_base=SEED, **kw)
    tails = target.run_tails(n, q=E2E_QS, run_begin=E2E_BEGIN, seed_base=SEED, **kw)
    return res, quant, tails


def test_gpu_bootstrap_default_network_against_oracle(msim, oracle, monkeypatch):
    """setup_miners() at 10^9 ms, where the 1 % miners' found counts are heavily tied; whole and in three chunks."""
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, SHORT_MS)
    sets = [_oracle(oracle, ("default", SHORT_MS), miners, 257, SHORT_MS)]
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 9))
    _check_result(res, sets, "default", quant, tails)
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    parts = sim.run_bootstrap(257, items=_items(msim, 1, 9), qs=E2E_QS, replicates=E2E_B, boot_seed=BOOT_SEED,
                              run_begin=E2E_BEGIN, seed_base=SEED)
    assert parts.rows.tolist() == res.rows.tolist() and parts.W == res.W
    monkeypatch.delenv("MSIM_MOMENTS_CHUNK_RUNS")
    own = sim.run_bootstrap(257, replicates=E2E_B, boot_seed=BOOT_SEED, run_begin=E2E_BEGIN, seed_base=SEED)  # defaults
    assert own.items == msim.own_bootstrap(1, 9) and own.rows.tolist() == res.rows[:9].tolist()


def test_gpu_bootstrap_year_in_three_chunks_against_oracle(msim, oracle, monkeypatch):
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, YEAR_MS)
    sets = [_oracle(oracle, ("default", YEAR_MS), miners, 257, YEAR_MS)]
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 9))
    _check_result(res, sets, "year", quant, tails)


def test_gpu_bootstrap_selfish_against_oracle(msim, oracle):
    miners = msim.setup_miners(1000, selfish_perc=40)
    sim = msim.Simulation(miners, SHORT_MS)
    assert sim.pipeline_info(257)["uses_pipeline"] == 3
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 9))
    _check_result(res, [_oracle(oracle, "selfish", miners, 257, SHORT_MS)], "selfish", quant, tails)


def test_gpu_bootstrap_wide_network_against_oracle(msim, oracle):
    miners = [msim.Miner(k, 6 if k < 15 else 5, 1000) for k in range(17)]
    sim = msim.Simulation(miners, 30 * DAY)
    assert sim.wide
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 17))
    _check_result(res, [_oracle(oracle, "wide17", miners, 257, 30 * DAY)], "wide", quant, tails)


def test_gpu_bootstrap_general_engine_against_oracle(msim, oracle):
    miners = [msim.Miner(k, 20, 1000, True) for k in range(5)]
    sim = msim.Simulation(miners, 3 * DAY)
    assert sim.pipeline_info(257)["uses_pipeline"] == 4
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 5))
    _check_result(res, [_oracle(oracle, "general", miners, 257, 3 * DAY)], "general", quant, tails)


def test_gpu_bootstrap_sweep_difference_against_oracle(msim, oracle):
    """A two-point propagation_sweep: every item at both points, and miner 7's q = 0.05 share at 10 s minus the same
    seeds' at 100 ms, replicate by replicate."""
    miners = msim.setup_miners()
    props = (10_000, 100)
    sw = msim.propagation_sweep(miners, props, SHORT_MS)
    sets = [_oracle(oracle, ("default", prop), msim.setup_miners(prop), 257, SHORT_MS) for prop in props]
    items = _items(msim, 2, 9) + msim.across_points(7, 2, "share", 0)
    res, quant, tails = _run_all(sw, 257, items)
    _check_result(res, sets, "sweep", quant, tails)
    i, j = len(items) - 2, len(items) - 1
    assert (res.items[i].point, res.items[j].point) == (0, 1)
    for sf in (False, True):
        d = res.difference(i, j, 0.9, shortfall=sf)
        xs = res.shortfalls(i) if sf else res.values(i)
        ys = res.shortfalls(j) if sf else res.values(j)
        assert (d.data, d.diffs, d.variance, d.interval) == br.difference(xs, ys, 0.9)
        assert len(d.diffs) == E2E_B - 1 and d.data == Fraction(xs[0]) - Fraction(ys[0])


def test_gpu_bootstrap_classes_against_oracle(msim, oracle):
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    sim = msim.Simulation(miners, SHORT_MS)
    f, s, L = _oracle(oracle, ("default", SHORT_MS), miners, 257, SHORT_MS)
    cf, cs = cls.fold(f, s, cmap, len(members))
    res, quant, tails = _run_all(sim, 257, _items(msim, 1, 8), class_of=cmap)
    assert len(res.order[0]) == 8 and len(res.points[0].stats_total) == 9
    _check_result(res, [(cf, cs, L)], "classes", quant, tails)
    lines = msim.report_bootstrap(miners, res, members=members).splitlines()
    assert len(lines) == 16 and lines[7].startswith("  - Class 7 (2 miners, 2% of network hashrate) share q0.05 = ")


def test_gpu_bootstrap_launch_methods_and_report_agree(msim):
    """Simulation.launch_boot_* on the simulation's own launch against run_bootstrap, and report_bootstrap and
    BootstrapResult against the raw words."""
    import math

    import torch

    from miningsimulation_amd import bootstrap as bs

    miners = msim.setup_miners()
    sim = msim.Simulation(miners)
    n, B, dev = 64, 33, torch.device("cuda", 0)
    res = sim.run_bootstrap(n, qs=(0.05,), replicates=B, boot_seed=BOOT_SEED, run_begin=0, seed_base=SEED)
    sums = torch.zeros((9, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((n, 9, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.empty(sim.workspace_bytes(n), dtype=torch.uint8, device=dev)
    sim.launch(n, 0, SEED, sums, ws, status, d_per_run=rec, d_best_height=bh)
    d_W = torch.zeros(B, dtype=torch.int64, device=dev)
    msim.launch_boot_weights(BOOT_SEED, 0, n, B, d_W)
    W = d_W.cpu().tolist()
    assert W == res.W
    bws = torch.full((bs.boot_workspace_bytes(9, B) // 8,), -1, dtype=torch.int64, device=dev)
    rows = torch.full((9, B, 5), -1, dtype=torch.int64, device=dev)
    bstatus = torch.zeros(1, dtype=torch.int32, device=dev)
    sim.launch_boot_begin(res.items, B, msim.boot_ranks(W, (0.05,)), 1, bws)
    for pass_ in range(8):
        sim.launch_boot_count(n, rec, bh, BOOT_SEED, 0, 9, B, pass_, bws)
        sim.launch_boot_step(9, B, pass_, bws, rows, bstatus)
    sim.launch_boot_below(n, rec, bh, BOOT_SEED, 0, 9, B, bws, rows)
    torch.cuda.synchronize()
    assert rows.cpu().numpy().view(np.uint64).tolist() == res.rows.tolist() and int(bstatus.item()) == 0
    # the result's statistics from the raw words
    for i in range(9):
        raw = res.rows[i].tolist()
        vals = [r[0] for r in raw]
        assert res.n_empty(i) == 0 and res.values(i) == vals
        assert res.variance(i) == br.variance(vals) and res.se(i) == math.sqrt(float(br.variance(vals)))
        es = [br.shortfall(tuple(r), W[b], 0.05) for b, r in enumerate(raw)]
        assert res.shortfalls(i) == es and res.shortfall_se(i) == math.sqrt(float(br.variance(es)))
        assert res.interval(i, 0.9) == br.interval(vals, 0.9)
    text = msim.report_bootstrap(miners, res).splitlines()
    assert len(text) == 9
    v0, se0 = res.values(0)[0] * 2.0 ** -32 * 100, res.se(0) * 2.0 ** -32 * 100
    assert text[0].startswith(f"  - Miner 0 (30% of network hashrate) share q0.05 = {v0:g}% (SE {se0:g}%, 95% interval ")
    assert text[0].endswith(f"; {B - 1} replicates, 0 empty.")

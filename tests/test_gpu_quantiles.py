"""The rank selection kernels (msim_rank.hip) and the entry points over them, on the device.

Synthetic records through msim_rank_launch and the three primitives, compared as (value, below, equal) triples with
tests/rank_reference.py at run, column, point and rank counts around the kernels' tile, lane and workgroup
boundaries; then the end-to-end cases against the oracle's per-run counters sorted on the host. Every comparison is
exact."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import classes_reference as cls
import rank_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
DAY = 86_400_000
SHORT_MS = 10**9
E2E_BEGIN = 7000
RUN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
M_COUNTS = (1, 2, 9, 17, 257)
POINT_COUNTS = (1, 3)
QS = (0.05, 0.5, 0.95)


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


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _buffers(m, points, n_ranks, fill=None):
    """(workspace uint8, out int64 [points, m, 4, n_ranks, 3] filled with -1, status int32 [1] = 0) on the device."""
    import torch

    from miningsimulation_amd import _lib

    dev = torch.device("cuda", 0)
    ws = torch.empty(_lib.lib.msim_rank_workspace_bytes(m, points, n_ranks), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    out = torch.full((points, m, 4, n_ranks, 3), -1, dtype=torch.int64, device=dev)
    return ws, out, torch.zeros(1, dtype=torch.int32, device=dev)


def _select(m, points, runs, d_rec, d_bh, ranks, fill=None):
    """msim_rank_launch -> (order[point][column][quantity][j] triples as lists, status word)."""
    import torch

    from miningsimulation_amd import _lib

    ws, out, status = _buffers(m, points, len(ranks), fill)
    rk = (ctypes.c_uint64 * len(ranks))(*ranks)
    rc = _lib.lib.msim_rank_launch(m, points, runs, _p(d_rec), _p(d_bh), rk, len(ranks), _p(out), _p(status), _p(ws),
                                   ws.numel(), None)
    assert rc == _lib.MSIM_OK, rc
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).tolist(), int(status.item())


class _Data:
    """Synthetic records of the largest shape for one column count, one independent set per point; slices of it
    are the smaller shapes."""

    def __init__(self, m, shift=0):
        pmax, rmax = max(POINT_COUNTS), max(RUN_COUNTS)
        sets = [rr.synthetic(rmax, m, shift=shift, seed=100 * m + p) for p in range(pmax)]
        self.f = np.stack([x[0] for x in sets])
        self.s = np.stack([x[1] for x in sets])
        self.L = np.stack([x[2] for x in sets])
        for a in (self.f, self.s, self.L):
            a.setflags(write=False)

    def device(self, points, runs):
        return (_dev(rr.records(self.f[:points, :runs], self.s[:points, :runs])), _dev(self.L[:points, :runs]))

    def want(self, points, runs, ranks):
        return [rr.select(self.f[p, :runs], self.s[p, :runs], self.L[p, :runs], ranks) for p in range(points)]


def _check(got, want, what):
    for p, (g, w) in enumerate(zip(got, want)):
        bad = rr.diff(g, w)
        assert not bad, (what, p, bad[:8])


@pytest.mark.parametrize("m", M_COUNTS)
def test_gpu_rank_synthetic(msim, m):
    """Every run count and point count with rank lists of 1, 3, 5 and 32 ranks at one column count. Below nine
    columns the patterns are shifted so that the extreme columns are among them."""
    data = _Data(m, shift=3 if m < 9 else 0)
    for points in POINT_COUNTS:
        for runs in RUN_COUNTS:
            d_rec, d_bh = data.device(points, runs)
            for nr, ranks in rr.rank_lists(runs).items():
                got, status = _select(m, points, runs, d_rec, d_bh, ranks)
                assert status == 0
                _check(got, data.want(points, runs, ranks), (m, points, runs, nr))


def test_gpu_rank_1026_columns(msim):
    data = _Data(1026)
    for points in POINT_COUNTS:
        d_rec, d_bh = data.device(points, 65)
        for nr, ranks in rr.rank_lists(65).items():
            got, status = _select(1026, points, 65, d_rec, d_bh, ranks)
            assert status == 0
            _check(got, data.want(points, 65, ranks), (points, nr))


def test_gpu_rank_all_equal_and_extremes(msim):
    """The named columns at 513 runs: equal == N where a column is constant, bit 32, the 0xFF top byte, L == 0."""
    data = _Data(9)
    d_rec, d_bh = data.device(1, 513)
    got, _ = _select(9, 1, 513, d_rec, d_bh, [256, 0, 512])
    col = got[0]
    assert all(col[0][q][j] == [0, 0, 513] for q in range(4) for j in range(3))             # all zero
    assert col[1][0] == [[6, 0, 513]] * 3 and col[1][1] == [[2, 0, 513]] * 3                 # all equal
    assert col[1][3][0][1:] == [0, 513]
    assert col[2][2][2][0] == 1 << 32                                                        # f == L: bit 32
    assert col[3][3][2][0] == 2**64 - 2**32 and col[3][3][2][2] == 256                       # top byte 0xFF
    n_zero = int((data.L[0, :513] == 0).sum())
    assert col[4][2][1] == [0, 0, n_zero] and col[4][0][1] == [5, 0, 513]                    # L == 0 with f > 0
    assert [c[0] for c in col[7][0]] == [257, 1, 513]                                        # strictly increasing
    _check(got, data.want(1, 513, [256, 0, 512]), "extremes")


def test_gpu_rank_several_workgroups(msim, monkeypatch):
    """MSIM_RANK_TEST_WG_RUNS=64: 513 runs are nine workgroups along the runs; the result is the unset one's."""
    data = _Data(17)
    d_rec, d_bh = data.device(3, 513)
    ranks = rr.rank_lists(513)[32]
    whole, _ = _select(17, 3, 513, d_rec, d_bh, ranks)
    monkeypatch.setenv("MSIM_RANK_TEST_WG_RUNS", "64")
    parts, status = _select(17, 3, 513, d_rec, d_bh, ranks)
    assert status == 0 and parts == whole
    _check(parts, data.want(3, 513, ranks), "nine workgroups")
    monkeypatch.setenv("MSIM_RANK_TEST_WG_RUNS", "1")
    ones, _ = _select(17, 1, 65, *data.device(1, 65), rr.rank_lists(65)[5])
    _check(ones, data.want(1, 65, rr.rank_lists(65)[5]), "one run per workgroup")


def test_gpu_rank_workspace_filled_with_ff(msim):
    """begin clears everything the later launches read."""
    data = _Data(9)
    d_rec, d_bh = data.device(3, 257)
    for nr, ranks in rr.rank_lists(257).items():
        clean, _ = _select(9, 3, 257, d_rec, d_bh, ranks, fill=0)
        dirty, status = _select(9, 3, 257, d_rec, d_bh, ranks, fill=0xFF)
        assert status == 0 and dirty == clean
    _check(dirty, data.want(3, 257, ranks), "0xFF")


def _primitives(m, points, buffers, ranks, fill=0xFF):
    """begin, then per pass one count per (runs, d_rec, d_bh) buffer and one step."""
    import torch

    from miningsimulation_amd import _lib

    lib = _lib.lib
    ws, out, status = _buffers(m, points, len(ranks), fill)
    rk = (ctypes.c_uint64 * len(ranks))(*ranks)
    assert lib.msim_rank_begin_launch(m, points, rk, len(ranks), _p(ws), ws.numel(), None) == 0
    for p in range(8):
        for runs, d_rec, d_bh in buffers:
            assert lib.msim_rank_count_launch(m, points, runs, _p(d_rec), _p(d_bh), p, _p(ws), ws.numel(), None) == 0
        assert lib.msim_rank_step_launch(m, points, p, _p(ws), ws.numel(), _p(out) if p == 7 else None, _p(status), None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).tolist(), int(status.item())


def test_gpu_rank_two_buffers_through_the_primitives(msim):
    """100 + 157 runs through begin / count x 2 / step equal msim_rank_launch on the 257 runs in one buffer."""
    data = _Data(9)
    f, s, L = data.f[0, :257], data.s[0, :257], data.L[0, :257]
    ranks = rr.rank_lists(257)[32]
    one, _ = _select(9, 1, 257, _dev(rr.records(f, s)), _dev(L), ranks)
    two, status = _primitives(9, 1, [(100, _dev(rr.records(f[:100], s[:100])), _dev(L[:100])),
                                     (157, _dev(rr.records(f[100:], s[100:])), _dev(L[100:]))], ranks)
    assert status == 0 and two == one
    _check(two, data.want(1, 257, ranks), "two buffers")


def test_gpu_rank_past_the_runs_sets_the_status(msim):
    """A rank >= N given straight to the primitives: the status word is non-zero, that rank's rows are not written,
    and the other ranks' rows are correct."""
    data = _Data(9)
    d_rec, d_bh = data.device(1, 65)
    ranks = [65, 32, 0, 2**64 - 1, 64, 32]
    got, status = _primitives(9, 1, [(65, d_rec, d_bh)], ranks)
    assert status != 0
    _check(got, data.want(1, 65, ranks), "bad rank")
    untouched = [2**64 - 1] * 3  # the fill of `out`
    assert all(got[0][k][q][j] == untouched for k in range(9) for q in range(4) for j in (0, 3))
    got, status = _select(9, 1, 65, d_rec, d_bh, ranks)
    assert status != 0
    _check(got, data.want(1, 65, ranks), "bad rank, one launch")


def test_gpu_rank_refused_launches_write_nothing(msim):
    import torch

    from miningsimulation_amd import _lib

    lib = _lib.lib
    data = _Data(9)
    d_rec, d_bh = data.device(1, 65)
    ws, out, status = _buffers(9, 1, 3, fill=0xFF)
    rk = (ctypes.c_uint64 * 3)(0, 1, 2)
    E = _lib.MSIM_E_INVALID
    assert lib.msim_rank_begin_launch(9, 1, rk, 3, _p(ws), ws.numel() - 1, None) == E
    assert lib.msim_rank_begin_launch(9, 1, rk, 33, _p(ws), ws.numel(), None) == E
    assert lib.msim_rank_count_launch(9, 1, 65, _p(d_rec), _p(d_bh), 8, _p(ws), ws.numel(), None) == E
    assert lib.msim_rank_step_launch(9, 1, 7, _p(ws), ws.numel(), None, _p(status), None) == E
    assert lib.msim_rank_launch(9, 1, 0, _p(d_rec), _p(d_bh), rk, 3, _p(out), _p(status), _p(ws), ws.numel(), None) == E
    # a count and a step on a workspace that no begin prepared do nothing
    assert lib.msim_rank_count_launch(9, 1, 65, _p(d_rec), _p(d_bh), 0, _p(ws), ws.numel(), None) == 0
    assert lib.msim_rank_step_launch(9, 1, 7, _p(ws), ws.numel(), _p(out), _p(status), None) == 0
    torch.cuda.synchronize()
    assert (ws == 0xFF).all() and (out == -1).all() and int(status.item()) == 0


# ---------------------------------------------------------------- end to end against the oracle
_ORACLE = {}


def _oracle(oracle, key, miners, n_runs, duration, total_weight=100, begin=E2E_BEGIN):
    if key not in _ORACLE:
        f, s, _, _ = oracle.run_batch([m.perc for m in miners], [m.propagation_ms for m in miners],
                                      [m.is_selfish for m in miners], duration, n_runs, begin, SEED, threads=16,
                                      total_weight=total_weight)
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[key] = (f, s, f.sum(axis=1))
    return _ORACLE[key]


def _as_lists(order_point):
    return [[[list(o) for o in row] for row in col] for col in order_point]


def _check_result(res, point, f, s, L, what):
    bad = rr.diff(_as_lists(res.order[point]), rr.select(f, s, L, res.ranks))
    assert not bad, (what, bad[:8])


def test_gpu_quantiles_default_network_against_oracle(msim, oracle, monkeypatch):
    """setup_miners() at 1 s on the honest pipeline, 257 runs of 10^9 ms: quantiles, explicit ranks, the three-buffer
    run (MSIM_MOMENTS_CHUNK_RUNS=100), and the median inside hist_quantile's bin."""
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, SHORT_MS)
    assert not sim.wide
    f, s, L = _oracle(oracle, "default", miners, 257, SHORT_MS)
    res = sim.run_quantiles(257, qs=QS, run_begin=E2E_BEGIN, seed_base=SEED)
    assert res.ranks == [msim.quantile_rank(257, q) for q in QS] == [12, 128, 244] and res.n_runs == 257
    _check_result(res, 0, f, s, L, "default")
    plain = sim.run(257, E2E_BEGIN, SEED, 0)
    assert res.points[0].stats_total == plain.stats_total
    assert [(x.blocks_found, x.share_lo) for x in res.points[0].sums] == [(x.blocks_found, x.share_lo) for x in plain.sums]
    ranks = rr.rank_lists(257)[32]
    by_rank = sim.run_quantiles(257, ranks=ranks, run_begin=E2E_BEGIN, seed_base=SEED)
    assert by_rank.qs is None and by_rank.ranks == ranks
    _check_result(by_rank, 0, f, s, L, "default, 32 ranks")
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    parts = sim.run_quantiles(257, ranks=ranks, run_begin=E2E_BEGIN, seed_base=SEED)
    monkeypatch.delenv("MSIM_MOMENTS_CHUNK_RUNS")
    assert parts.order == by_rank.order and parts.points[0].stats_total == by_rank.points[0].stats_total
    # the exact median lies inside the bin hist_quantile returns for the same runs
    spec = msim.HistSpec.covering(0.0, 1.0, 256)
    h = sim.run_moments(257, E2E_BEGIN, SEED, 0, hist=spec).hist
    for k in range(9):
        for w, which in enumerate(("share", "rate")):
            lo, hi = msim.hist_quantile(h[k, w], spec, 0.5, which)
            assert lo <= res.value(k, which, 1) < hi, (k, which)
    text = msim.report_quantiles(miners, res).splitlines()
    assert len(text) == 9 and text[0].startswith("  - Miner 0 (30% of network hashrate) blocks found: q0.05 = ")


def test_gpu_quantiles_selfish_against_oracle(msim, oracle):
    """One selfish network on the entity engine."""
    miners = msim.setup_miners(1000, selfish_perc=40)
    sim = msim.Simulation(miners, SHORT_MS)
    assert sim.pipeline_info(257)["uses_pipeline"] == 3
    f, s, L = _oracle(oracle, "selfish", miners, 257, SHORT_MS)
    res = sim.run_quantiles(257, qs=(0.0, 0.05, 0.5, 0.95, 1.0), run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, 0, f, s, L, "selfish")
    assert res.order[0][0][0][0].value == int(f[:, 0].min()) and res.order[0][0][0][4].value == int(f[:, 0].max())


def test_gpu_quantiles_wide_network_against_oracle(msim, oracle):
    """A 17-miner network on the large-network pipeline."""
    miners = [msim.Miner(k, 6 if k < 15 else 5, 1000) for k in range(17)]
    sim = msim.Simulation(miners, 30 * DAY)
    assert sim.wide
    f, s, L = _oracle(oracle, "wide17", miners, 65, 30 * DAY)
    res = sim.run_quantiles(65, qs=QS, run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, 0, f, s, L, "wide")


def test_gpu_quantiles_general_engine_against_oracle(msim, oracle):
    """A 3-day run of a network the general engine serves (five selfish miners)."""
    miners = [msim.Miner(k, 20, 1000, True) for k in range(5)]
    sim = msim.Simulation(miners, 3 * DAY)
    assert sim.pipeline_info(65)["uses_pipeline"] == 4
    f, s, L = _oracle(oracle, "general", miners, 65, 3 * DAY)
    res = sim.run_quantiles(65, qs=QS, run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, 0, f, s, L, "general")


def test_gpu_quantiles_sweep_against_oracle(msim, oracle):
    """A two-point propagation_sweep: every point's quantiles against its own oracle runs."""
    miners = msim.setup_miners()
    props = (10_000, 100)
    sw = msim.propagation_sweep(miners, props, SHORT_MS)
    res = sw.run_quantiles(257, qs=QS, run_begin=E2E_BEGIN, seed_base=SEED)
    assert len(res.order) == 2 and len(res.points) == 2
    for p, prop in enumerate(props):
        f, s, L = _oracle(oracle, ("default", prop), msim.setup_miners(prop), 257, SHORT_MS)
        _check_result(res, p, f, s, L, ("sweep", prop))
    assert res.order[0] != res.order[1]


def test_gpu_quantiles_classes_against_oracle(msim, oracle, monkeypatch):
    """class_of=: the oracle's counters through tests/classes_reference.py's fold, then the reference; chunked too."""
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    sim = msim.Simulation(miners, SHORT_MS)
    f, s, L = _oracle(oracle, "default", miners, 257, SHORT_MS)
    cf, cs = cls.fold(f, s, cmap, len(members))
    res = sim.run_quantiles(257, qs=QS, class_of=cmap, run_begin=E2E_BEGIN, seed_base=SEED)
    assert len(res.order[0]) == len(members) == 8 and len(res.points[0].stats_total) == 9
    _check_result(res, 0, cf, cs, L, "classes")
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    parts = sim.run_quantiles(257, qs=QS, class_of=cmap, run_begin=E2E_BEGIN, seed_base=SEED)
    assert parts.order == res.order
    lines = msim.report_quantiles(miners, res, members=members).splitlines()
    assert len(lines) == 8 and lines[7].startswith("  - Class 7 (2 miners, 2% of network hashrate) blocks found: ")


def test_gpu_quantiles_launch_methods(msim):
    """launch_rank_begin / count / step on a Simulation's own launch, beside launch_moments: equal to run_quantiles."""
    import torch

    sim = msim.Simulation(msim.setup_miners(), SHORT_MS)
    n, dev = 130, torch.device("cuda", 0)
    ranks = [msim.quantile_rank(n, q) for q in QS]
    sums = torch.zeros((9, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((n, 9, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.empty(sim.workspace_bytes(n), dtype=torch.uint8, device=dev)
    sim.launch(n, E2E_BEGIN, SEED, sums, ws, status, d_per_run=rec, d_best_height=bh)
    rws = torch.empty(sim.rank_workspace_bytes(3), dtype=torch.uint8, device=dev)
    out = torch.zeros((9, 4, 3, 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)
    sim.launch_rank_begin(ranks, rws)
    for p in range(8):
        sim.launch_rank_count(n, rec, bh, p, rws)
        sim.launch_rank_step(p, rws, out if p == 7 else None, rst)
    torch.cuda.synchronize()
    want = sim.run_quantiles(n, qs=QS, run_begin=E2E_BEGIN, seed_base=SEED)
    assert msim.order_stats_from_words(out.cpu().numpy(), 1, 9, 3) == want.order and int(rst.item()) == 0
    off, words = sim.rank_counts_view(3)
    assert (rws[off:off + 8 * words] == 0).all()  # the last step left the counts cleared
    with pytest.raises(ValueError):
        sim.launch_rank_begin(ranks, rws[:-1])


# ---------------------------------------------------------------- the driver
def test_gpu_quantiles_host_driver(msim):
    """host/msim_main --quantiles 0.05,0.5,0.95: its lines are report_quantiles's and its `quantiles` object is
    run_quantiles's order, for miners and for classes."""
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    sim = msim.Simulation(miners)
    res = sim.run_quantiles(64, qs=QS, run_begin=0, seed_base=SEED)
    cres = sim.run_quantiles(64, qs=QS, class_of=cmap, run_begin=0, seed_base=SEED)
    base = [exe, "1", str(SEED), "default", "--runs", "64", "--quantiles", "0.05,0.5,0.95"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-9:] == msim.report_quantiles(miners, res).splitlines()
    r = subprocess.run(base + ["--classes"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-8:] == msim.report_quantiles(miners, cres, members=members).splitlines()
    for extra, want, cols in (([], res, "miners"), (["--classes"], cres, "classes")):
        r = subprocess.run(base + ["--json"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = json.loads(r.stdout.strip().splitlines()[-1])["quantiles"]
        assert got["columns"] == cols and got["q"] == list(QS) and got["ranks"] == want.ranks
        assert got["order"] == _as_lists(want.order[0])


def test_gpu_quantiles_host_driver_sweep(msim, tmp_path):
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    props = (10_000, 100)
    points = [msim.setup_miners(p) for p in props]
    spec = {"runs": 65, "seed_base": SEED, "duration_ms": SHORT_MS,
            "points": [{"miners": [{"id": mn.id, "perc": mn.perc, "propagation_ms": mn.propagation_ms,
                                    "selfish": False} for mn in pt]} for pt in points]}
    path = tmp_path / "sweep.json"
    path.write_text(json.dumps(spec))
    res = msim.Sweep(points, SHORT_MS).run_quantiles(65, qs=(0.5, 1.0), run_begin=0, seed_base=SEED)
    r = subprocess.run([exe, "--sweep", str(path), "--quantiles", "0.5,1", "--json"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got = [json.loads(ln)["quantiles"] for ln in r.stdout.strip().splitlines()[-2:]]
    assert [g["order"] for g in got] == [_as_lists(res.order[p]) for p in range(2)]
    r = subprocess.run([exe, "--sweep", str(path), "--quantiles", "0.5,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = [ln for p in range(2) for ln in msim.report_quantiles(points[p], res, point=p).splitlines()]
    assert [ln for ln in r.stdout.splitlines() if " blocks found: q" in ln] == want

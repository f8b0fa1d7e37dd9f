"""The tail kernel (msim_tail.hip) and the entry points over it, on the device.

Synthetic records through msim_tail_launch, compared word by word with tests/tail_reference.py at item and run counts
around the kernel's tile (128 items), lane and workgroup boundaries; then the end-to-end cases against the oracle's
per-run counters, where n_below / n_equal must also reproduce the selection kernels' below / equal. Every comparison
is exact."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import classes_reference as cls
import rank_reference as rr
import tail_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
DAY = 86_400_000
YEAR_MS = 31_556_952_000
SHORT_MS = 10**9
E2E_BEGIN = 7000
TILE = 128
RUN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
ITEM_COUNTS = (1, 2, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
POINT_COUNTS = (1, 3)
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


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _launch(m, points, runs, d_rec, d_bh, items, fill=0xFF, n_items=None):
    """msim_tail_launch -> [n_items][42] rows as lists; the output is pre-filled with 0xFF."""
    import torch

    from miningsimulation_amd import _lib

    d_items = _dev(tr.item_words(items))
    out = torch.full((len(items), tr.WORDS), -1 if fill == 0xFF else fill, dtype=torch.int64, device=d_items.device)
    rc = _lib.lib.msim_tail_launch(m, points, runs, _p(d_rec), _p(d_bh), _p(d_items), len(items) if n_items is None else n_items,
                                   _p(out), None)
    assert rc == _lib.MSIM_OK, rc
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).tolist()


class _Data:
    """Synthetic records of the largest shape for one column count, one independent set per point; slices of it are
    the smaller shapes, each with its reference and its pool of items."""

    def __init__(self, m, shift=0, runs=max(RUN_COUNTS)):
        self.m = m
        self.f, self.s, self.L = tr.synthetic_points(max(POINT_COUNTS), runs, m, shift=shift, seed=100 * m)
        for a in (self.f, self.s, self.L):
            a.setflags(write=False)
        self._refs = {}

    def ref(self, points, runs):
        if (points, runs) not in self._refs:
            self._refs[(points, runs)] = tr.Reference(self.f[:points, :runs], self.s[:points, :runs], self.L[:points, :runs])
        return self._refs[(points, runs)]

    def device(self, points, runs):
        return (_dev(rr.records(self.f[:points, :runs], self.s[:points, :runs])), _dev(self.L[:points, :runs]))

    def items(self, points, runs, count, with_bad=False):
        """`count` items spread over the pool of every column x quantity x threshold, own and cross-point."""
        pool = tr.make_items(self.ref(points, runs), with_bad=with_bad)
        step = max(1, len(pool) // count) | 1  # odd: the pool alternates own and cross items
        picked = pool[::step][:count]
        return picked + pool[:count - len(picked)]


_DATA = {}


def data(m=9):
    if m not in _DATA:
        _DATA[m] = _Data(m)
    return _DATA[m]


def _check(got, want, what):
    bad = tr.diff(got, want)
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("runs", RUN_COUNTS)
def test_gpu_tail_synthetic(msim, runs):
    """Every item count and point count at one run count: one thread row per item up to two tiles plus one."""
    d = data()
    for points in POINT_COUNTS:
        d_rec, d_bh = d.device(points, runs)
        r = d.ref(points, runs)
        for count in ITEM_COUNTS:
            items = d.items(points, runs, count)
            assert len(items) == count and (points == 1 or count < 9 or any(it[0] != it[3] for it in items))
            _check(_launch(9, points, runs, d_rec, d_bh, items), r.all_words(items), (points, runs, count))


def test_gpu_tail_every_threshold_and_quantity(msim):
    """The whole pool at 513 runs and 3 points: all four quantities, thresholds 0, minimum, tied median, maximum and
    2^64 - 1, the all-equal column, the L == 0 records, cross-point items."""
    d = data()
    r = d.ref(3, 513)
    pool = tr.make_items(r, with_bad=False)
    assert {it[2] for it in pool} == {0, 1, 2, 3} and {it[6] for it in pool} >= {0, U64}
    got = _launch(9, 3, 513, *d.device(3, 513), pool)
    _check(got, r.all_words(pool), "pool")
    for it, row in zip(pool, got):
        if it[6] == U64:
            assert row[0] + row[1] == 513
        if it[6] == 0:
            assert row[0] == 0


def test_gpu_tail_1026_columns(msim):
    """own_tails of a 1 026-column buffer at 65 runs: nine tiles, the last one of two items."""
    import miningsimulation_amd as m

    d = _Data(1026, runs=65)
    for points in POINT_COUNTS:
        r = d.ref(points, 65)
        specs = m.own_tails(points, 1026, "share") if points == 1 else m.own_tails(points, 1026, "found")[1026:]
        items = [(sp.cond_point, sp.cond_column, sp.quantity, sp.target_point, sp.target_column, 0,
                  tr.thresholds(r.keys[sp.cond_point][sp.quantity][:, sp.cond_column])[2]) for sp in specs]
        _check(_launch(1026, points, 65, *d.device(points, 65), items), r.all_words(items), points)


def test_gpu_tail_several_workgroups(msim, monkeypatch):
    """MSIM_TAIL_TEST_WG_RUNS=64: 513 runs are nine workgroups along the runs; the result is the unset one's."""
    d = data()
    d_rec, d_bh = d.device(3, 513)
    items = d.items(3, 513, 2 * TILE + 1)
    whole = _launch(9, 3, 513, d_rec, d_bh, items)
    monkeypatch.setenv("MSIM_TAIL_TEST_WG_RUNS", "64")
    parts = _launch(9, 3, 513, d_rec, d_bh, items)
    assert parts == whole
    _check(parts, d.ref(3, 513).all_words(items), "nine workgroups")
    monkeypatch.setenv("MSIM_TAIL_TEST_WG_RUNS", "1")
    ones = _launch(9, 1, 65, *d.device(1, 65), d.items(1, 65, 9))
    _check(ones, d.ref(1, 65).all_words(d.items(1, 65, 9)), "one run per workgroup")


def test_gpu_tail_out_of_range_items_stay_zero(msim):
    """Out-of-range items among valid neighbours leave their 42 words zero (the output held 0xFF); a zero fill and
    the 0xFF fill give the same words."""
    d = data()
    r = d.ref(3, 257)
    pool = tr.make_items(r, with_bad=True)
    bad = [i for i, it in enumerate(pool) if not tr.item_ok(it, 3, 9)]
    assert len(bad) == 6
    items = pool[:40] + pool[-8:]
    got = _launch(9, 3, 257, *d.device(3, 257), items)
    _check(got, r.all_words(items), "bad items")
    assert sum(row == [0] * 42 and not tr.item_ok(it, 3, 9) for it, row in zip(items, got)) == 6
    assert _launch(9, 3, 257, *d.device(3, 257), items, fill=0) == got


def test_gpu_tail_refused_launches_write_nothing(msim):
    import torch

    from miningsimulation_amd import _lib

    lib = _lib.lib
    d = data()
    d_rec, d_bh = d.device(1, 65)
    items = d.items(1, 65, 9)
    d_items = _dev(tr.item_words(items))
    out = torch.full((9, 42), -1, dtype=torch.int64, device=d_items.device)
    E = _lib.MSIM_E_INVALID
    ok = dict(m=9, points=1, runs=65, rec=d_rec, bh=d_bh, items=d_items, n=9, out=out)
    for ch in (dict(m=0), dict(points=0), dict(runs=0), dict(runs=1 << 32), dict(rec=None), dict(bh=None),
               dict(items=None), dict(n=0), dict(n=65535 * 128 + 1)):
        a = dict(ok, **ch)
        assert lib.msim_tail_launch(a["m"], a["points"], a["runs"], _p(a["rec"]), _p(a["bh"]), _p(a["items"]), a["n"],
                                    _p(a["out"]), None) == E, ch
    assert lib.msim_tail_launch(9, 1, 65, _p(d_rec), _p(d_bh), _p(d_items), 9, None, None) == E
    torch.cuda.synchronize()
    assert (out == -1).all()
    # fewer items than the buffer holds: the rows past them keep their fill
    lib.msim_tail_launch(9, 1, 65, _p(d_rec), _p(d_bh), _p(d_items), 4, _p(out), None)
    torch.cuda.synchronize()
    assert (out[4:] == -1).all() and out[:4].cpu().numpy().view(np.uint64).tolist() == d.ref(1, 65).all_words(items[:4])


def test_gpu_tail_two_buffers_add_to_one(msim):
    """100 + 157 runs through two launches, added on the host, equal the 257 runs in one buffer."""
    d = data()
    f, s, L = d.f[:3, :257], d.s[:3, :257], d.L[:3, :257]
    items = d.items(3, 257, TILE + 1)
    one = _launch(9, 3, 257, *d.device(3, 257), items)
    a = _launch(9, 3, 100, _dev(rr.records(f[:, :100], s[:, :100])), _dev(L[:, :100]), items)
    b = _launch(9, 3, 157, _dev(rr.records(f[:, 100:], s[:, 100:])), _dev(L[:, 100:]), items)
    assert [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a, b)] == one
    _check(one, d.ref(3, 257).all_words(items), "two buffers")


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


def _check_result(res, sets, what):
    """Everything a TailResult holds against the reference over `sets` = [(f, s, L)] per point: the order statistics,
    n_below / n_equal against them, every tail word, the total moments, and the means."""
    f, s, L = (np.stack([x[i] for x in sets]) for i in range(3))
    r = tr.Reference(f, s, L)
    for p in range(len(sets)):
        order = [[[list(o) for o in row] for row in col] for col in res.order[p]]
        bad = rr.diff(order, rr.select(f[p], s[p], L[p], res.ranks))
        assert not bad, (what, p, bad[:8])
    items = []
    for sp, it, t in zip(res.specs, res.items, res.tails):
        o = res.order[sp.cond_point][sp.cond_column][sp.quantity][sp.rank_index]
        assert it.value == o.value and (t["n_below"], t["n_equal"]) == (o.below, o.equal), (what, sp)
        items.append((it.cond_point, it.cond_column, it.quantity, it.target_point, it.target_column, 0, it.value))
    _check(res.tail_words.tolist(), r.all_words(items), what)
    assert res.moment_words.tolist() == [[r.total(p, k) for k in range(r.m)] for p in range(r.n_points)], what
    for i, sp in enumerate(res.specs):
        want = tr.mean_k(res.tail_words[i].tolist(), r.total(sp.target_point, sp.target_column), res.n_runs, res.k(i))
        assert list(res.means(i).values()) == [float(x) for x in want], (what, sp)


def _specs(msim, m, n_ranks=2):
    """Every column's own share at rank 0 and own found at the last rank, and everyone given the last column's found."""
    return (msim.own_tails(1, m, "share", 0) + msim.own_tails(1, m, "found", n_ranks - 1) +
            msim.tails_given(0, m - 1, "found", m, n_ranks - 1) + msim.tails_given(0, 0, "rate", m, 0))


@pytest.mark.parametrize("duration", (SHORT_MS, YEAR_MS))
def test_gpu_tails_default_network_against_oracle(msim, oracle, monkeypatch, duration):
    """setup_miners() on the honest pipeline, 257 runs in three chunks (MSIM_MOMENTS_CHUNK_RUNS=100): at 10^9 ms the
    1 % miners' found counts are heavily tied."""
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, duration)
    f, s, L = _oracle(oracle, ("default", duration), miners, 257, duration)
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    res = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 9), run_begin=E2E_BEGIN, seed_base=SEED)
    monkeypatch.delenv("MSIM_MOMENTS_CHUNK_RUNS")
    assert res.ranks == [12, 128] and res.n_runs == 257
    _check_result(res, [(f, s, L)], ("default", duration))
    if duration == SHORT_MS:
        assert res.order[0][8][0][1].equal > 5                        # the ties the case is about
        whole = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 9), run_begin=E2E_BEGIN, seed_base=SEED)
        assert whole.tail_words.tolist() == res.tail_words.tolist() and whole.order == res.order
        plain = sim.run_quantiles(257, qs=(0.05, 0.5), run_begin=E2E_BEGIN, seed_base=SEED)
        assert plain.order == res.order and plain.points[0].stats_total == res.points[0].stats_total
        own = sim.run_tails(257, run_begin=E2E_BEGIN, seed_base=SEED)  # the defaults: own share at q = 0.05
        assert own.specs == msim.own_tails(1, 9) and own.tails[:9] == res.tails[:9]
        k = np.sort(rr.keys(f, s, L)[2][:, 7])
        assert own.expected_shortfall(7) * 13 == int(k[:13].sum())    # the mean of the 13 smallest shares, exactly


def test_gpu_tails_selfish_against_oracle(msim, oracle):
    miners = msim.setup_miners(1000, selfish_perc=40)
    sim = msim.Simulation(miners, SHORT_MS)
    assert sim.pipeline_info(257)["uses_pipeline"] == 3
    f, s, L = _oracle(oracle, "selfish", miners, 257, SHORT_MS)
    res = sim.run_tails(257, q=(0.05, 0.95), specs=_specs(msim, 9), run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, [(f, s, L)], "selfish")


def test_gpu_tails_wide_network_against_oracle(msim, oracle):
    miners = [msim.Miner(k, 6 if k < 15 else 5, 1000) for k in range(17)]
    sim = msim.Simulation(miners, 30 * DAY)
    assert sim.wide
    f, s, L = _oracle(oracle, "wide17", miners, 257, 30 * DAY)
    res = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 17), run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, [(f, s, L)], "wide")


def test_gpu_tails_general_engine_against_oracle(msim, oracle):
    miners = [msim.Miner(k, 20, 1000, True) for k in range(5)]
    sim = msim.Simulation(miners, 3 * DAY)
    assert sim.pipeline_info(257)["uses_pipeline"] == 4
    f, s, L = _oracle(oracle, "general", miners, 257, 3 * DAY)
    res = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 5), run_begin=E2E_BEGIN, seed_base=SEED)
    _check_result(res, [(f, s, L)], "general")


def test_gpu_tails_sweep_against_oracle(msim, oracle, monkeypatch):
    """A three-point propagation_sweep with cross-point specs: in the seeds that are miner 7's worst at 10 s, what the
    same seeds gave at 1 s and at 100 ms."""
    miners = msim.setup_miners()
    props = (10_000, 1000, 100)
    sw = msim.propagation_sweep(miners, props, SHORT_MS)
    sets = [_oracle(oracle, ("default", prop), msim.setup_miners(prop), 257, SHORT_MS) for prop in props]
    specs = (msim.own_tails(3, 9) + msim.tails_given(0, 7, "share", 9, target_point=2) +
             msim.tails_given(0, 7, "share", 9, target_point=1) + msim.tails_given(2, 0, "stale", 9, 1, target_point=0))
    res = sw.run_tails(257, q=(0.05, 0.5), specs=specs, run_begin=E2E_BEGIN, seed_base=SEED)
    assert len(res.order) == 3 and len(res.moments) == 3
    _check_result(res, sets, "sweep")
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    parts = sw.run_tails(257, q=(0.05, 0.5), specs=specs, run_begin=E2E_BEGIN, seed_base=SEED)
    assert parts.tail_words.tolist() == res.tail_words.tolist() and parts.moment_words.tolist() == res.moment_words.tolist()


def test_gpu_tails_classes_against_oracle(msim, oracle, monkeypatch):
    """class_of=: the oracle's counters through tests/classes_reference.py's fold, then the reference; chunked too."""
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    sim = msim.Simulation(miners, SHORT_MS)
    f, s, L = _oracle(oracle, ("default", SHORT_MS), miners, 257, SHORT_MS)
    cf, cs = cls.fold(f, s, cmap, len(members))
    res = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 8), class_of=cmap, run_begin=E2E_BEGIN, seed_base=SEED)
    assert len(res.order[0]) == len(members) == 8 and len(res.points[0].stats_total) == 9
    _check_result(res, [(cf, cs, L)], "classes")
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "100")
    parts = sim.run_tails(257, q=(0.05, 0.5), specs=_specs(msim, 8), class_of=cmap, run_begin=E2E_BEGIN, seed_base=SEED)
    assert parts.tail_words.tolist() == res.tail_words.tolist()
    lines = msim.report_tails(miners, res, members=members).splitlines()
    assert len(lines) == 8 and lines[7].startswith("  - Class 7 (2 miners, 2% of network hashrate) in its worst 13 of 257 runs")


# ---------------------------------------------------------------- launch wrappers, report and the driver
def test_gpu_tails_launch_report_and_driver_agree(msim):
    """launch_tails on a Simulation's own launch, run_tails, report_tails and host/msim_main --tails (text and
    --json), for miners and for classes, on 64 runs of a year."""
    import torch

    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    sim = msim.Simulation(miners)
    n, dev = 64, torch.device("cuda", 0)
    res = sim.run_tails(n, q=0.05, run_begin=0, seed_base=SEED)
    cres = sim.run_tails(n, q=0.05, class_of=cmap, run_begin=0, seed_base=SEED)
    # the launch wrapper on the records of the simulation's own launch
    sums = torch.zeros((9, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((n, 9, 2), dtype=torch.int32, device=dev)
    bh = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.empty(sim.workspace_bytes(n), dtype=torch.uint8, device=dev)
    sim.launch(n, 0, SEED, sums, ws, status, d_per_run=rec, d_best_height=bh)
    d_items = torch.from_numpy(msim.items_words(res.items).view(np.int32)).to(dev)
    out = torch.full((9, 42), -1, dtype=torch.int64, device=dev)
    sim.launch_tails(n, rec, bh, d_items, 9, out)
    torch.cuda.synchronize()
    assert msim.tails_from_words(out.cpu().numpy()) == res.tails
    with pytest.raises(ValueError):
        sim.launch_tails(n, rec, bh, d_items, 10, out)
    # the report and the driver
    text = msim.report_tails(miners, res).splitlines()
    assert len(text) == 9 and text[0].startswith("  - Miner 0 (30% of network hashrate) in its worst 4 of 64 runs found ")
    base = [exe, "1", str(SEED), "default", "--runs", str(n), "--tails", "0.05"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-9:] == text
    r = subprocess.run(base + ["--classes"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-8:] == msim.report_tails(miners, cres, members=members).splitlines()
    for extra, want, cols in (([], res, "miners"), (["--classes"], cres, "classes")):
        r = subprocess.run(base + ["--json"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = json.loads(r.stdout.strip().splitlines()[-1])["tails"]
        assert (got["columns"], got["q"], got["rank"], got["k"]) == (cols, 0.05, want.ranks[0], want.ranks[0] + 1)
        assert len(got["tail"]) == len(want.specs)
        for i, t in enumerate(got["tail"]):
            mu = want.means(i)
            assert (t["value"], t["n_below"], t["n_equal"]) == (want.items[i].value, want.tails[i]["n_below"],
                                                                want.tails[i]["n_equal"])
            assert [t[q] for q in ("found", "stale", "share", "rate")] == list(mu.values())


def test_gpu_tails_host_driver_sweep(msim, tmp_path):
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
    res = msim.Sweep(points, SHORT_MS).run_tails(65, q=0.5, run_begin=0, seed_base=SEED)
    r = subprocess.run([exe, "--sweep", str(path), "--tails", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = [ln for p in range(2) for ln in msim.report_tails(points[p], res, point=p).splitlines()]
    assert [ln for ln in r.stdout.splitlines() if " in its worst " in ln] == want
    r = subprocess.run([exe, "--sweep", str(path), "--tails", "0.5", "--json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [json.loads(ln)["tails"] for ln in r.stdout.strip().splitlines()[-2:]]
    for p in range(2):
        assert [t["share"] for t in got[p]["tail"]] == [res.means(p * 9 + c)["share"] for c in range(9)]

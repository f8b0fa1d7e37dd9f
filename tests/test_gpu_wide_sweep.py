"""Sweeps on the large-network pipeline on the device (msim_sweep_create_ex on points that are all wide;
miningsimulation_amd/csrc/msim_widesplit.h): with flags 0 one plain wide launch per point, with
MSIM_SWEEP_SHARED_DRAWS one W1 pass per draw group on the envelope network, the split kernel WS, then W2 and W3 per
point.

Every comparison is exact: found, stale and best height of every run against the oracle (total_weight = W), sums
byte for byte against Simulation(point, total_weight=W).run and against the flags-0 sweep at the same seeds. Run
counts are no multiples of 4 or 8 (67), so W1's and W3's last workgroups are ragged. The oracle's counters are
computed once per network and shared."""
import os
import random

import numpy as np
import pytest

import cross_reference as cref
import moments_reference as ref
import wide_sweep_native

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YEAR = 31_556_952_000
DAY = 86_400_000
D = 10**9
N = 67
BASE = 1000
H9 = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _weights(m, seed):
    """Integer weights with zeros; W != 100."""
    rng = random.Random(seed)
    w = [rng.choice([0, 1, 2, 5, 40, 300]) for _ in range(m)]
    w[0] = 0
    w[rng.randrange(1, m)] += 500
    assert sum(w) != 100
    return w


_REF = {}


def _oracle(oracle, w, props, duration, n, begin=0):
    k = (tuple(w), tuple(props), duration, n, begin)
    if k not in _REF:
        f, s, _, _ = oracle.run_batch(list(w), list(props), [0] * len(w), duration, n, begin, BASE, threads=16,
                                      total_weight=sum(w))
        f.setflags(write=False)
        s.setflags(write=False)
        _REF[k] = (f, s)
    return _REF[k]


def _net(msim, w, props):
    return [msim.Miner(k, w[k], props[k]) for k in range(len(w))]


def _sum_bytes(res):
    return b"".join(bytes(x) for x in res.sums)


def _shared(msim, points, W, duration=D, n=N):
    sw = msim.Sweep(points, duration, shared_draws=True, total_weight=W)
    assert sw.plan(n)["engine"] == 2, sw.plan(n)
    return sw


def _check_points(msim, oracle, sw, points, W, duration, n, begin=0, singles=True, flags0=True):
    out = sw.run(n, run_begin=begin, seed_base=BASE, per_run=True)
    plain = msim.Sweep(points, duration, total_weight=W) if flags0 else None
    if flags0:
        assert plain.plan(n)["engine"] == 2 and plain.plan(n)["draw_groups"] == len(points) and plain.group_of(0) == -1
        plain = plain.run(n, run_begin=begin, seed_base=BASE, per_run=True)
    for p, (res, pt) in enumerate(zip(out, points)):
        f, s = _oracle(oracle, [m.perc for m in pt], [m.propagation_ms for m in pt], duration, n, begin)
        assert np.array_equal(res.found.astype(np.int64), f), (p, np.argwhere(res.found != f)[:5])
        assert np.array_equal(res.stale.astype(np.int64), s), (p, np.argwhere(res.stale != s)[:5])
        assert np.array_equal(res.best_height.astype(np.int64), f.sum(axis=1)), p
        if singles:
            one = msim.Simulation(pt, duration, total_weight=W).run(n, run_begin=begin, seed_base=BASE)
            assert _sum_bytes(res) == _sum_bytes(one), p
        if flags0:
            assert _sum_bytes(res) == _sum_bytes(plain[p]), p
            assert np.array_equal(res.found, plain[p].found) and np.array_equal(res.stale, plain[p].stale), p
    return out


@pytest.mark.parametrize("m", [3, 17, 300])
def test_uniform_delays(msim, oracle, m):
    w = _weights(m, m)
    points = [_net(msim, w, [d] * m) for d in (10_000, 1_000, 100, 0)]
    sw = _shared(msim, points, sum(w))
    assert sw.plan(N)["draw_groups"] == 1 and sw.plan(N)["largest_group"] == 4
    assert [sw.group_of(p) for p in range(4)] == [0] * 4
    _check_points(msim, oracle, sw, points, sum(w), D, N)


def test_readme_example_forced_wide_equals_the_golden_vectors(msim, monkeypatch):
    """10 s / 1 s / 100 ms on the README percentages through the wide path: the reference-pinned arrays."""
    monkeypatch.setenv("MSIM_FORCE_WIDE", "1")
    z = np.load(os.path.join(GOLD, "oracle_vectors.npz"))
    names = ("c1_prop10s", "default_prop1s", "c2_prop100ms")
    points = []
    for name in names:
        p, q, s = z[name + "_config"].tolist()
        assert not any(s)
        points.append(_net(msim, p, q))
    sw = msim.Sweep(points, YEAR, shared_draws=True)
    plan = sw.plan(64)
    assert plan["engine"] == 2 and plan["draw_groups"] == 1 and plan["largest_group"] == 3
    monkeypatch.delenv("MSIM_FORCE_WIDE")  # the envelope is created wide whatever the switch says at launch
    for res, name in zip(sw.run(64, 0, BASE, 0, per_run=True), names):
        assert np.array_equal(res.found.astype(np.int64), z[name + "_found"]), name
        assert np.array_equal(res.stale.astype(np.int64), z[name + "_stale"]), name
        assert np.array_equal(res.best_height.astype(np.int64), z[name + "_best_height"]), name


@pytest.mark.parametrize("duration,n", [(40 * DAY, 32), (YEAR, 16)])
def test_c5_network(msim, oracle, duration, n):
    """1 026 miners at 10 s / 1 s / 100 ms; the year has about 900 envelope candidates per run (several 64-entry
    batches of WS and of W3's walk)."""
    net = msim.c5_network()
    w = [mn.perc for mn in net]
    points = [_net(msim, w, [d] * len(w)) for d in (10_000, 1_000, 100)]
    sw = msim.propagation_sweep(net, (10_000, 1_000, 100), duration, total_weight=msim.C5_TOTAL_WEIGHT)
    assert sw.plan(n)["engine"] == 2 and sw.plan(n)["draw_groups"] == 1
    _check_points(msim, oracle, sw, points, msim.C5_TOTAL_WEIGHT, duration, n, begin=3, flags0=duration != YEAR)


def test_readme_example_c5_contrasts(msim):
    """The README's large-network example: run_contrasts of the c5 propagation sweep against its 100 ms point, cross
    sums and moments against the references computed from the same sweep's records."""
    n, duration = 16, 40 * DAY
    sw = msim.propagation_sweep(msim.c5_network(), (10_000, 1_000, 100), duration, total_weight=msim.C5_TOTAL_WEIGHT)
    pairs = msim.pairs_vs_baseline(3, 1026, baseline=2)
    con = sw.run_contrasts(n, pairs, 3, BASE, 0)
    runs = sw.run(n, run_begin=3, seed_base=BASE, per_run=True)
    data = [(r.found, r.stale, r.best_height) for r in runs]
    bad = cref.diff(con.cross, cref.expected(cref.columns(data), [tuple(q) for q in pairs]))
    assert not bad, bad[:8]
    for p, d in enumerate(data):
        assert not ref.diff(con.points[p].moments, ref.expected(*d)), p
        assert _sum_bytes(con.points[p]) == _sum_bytes(runs[p])
    assert len(msim.contrasts(con)) == len(pairs)


def test_dense_forks(msim, oracle, monkeypatch):
    """A 9-miner W = 100 network forced wide at 60 s / 20 s / 5 s: more than 64 envelope candidates per run."""
    monkeypatch.setenv("MSIM_FORCE_WIDE", "1")
    points = [_net(msim, H9, [d] * 9) for d in (60_000, 20_000, 5_000)]
    sw = _shared(msim, points, 100)
    assert sw.plan(N)["draw_groups"] == 1
    cnt = wide_sweep_native.run_group(H9, [[60_000] * 9], 100, D, 8)[3]
    assert cnt[0].min() > 64
    _check_points(msim, oracle, sw, points, 100, D, N)


def test_heterogeneous_groups_and_a_singleton(msim, oracle):
    """Group 0's envelope is none of its points; group 1 is a plain pair; point 3 runs alone."""
    tail = [7, 1, 1, 2, 5, 3, 0, 6, 4, 9, 8, 2, 1, 6, 5]
    wa, wb, ws = [41, 0] + tail, [20, 21] + tail, [19, 22] + tail  # W = 101
    a = [10_000] + [100] * 16
    b = [100] + [10_000] * 16
    c = [1000 * (k % 9) for k in range(17)]
    points = [_net(msim, wa, a), _net(msim, wb, [1_000] * 17), _net(msim, wa, b), _net(msim, ws, [2_000] * 17),
              _net(msim, wb, [50] * 17), _net(msim, wa, c)]
    sw = _shared(msim, points, 101)
    assert sw.plan(N)["draw_groups"] == 3 and sw.plan(N)["largest_group"] == 3
    assert [sw.group_of(p) for p in range(6)] == [0, 1, 0, 2, 1, 0]
    _check_points(msim, oracle, sw, points, 101, D, N)


@pytest.mark.parametrize("duration", [0, 1, 600_000, 3 * DAY])
def test_durations(msim, oracle, duration):
    w = _weights(17, 40)
    points = [_net(msim, w, [d] * 17) for d in (60_000, 10_000, 0)]
    _check_points(msim, oracle, _shared(msim, points, sum(w), duration), points, sum(w), duration, N)


def test_slices(msim, oracle, monkeypatch):
    w = _weights(17, 41)
    points = [_net(msim, w, [d] * 17) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points, sum(w))
    whole = sw.run(600, seed_base=BASE, per_run=True)
    monkeypatch.setenv("MSIM_MAX_SLICE_RUNS", "256")
    assert sw.plan(600)["slice_runs"] == 256
    cut = _check_points(msim, oracle, sw, points, sum(w), D, 600, singles=False, flags0=False)
    for a, b in zip(whole, cut):
        assert _sum_bytes(a) == _sum_bytes(b)
        assert np.array_equal(a.found, b.found) and np.array_equal(a.stale, b.stale)
        assert np.array_equal(a.best_height, b.best_height)


@pytest.mark.parametrize("runs", ["1", "8"])
def test_w1_runs_per_workgroup(msim, oracle, monkeypatch, runs):
    monkeypatch.setenv("MSIM_W1_RUNS", runs)
    w = _weights(17, 41)
    points = [_net(msim, w, [d] * 17) for d in (10_000, 1_000, 100)]
    _check_points(msim, oracle, _shared(msim, points, sum(w)), points, sum(w), D, N, singles=False, flags0=False)


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


def test_dirty_workspace(msim):
    import torch

    w = _weights(17, 41)
    points = [_net(msim, w, [d] * 17) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points, sum(w))
    nb = sw.workspace_bytes(N)
    clean = _launch(sw, N, torch.zeros(nb, dtype=torch.uint8, device="cuda"), 0)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    dirty = _launch(sw, N, ws, -1)
    again = _launch(sw, N, ws, -1)  # the same workspace, now holding the first launch's lists and records
    for a, b, c in zip(clean, dirty, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert clean[3].tolist() == [0, 0]


def test_group_whose_envelope_is_not_taken_is_split(msim, oracle):
    """tests/test_wide_sweep_host.py's case on the device: B leaves the group, A and C share their draws."""
    net = msim.c5_network()
    w = [mn.perc for mn in net]
    a = _net(msim, w, [25_000 if k < 2 else 0 for k in range(len(w))])
    b = _net(msim, w, [0 if k < 2 else 36_000 for k in range(len(w))])
    c = _net(msim, w, [100] * len(w))
    sw = msim.Sweep([a, b, c], YEAR, shared_draws=True, total_weight=msim.C5_TOTAL_WEIGHT)
    assert sw.plan(16)["engine"] == 2 and sw.plan(16)["draw_groups"] == 2
    assert [sw.group_of(p) for p in range(3)] == [0, 1, 0]
    _check_points(msim, oracle, sw, [a, b, c], msim.C5_TOTAL_WEIGHT, YEAR, 16, singles=False, flags0=False)


# ------------------------------------------------------------------ lowered capacities
CAP_DELAYS = (30_000, 28_000, 26_000)


def _cap_case(msim):
    w = _weights(17, 42)
    points = [_net(msim, w, [d] * 17) for d in CAP_DELAYS]
    cnt = wide_sweep_native.run_group(w, [[d] * 17 for d in CAP_DELAYS], sum(w), D, N, BASE)[3]
    return w, points, cnt


def _check_unwritten(oracle, w, out, failed):
    """failed: [points][runs] bool. Failed runs are left unwritten (0xFF), every other run equals the oracle."""
    sums, rec, bh, st = out
    assert st.tolist() == [0, int(failed.sum())]
    for p, d in enumerate(CAP_DELAYS):
        f, s = _oracle(oracle, w, [d] * 17, D, N)
        bad = failed[p]
        assert (rec[p][bad] == -1).all() and (bh[p][bad] == -1).all(), p
        assert np.array_equal(rec[p][~bad][:, :, 0].astype(np.int64), f[~bad]), p
        assert np.array_equal(rec[p][~bad][:, :, 1].astype(np.int64), s[~bad]), p
        assert np.array_equal(bh[p][~bad].astype(np.int64), f[~bad].sum(axis=1)), p
        assert np.array_equal(sums[p, :, 0], f[~bad].sum(axis=0)) and np.array_equal(sums[p, :, 1], s[~bad].sum(axis=0))


def test_lowered_envelope_capacity_fails_the_run_at_every_point(msim, oracle, monkeypatch):
    import torch

    w, points, cnt = _cap_case(msim)
    cap = int(np.sort(cnt[0])[N // 2])
    over = cnt[0] > cap
    assert over.any() and not over.all()
    sw = _shared(msim, points, sum(w))
    monkeypatch.setenv("MSIM_WIDE_TEST_RCAP", str(cap))
    ws = torch.zeros(sw.workspace_bytes(N), dtype=torch.uint8, device="cuda")
    out = _launch(sw, N, ws, -1)
    _check_unwritten(oracle, w, out, np.stack([over] * 3))


def test_lowered_point_capacity_fails_that_point_only(msim, oracle, monkeypatch):
    import torch

    w, points, cnt = _cap_case(msim)
    lo, hi = int(cnt[1:].min(axis=1).max()), int(cnt[1:].max(axis=1).min()) - 1
    assert lo <= hi, (lo, hi)
    cap = (lo + hi) // 2
    over = cnt[1:] > cap
    assert over.any(axis=1).all() and not over.all(axis=1).any()
    assert len({o.tobytes() for o in over}) > 1  # the sets differ between points
    sw = _shared(msim, points, sum(w))
    monkeypatch.setenv("MSIM_WIDE_TEST_POINT_RCAP", str(cap))
    ws = torch.zeros(sw.workspace_bytes(N), dtype=torch.uint8, device="cuda")
    out = _launch(sw, N, ws, -1)
    _check_unwritten(oracle, w, out, over)
    with pytest.raises(Exception):  # msim_sweep_run reports MSIM_E_CAPACITY
        sw.run(N, seed_base=BASE)


# ------------------------------------------------------------------ the layers on msim_sweep_launch
def test_moments_contrasts_and_multi(msim):
    w = _weights(17, 43)
    points = [_net(msim, w, [d] * 17) for d in (10_000, 1_000, 100)]
    sw = _shared(msim, points, sum(w))
    runs = sw.run(N, run_begin=9, seed_base=BASE, per_run=True)
    data = [(r.found, r.stale, r.best_height) for r in runs]
    mom = sw.run_moments(N, 9, BASE, 0)
    pairs = msim.pairs_vs_baseline(3, 17, baseline=2)
    con = sw.run_contrasts(N, pairs, 9, BASE, 0)
    for p, d in enumerate(data):
        want = ref.expected(*d)
        assert not ref.diff(mom[p].moments, want), p
        assert not ref.diff(con.points[p].moments, want), p
        assert _sum_bytes(mom[p]) == _sum_bytes(runs[p]) == _sum_bytes(con.points[p])
    bad = cref.diff(con.cross, cref.expected(cref.columns(data), [tuple(q) for q in pairs]))
    assert not bad, bad[:8]
    assert any(any(int(v) for v in c.values()) for c in con.cross)
    multi = sw.run_multi(N, 9, BASE, devices=(0,))
    for a, b in zip(multi, runs):
        assert _sum_bytes(a) == _sum_bytes(b)

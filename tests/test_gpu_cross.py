"""The cross kernel (msim_cross.hip) and the entry points over it, on the device.

Synthetic records reach every extreme of the term and limb arithmetic (tests/moments_cases.py) at run and pair
counts around the kernel's tile, row and chunk boundaries; the end-to-end cases tie the sums to the oracle's
counters of both sides of every pair. Every comparison of sums is exact integer equality against
tests/cross_reference.py."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cross_reference as cref
import instantiation_networks as nets
import moments_cases
import moments_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
E2E_RUNS = 257
E2E_DURATION_MS = 10**9  # as tests/test_gpu_moments.py
E2E_BEGIN = 7000
RUN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
PAIR_COUNTS = (1, 3, 63, 64, 65, 255, 256, 257, 1025)
U32 = 0xFFFFFFFF
README_PERCS = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


_CASES = {}


def _case(n, m, points):
    """Synthetic records of `points` points, their reference columns and device tensors, built once per shape."""
    import torch

    key = (n, m, points)
    if key not in _CASES:
        data = [moments_cases.synthetic(n, m, seed=17 * p + n + m) for p in range(points)]
        for d in data:
            for a in d:
                a.setflags(write=False)
        dev = torch.device("cuda", 0)
        rec = np.stack([moments_cases.records(f, s) for f, s, _ in data])
        bh = np.stack([L for _, _, L in data])
        _CASES[key] = (data, cref.columns(data), torch.from_numpy(rec.view(np.int32)).to(dev),
                       torch.from_numpy(bh.view(np.int32)).to(dev))
    return _CASES[key]


_EXPECTED = {}


def _expected(cols, pairs):
    """cross_reference.expected, each distinct pair of one case computed once (the lists repeat their pairs)."""
    memo = _EXPECTED.setdefault(id(cols), {})
    new = [q for q in dict.fromkeys(tuple(q) for q in pairs) if q not in memo]
    memo.update(zip(new, cref.expected(cols, new)))
    return [memo[tuple(q)] for q in pairs]


def pair_list(n_pairs, points, m, seed):
    """n_pairs pairs mixing the canonical lists (against a baseline, between miners), self pairs, duplicates and a
    scrambled order: the first half keeps the canonical miner-minor order, the second half is shuffled."""
    pool = [(p, k, 0, k) for p in range(1, points) for k in range(m)]
    pool += [(p, i, p, j) for p in range(points) for i in range(m) for j in range(i + 1, m)]
    pool += [(p, k, p, k) for p in range(points) for k in range(m)]
    pool += [(p, i, q, j) for p in range(points) for q in range(points) for i in range(m) for j in range(m)]
    out = [pool[i % len(pool)] for i in range(n_pairs)]  # wraps: duplicates
    rng = np.random.default_rng(seed)
    half = n_pairs // 2
    tail = out[half:]
    rng.shuffle(tail)
    return out[:half] + [tuple(int(x) for x in q) for q in tail]


def _ff(shape):
    import torch

    t = torch.empty(shape, dtype=torch.int64, device=torch.device("cuda", 0))
    t.view(torch.uint8).fill_(0xFF)
    return t


def _pairs_tensor(pairs):
    import torch

    a = np.asarray(pairs, dtype=np.uint32).reshape(-1, 4)
    return torch.from_numpy(a.view(np.int32)).to(torch.device("cuda", 0))


def _launch(n, m, points, rec, bh, pairs, out=None):
    """msim_cross_launch into a 0xFF-filled output; the joined sums per pair."""
    import torch

    from miningsimulation_amd.contrasts import cross_from_words
    from miningsimulation_amd.simulation import _launch_cross

    out = _ff((len(pairs), 12)) if out is None else out
    _launch_cross(m, points, n, rec, bh, _pairs_tensor(pairs), len(pairs), out, None)
    torch.cuda.synchronize()
    return cross_from_words(out.cpu().numpy().view(np.uint64)[:len(pairs)])


@pytest.mark.parametrize("points", [1, 3])
@pytest.mark.parametrize("m", [1, 3, 17])
def test_gpu_cross_synthetic(msim, m, points):
    """Every run count against every pair count at one (M, points): the tile, row and chunk boundaries."""
    for n in RUN_COUNTS:
        data, cols, rec, bh = _case(n, m, points)
        for n_pairs in PAIR_COUNTS:
            pairs = pair_list(n_pairs, points, m, seed=n + n_pairs)
            bad = cref.diff(_launch(n, m, points, rec, bh, pairs), _expected(cols, pairs))
            assert not bad, (n, n_pairs, m, points, bad[:8])


def test_gpu_cross_canonical_lists(msim):
    """pairs_vs_baseline and pairs_between_miners as the library builds them, 513 runs of 3 points x 17 miners."""
    data, cols, rec, bh = _case(513, 17, 3)
    for pairs in (msim.pairs_vs_baseline(3, 17), msim.pairs_vs_baseline(3, 17, baseline=2),
                  msim.pairs_between_miners(17, point=1)):
        bad = cref.diff(_launch(513, 17, 3, rec, bh, pairs), cref.expected(cols, [tuple(q) for q in pairs]))
        assert not bad, bad[:8]


@pytest.mark.parametrize("n_pairs", [7, 300])
def test_gpu_cross_out_of_range_pairs(msim, n_pairs):
    """Pairs outside the records first, last and in the middle of a tile: their words are all zero, every other
    pair is unchanged, and nothing outside the buffers is read."""
    n, m, points = 257, 3, 3
    data, cols, rec, bh = _case(n, m, points)
    good = pair_list(n_pairs, points, m, seed=5)
    want = cref.expected(cols, good)
    bad_pairs = [(points, 0, 0, 0), (0, m, 0, 0), (0, 0, points, 0), (0, 0, 0, m), (U32, U32, U32, U32),
                 (0, 0, U32, 0), (1 << 31, 0, 0, 0)]
    mixed, where = list(good), []
    for i, at in enumerate((0, n_pairs // 2, n_pairs // 2 + 1, len(good))):
        at += i  # earlier insertions shift the later ones
        mixed.insert(at, bad_pairs[i])
        where.append(at)
    mixed += bad_pairs[4:]
    where += list(range(len(mixed) - 3, len(mixed)))
    got = _launch(n, m, points, rec, bh, mixed)
    assert [got[i] for i in range(len(mixed)) if i not in where] == want
    for i in where:
        assert not any(got[i].values()), (i, mixed[i])
    assert not cref.diff(got, cref.expected(cols, mixed))


def test_gpu_cross_overwrites_its_outputs(msim):
    """Two launches in a row into the same 0xFF-filled output: each gives its own input's result."""
    m, points = 17, 3
    out = _ff((300, 12))
    for n, n_pairs in ((257, 300), (65, 64)):
        data, cols, rec, bh = _case(n, m, points)
        pairs = pair_list(n_pairs, points, m, seed=n)
        bad = cref.diff(_launch(n, m, points, rec, bh, pairs, out), cref.expected(cols, pairs))
        assert not bad, (n, bad[:8])


def test_gpu_cross_launch_rejects_bad_arguments(msim):
    import ctypes

    import torch

    from miningsimulation_amd import _lib
    from miningsimulation_amd.simulation import _launch_cross

    data, cols, rec, bh = _case(2, 3, 1)
    pairs = _pairs_tensor([(0, 0, 0, 1), (0, 1, 0, 2)])
    out = _ff((2, 12))
    for args in ((3, 1, 3, rec, bh, pairs, 2, out), (3, 2, 2, rec, bh, pairs, 2, out),   # more runs / points
                 (3, 1, 2, rec, bh, pairs, 3, out)):                                     # more pairs
        with pytest.raises(ValueError):
            _launch_cross(*args, None)
    p = (lambda t: ctypes.c_void_p(t.data_ptr()))
    ok = dict(m=3, points=1, runs=2, rec=p(rec), bh=p(bh), pairs=p(pairs), n_pairs=2, out=p(out))
    for change in (dict(m=0), dict(points=0), dict(runs=0), dict(runs=1 << 32), dict(n_pairs=0),
                   dict(n_pairs=16776961), dict(rec=None), dict(bh=None),
                   dict(pairs=None), dict(out=None)):
        a = dict(ok, **change)
        rc = _lib.lib.msim_cross_launch(a["m"], a["points"], a["runs"], a["rec"], a["bh"], a["pairs"], a["n_pairs"],
                                        a["out"], None)
        assert rc == _lib.MSIM_E_INVALID, change
    torch.cuda.synchronize()
    assert (out.view(torch.uint8) == 0xFF).all()  # a rejected launch writes nothing


# ---------------------------------------------------------------- end to end
_ORACLE = {}


def _oracle(oracle, key, percs, props, selfish, n_runs=E2E_RUNS):
    if (key, n_runs) not in _ORACLE:
        f, s, _, _ = oracle.run_batch(percs, props, selfish, E2E_DURATION_MS, n_runs, E2E_BEGIN, SEED, threads=16,
                                      total_weight=100)
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[(key, n_runs)] = (f, s, f.sum(axis=1))
    return _ORACLE[(key, n_runs)]


def _check_result(res, data, pairs, what):
    """Cross sums and moments of a ContrastResult against the oracle's counters of every point."""
    assert [tuple(q) for q in res.pairs] == [tuple(q) for q in pairs] and res.n_runs == data[0][0].shape[0]
    bad = cref.diff(res.cross, cref.expected(cref.columns(data), [tuple(q) for q in pairs]))
    assert not bad, (what, bad[:8])
    for p, d in enumerate(data):
        bad = ref.diff(res.points[p].moments, ref.expected(*d))
        assert not bad, (what, p, bad[:8])


def test_gpu_cross_selfish_sweep(msim, oracle):
    """The one-selfish network and its honest twin (tests/test_gpu_moments.py's two-point sweep) through
    Sweep.run_contrasts: cross sums from the oracle's counters of both networks, the rest as Sweep.run_moments."""
    m = 9
    c = nets.case("selfish_uniform_1s", m)
    pts = [[msim.Miner(k, c["percs"][k], c["props"][k], sel and c["selfish"][k]) for k in range(m)]
           for sel in (True, False)]
    sw = msim.Sweep(pts, E2E_DURATION_MS)
    pairs = msim.pairs_vs_baseline(2, m, baseline=1)  # the selfish network against its twin
    res = sw.run_contrasts(E2E_RUNS, pairs, E2E_BEGIN, SEED, 0)
    data = [_oracle(oracle, ("s1s", sel), c["percs"], c["props"], [sel and x for x in c["selfish"]])
            for sel in (True, False)]
    _check_result(res, data, pairs, "selfish sweep")
    plain = sw.run_moments(E2E_RUNS, E2E_BEGIN, SEED, 0)
    for a, b in zip(res.points, plain):
        assert a.moments == b.moments and a.stats_total == b.stats_total and a.n_runs == b.n_runs
        assert [tuple(getattr(x, f) for f, _ in x._fields_) for x in a.sums] == \
               [tuple(getattr(x, f) for f, _ in x._fields_) for x in b.sums]
    con = msim.contrasts(res)
    assert con[0]["share_diff"] > 0.0 and con[0]["share_diff_se"] > 0.0  # the selfish miner gains


def test_gpu_cross_honest_sweep(msim, oracle):
    """10 s / 1 s / 100 ms on the README percentages, same runs and seeds: sums exact against the oracle,
    contrasts() within 1e-13 of the fractions reference, and the pairing is real: for miner 0's share, 10 s against
    100 ms, the paired error is more than ten times below the independent one (the oracle gives 13.3)."""
    m = len(README_PERCS)
    props = (10_000, 1_000, 100)
    sw = msim.Sweep([msim.setup_miners(p) for p in props], E2E_DURATION_MS)
    assert [x.perc for x in sw.sims[0].miners] == README_PERCS
    pairs = msim.pairs_vs_baseline(3, m, baseline=2)  # against 100 ms
    res = sw.run_contrasts(E2E_RUNS, pairs, E2E_BEGIN, SEED, 0)
    data = [_oracle(oracle, ("readme", p), README_PERCS, [p] * m, [False] * m) for p in props]
    _check_result(res, data, pairs, "honest sweep")
    mo = [ref.expected(*d) for d in data]
    con = msim.contrasts(res)
    for i, q in enumerate(pairs):
        want = cref.contrast(mo[q[0]][q[1]], mo[q[2]][q[3]], res.cross[i], E2E_RUNS)
        for name in cref.FIELDS:
            err = cref.field_error(name, con[i][name], want[name])
            assert err <= 1e-13, (q, name, con[i][name], want[name], err)
    assert tuple(pairs[0]) == (0, 0, 2, 0)
    errs = [msim.error_bars(r)[0]["share_se"] for r in res.points]
    independent = math.hypot(errs[0], errs[2])
    print(f"miner 0 share, 10 s vs 100 ms: diff {con[0]['share_diff']:.6g} paired se {con[0]['share_diff_se']:.6g} "
          f"independent se {independent:.6g} corr {con[0]['share_corr']:.4f}")
    assert con[0]["share_diff_se"] * 10 < independent


def test_gpu_cross_between_miners(msim, oracle):
    """Simulation.run_contrasts with pairs_between_miners on the 10 s README network against the oracle; miners 0
    and 1 of one network are negatively correlated."""
    m = len(README_PERCS)
    sim = msim.Simulation(msim.setup_miners(10_000), E2E_DURATION_MS)
    pairs = msim.pairs_between_miners(m)
    res = sim.run_contrasts(E2E_RUNS, pairs, E2E_BEGIN, SEED, 0)
    data = [_oracle(oracle, ("readme", 10_000), README_PERCS, [10_000] * m, [False] * m)]
    _check_result(res, data, pairs, "between miners")
    plain = sim.run_moments(E2E_RUNS, E2E_BEGIN, SEED, 0)
    assert res.points[0].moments == plain.moments and res.points[0].stats_total == plain.stats_total
    assert msim.contrasts(res)[0]["share_corr"] < 0.0
    with pytest.raises(ValueError):
        sim.run_contrasts(E2E_RUNS, [(1, 0, 0, 0)], E2E_BEGIN, SEED, 0)  # a single config has one point


@pytest.mark.parametrize("sweep", [False, True], ids=["run", "sweep"])
def test_gpu_cross_chunked_equals_unchunked(msim, monkeypatch, sweep):
    """MSIM_MOMENTS_CHUNK_RUNS=256 on 513 runs: three chunks, cross words added limb by limb on the host."""
    m = len(README_PERCS)
    if sweep:
        obj = msim.Sweep([msim.setup_miners(p) for p in (10_000, 100)], E2E_DURATION_MS)
        pairs = msim.pairs_vs_baseline(2, m) + msim.pairs_between_miners(m, point=1)
    else:
        obj = msim.Simulation(msim.setup_miners(10_000), E2E_DURATION_MS)
        pairs = msim.pairs_between_miners(m)
    run = (lambda: obj.run_contrasts(513, pairs, E2E_BEGIN, SEED, 0))
    whole = run()
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "256")
    parts = run()
    assert whole.cross == parts.cross and whole.cross[0]["found_found"] > 0
    for a, b in zip(whole.points, parts.points):
        assert a.moments == b.moments and a.stats_total == b.stats_total
    for c, d in zip(msim.contrasts(whole), msim.contrasts(parts)):
        assert all(c[k] == d[k] or (math.isnan(c[k]) and math.isnan(d[k])) for k in cref.FIELDS)


def test_gpu_cross_host_driver_contrast_json(msim, tmp_path):
    """host/msim_main --sweep .. --contrast 0 --json: its `contrast` objects are contrasts() of
    Sweep.run_contrasts, the text form's lines are report_contrasts, and an out-of-range point is a usage error."""
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    m = 5
    c = nets.case("selfish_uniform_1s", m)
    props = (1000, 10_000, 100)
    spec = {"runs": E2E_RUNS, "seed_base": SEED, "duration_ms": E2E_DURATION_MS,
            "points": [{"miners": [{"id": k, "perc": c["percs"][k], "propagation_ms": p,
                                    "selfish": bool(c["selfish"][k])} for k in range(m)]} for p in props]}
    path = tmp_path / "sweep.json"
    path.write_text(json.dumps(spec))
    sw = msim.Sweep([[msim.Miner(k, c["percs"][k], p, bool(c["selfish"][k])) for k in range(m)] for p in props],
                    E2E_DURATION_MS)
    for base in (0, 1):
        res = sw.run_contrasts(E2E_RUNS, msim.pairs_vs_baseline(3, m, baseline=base), 0, SEED, 0)
        want = msim.contrasts(res)
        r = subprocess.run([exe, "--sweep", str(path), "--contrast", str(base), "--errors", "--json"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = [json.loads(ln) for ln in r.stdout.strip().splitlines()[-3:]]
        assert [g["point"] for g in got] == [0, 1, 2]
        others = [p for p in range(3) if p != base]
        assert all("contrast" not in x for x in got[base]["miners"])
        for j, p in enumerate(others):
            for k in range(m):
                mine = {f: (None if math.isnan(v) else v) for f, v in want[j * m + k].items()}
                assert got[p]["miners"][k]["contrast"] == mine, (base, p, k)
                assert got[p]["miners"][k]["errors"] == msim.error_bars(res.points[p])[k]
        assert want[0]["share_diff_se"] > 0.0 and not math.isnan(want[0]["share_corr"])
        r = subprocess.run([exe, "--sweep", str(path), "--contrast", str(base)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if " vs point " in ln]
        assert lines == msim.report_contrasts(res).splitlines()
        plain = [ln for ln in r.stdout.splitlines() if ln.startswith("  - Miner") and " vs point " not in ln]
        assert len(plain) == 3 * m and not any("±" in ln for ln in plain)  # --errors was not given
    for bad in ("3", "-1"):
        r = subprocess.run([exe, "--sweep", str(path), "--contrast", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "contrast" in r.stderr, (bad, r.returncode, r.stderr)

"""The fold kernel (msim_fold.hip) and the class entry points over it, on the device.

Synthetic full-range records through msim_fold_launch alone, byte-equal with tests/classes_reference.py at miner, run
and point counts around the kernel's lane, segment, tile and class-tile boundaries; then the ties to the per-miner
path and the end-to-end cases against the oracle's counters folded by the reference. Every comparison is exact."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import classes_reference as cls
import cross_reference as cref
import moments_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
DAY = 86_400_000
E2E_DURATION_MS = 30 * DAY
E2E_BEGIN = 7000
M_COUNTS = (1, 2, 9, 15, 16, 63, 64, 65, 257, 1026, 4100)
RUN_COUNTS = (1, 63, 64, 65, 257, 1000)
POINT_COUNTS = (1, 3)
U32 = 0xFFFFFFFF
SPEC = dict(bins=64, share_shift=26, rate_shift=24, share_lo=0, rate_lo=0)


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


def _ff(shape):
    import torch

    t = torch.empty(shape, dtype=torch.int32, device=torch.device("cuda", 0))
    t.view(torch.uint8).fill_(0xFF)
    return t


def _fold(m, points, runs, d_rec, cmap, nc, out=None):
    """msim_fold_launch into a 0xFF-filled output [points, runs, nc, 2] (int32 on the device)."""
    import torch

    from miningsimulation_amd.simulation import _launch_fold

    out = _ff((points, runs, nc, 2)) if out is None else out
    _launch_fold(m, points, runs, d_rec, _dev(np.asarray(cmap, dtype=np.uint32)), nc, out, None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("m", M_COUNTS)
def test_gpu_fold_synthetic(msim, m):
    """Every run count and point count against every named map at one miner count. The records are full-range
    uint32, so class sums wrap; the reference fold of the largest shape is computed once per map and sliced."""
    import torch

    pmax, rmax = max(POINT_COUNTS), max(RUN_COUNTS)
    rng = np.random.default_rng(4000 + m)
    rec = rng.integers(0, 1 << 32, size=(pmax, rmax, m, 2), dtype=np.uint64).astype(np.uint32)
    rec.setflags(write=False)
    flat_f, flat_s = rec[..., 0].reshape(pmax * rmax, m), rec[..., 1].reshape(pmax * rmax, m)
    want = {}
    for name, (cmap, nc) in cls.maps(m).items():
        cf, cs = cls.fold(flat_f, flat_s, cmap, nc)
        want[name] = _dev(cls.records(cf, cs).reshape(pmax, rmax, nc, 2))
    for points in POINT_COUNTS:
        for runs in RUN_COUNTS:
            d_rec = _dev(rec[:points, :runs])
            for name, (cmap, nc) in cls.maps(m).items():
                got = _fold(m, points, runs, d_rec, cmap, nc)
                assert torch.equal(got, want[name][:points, :runs].contiguous()), (m, points, runs, name)
    if m >= 2:  # the identity map's output bytes are its input's
        assert torch.equal(_fold(m, pmax, rmax, _dev(rec), list(range(m)), m), _dev(rec))


def test_gpu_fold_class_sums_of_exactly_2_32_minus_1(msim):
    """A class whose found blocks add up to exactly 2^32 - 1 and whose stale blocks add up to 2^32 + 5, its members
    spread over lanes, trips and both sides of a lane's cell change; run 1 holds 2^32 in 1 024 equal parts."""
    m, runs = 1026, 5
    f = np.zeros((runs, m), dtype=np.uint32)
    s = np.zeros((runs, m), dtype=np.uint32)
    f[0, 2], f[0, 66], f[0, 67], f[0, 1025] = 0xFFFFFF00, 0xF0, 0x0E, 1
    s[0, 2], s[0, 66], s[0, 1025] = U32, 3, 3
    f[1, 2:] = 1 << 22
    f[:, 0], s[:, 1] = 7, 9
    cmap, _ = msim.classes_of(msim.c5_network())
    got = _fold(m, 1, runs, _dev(cls.records(f, s)), cmap, 3).cpu().numpy().view(np.uint32)[0]
    assert (int(got[0, 2, 0]), int(got[0, 2, 1])) == (U32, 5) and int(got[1, 2, 0]) == 0
    cf, cs = cls.fold(f, s, cmap, 3)
    assert np.array_equal(got[..., 0], cf) and np.array_equal(got[..., 1], cs)
    assert (got[:, 0, 0] == 7).all() and (got[:, 1, 1] == 9).all()


def test_gpu_fold_overwrites_and_rejects(msim):
    """Two launches in a row into one 0xFF-filled buffer give each its own result; a refused launch writes nothing."""
    import torch

    from miningsimulation_amd import _lib

    m, runs = 65, 257
    rng = np.random.default_rng(5)
    rec = rng.integers(0, 1 << 32, size=(1, runs, m, 2), dtype=np.uint64).astype(np.uint32)
    d_rec = _dev(rec)
    out = _ff((1, runs, m, 2))
    for name in ("identity", "one_empty", "two"):
        cmap, nc = cls.maps(m)[name]
        cf, cs = cls.fold(rec[0, :, :, 0], rec[0, :, :, 1], cmap, nc)
        got = _fold(m, 1, runs, d_rec, cmap, nc, out).view(-1)[:runs * nc * 2].cpu().numpy().view(np.uint32)
        assert np.array_equal(got.reshape(runs, nc, 2), cls.records(cf, cs)), name
    out = _ff((1, runs, m, 2))
    d_map = _dev(np.zeros(m, dtype=np.uint32))
    p = (lambda t: ctypes.c_void_p(t.data_ptr()))
    ok = dict(m=m, points=1, runs=runs, rec=p(d_rec), cmap=p(d_map), nc=2, out=p(out))
    for change in (dict(m=0), dict(points=0), dict(points=65536), dict(runs=0), dict(runs=1 << 32), dict(nc=0),
                   dict(nc=m + 1), dict(rec=None), dict(cmap=None), dict(out=None)):
        a = dict(ok, **change)
        rc = _lib.lib.msim_fold_launch(a["m"], a["points"], a["runs"], a["rec"], a["cmap"], a["nc"], a["out"], None)
        assert rc == _lib.MSIM_E_INVALID, change
    torch.cuda.synchronize()
    assert (out.view(torch.uint8) == 0xFF).all()
    with pytest.raises(ValueError):  # a buffer smaller than the launch writes
        _fold(m, 1, runs, d_rec, list(range(m)), m, _ff((1, runs, m - 1, 2)))


def test_gpu_run_classes_rejects_a_bad_map(msim):
    from miningsimulation_amd import _lib

    sim = msim.Simulation(msim.setup_miners(), E2E_DURATION_MS)
    u32 = ctypes.c_uint32
    stats, mom = (_lib.MsimStats * 9)(), (_lib.MsimMoments * 9)()
    for cmap, nc in (((u32 * 9)(0, 0, 0, 0, 0, 0, 0, 0, 2), 2), ((u32 * 9)(), 0), ((u32 * 9)(), 10), (None, 1)):
        rc = _lib.lib.msim_run_classes(sim.handle, 0, 16, SEED, 0, cmap, nc, None, 0, stats, None, mom, None, None, None)
        assert rc == _lib.MSIM_E_INVALID, nc
    with pytest.raises(ValueError):
        sim.run_classes(16, [0] * 8 + [2], n_classes=2)
    with pytest.raises(ValueError):
        sim.run_classes(16, [0] * 9, pairs=[(0, 0, 0, 1)])  # one class: class 1 does not exist


# ---------------------------------------------------------------- ties to the per-miner path
def test_gpu_classes_identity_equals_run_moments(msim):
    """The identity map: run_classes(...).moments are run_moments(...).moments word for word; a class holding the
    single miner k gives miner k's row."""
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, E2E_DURATION_MS)
    hist = msim.HistSpec(**SPEC)
    plain = sim.run_moments(300, E2E_BEGIN, SEED, 0, hist=hist)
    ident = sim.run_classes(300, list(range(9)), hist=hist, run_begin=E2E_BEGIN, seed_base=SEED)
    assert ident.moments == plain.moments and np.array_equal(ident.hist, plain.hist)
    assert ident.stats_total == plain.stats_total and ident.n_runs == 300
    assert plain.moments[0]["found_sq"] > 0
    for k in (0, 4, 8):
        cmap, _ = msim.classes_from_groups(9, [[k]])
        one = sim.run_classes(300, cmap, run_begin=E2E_BEGIN, seed_base=SEED)
        assert one.moments == [plain.moments[k]] and one.stats_total == plain.stats_total


# ---------------------------------------------------------------- end to end against the oracle
_ORACLE = {}


def _oracle(oracle, key, miners, n_runs, total_weight=100, begin=E2E_BEGIN):
    if key not in _ORACLE:
        f, s, _, _ = oracle.run_batch([m.perc for m in miners], [m.propagation_ms for m in miners],
                                      [m.is_selfish for m in miners], E2E_DURATION_MS, n_runs, begin, SEED, threads=16,
                                      total_weight=total_weight)
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[key] = (f, s, f.sum(axis=1))
    return _ORACLE[key]


def _check_point(res, f, s, L, cmap, nc, what):
    """A point's nine joined sums per class and its histogram against the oracle's counters through the reference fold."""
    cf, cs = cls.fold(f, s, cmap, nc)
    bad = ref.diff(res.moments, ref.expected(cf, cs, L))
    assert not bad, (what, bad[:8])
    if res.hist is not None:
        assert np.array_equal(res.hist, ref.expected_hist(cf, cs, L, *SPEC.values())), what
    return cf, cs


def test_gpu_classes_default_network_against_oracle(msim, oracle):
    miners = msim.setup_miners()
    cmap, members = msim.classes_of(miners)
    res = msim.Simulation(miners, E2E_DURATION_MS).run_classes(300, cmap, hist=msim.HistSpec(**SPEC),
                                                               run_begin=E2E_BEGIN, seed_base=SEED)
    f, s, L = _oracle(oracle, ("default", 1000), miners, 300)
    _check_point(res, f, s, L, cmap, len(members), "default")
    assert len(res.moments) == 8 and len(res.stats_total) == 9
    assert "Class 7 (2 miners, 2% of network hashrate)" in msim.report_classes(miners, members, res)


def test_gpu_classes_selfish_against_oracle(msim, oracle):
    """Everyone but the selfish miner as one class."""
    miners = msim.PRESETS["c3"]()
    cmap, members = msim.classes_from_groups(9, [[0], list(range(1, 9))])
    res = msim.Simulation(miners, E2E_DURATION_MS).run_classes(128, cmap, hist=msim.HistSpec(**SPEC),
                                                               run_begin=E2E_BEGIN, seed_base=SEED)
    f, s, L = _oracle(oracle, "c3", miners, 128)
    cf, _ = _check_point(res, f, s, L, cmap, 2, "selfish")
    assert np.array_equal(cf.sum(axis=1), L)  # the two classes hold every block of the best chain


def test_gpu_classes_c5_against_oracle(msim, oracle):
    """configs[4] at the size smoke() runs: pools and the 1 024 small miners as three columns."""
    miners = msim.c5_network()
    cmap, members = msim.classes_of(miners)
    assert [len(g) for g in members] == [1, 1, 1024]
    sim = msim.Simulation(miners, E2E_DURATION_MS, total_weight=msim.C5_TOTAL_WEIGHT)
    res = sim.run_classes(16, cmap, hist=msim.HistSpec(**SPEC), run_begin=0, seed_base=SEED)
    f, s, L = _oracle(oracle, "c5", miners, 16, msim.C5_TOTAL_WEIGHT, begin=0)
    _check_point(res, f, s, L, cmap, 3, "c5")
    sums = sim.run(16, 0, SEED, 0).sums
    for c, g in enumerate(members):
        assert res.moments[c]["found"] == sum(sums[k].blocks_found for k in g)
        assert res.moments[c]["stale"] == sum(sums[k].stale_blocks for k in g)
    assert [(x.blocks_found, x.stale_blocks) for x in res.sums] == [(x.blocks_found, x.stale_blocks) for x in sums]


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared_draws"])
def test_gpu_classes_sweep_contrasts_against_oracle(msim, oracle, shared):
    """10 s / 1 s / 100 ms on the default hashrates, every class of every other point against 100 ms: cross words,
    moments and contrasts against the references on the folded oracle counters."""
    miners = msim.setup_miners()
    props = (10_000, 1_000, 100)
    if shared:
        sw = msim.propagation_sweep(miners, props, E2E_DURATION_MS)
    else:
        sw = msim.Sweep([msim.setup_miners(p) for p in props], E2E_DURATION_MS)
    cmap, members = msim.classes_of(miners)
    nc = len(members)
    pairs = msim.pairs_vs_baseline(3, nc, baseline=2)
    res = sw.run_classes(257, cmap, pairs=pairs, run_begin=E2E_BEGIN, seed_base=SEED)
    assert isinstance(res, msim.ContrastResult) and [tuple(q) for q in res.pairs] == [tuple(q) for q in pairs]
    data = []
    for p, prop in enumerate(props):
        f, s, L = _oracle(oracle, ("default", prop, 257), msim.setup_miners(prop), 257)
        cf, cs = _check_point(res.points[p], f, s, L, cmap, nc, ("sweep", prop))
        data.append((cf, cs, L))
    bad = cref.diff(res.cross, cref.expected(cref.columns(data), [tuple(q) for q in pairs]))
    assert not bad, bad[:8]
    mo = [ref.expected(*d) for d in data]
    con = msim.contrasts(res)
    for i, q in enumerate(pairs):
        want = cref.contrast(mo[q[0]][q[1]], mo[q[2]][q[3]], res.cross[i], 257)
        for name in cref.FIELDS:
            err = cref.field_error(name, con[i][name], want[name])
            assert err <= 1e-13, (q, name, con[i][name], want[name], err)
    assert len(msim.report_contrasts(res).splitlines()) == 2 * nc
    plain = sw.run_classes(257, cmap, run_begin=E2E_BEGIN, seed_base=SEED)
    assert [r.moments for r in plain] == [r.moments for r in res.points]


# ---------------------------------------------------------------- chunks and shards
def test_gpu_classes_chunks_and_shards(msim, monkeypatch):
    miners = msim.setup_miners()
    sim = msim.Simulation(miners, E2E_DURATION_MS)
    cmap, members = msim.classes_of(miners)
    pairs = msim.pairs_between_miners(len(members))
    hist = msim.HistSpec(**SPEC)
    run = (lambda n, b, **kw: sim.run_classes(n, cmap, run_begin=b, seed_base=SEED, **kw))
    whole, whole_h = run(300, E2E_BEGIN, pairs=pairs), run(300, E2E_BEGIN, hist=hist)
    a, b = run(150, E2E_BEGIN, hist=hist), run(150, E2E_BEGIN + 150, hist=hist)
    for x, y, z in zip(whole_h.moments, a.moments, b.moments):
        assert x == {k: y[k] + z[k] for k in x}
    assert np.array_equal(whole_h.hist, a.hist + b.hist)
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "128")
    parts, parts_h = run(300, E2E_BEGIN, pairs=pairs), run(300, E2E_BEGIN, hist=hist)
    assert parts.cross == whole.cross and parts.points[0].moments == whole.points[0].moments
    assert parts_h.moments == whole_h.moments and np.array_equal(parts_h.hist, whole_h.hist)
    assert whole.points[0].moments == whole_h.moments and whole.cross[0]["found_found"] > 0


# ---------------------------------------------------------------- the driver
def test_gpu_classes_host_driver_json(msim):
    """host/msim_main --runs 256 1 1000 c5 --errors --classes --json: its `classes` entries are error_bars() of
    Python's run_classes for the same seeds; the text form's class lines are report_classes's."""
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    miners = msim.c5_network()
    cmap, members = msim.classes_of(miners)
    res = msim.Simulation(miners, total_weight=msim.C5_TOTAL_WEIGHT).run_classes(256, cmap, run_begin=0, seed_base=SEED)
    want = msim.error_bars(res)
    r = subprocess.run([exe, "1", str(SEED), "c5", "--runs", "256", "--errors", "--classes", "--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["runs"] == 256 and len(got["miners"]) == 1026 and "errors" in got["miners"][0]
    assert [c["members"] for c in got["classes"]] == [1, 1, 1024]
    for c, e in zip(got["classes"], want):
        assert c["errors"] == {k: (None if math.isnan(v) else v) for k, v in e.items()}
    r = subprocess.run([exe, "1", str(SEED), "c5", "--runs", "256", "--errors", "--classes"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-3:] == msim.report_classes(miners, members, res).splitlines()
    assert sum(ln.startswith("  - Miner") for ln in lines) == 1026  # the class lines follow the miners' lines


def test_gpu_classes_host_driver_sweep_contrast(msim, tmp_path):
    """host/msim_main --sweep .. --classes --contrast 2 [--json]: the classes are those of the first point's miners,
    the `classes` entries carry error_bars() and contrasts() of Sweep.run_classes, and the text form's class and
    contrast lines are report_classes's and report_contrasts's with "Class" for "Miner"."""
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    props = (10_000, 1_000, 100)
    points = [msim.setup_miners(p) for p in props]
    spec = {"runs": 257, "seed_base": SEED, "duration_ms": E2E_DURATION_MS,
            "points": [{"miners": [{"id": mn.id, "perc": mn.perc, "propagation_ms": mn.propagation_ms,
                                    "selfish": False} for mn in pt]} for pt in points]}
    path = tmp_path / "sweep.json"
    path.write_text(json.dumps(spec))
    cmap, members = msim.classes_of(points[0])
    nc = len(members)
    res = msim.Sweep(points, E2E_DURATION_MS).run_classes(257, cmap, pairs=msim.pairs_vs_baseline(3, nc, baseline=2),
                                                          run_begin=0, seed_base=SEED)
    con = msim.contrasts(res)
    null = (lambda d: {k: (None if math.isnan(v) else v) for k, v in d.items()})
    r = subprocess.run([exe, "--sweep", str(path), "--contrast", "2", "--classes", "--json"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [json.loads(ln) for ln in r.stdout.strip().splitlines()[-3:]]
    for p in range(3):
        errs = msim.error_bars(res.points[p])
        assert [c["members"] for c in got[p]["classes"]] == [len(g) for g in members]
        assert all("contrast" not in x and "errors" not in x for x in got[p]["miners"])
        for c in range(nc):
            assert got[p]["classes"][c]["errors"] == null(errs[c]), (p, c)
            if p == 2:
                assert "contrast" not in got[p]["classes"][c]
            else:
                assert got[p]["classes"][c]["contrast"] == null(con[p * nc + c]), (p, c)
    r = subprocess.run([exe, "--sweep", str(path), "--contrast", "2", "--classes"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [ln for ln in lines if " vs point " in ln] == \
        msim.report_contrasts(res).replace("  - Miner ", "  - Class ").splitlines()
    want = [ln for p in range(3) for ln in msim.report_classes(points[p], members, res.points[p]).splitlines()]
    assert [ln for ln in lines if ln.startswith("  - Class") and " vs point " not in ln] == want

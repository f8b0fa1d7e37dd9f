"""The moments kernel (msim_moments.hip) and the entry points over it, on the device.

Synthetic records reach every extreme of the term and limb arithmetic (tests/moments_cases.py) at run and miner
counts around the kernel's tile and row boundaries; the end-to-end cases tie the kernel's divisions to every
engine's own msim_sums and to the oracle's counters. Every comparison is exact integer equality against
tests/moments_reference.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import instantiation_networks as nets
import moments_cases
import moments_reference as ref
import sums_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1000
E2E_RUNS = 257
E2E_DURATION_MS = 10**9  # as tests/test_gpu_sums.py: ~1 667 blocks a run, stale blocks in every run
E2E_BEGIN = 7000
RUN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
MINER_COUNTS = (1, 3, 15, 16, 17, 64, 65, 257)


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _spec(msim, bins):
    # share terms run to 2^64 - 2^32 in the synthetic records: bins over [2^20, ~2^33) and [0, ~2^34) leave
    # counts in the underflow bin, the overflow bin and in between
    return msim.HistSpec(bins, share_shift=msim.HistSpec.shift_covering(1 << 20, 1 << 33, bins),
                         rate_shift=msim.HistSpec.shift_covering(0, 1 << 34, bins), share_lo=1 << 20, rate_lo=0)


_CASES = {}


def _case(n, m, points):
    """Synthetic records of `points` points and their reference moments, built once per shape (read-only)."""
    key = (n, m, points)
    if key not in _CASES:
        data = [moments_cases.synthetic(n, m, seed=17 * p + n + m) for p in range(points)]
        want = [ref.expected(*d) for d in data]
        for d in data:
            for a in d:
                a.setflags(write=False)
        _CASES[key] = (data, want)
    return _CASES[key]


def _device_inputs(data):
    import torch

    dev = torch.device("cuda", 0)
    rec = np.stack([moments_cases.records(f, s) for f, s, _ in data])
    bh = np.stack([L for _, _, L in data])
    return (torch.from_numpy(rec.view(np.int32)).to(dev), torch.from_numpy(bh.view(np.int32)).to(dev))


def _ff(shape):
    import torch

    t = torch.empty(shape, dtype=torch.int64, device=torch.device("cuda", 0))
    t.view(torch.uint8).fill_(0xFF)
    return t


def _launch(msim, n, m, points, rec, bh, spec):
    """msim_moments_launch into 0xFF-filled outputs; (words [points, M, 20], hist or None) as uint64 arrays."""
    from miningsimulation_amd.simulation import _launch_moments

    mom = _ff((points, m, 20))
    hist = _ff((points, m, 2, spec.bins + 2)) if spec else None
    _launch_moments(m, points, n, rec, bh, mom, spec, hist, None)
    return mom, hist


def _check(msim, mom, hist, data, want, spec, what):
    from miningsimulation_amd.moments import moments_from_words

    words = mom.cpu().numpy().view(np.uint64)
    for p, (f, s, L) in enumerate(data):
        bad = ref.diff(moments_from_words(words[p]), want[p])
        assert not bad, (what, p, bad[:8])
    if spec:
        h = hist.cpu().numpy().view(np.uint64)
        for p, (f, s, L) in enumerate(data):
            exp = ref.expected_hist(f, s, L, spec.bins, spec.share_shift, spec.rate_shift, spec.share_lo, spec.rate_lo)
            assert np.array_equal(h[p], exp), (what, p, np.argwhere(h[p] != exp)[:5])
            assert (h[p].sum(axis=2) == f.shape[0]).all(), (what, p)


@pytest.mark.parametrize("bins", [0, 1, 64, 1024], ids=["nohist", "b1", "b64", "b1024"])
@pytest.mark.parametrize("points", [1, 3])
@pytest.mark.parametrize("m", MINER_COUNTS)
def test_gpu_moments_synthetic(msim, m, points, bins):
    """Every run count at one (M, points, bins): one upload of the 513-run records per count, no simulation."""
    import torch

    spec = _spec(msim, bins) if bins else None
    for n in RUN_COUNTS:
        data, want = _case(n, m, points)
        rec, bh = _device_inputs(data)
        mom, hist = _launch(msim, n, m, points, rec, bh, spec)
        torch.cuda.synchronize()
        _check(msim, mom, hist, data, want, spec, (n, m, points, bins))


@pytest.mark.parametrize("bins", [0, 64], ids=["nohist", "b64"])
def test_gpu_moments_c5_sized(msim, bins):
    """M = 1 026 (the shipped large network's miner count) x 513 runs: several miner tiles, the last one ragged."""
    import torch

    spec = _spec(msim, bins) if bins else None
    data, want = _case(513, 1026, 1)
    rec, bh = _device_inputs(data)
    mom, hist = _launch(msim, 513, 1026, 1, rec, bh, spec)
    torch.cuda.synchronize()
    _check(msim, mom, hist, data, want, spec, ("c5 sized", bins))


def test_gpu_moments_overwrites_its_outputs(msim):
    """Two launches in a row into the same 0xFF-filled outputs: each gives its own input's result."""
    import torch

    from miningsimulation_amd.simulation import _launch_moments

    spec = _spec(msim, 64)
    m = 17
    mom = _ff((1, m, 20))
    hist = _ff((1, m, 2, spec.bins + 2))
    for n in (257, 65):
        data, want = _case(n, m, 1)
        rec, bh = _device_inputs(data)
        _launch_moments(m, 1, n, rec, bh, mom, spec, hist, None)
        torch.cuda.synchronize()
        _check(msim, mom, hist, data, want, spec, ("overwrite", n))


def test_gpu_moments_launch_rejects_bad_arguments(msim):
    import ctypes

    import torch

    from miningsimulation_amd import _lib
    from miningsimulation_amd.simulation import _launch_moments

    data, _ = _case(2, 3, 1)
    rec, bh = _device_inputs(data)
    mom = _ff((1, 3, 20))
    with pytest.raises(ValueError):
        _launch_moments(3, 1, 3, rec, bh, mom, None, None, None)  # more runs than the buffers hold
    bad = _lib.MsimHistSpec(1025, 0, 0, 0, 0)
    hist = _ff((1, 3, 2, 1027))
    rc = _lib.lib.msim_moments_launch(3, 1, 2, ctypes.c_void_p(rec.data_ptr()), ctypes.c_void_p(bh.data_ptr()),
                                      ctypes.byref(bad), ctypes.c_void_p(mom.data_ptr()),
                                      ctypes.c_void_p(hist.data_ptr()), None)
    assert rc == _lib.MSIM_E_INVALID
    torch.cuda.synchronize()
    assert (mom.view(torch.uint8) == 0xFF).all()  # a rejected launch writes nothing


# ---------------------------------------------------------------- end to end, every engine
ROUTES = {
    "per_lane": ("honest_10s", {"MSIM_NO_PIPELINE": "1"}, 0),
    "pipeline": ("honest_10s", {}, 1),
    "wide": ("honest_10s", {"MSIM_FORCE_WIDE": "1"}, 2),
    "e1": ("selfish_uniform_1s", {}, 3),
    "e2": ("selfish_uniform_1s", {"MSIM_SEL_FORCE_RETRY": "1"}, 3),
    "general": ("honest_10s", {"MSIM_FORCE_GENERAL": "1"}, 4),
}
_ORACLE = {}


def _oracle(oracle, name, m, c):
    key = (name, m)
    if key not in _ORACLE:
        f, s, _, _ = oracle.run_batch(c["percs"], c["props"], c["selfish"], E2E_DURATION_MS, E2E_RUNS, E2E_BEGIN, SEED,
                                      threads=16, total_weight=c["W"])
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[key] = (f, s, ref.expected(f, s, f.sum(axis=1)))
    return _ORACLE[key]


def _sim(msim, c, duration=E2E_DURATION_MS):
    miners = [msim.Miner(i, p, q, bool(s)) for i, (p, q, s) in enumerate(zip(c["percs"], c["props"], c["selfish"]))]
    return msim.Simulation(miners, duration, total_weight=c["W"])


def _first_is_the_sums(res, what):
    got = [(mo["found"], mo["stale"], mo["share"], mo["rate"]) for mo in res.moments]
    bad = sums_reference.diff(got, sums_reference.combined(res.sums))
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("m", [3, 15])
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_moments_end_to_end(msim, oracle, monkeypatch, route, m):
    name, env, path = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = nets.case(name, m)
    sim = _sim(msim, c)
    assert sim.pipeline_info(E2E_RUNS)["uses_pipeline"] == path, sim.pipeline_info(E2E_RUNS)
    f, s, want = _oracle(oracle, name, m, c)
    assert (s.sum(axis=1) > 0).all()  # stale blocks in every run
    spec = msim.HistSpec.covering(0.0, 1.0, 64)
    res = sim.run_moments(E2E_RUNS, E2E_BEGIN, SEED, 0, hist=spec)
    bad = ref.diff(res.moments, want)
    assert not bad, (route, m, bad[:8])
    _first_is_the_sums(res, (route, m))
    exp = ref.expected_hist(f, s, f.sum(axis=1), spec.bins, spec.share_shift, spec.rate_shift, spec.share_lo, spec.rate_lo)
    assert np.array_equal(res.hist, exp)
    plain = sim.run(E2E_RUNS, E2E_BEGIN, SEED, 0)
    assert res.stats_total == plain.stats_total
    assert sums_reference.combined(res.sums) == sums_reference.combined(plain.sums)


def test_gpu_moments_two_point_sweep(msim, oracle):
    """The one-selfish network and its honest twin through Sweep.run_moments, per point against the oracle."""
    m = 9
    c = nets.case("selfish_uniform_1s", m)
    twin = dict(c, selfish=[False] * m)
    pts = [[msim.Miner(k, c["percs"][k], c["props"][k], sel and c["selfish"][k]) for k in range(m)]
           for sel in (True, False)]
    sw = msim.Sweep(pts, E2E_DURATION_MS)
    spec = msim.HistSpec.covering(0.0, 1.0, 64)
    out = sw.run_moments(E2E_RUNS, E2E_BEGIN, SEED, 0, hist=spec)
    plain = sw.run(E2E_RUNS, E2E_BEGIN, SEED, 0)
    for p, (nm, net) in enumerate((("selfish_uniform_1s", c), ("twin", twin))):
        f, s, want = _oracle(oracle, nm, m, net)
        bad = ref.diff(out[p].moments, want)
        assert not bad, (p, bad[:8])
        _first_is_the_sums(out[p], ("sweep", p))
        assert out[p].stats_total == plain[p].stats_total
        assert (out[p].hist.sum(axis=2) == E2E_RUNS).all()
        exp = ref.expected_hist(f, s, f.sum(axis=1), spec.bins, spec.share_shift, spec.rate_shift, 0, 0)
        assert np.array_equal(out[p].hist, exp)


@pytest.mark.parametrize("sweep", [False, True], ids=["run", "sweep"])
def test_gpu_moments_chunked_equals_unchunked(msim, monkeypatch, sweep):
    """MSIM_MOMENTS_CHUNK_RUNS=256 on 513 runs: three chunks, added limb by limb on the host."""
    m = 9
    c = nets.case("selfish_uniform_1s", m)
    spec = msim.HistSpec.covering(0.0, 1.0, 64)
    if sweep:
        pts = [[msim.Miner(k, c["percs"][k], c["props"][k], sel and c["selfish"][k]) for k in range(m)]
               for sel in (True, False)]
        obj = msim.Sweep(pts, E2E_DURATION_MS)
    else:
        obj = _sim(msim, c)
    run = (lambda: obj.run_moments(513, E2E_BEGIN, SEED, 0, hist=spec))
    whole = run()
    monkeypatch.setenv("MSIM_MOMENTS_CHUNK_RUNS", "256")
    parts = run()
    for a, b in zip(whole if sweep else [whole], parts if sweep else [parts]):
        assert a.moments == b.moments
        assert np.array_equal(a.hist, b.hist)
        assert a.stats_total == b.stats_total
        assert sums_reference.combined(a.sums) == sums_reference.combined(b.sums)
    assert (whole[0] if sweep else whole).moments[0]["found"] > 0


def test_gpu_moments_host_driver_errors_json(msim, tmp_path):
    """host/msim_main --errors --json on a small network: its `errors` are error_bars of run_moments."""
    exe = os.path.join(ROOT, "host", "msim_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "host")], check=True)
    m = 5
    c = nets.case("selfish_uniform_1s", m)
    spec = {"runs": E2E_RUNS, "seed_base": SEED, "duration_ms": E2E_DURATION_MS,
            "points": [{"miners": [{"id": k, "perc": c["percs"][k], "propagation_ms": c["props"][k],
                                    "selfish": bool(c["selfish"][k])} for k in range(m)]}]}
    path = tmp_path / "net.json"
    path.write_text(json.dumps(spec))
    r = subprocess.run([exe, "--sweep", str(path), "--errors", "--json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    res = _sim(msim, c).run_moments(E2E_RUNS, 0, SEED, 0)
    want = msim.error_bars(res)
    assert len(got["miners"]) == m
    for k in range(m):
        assert got["miners"][k]["errors"] == want[k], (k, got["miners"][k]["errors"], want[k])
        assert want[k]["found_se"] > 0.0 and want[k]["share_se"] > 0.0
    # and the report form appends the columns report_with_errors does
    r = subprocess.run([exe, "--sweep", str(path), "--errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("  - Miner")]
    mine = msim.report_with_errors(_sim(msim, c).miners, res, E2E_DURATION_MS).splitlines()[1:]
    assert lines == mine

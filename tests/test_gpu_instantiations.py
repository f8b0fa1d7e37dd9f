"""Every per-miner-count instantiation on the device, against the oracle.

MSIM_FOR_EACH_M compiles K2 (lean and mid), K3, the per-lane kernel, E1 and E2 once per M = 1..15, E1 and E2 also
per selfish class and for uniform / mixed delays; registers, spills, occupancy (k2_waves) and E1's static LDS differ
per M, and the host harness (the same headers compiled for x86) sees none of that. The other GPU tests reach a few
miner counts through seeded random draws; here each (case, M) of tests/instantiation_networks.py is its own test,
so a failure names the kernel family and the miner count.

Bar: per-run found, stale and best height identical to the oracle, 70 runs (one wave and a ragged second) of
5e9 ms; each case first asserts the path msim_pipeline_info reports, so it cannot pass on another engine."""
import numpy as np
import pytest

import instantiation_networks as nets

pytestmark = pytest.mark.gpu

N = nets.N_RUNS
D = nets.DURATION_MS
SEED_BASE = 1000


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _begin(m):
    return 100 * m  # another run range per miner count


def _same_as_oracle(res, f, s, what):
    assert np.array_equal(res.found.astype(np.int64), f), (what, np.argwhere(res.found != f)[:5])
    assert np.array_equal(res.stale.astype(np.int64), s), (what, np.argwhere(res.stale != s)[:5])
    assert np.array_equal(res.best_height.astype(np.int64), f.sum(axis=1)), what


@pytest.mark.parametrize("name,m", nets.MATRIX, ids=[f"{n}-M{m}" for n, m in nets.MATRIX])
def test_gpu_instantiation_vs_oracle(msim, oracle, monkeypatch, name, m):
    c = nets.case(name, m)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    miners = [msim.Miner(k, c["percs"][k], c["props"][k], c["selfish"][k]) for k in range(m)]
    sim = msim.Simulation(miners, D, total_weight=c["W"])
    assert sim.pipeline_info(N)["uses_pipeline"] == c["path"], sim.pipeline_info(N)
    f, s = nets.oracle_counters(oracle, name, m, _begin(m), SEED_BASE)
    if name == "honest_10s" and m >= 2:
        assert s.sum() > 0  # stale blocks: K2's episodes really ran
    res = sim.run(N, _begin(m), SEED_BASE, 0, per_run=True)
    _same_as_oracle(res, f, s, (name, m))


@pytest.mark.parametrize("m", range(2, 16))
def test_gpu_instantiation_sweep_vs_oracle(msim, oracle, m):
    """The one-selfish uniform network and its honest twin as a 2-point sweep (the honest point through the
    selfish instantiation), 70 runs per point."""
    c = nets.case("selfish_uniform_1s", m)
    pts = [[msim.Miner(k, c["percs"][k], c["props"][k], sel and c["selfish"][k]) for k in range(m)]
           for sel in (True, False)]
    sw = msim.Sweep(pts, D)
    for sim in sw.sims:
        assert sim.pipeline_info(N)["uses_pipeline"] in (1, 3)  # alone: E1, or the honest pipeline for the twin
    assert sw.sims[0].pipeline_info(N)["uses_pipeline"] == 3
    out = sw.run(N, _begin(m), SEED_BASE, 0, per_run=True)
    f, s = nets.oracle_counters(oracle, "selfish_uniform_1s", m, _begin(m), SEED_BASE)
    _same_as_oracle(out[0], f, s, ("sweep selfish", m))
    hf, hs, _, _ = oracle.run_batch(c["percs"], c["props"], [False] * m, D, N, _begin(m), SEED_BASE, threads=16)
    _same_as_oracle(out[1], hf, hs, ("sweep honest twin", m))

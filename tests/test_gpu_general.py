"""The general engine G (msim_general.h, msim_general.hip) on the GPU, through the C ABI, against the oracle:
per-run found and stale counters bit-exact.

G serves every network with selfish miners that the entity engine does not (more than 4 selfish miners, a
selfish miner in a network of more than 15 miners) and finishes the runs the entity engine cannot (a
selfish majority whose withheld chain outgrows the 16-height window). These are exactly the networks
round 2 rejected with MSIM_E_SELFISH / MSIM_E_CAPACITY (Missing #1-#2, Weak #10)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DAY = 86_400_000
D = 31_556_952_000


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _rand_weights(m, rng, total=100):
    cuts = sorted(rng.sample(range(1, total), m - 1)) if m > 1 else []
    b = [0] + cuts + [total]
    return [b[i + 1] - b[i] for i in range(m)]


def _status(sim, n, seed):
    """A second launch of the same runs through msim_launch: its status words, and the five counter words at the head
    of the workspace (msim_general_launch.h GEN_C_*: flagged, failed, tier lists 1..3)."""
    import torch

    m = len(sim.miners)
    ws = torch.zeros(sim.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    sums = torch.zeros((m, 6), dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    sim.launch(n, 0, seed, sums, ws, st)
    torch.cuda.synchronize()
    return st.cpu().numpy().astype(np.int64), ws[:20].cpu().numpy().view(np.uint32).astype(np.int64), sums.cpu().numpy()


def _vs_oracle(msim, oracle, p, q, s, n, seed, dur, W=100, path=None, ids=None, status=False):
    """The result of msim_run; with status=True the pair (result, _status of a second launch), whose sums must be the
    first launch's."""
    ids = list(range(len(p))) if ids is None else ids
    miners = [msim.Miner(ids[k], p[k], q[k], bool(s[k])) for k in range(len(p))]
    sim = msim.Simulation(miners, dur, total_weight=W)
    if path is not None:
        assert sim.pipeline_info(n)["uses_pipeline"] == path
    res = sim.run(n, 0, seed, 0, per_run=True)
    f, st, sh, rt = oracle.run_batch(p, q, s, dur, n, 0, seed, threads=16, total_weight=W, ids=ids)
    assert np.array_equal(res.found.astype(np.int64), f), (p, q, s, dur, seed)
    assert np.array_equal(res.stale.astype(np.int64), st), (p, q, s, dur, seed)
    if len(set(ids)) == len(ids) and 0xFFFFFFFF not in ids:
        assert np.array_equal(res.best_height.astype(np.int64), f.sum(axis=1))
    # MinerStats summed in run order (main.cpp:211-217): the exact f64 aggregate
    for k in range(len(p)):
        assert res.stats_total[k].blocks_found == int(f[:, k].sum())
        assert res.stats_total[k].blocks_share == sum(sh[:, k].tolist())
        assert res.stats_total[k].stale_rate == sum(rt[:, k].tolist())
    if status:
        st, counts, sums = _status(sim, n, seed)
        assert sums.tobytes() == np.array([[getattr(x, f) for f, _ in x._fields_] for x in res.sums], dtype=np.int64).tobytes()
        return res, (st, counts)
    return res


def test_gpu_general_100_miners_one_selfish(msim, oracle):
    """A 100-miner network (integer weights, W = 1000) with one selfish miner at 30 %, 1 s delays."""
    rng = random.Random(5)
    p = [300] + _rand_weights(99, rng, 700)
    _vs_oracle(msim, oracle, p, [1000] * 100, [True] + [False] * 99, 64, 77, 7 * DAY, W=1000, path=4)


def test_gpu_general_majority_two_selfish(msim, oracle):
    """Two selfish miners holding 70 % (the entity engine flags these runs; E2 hands G those it cannot finish):
    E1 flags at least one run, nothing fails, status[0] is what E1 flagged, G's first list holds no more than that,
    and each tier's list no more than the one before."""
    _, (st, counts) = _vs_oracle(msim, oracle, [35, 35, 20, 10], [1000] * 4, [True, True, False, False], 64, 4242,
                                 30 * DAY, path=3, status=True)
    print(f"two selfish miners, 64 runs: status {st.tolist()}, counters {counts.tolist()}")
    assert st[1] == 0 and counts[1] == 0, (st, counts)
    assert counts[0] > 0, (st, counts)
    assert st[0] == counts[0] >= counts[2] >= counts[3] >= counts[4], (st, counts)


def test_gpu_general_selfish_majority_one_miner(msim, oracle):
    """One selfish miner with 60 % for a year: its lead grows all year (a run whose selfish miner never has to reveal
    ends with none of its blocks in the best chain). The entity engine's settled form (msim_selm.h) serves a single
    selfish miner whatever its lead, so E1 flags none of these runs and none reaches G: the status and the five
    counter words of the launch are 0. G's last window is reached on the device through lowered windows
    (tests/test_gpu_general_tiers.py)."""
    _, (st, counts) = _vs_oracle(msim, oracle, [60, 25, 15], [100, 100, 100], [True, False, False], 16, 99, D, path=3,
                                 status=True)
    assert st.tolist() == [0, 0] and counts.tolist() == [0] * 5, (st, counts)


def test_gpu_general_many_selfish(msim, oracle):
    """Six selfish miners (the entity engine serves at most four), random networks up to 15 miners."""
    _vs_oracle(msim, oracle, [10] * 6 + [20, 20], [1000] * 8, [True] * 6 + [False] * 2, 64, 7, 30 * DAY, path=4)
    rng = random.Random(31)
    for _ in range(4):
        m = rng.randint(6, 15)
        p = _rand_weights(m, rng)
        s = [k < 5 for k in range(m)]
        rng.shuffle(s)
        q = [rng.choice([0, 100, 1000, 10_000]) for _ in range(m)]
        _vs_oracle(msim, oracle, p, q, s, 32, rng.randrange(2**32), 30 * DAY, path=4)


def test_gpu_general_forced_equals_fast_paths(msim, oracle, monkeypatch):
    """MSIM_FORCE_GENERAL routes BASELINE configs[1] / configs[2] networks onto G: same counters as the
    oracle (and hence as the pipelines and the entity engine)."""
    monkeypatch.setenv("MSIM_FORCE_GENERAL", "1")
    for name in ("c2", "c3"):
        miners = msim.PRESETS[name]()
        p = [mm.perc for mm in miners]
        q = [mm.propagation_ms for mm in miners]
        s = [mm.is_selfish for mm in miners]
        _vs_oracle(msim, oracle, p, q, s, 256, 1000, D, path=4)


def test_gpu_general_as_e2_fallback(msim, oracle, monkeypatch):
    """MSIM_SEL_FORCE_RETRY + MSIM_SEL_FORCE_GEN: E1 flags every run, E2 hands every run to G, so G
    computes the whole configs[2] batch through the fallback lists: bit-exact per run."""
    monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
    monkeypatch.setenv("MSIM_SEL_FORCE_GEN", "1")
    miners = msim.PRESETS["c3"]()
    p = [mm.perc for mm in miners]
    q = [mm.propagation_ms for mm in miners]
    s = [mm.is_selfish for mm in miners]
    _vs_oracle(msim, oracle, p, q, s, 512, 1000, D, path=3)


def test_gpu_general_sweep(msim, oracle):
    """A sweep with a point only G serves runs every point on G: per-point per-run counters vs the oracle."""
    pts = [[msim.Miner(k, w, 1000, k < 5) for k, w in enumerate([10] * 7 + [15, 15])],
           msim.PRESETS["c3"](), msim.PRESETS["c2"]()]
    sw = msim.Sweep(pts, 30 * DAY)
    res = sw.run(32, 0, 500, 0, per_run=True)
    for i, miners in enumerate(pts):
        p = [mm.perc for mm in miners]
        q = [mm.propagation_ms for mm in miners]
        s = [mm.is_selfish for mm in miners]
        f, st, _, _ = oracle.run_batch(p, q, s, 30 * DAY, 32, 0, 500, threads=16)
        assert np.array_equal(res[i].found.astype(np.int64), f), i
        assert np.array_equal(res[i].stale.astype(np.int64), st), i


def test_gpu_general_large_honest_network(msim, oracle):
    """5 000 honest miners (more than the large-network pipeline's 4 096): G, per run vs the oracle."""
    rng = random.Random(11)
    p = [2000, 1500] + [rng.randint(1, 3) for _ in range(4998)]
    W = sum(p)
    _vs_oracle(msim, oracle, p, [1000] * 5000, [False] * 5000, 32, 321, DAY, W=W, path=4)


def test_gpu_general_shared_ids(msim, oracle):
    """Miners sharing an id (the reference accepts them): shared block identity (simulation.h:35-38), stale
    counting (simulation.h:133) and found counts (main.cpp:24-26), bit-exact per run, on G."""
    _vs_oracle(msim, oracle, [30, 29, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [False] * 9, 64, 1000, 30 * DAY,
               path=4, ids=[0, 1, 2, 0, 4, 5, 1, 7, 0])
    _vs_oracle(msim, oracle, [40, 19, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [True] + [False] * 8, 64, 99, 30 * DAY,
               path=4, ids=[5, 5, 2, 3, 4, 5, 6, 7, 8])
    _vs_oracle(msim, oracle, [34, 33, 33], [0, 0, 0], [False] * 3, 32, 7, 7 * DAY, path=4, ids=[9, 9, 9])


def test_gpu_general_genesis_id(msim, oracle):
    """A miner with id UINT_MAX (Genesis's id, simulation.h:31-33) counts Genesis among its found blocks."""
    U = 0xFFFFFFFF
    _vs_oracle(msim, oracle, [30, 29, 12, 11, 8, 5, 3, 1, 1], [100] * 9, [False] * 9, 64, 1000, 30 * DAY,
               path=4, ids=[U, 1, 2, 3, 4, 5, 6, 7, 8])
    _vs_oracle(msim, oracle, [40, 19, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [True] + [False] * 8, 64, 5, 30 * DAY,
               path=4, ids=[0, 1, 2, 3, 4, 5, 6, 7, U])
    _vs_oracle(msim, oracle, [60, 40], [10, 10], [False, False], 8, 3, 0, path=4, ids=[U, U])

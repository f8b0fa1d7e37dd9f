"""The slice loops of a launch on the device, and the run-index arithmetic that goes with them.

Four paths cut a launch into slices that reuse one workspace: the honest pipeline (launch_pipeline), the
large-network pipeline (launch_wide) and E1 for a single network and for a sweep (sel_launch_impl). A second slice
begins only past 16 GiB of workspace or 2^22 runs per point, so the test switch MSIM_MAX_SLICE_RUNS=256 caps a
slice at 256 runs here: 805 runs are three full slices and a ragged fourth of 37, on a workspace that still holds
the previous slice's lists, slots and records. Every test asserts msim_pipeline_info's slice_runs == 256 < n first,
so none can pass on a single slice, and every comparison is exact (found, stale, best height of every run).

The last section feeds the per-run seeds (seed_base + 2r) mod 2^32 run indices that wrap, against oracle.run with
the two seeds computed here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DAY = 86_400_000
D30 = 30 * DAY
SWITCH = "MSIM_MAX_SLICE_RUNS"
P9 = [30, 29, 12, 11, 8, 5, 3, 1, 1]
C5_W = [30720, 29696] + [41] * 1024
C5_TOTAL = 102_400


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


_REF = {}


def _oracle(oracle, p, q, s, duration, n, begin, base=1000, W=100):
    """(found, stale) of runs [begin, begin + n) from the oracle: computed once per network, read-only."""
    k = (tuple(p) if len(p) < 20 else len(p), tuple(q[:16]), tuple(s[:16]), duration, n, begin, base, W)
    if k not in _REF:
        f, st, _, _ = oracle.run_batch(p, q, [bool(x) for x in s], duration, n, begin, base, threads=16, total_weight=W)
        f.setflags(write=False)
        st.setflags(write=False)
        _REF[k] = (f, st)
    return _REF[k]


def _pqs(miners):
    return [m.perc for m in miners], [m.propagation_ms for m in miners], [m.is_selfish for m in miners]


def _same_as_oracle(res, ref, what=None):
    f, s = ref
    assert np.array_equal(res.found.astype(np.int64), f), (what, np.argwhere(res.found != f)[:5])
    assert np.array_equal(res.stale.astype(np.int64), s), (what, np.argwhere(res.stale != s)[:5])
    assert np.array_equal(res.best_height.astype(np.int64), f.sum(axis=1)), what


def _sum_bytes(res):
    return b"".join(bytes(x) for x in res.sums)


def _capped(monkeypatch, sim, n, path):
    """Sets the switch and asserts that `sim` then runs n runs in slices of 256 on the given path."""
    monkeypatch.setenv(SWITCH, "256")
    info = sim.pipeline_info(n)
    assert n > 256 and info["slice_runs"] == 256 and info["uses_pipeline"] == path, info
    return info


class _Uncapped:
    """with _Uncapped(monkeypatch): the switch is unset inside, and back afterwards."""

    def __init__(self, monkeypatch):
        self.cm = monkeypatch.context()

    def __enter__(self):
        self.cm.__enter__().delenv(SWITCH, raising=False)

    def __exit__(self, *a):
        return self.cm.__exit__(*a)


def _launch(sim, n, begin, base=1000, fill=0x00, records=True):
    """One device-resident launch (msim_launch) on a workspace filled with `fill`: (sums, records, best height,
    status) on the host."""
    import torch

    dev = torch.device("cuda", 0)
    m = len(sim.miners)
    ws = torch.full((sim.workspace_bytes(n),), fill, dtype=torch.uint8, device=dev)
    sums = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    rec = torch.zeros((n, m, 2), dtype=torch.int32, device=dev) if records else None
    bh = torch.zeros(n, dtype=torch.int32, device=dev) if records else None
    sim.launch(n, begin, base, sums, ws, status, d_per_run=rec, d_best_height=bh)
    torch.cuda.synchronize()
    return (sums.cpu(), rec.cpu() if records else None, bh.cpu() if records else None, status.cpu().tolist())


# ---------------------------------------------------------------- 1. honest pipeline
@pytest.mark.parametrize("preset", ["c2", "c1"])
def test_gpu_slices_honest_pipeline_vs_oracle(msim, oracle, monkeypatch, preset):
    """The 9-miner preset at 100 ms (c2: K2 lean) and at 10 s (c1: K2 mid, rho ~ 1.7 %, chunked list reservation
    with hole marking), 30 days, four slices: K3's rel_begin + r in the records, parts + (off / K3_TPB) * 6 * M,
    the per-slice reset of the list counter. The fixed-point sums equal the single-slice launch's byte for byte."""
    n, begin = 805, 4096
    miners = msim.PRESETS[preset]()
    sim = msim.Simulation(miners, D30)
    _capped(monkeypatch, sim, n, 1)
    res = sim.run(n, begin, 1000, 0, per_run=True)
    _same_as_oracle(res, _oracle(oracle, *_pqs(miners), D30, n, begin))
    with _Uncapped(monkeypatch):
        one = msim.Simulation(miners, D30)
        assert one.pipeline_info(n)["slice_runs"] >= n
        whole = one.run(n, begin, 1000, 0, per_run=True)
    assert _sum_bytes(res) == _sum_bytes(whole)


# ---------------------------------------------------------------- 2. retries from later slices
# The pipeline takes a network only below 262 s delays and a fork rate of 8 %, and every capacity of K1-K3 has an
# 8-sigma margin there: K3 flags a run for the retry kernel by an event no test can wait for (the CPU harness of
# the same lane bodies flags none of 600 runs of 1e10 ms at 48 s or at 250 s delays). The 300 s network of
# test_gpu_retry_path_huge_delays does retry, but on the per-lane kernel (its fork rate is 39 %), which has no
# slices. So the retries here are forced: MSIM_PIPE_FORCE_RETRY makes K3 flag every run, as MSIM_SEL_FORCE_RETRY
# does for E1. The network is the same nine miners at 48 s, the longest uniform delay the pipeline takes.
RETRY_Q = [48_000] * 9
RETRY_D = 10**10


def test_gpu_slices_retries_from_later_slices(msim, oracle, monkeypatch):
    """K3 of slices 2 and 3 appends rel_begin + r to the retry list; the retry kernel reads those as indices
    relative to the launch's first run (seeds and record rows). First, uncapped: the ranges [256, 512) and
    [512, 600) launched on their own do retry (status[0] != 0). Then the 600 runs capped at 256: every run
    retried, none failed, all equal to the oracle."""
    n = 600
    monkeypatch.setenv("MSIM_PIPE_FORCE_RETRY", "1")
    miners = [msim.Miner(k, P9[k], RETRY_Q[k]) for k in range(9)]
    sim = msim.Simulation(miners, RETRY_D)
    assert sim.pipeline_info(n)["uses_pipeline"] == 1 and sim.pipeline_info(n)["slice_runs"] >= n
    retried = [_launch(sim, cnt, b, records=False)[3][0] for b, cnt in ((256, 256), (512, 88))]
    assert retried[0] != 0 or retried[1] != 0, retried
    _capped(monkeypatch, sim, n, 1)
    sums, rec, bh, status = _launch(sim, n, 0)
    assert status == [n, 0], status
    f, s = _oracle(oracle, P9, RETRY_Q, [0] * 9, RETRY_D, n, 0)
    assert np.array_equal(rec[:, :, 0].numpy().astype(np.int64), f)
    assert np.array_equal(rec[:, :, 1].numpy().astype(np.int64), s)
    assert np.array_equal(bh.numpy().astype(np.int64), f.sum(axis=1))
    assert sums[:, 0].tolist() == f.sum(axis=0).tolist() and sums[:, 1].tolist() == s.sum(axis=0).tolist()


def test_gpu_slices_long_delay_pipeline_vs_oracle(msim, oracle, monkeypatch):
    """The same 48 s network without forcing: K2's mid machine at the pipeline's highest fork rate, three slices."""
    n = 600
    miners = [msim.Miner(k, P9[k], RETRY_Q[k]) for k in range(9)]
    sim = msim.Simulation(miners, RETRY_D)
    _capped(monkeypatch, sim, n, 1)
    _same_as_oracle(sim.run(n, 0, 1000, 0, per_run=True), _oracle(oracle, P9, RETRY_Q, [0] * 9, RETRY_D, n, 0))


def test_gpu_switch_leaves_the_per_lane_kernel_alone(msim, oracle, monkeypatch):
    """The 300 s network of test_gpu_retry_path_huge_delays runs on the per-lane kernel and its retry kernel, which
    have no slices: with the switch set it reports no slice size and still equals the oracle on 600 runs."""
    n = 600
    monkeypatch.setenv(SWITCH, "256")
    sim = msim.Simulation([msim.Miner(k, P9[k], 300_000) for k in range(9)], RETRY_D)
    info = sim.pipeline_info(n)
    assert info["uses_pipeline"] == 0 and info["slice_runs"] == 0, info
    _same_as_oracle(sim.run(n, 0, 1000, 0, per_run=True), _oracle(oracle, P9, [300_000] * 9, [0] * 9, RETRY_D, n, 0))


# ---------------------------------------------------------------- 3. device-resident launch, dirty workspace
@pytest.mark.parametrize("preset", ["c1", "c2"])
def test_gpu_slices_dirty_workspace_equals_clean(msim, monkeypatch, preset):
    """msim_launch with records on a workspace of 0xFF bytes, four slices: every slice after the first also starts
    on its predecessor's lists, slots and records. Equal to the single-slice launch on a zeroed workspace."""
    import torch

    n, begin = 805, 4096
    sim = msim.Simulation(msim.PRESETS[preset](), D30)
    assert sim.pipeline_info(n)["slice_runs"] >= n
    clean = _launch(sim, n, begin, fill=0x00)
    assert clean[3][1] == 0
    _capped(monkeypatch, sim, n, 1)
    dirty = _launch(sim, n, begin, fill=0xFF)
    assert dirty[3][1] == 0, dirty[3]
    for a, b in zip(clean[:3], dirty[:3]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. large-network pipeline
@pytest.fixture(scope="module")
def c5_ref(oracle):
    return _oracle(oracle, C5_W, [1000] * 1026, [0] * 1026, 3 * DAY, 525, 0, W=C5_TOTAL)


def _c5(msim):
    sim = msim.Simulation(msim.c5_network(), 3 * DAY, total_weight=C5_TOTAL)
    assert sim.wide
    return sim


def test_gpu_slices_wide_vs_oracle(msim, c5_ref, monkeypatch):
    """configs[4]'s network (1 026 miners, W = 102 400), 3 days, two slices and 13 runs: W3's out.rel_begin + r,
    the per-slice reset of the work and retry counters. The sums' exact values equal the single-slice launch's
    (its workgroups split the Q32.32 limbs differently, so the limbs themselves may differ)."""
    n = 525
    sim = _c5(msim)
    _capped(monkeypatch, sim, n, 2)
    res = sim.run(n, 0, 1000, 0, per_run=True)
    _same_as_oracle(res, c5_ref)
    with _Uncapped(monkeypatch):
        one = _c5(msim)
        assert one.pipeline_info(n)["slice_runs"] >= n
        whole = one.run(n, 0, 1000, 0, per_run=True)
    for a, b in zip(res.sums, whole.sums):
        assert (a.blocks_found, a.stale_blocks) == (b.blocks_found, b.stale_blocks)
        assert (a.share_hi << 32) + a.share_lo == (b.share_hi << 32) + b.share_lo
        assert (a.rate_hi << 32) + a.rate_lo == (b.rate_hi << 32) + b.rate_lo


@pytest.mark.parametrize("runs", ["1", "2", "4", "8"])
def test_gpu_wide_ragged_workgroups(msim, c5_ref, monkeypatch, runs):
    """13 runs, uncapped: no multiple of W1's runs per workgroup (MSIM_W1_RUNS) nor of the layout's rounding to 4."""
    monkeypatch.setenv("MSIM_W1_RUNS", runs)
    res = _c5(msim).run(13, 0, 1000, 0, per_run=True)
    _same_as_oracle(res, (c5_ref[0][:13], c5_ref[1][:13]), runs)


# ---------------------------------------------------------------- 5. E1, single network
@pytest.mark.parametrize("forced", [False, True], ids=["e1", "forced_retry"])
def test_gpu_slices_e1_vs_oracle(msim, oracle, monkeypatch, forced):
    """configs[2]'s network, 30 days, four slices: E1's partial row a.s0 / TPB + blk, rel = a.s0 + lr, the cold-slot
    lane index. Forced (MSIM_SEL_FORCE_RETRY): E2 runs after the slice loop with s0 = 0 over the runs every slice
    flagged."""
    n, begin = 805, 4096
    if forced:
        monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
    miners = msim.PRESETS["c3"]()
    sim = msim.Simulation(miners, D30)
    _capped(monkeypatch, sim, n, 3)
    _same_as_oracle(sim.run(n, begin, 1000, 0, per_run=True), _oracle(oracle, *_pqs(miners), D30, n, begin))


# ---------------------------------------------------------------- 6. E1, sweep
def test_gpu_slices_sweep_vs_oracle(msim, oracle, monkeypatch):
    """Four points, 600 runs per point in three slices: a selfish point, an honest point through the selfish
    instantiation, a 30 s point, and a point with two selfish miners (two selfish-class groups launch per slice).
    Every point equals the oracle run by run, and the sums equal the single-slice sweep's byte for byte."""
    rpp, begin = 600, 123
    two = [msim.Miner(k, P9[k], 1000, k in (0, 2)) for k in range(9)]  # 30 % + 12 % selfish
    pts = [msim.setup_miners(1000, selfish_perc=40), msim.setup_miners(100), msim.setup_miners(30000, selfish_perc=45), two]
    sw = msim.Sweep(pts, D30)
    whole = sw.run(rpp, begin, 1000, 0)
    # a sweep has no msim_pipeline_info of its own: its slices come from the same layout function (sel_ws_layout)
    # as its selfish points', whose info is asserted here
    _capped(monkeypatch, sw.sims[0], rpp, 3)
    out = sw.run(rpp, begin, 1000, 0, per_run=True)
    for i, (miners, res, one) in enumerate(zip(pts, out, whole)):
        _same_as_oracle(res, _oracle(oracle, *_pqs(miners), D30, rpp, begin), i)
        assert _sum_bytes(res) == _sum_bytes(one), i


# ---------------------------------------------------------------- seed wrap-around
WRAPS = [(2**32 - 100, 0), (1000, 2**31 - 32), (1000, 2**32 + 5)]  # (seed_base, run_begin)
WRAP_N = 128


def _wrap_networks(msim):
    return {"c2": (msim.PRESETS["c2"](), D30, 100, 1), "c3": (msim.PRESETS["c3"](), D30, 100, 3),
            "c5": (msim.c5_network(), 3 * DAY, C5_TOTAL, 2)}


@pytest.mark.parametrize("base,begin", WRAPS, ids=["base_wraps_mid_launch", "2r_wraps", "run_index_above_2^32"])
@pytest.mark.parametrize("net", ["c2", "c3", "c5"])
def test_gpu_seed_wraparound(msim, oracle, net, base, begin):
    """(seed_base + 2r) mod 2^32 with a 64-bit run index r, as K1, the per-lane kernel, E1, E2 and W1 feed it: 128
    runs whose seeds wrap inside the launch, or whose run index has bits above 2^31 / 2^32. Expected: oracle.run per
    run with both seeds computed here, not by run_batch's own convention."""
    miners, duration, W, path = _wrap_networks(msim)[net]
    sim = msim.Simulation(miners, duration, total_weight=W)
    assert sim.pipeline_info(WRAP_N)["uses_pipeline"] == path
    res = sim.run(WRAP_N, begin, base, 0, per_run=True)
    p, q, s = _pqs(miners)
    for i in range(WRAP_N):
        r = begin + i
        si, sp = (base + 2 * r) & 0xFFFFFFFF, (base + 2 * r + 1) & 0xFFFFFFFF
        rc, fs, best = oracle.run(p, q, s, duration, si, sp, total_weight=W)
        assert rc == 0
        assert np.array_equal(res.found[i].astype(np.int64), fs[:, 0]), (net, base, begin, i)
        assert np.array_equal(res.stale[i].astype(np.int64), fs[:, 1]), (net, base, begin, i)
        assert int(res.best_height[i]) == best, (net, base, begin, i)

"""The device's fixed-point sums (msim_sums) on every engine, against an exact reference.

msim_sums is what the product ships: bench.py times it, host/msim_main prints it, msim_run_multi all-reduces it and
msim_run returns it whenever no per-run records are requested. Seven pieces of device code produce it (the per-lane
kernel and its retry, the sweep kernel with its atomic retry sums, K3, E1 / E2 with their finalize, W3's LDS
accumulators and limb-splitting flush, G's global atomics, and the host's conversion); the other GPU tests compare
sums with other device sums, or read the records only.

Bar: tests/sums_reference.py rebuilds every per-run term bit for bit from the oracle's integer counters, and the
combined value (hi << 32) + lo of a sum does not depend on how runs were split into waves, workgroups, slices or
atomics, so every comparison is exact integer equality, no tolerance anywhere. Each test first asserts the path
msim_pipeline_info reports, so it cannot pass on another engine. A failure names the miner, the field and both
integers."""
from fractions import Fraction

import numpy as np
import pytest

import instantiation_networks as nets
import sums_reference as ref

pytestmark = pytest.mark.gpu

N = nets.N_RUNS
D = nets.DURATION_MS
SEED = 1000
DAY = 86_400_000
DEFAULT_PERCS = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _begin(m):
    return 100 * m  # another run range per miner count (as tests/test_gpu_instantiations.py: the oracle cache is shared)


def _net(percs, props, selfish, W=100, ids=None):
    return {"percs": list(percs), "props": list(props), "selfish": [bool(x) for x in selfish], "W": W,
            "ids": list(range(len(percs))) if ids is None else list(ids)}


def _sim(msim, c, duration=D):
    ids = c.get("ids") or range(len(c["percs"]))
    miners = [msim.Miner(i, p, q, bool(s)) for i, p, q, s in zip(ids, c["percs"], c["props"], c["selfish"])]
    return msim.Simulation(miners, duration, total_weight=c["W"])


def _path(sim, n, want):
    info = sim.pipeline_info(n)
    assert info["uses_pipeline"] == want, info


def _exact(got, want, what, fields=range(4)):
    bad = ref.diff(got, want, fields)
    assert not bad, (what, bad[:8])


def _stats_are_the_sums(stats_total, want, what):
    """msim_run without records: out_sums is msim_sums_to_stats of the device sums (one rounding of the exact value)."""
    for k, w in enumerate(want):
        st = stats_total[k]
        assert st.blocks_found == w[0], (what, k, st.blocks_found, w[0])
        assert st.blocks_share == float(Fraction(w[2], 1 << 32)), (what, k, st.blocks_share, w[2])
        assert st.stale_rate == float(Fraction(w[3], 1 << 32)), (what, k, st.stale_rate, w[3])


_BATCH = {}


def _oracle(oracle, key, c, duration, n, begin):
    """(found, stale, share, rate) of a network from the oracle, computed once per key; the arrays are read-only."""
    if key not in _BATCH:
        out = oracle.run_batch(c["percs"], c["props"], c["selfish"], duration, n, begin, SEED, threads=16,
                               total_weight=c["W"], ids=c.get("ids"))
        for a in out:
            a.setflags(write=False)
        _BATCH[key] = out
    return _BATCH[key]


# ---------------------------------------------------------------- 1. every instantiation, without records
@pytest.mark.parametrize("name,m", nets.MATRIX, ids=[f"{n}-M{m}" for n, m in nets.MATRIX])
def test_gpu_sums_instantiation_vs_reference(msim, oracle, monkeypatch, name, m):
    """Each (case, M) of tests/instantiation_networks.py in the form the benchmark launches (records == nullptr,
    best_h == nullptr: the kernels branch on those pointers), then with records: the same sums either way."""
    c = nets.case(name, m)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    sim = _sim(msim, c)
    _path(sim, N, c["path"])
    f, s = nets.oracle_counters(oracle, name, m, _begin(m), SEED)
    want = ref.expected(f, s, f.sum(axis=1))
    res = sim.run(N, _begin(m), SEED)
    assert res.found is None
    _exact(ref.combined(res.sums), want, (name, m, "no records"))
    _stats_are_the_sums(res.stats_total, want, (name, m))
    rec = sim.run(N, _begin(m), SEED, 0, per_run=True)
    _exact(ref.combined(rec.sums), want, (name, m, "with records"))
    for k in range(m):
        assert rec.stats_total[k].blocks_found == want[k][0], (name, m, k)


# ---------------------------------------------------------------- 2. sweep sums per M
@pytest.mark.parametrize("forced", [False, True], ids=["e1", "forced_retry"])
@pytest.mark.parametrize("m", range(2, 16))
def test_gpu_sums_sweep_vs_reference(msim, oracle, monkeypatch, m, forced):
    """The two-point sweep of test_gpu_instantiation_sweep_vs_oracle (the one-selfish uniform network and its honest
    twin through the selfish instantiation) without records: E1 + finalize, and E2's atomic retry sums per point."""
    if forced:
        monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
    c = nets.case("selfish_uniform_1s", m)
    twin = dict(c, selfish=[False] * m)
    pts = [[msim.Miner(k, c["percs"][k], c["props"][k], sel and c["selfish"][k]) for k in range(m)]
           for sel in (True, False)]
    sw = msim.Sweep(pts, D)
    for sim in sw.sims:
        assert sim.pipeline_info(N)["uses_pipeline"] in (1, 3)  # alone: E1, or the honest pipeline for the twin
    assert sw.sims[0].pipeline_info(N)["uses_pipeline"] == 3    # so the sweep runs every point on the entity engine
    out = sw.run(N, _begin(m), SEED)
    f, s = nets.oracle_counters(oracle, "selfish_uniform_1s", m, _begin(m), SEED)
    _exact(ref.combined(out[0].sums), ref.expected(f, s, f.sum(axis=1)), ("sweep selfish", m, forced))
    hf, hs, _, _ = _oracle(oracle, ("twin", m), twin, D, N, _begin(m))
    _exact(ref.combined(out[1].sums), ref.expected(hf, hs, hf.sum(axis=1)), ("sweep honest twin", m, forced))
    _stats_are_the_sums(out[0].stats_total, ref.expected(f, s, f.sum(axis=1)), ("sweep selfish", m, forced))


def _fill_ff(shape, dtype):
    import torch

    t = torch.empty(shape, dtype=dtype, device=torch.device("cuda", 0))
    t.view(torch.uint8).fill_(0xFF)
    return t


def _dirty_buffers(obj, n, m, points=None):
    """d_sums, d_status, d_per_run, d_best_height and the workspace of a launch (or a sweep launch of `points`
    points), every byte 0xFF."""
    import torch

    lead = () if points is None else (points,)
    return {"sums": _fill_ff(lead + (m, 6), torch.int64), "status": _fill_ff((2,), torch.int32),
            "rec": _fill_ff(lead + (n, m, 2), torch.int32), "bh": _fill_ff(lead + (n,), torch.int32),
            "ws": _fill_ff((obj.workspace_bytes(n),), torch.uint8)}


def _launch(obj, b, n, begin, records=True):
    """msim_launch / msim_sweep_launch into the buffers b on the default stream; returns copies of the outputs
    (made on the same stream, so a following launch into b does not disturb them)."""
    obj.launch(n, begin, SEED, b["sums"], b["ws"], b["status"], d_per_run=b["rec"] if records else None,
               d_best_height=b["bh"] if records else None)
    return {k: b[k].clone() for k in ("sums", "status", "rec", "bh")}


def _launch_matches(out, f, s, what, p=None):
    """One launch's copied outputs (point p of a sweep) against the oracle's counters: records, best height, sums."""
    pick = (lambda t: t.cpu().numpy()) if p is None else (lambda t: t[p].cpu().numpy())
    rec = pick(out["rec"]).astype(np.int64)
    assert np.array_equal(rec[:, :, 0], f), (what, "found", np.argwhere(rec[:, :, 0] != f)[:5])
    assert np.array_equal(rec[:, :, 1], s), (what, "stale", np.argwhere(rec[:, :, 1] != s)[:5])
    assert np.array_equal(pick(out["bh"]).astype(np.int64), f.sum(axis=1)), (what, "best height")
    _exact(ref.combined(pick(out["sums"])), ref.expected(f, s, f.sum(axis=1)), what)


# Delays of 10 minutes (the mean block interval): runs keep more blocks in flight than the fast sweep kernel holds
# (one per miner + NX_FAST = 4), so its retry pass computes them and adds their terms with atomics.
SWEEP_RETRY_PROP_MS = 600_000


def _honest_sweep(msim, m):
    p = nets.percs(m)
    nw = [_net(p, [q] * m, [False] * m) for q in (SWEEP_RETRY_PROP_MS, 10_000)]
    sw = msim.Sweep([[msim.Miner(k, p[k], c["props"][k]) for k in range(m)] for c in nw], D)
    for sim in sw.sims:  # honest narrow networks with percentages: together they run on the per-lane sweep kernel
        assert sim.pipeline_info(N)["uses_pipeline"] in (0, 1) and not sim.wide
    return sw, nw


@pytest.mark.parametrize("m", range(1, 16))
def test_gpu_sums_honest_sweep_vs_reference(msim, oracle, m):
    """A sweep of honest networks alone runs on msim_sweep_kernel<M>: stats_terms<M>, block_reduce_store<M>, and
    the retry pass's atomic per-point sums (the first point's delays overflow the fast capacities). No records."""
    import torch

    sw, nw = _honest_sweep(msim, m)
    b = _dirty_buffers(sw, N, m, points=2)
    out = _launch(sw, b, N, _begin(m), records=False)
    torch.cuda.synchronize()
    status = out["status"].cpu().tolist()
    assert status[1] == 0 and 0 <= status[0] <= 2 * N, status
    if m >= 2:
        assert status[0] > 0, status  # the retry pass really ran (a lone miner has nothing in flight)
    for p, c in enumerate(nw):
        f, s, _, _ = _oracle(oracle, ("hsweep", m, p), c, D, N, _begin(m))
        _exact(ref.combined(out["sums"][p].cpu().numpy()), ref.expected(f, s, f.sum(axis=1)), ("honest sweep", m, p))


# ---------------------------------------------------------------- 3. run-count edges
# name -> (test switches, the path msim_pipeline_info must report). The path depends on the network and the
# switches only, never on the run count: a single run takes the same kernels as 513.
HONEST_ROUTES = {
    "pipeline": ({}, 1),
    "pipeline_retry": ({"MSIM_PIPE_FORCE_RETRY": "1"}, 1),  # K3 flags every run: the per-lane retry kernel sums them
    "per_lane": ({"MSIM_NO_PIPELINE": "1"}, 0),
    "wide": ({"MSIM_FORCE_WIDE": "1"}, 2),
    "general": ({"MSIM_FORCE_GENERAL": "1"}, 4),
}
SELFISH_ROUTES = {
    "e1": ({}, 3),
    "e2": ({"MSIM_SEL_FORCE_RETRY": "1"}, 3),
    "e2_general": ({"MSIM_SEL_FORCE_RETRY": "1", "MSIM_SEL_FORCE_GEN": "1"}, 3),  # E2 hands every run to G
    "general": ({"MSIM_FORCE_GENERAL": "1"}, 4),
}
ROUTES = [("honest_10s", r) for r in HONEST_ROUTES] + [("selfish_uniform_1s", r) for r in SELFISH_ROUTES]
ROUTE_IDS = [f"{n.split('_')[0]}-{r}" for n, r in ROUTES]
# an empty wave, a single lane, one wave, a ragged second, one workgroup less one lane, full, plus one, two and a lane
EDGE_RUNS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
EDGE_BEGIN = 7000
EDGE_DURATION_MS = 10**9  # ~1 667 blocks a run (stale blocks in every run of both networks): G's lanes stay short


def _route(monkeypatch, name, route):
    env, path = (HONEST_ROUTES if name.startswith("honest") else SELFISH_ROUTES)[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return path


@pytest.mark.parametrize("n", EDGE_RUNS)
@pytest.mark.parametrize("m", [3, 15])
@pytest.mark.parametrize("name,route", ROUTES, ids=ROUTE_IDS)
def test_gpu_sums_run_count_edges(msim, oracle, monkeypatch, name, route, m, n):
    """The first n runs of one 513-run oracle batch per network: records, best height and sums, with and without
    records. Small counts leave a reduction with an empty wave, a single lane, or a retry workgroup with no
    flagged run."""
    path = _route(monkeypatch, name, route)
    c = nets.case(name, m)
    sim = _sim(msim, c, EDGE_DURATION_MS)
    _path(sim, n, path)
    F, S, _, _ = _oracle(oracle, ("edge", name, m), c, EDGE_DURATION_MS, max(EDGE_RUNS), EDGE_BEGIN)
    f, s = F[:n], S[:n]
    L = f.sum(axis=1)
    want = ref.expected(f, s, L)
    # one run: the sums are that run's own terms
    what = (name, route, m, n) + ((("f", f[0].tolist()), ("stale", s[0].tolist()), ("L", int(L[0]))) if n == 1 else ())
    res = sim.run(n, EDGE_BEGIN, SEED, 0, per_run=True)
    assert np.array_equal(res.found.astype(np.int64), f), (what, np.argwhere(res.found != f)[:5])
    assert np.array_equal(res.stale.astype(np.int64), s), (what, np.argwhere(res.stale != s)[:5])
    assert np.array_equal(res.best_height.astype(np.int64), L), what
    _exact(ref.combined(res.sums), want, what + ("with records",))
    bare = sim.run(n, EDGE_BEGIN, SEED)
    _exact(ref.combined(bare.sums), want, what + ("no records",))
    _stats_are_the_sums(bare.stats_total, want, what)


# ---------------------------------------------------------------- 4. wide and general on their own networks
C5_WEIGHTS = [30720, 29696] + [41] * 1024


def _wide_sums(msim, oracle, key, c, duration, n, begin=0):
    sim = _sim(msim, c, duration)
    assert sim.wide
    _path(sim, n, 2)
    f, s, _, _ = _oracle(oracle, key, c, duration, n, begin)
    res = sim.run(n, begin, SEED)
    _exact(ref.combined(res.sums), ref.expected(f, s, f.sum(axis=1)), key)
    return f, s


@pytest.mark.parametrize("days,n", [(3, 525), (20, 64)])
def test_gpu_sums_wide_c5(msim, oracle, days, n):
    """BASELINE configs[4] (1 026 miners, W = 102 400): W3's LDS accumulators and its limb-splitting flush, read
    without records. 525 runs: two full 256-run slices of workgroups and a ragged rest."""
    c = _net(C5_WEIGHTS, [1000] * len(C5_WEIGHTS), [0] * len(C5_WEIGHTS), W=102400)
    f, s = _wide_sums(msim, oracle, ("c5", days, n), c, days * DAY, n)
    assert s.sum() > 0 and (f[:, 2:] == 0).any()  # stale blocks, and small miners without a block in a run


@pytest.mark.parametrize("m", [16, 17, 63, 64, 65, 255, 256, 257])
def test_gpu_sums_wide_miner_count_edges(msim, oracle, m):
    """W != 100 networks whose miner counts straddle the strides of W3's term loop (k += 64) and flush loop
    (k += 256); zero weights among them (miners that never find a block: all-zero rows of the sums)."""
    w = [[3, 0, 1, 2, 0, 5, 1][k % 7] for k in range(m)]
    w[0] += 500
    props = [[0, 1, 50, 700, 3000][k % 5] for k in range(m)]
    c = _net(w, props, [0] * m, W=sum(w))
    f, s = _wide_sums(msim, oracle, ("wide", m), c, 20 * DAY, 64, begin=m)
    assert s.sum() > 0 and (f.sum(axis=0) == 0).any() and (f.sum(axis=0) > 0).sum() > m // 2


def _general_sums(msim, oracle, key, c, duration, n, path=4, from_doubles=False):
    sim = _sim(msim, c, duration)
    _path(sim, n, path)
    f, s, sh, rt = _oracle(oracle, key, c, duration, n, 0)
    res = sim.run(n, 0, SEED)
    fields = range(4)
    if from_doubles:
        if not np.isfinite(sh).all():
            # a miner holding Genesis's id in a run without blocks: found = 1 over a best height of 0, the
            # reference's share is infinite and has no Q32.32 value; found, stale and rate remain
            sh = np.where(np.isfinite(sh), sh, 0.0)
            fields = (0, 1, 3)
        want = ref.expected_from_doubles(f, s, sh, rt)
    else:
        want = ref.expected(f, s, f.sum(axis=1))
    _exact(ref.combined(res.sums), want, key, fields)
    return f, s


def test_gpu_sums_general_100_miners_one_selfish(msim, oracle):
    """G's global atomics (found, stale, both limbs of share and rate), 100 miners, W = 1 000, no records."""
    w = [300] + [7 + (k * 13) % 3 - 1 for k in range(98)]
    w.append(1000 - sum(w))
    c = _net(w, [1000] * 100, [True] + [False] * 99, W=1000)
    f, s = _general_sums(msim, oracle, "g100", c, 7 * DAY, 64)
    assert s.sum() > 0


def test_gpu_sums_general_six_selfish(msim, oracle):
    c = _net([10] * 6 + [20, 20], [1000] * 8, [True] * 6 + [False] * 2)
    f, s = _general_sums(msim, oracle, "g6", c, 30 * DAY, 64)
    assert (s > f).any()  # rates above 1: G's rate_hi add


ID_NETWORKS = {  # the shared-id and Genesis-id networks of tests/test_gpu_general.py: (network, duration, runs)
    "shared_honest": (_net(DEFAULT_PERCS, [1000] * 9, [False] * 9, ids=[0, 1, 2, 0, 4, 5, 1, 7, 0]), 30 * DAY, 64),
    "shared_selfish": (_net([40, 19, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [True] + [False] * 8,
                            ids=[5, 5, 2, 3, 4, 5, 6, 7, 8]), 30 * DAY, 64),
    "shared_all": (_net([34, 33, 33], [0, 0, 0], [False] * 3, ids=[9, 9, 9]), 7 * DAY, 32),
    "genesis_honest": (_net(DEFAULT_PERCS, [100] * 9, [False] * 9, ids=[0xFFFFFFFF, 1, 2, 3, 4, 5, 6, 7, 8]), 30 * DAY, 64),
    "genesis_selfish": (_net([40, 19, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [True] + [False] * 8,
                             ids=[0, 1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF]), 30 * DAY, 64),
    "genesis_no_blocks": (_net([60, 40], [10, 10], [False, False], ids=[0xFFFFFFFF, 0xFFFFFFFF]), 0, 8),
}


@pytest.mark.parametrize("name", list(ID_NETWORKS))
def test_gpu_sums_general_id_networks(msim, oracle, name):
    """Miners sharing an id, or holding Genesis's: sum(found) is not the best height, so the oracle's own share and
    rate doubles are the reference (expected_from_doubles)."""
    c, duration, n = ID_NETWORKS[name]
    _general_sums(msim, oracle, ("ids", name), c, duration, n, from_doubles=True)


def test_gpu_sums_general_as_e2_fallback(msim, oracle, monkeypatch):
    """MSIM_SEL_FORCE_RETRY + MSIM_SEL_FORCE_GEN on configs[2], 30 days: G adds every run into the entity engine's
    retry sums, which its finalize joins with E1's (all-zero) partials."""
    monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
    monkeypatch.setenv("MSIM_SEL_FORCE_GEN", "1")
    c = _net([40, 19, 12, 11, 8, 5, 3, 1, 1], [1000] * 9, [True] + [False] * 8)
    _general_sums(msim, oracle, "c3-30d", c, 30 * DAY, 257, path=3)


# ---------------------------------------------------------------- 5. short durations
SHORT_ROUTES = [("honest", r) for r in HONEST_ROUTES] + [("selfish", r) for r in SELFISH_ROUTES]


@pytest.mark.parametrize("duration", [0, 1, 3_000_000])
@pytest.mark.parametrize("name,route", SHORT_ROUTES, ids=[f"{n}-{r}" for n, r in SHORT_ROUTES])
def test_gpu_sums_short_durations(msim, oracle, monkeypatch, name, route, duration):
    """The 9-miner default percentages (miner 0 selfish on the entity-engine routes), 257 runs: no blocks at all
    (all-zero sums, no 0/0), and 50 minutes, where the 1 % miners find nothing in most runs (found == 0 terms)."""
    path = _route(monkeypatch, name, route)
    c = _net(DEFAULT_PERCS, [1000] * 9, [name == "selfish"] + [False] * 8)
    n = 257
    sim = _sim(msim, c, duration)
    _path(sim, n, path)
    f, s, _, _ = _oracle(oracle, ("short", name, duration), c, duration, n, 0)
    want = ref.expected(f, s, f.sum(axis=1))
    if duration == 0:
        assert want == [(0, 0, 0, 0)] * 9
    if duration == 3_000_000:
        # runs where a 1 % miner finds nothing beside runs where it does, and runs without any block
        assert (f[:, 7:] == 0).any() and (f[:, 7:] > 0).any() and (f.sum(axis=1) == 0).any()
    res = sim.run(n, 0, SEED)
    _exact(ref.combined(res.sums), want, (name, route, duration, "no records"))
    _stats_are_the_sums(res.stats_total, want, (name, route, duration))
    rec = sim.run(n, 0, SEED, 0, per_run=True)
    assert np.array_equal(rec.found.astype(np.int64), f) and np.array_equal(rec.stale.astype(np.int64), s)
    _exact(ref.combined(rec.sums), want, (name, route, duration, "with records"))


# ---------------------------------------------------------------- 6. dirty outputs
DIRTY_RANGES = (1000, 5000)
DIRTY_RUNS = 257
# status[0] under the forced-retry switches: E1 flags every active lane (msim_sel_kernel: o.err = SERR_CAP, one
# atomicAdd on counts[0] per run, which msim_sel_finalize copies), K3 flags every run at its first check
# (msim_combine_kernel: one atomicAdd on err_count per run, which msim_finalize copies): the run count.
FLAGS_EVERY_RUN = ("pipeline_retry", "e2", "e2_general")


@pytest.mark.parametrize("name,route", ROUTES, ids=ROUTE_IDS)
def test_gpu_sums_dirty_outputs(msim, oracle, monkeypatch, name, route):
    """msim.h: "d_sums (overwritten)". Two launches in a row into the same buffers, which begin as 0xFF bytes
    (sums, status, records, best heights and the workspace); the atomic paths rely on a memset inside the launch.
    Each launch's outputs are those of its own run range."""
    import torch

    path = _route(monkeypatch, name, route)
    m, n = 7, DIRTY_RUNS
    c = nets.case(name, m)
    sim = _sim(msim, c)
    _path(sim, n, path)
    b = _dirty_buffers(sim, n, m)
    outs = [_launch(sim, b, n, begin) for begin in DIRTY_RANGES]
    torch.cuda.synchronize()
    for begin, out in zip(DIRTY_RANGES, outs):
        f, s, _, _ = _oracle(oracle, ("dirty", name, begin), c, D, n, begin)
        status = out["status"].cpu().tolist()
        assert status[1] == 0 and 0 <= status[0] <= n, (route, begin, status)
        if route in FLAGS_EVERY_RUN:
            assert status[0] == n, (route, begin, status)
        _launch_matches(out, f, s, (name, route, begin))


@pytest.mark.parametrize("kind", ["selfish", "selfish_forced_retry", "honest"])
def test_gpu_sums_dirty_outputs_sweep(msim, oracle, monkeypatch, kind):
    """msim_sweep_launch twice into the same 0xFF-filled buffers: a two-point sweep on the entity engine (with and
    without its forced retry, where every run of every point is flagged) and one on the per-lane sweep kernel."""
    import torch

    m, n = 7, DIRTY_RUNS
    if kind == "honest":
        sw, nw = _honest_sweep(msim, m)
    else:
        if kind == "selfish_forced_retry":
            monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
        c = nets.case("selfish_uniform_1s", m)
        nw = [c, dict(c, selfish=[False] * m)]
        sw = msim.Sweep([[msim.Miner(k, x["percs"][k], x["props"][k], x["selfish"][k]) for k in range(m)] for x in nw], D)
        assert sw.sims[0].pipeline_info(n)["uses_pipeline"] == 3
    b = _dirty_buffers(sw, n, m, points=2)
    outs = [_launch(sw, b, n, begin) for begin in DIRTY_RANGES]
    torch.cuda.synchronize()
    for begin, out in zip(DIRTY_RANGES, outs):
        status = out["status"].cpu().tolist()
        assert status[1] == 0 and 0 <= status[0] <= 2 * n, (kind, begin, status)
        if kind == "selfish_forced_retry":
            assert status[0] == 2 * n, (kind, begin, status)
        for p, x in enumerate(nw):
            f, s, _, _ = _oracle(oracle, ("dirty sweep", kind == "honest", p, begin), x, D, n, begin)
            _launch_matches(out, f, s, (kind, begin, "point", p), p)


# ---------------------------------------------------------------- 7. multi-GPU entry points at one device
def test_gpu_sums_multi_entry_points_one_device(msim, oracle):
    """msim_run_multi on the device list [0] and distributed.run_sharded in a world of one, on a 13-miner
    one-selfish network at 1 000 runs, against the reference (not against msim_run)."""
    import torch
    from miningsimulation_amd import distributed

    m, n = 13, 1000
    c = nets.case("selfish_uniform_1s", m)
    sim = _sim(msim, c)
    _path(sim, n, 3)
    f, s, _, _ = _oracle(oracle, ("multi", m), c, D, n, 0)
    want = ref.expected(f, s, f.sum(axis=1))
    res = sim.run_multi(n, 0, SEED, devices=[0])
    _exact(ref.combined(res.sums), want, "run_multi")
    _stats_are_the_sums(res.stats_total, want, "run_multi")
    sums = distributed.run_sharded(sim, n, SEED)
    torch.cuda.synchronize()
    _exact(ref.combined(sums.cpu().numpy()), want, "run_sharded")

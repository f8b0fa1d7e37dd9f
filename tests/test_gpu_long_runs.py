"""Runs longer than a year on the device, on every engine, against the recorded oracle counters of tests/long_runs.py
(tests/golden/long_runs.json): found, stale and best height of every run, the Q32.32 sums rebuilt from those counters
(tests/sums_reference.py, integer equality) and status[1] == 0. Every launch goes into outputs and a workspace of 0xFF
bytes.

What the cases cross (tests/long_runs.py): more than 65 535 blocks of one miner in a run and a draw segment of the
planner's longest length (the honest pipeline's u16 owner counts), best heights past the settled form's 16-bit guards
(msim_selm.h), and the same run lengths on the per-lane kernel, the shared-draw sweep, the large-network pipeline and
the general engine. The pipeline cases run planned for ONE wave slot (MSIM_K1_SLOTS=1 and two launches in flight: the
fewest, longest segments the planner lays out); before the planner bounded a segment to 65 504 blocks they were one
segment of up to 240 640 blocks, the u16 pair carried into its neighbour, and the run was not flagged.

The general engine walks a withheld chain at every event (as the reference does), so its selfish-majority case runs
30 days, not the 3.5 years of `selfish_majority`: the cost is quadratic in the withheld chain, which grows all run."""
import numpy as np
import pytest

import host_plans
import long_runs
import moments_reference
import pipeline_host_lib
import rank_reference
import sums_reference
from long_runs import CASES, Y

pytestmark = pytest.mark.gpu

U16 = 65_535
DAY = 86_400_000
EXTRA_SWITCHES = ("MSIM_SEL_FORCE_RETRY", "MSIM_SEL_FORCE_GEN", "MSIM_SEL_NO_MACRO", "MSIM_SEL_XTH", "MSIM_PIPE_FORCE_RETRY",
                  "MSIM_MOMENTS_CHUNK_RUNS")


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


@pytest.fixture(scope="module")
def host(native_tests):
    return pipeline_host_lib.load(native_tests["pipeline_host"])


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in host_plans.SWITCHES + EXTRA_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _launch(obj, n, points=0):
    """One launch of a Simulation (points = 0) or a Sweep into outputs and a workspace of 0xFF bytes: sums [.., M, 6]
    int64, records and best heights as int64 of their uint32 values, status."""
    import torch

    m = obj.m if points else len(obj.miners)
    lead = (points,) if points else ()
    ws = torch.full((obj.workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")
    sums = torch.full(lead + (m, 6), -1, dtype=torch.int64, device="cuda")
    rec = torch.full(lead + (n, m, 2), -1, dtype=torch.int32, device="cuda")
    bh = torch.full(lead + (n,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    obj.launch(n, 0, long_runs.BASE, sums, ws, st, rec, bh)
    torch.cuda.synchronize()
    sums, rec, bh, st = [t.cpu().numpy() for t in (sums, rec, bh, st)]
    return sums, rec.view(np.uint32).astype(np.int64), bh.view(np.uint32).astype(np.int64), st.view(np.uint32).astype(np.int64)


def _exact(out, want, what):
    """One network's launch against (found, stale, best height): every run, the sums, and no failed run."""
    sums, rec, bh, st = out
    f, s, L = want
    bad = np.argwhere(rec[:, :, 0] != f)
    assert bad.size == 0, (what, "found", bad[:4].tolist(), rec[bad[0][0], :, 0][:8].tolist(), f[bad[0][0]][:8].tolist())
    bad = np.argwhere(rec[:, :, 1] != s)
    assert bad.size == 0, (what, "stale", bad[:4].tolist())
    assert np.array_equal(bh, L), (what, "best height")
    assert st[1] == 0, (what, st.tolist())
    diff = sums_reference.diff(sums_reference.combined(sums), sums_reference.expected(f, s, L))
    assert not diff, (what, diff[:6])


def _sim(msim, name, delay=None, duration=None):
    c = CASES[name]
    return msim.Simulation(long_runs.miners(msim, c, delay), duration or c["duration"], c["W"])


# ------------------------------------------------------------------ the honest pipeline
@pytest.mark.parametrize("name", long_runs.HONEST)
def test_pipeline_planned_for_one_wave_slot(msim, host, monkeypatch, name):
    """The fewest, longest segments: status[0] is the host bodies' flagged count at the device's geometry, 0 for these
    networks, so a wrong K1 count cannot hide behind the retry kernel."""
    c = CASES[name]
    monkeypatch.setenv("MSIM_K1_SLOTS", "1")
    sim = _sim(msim, name)
    sim.set_concurrent_launches(2)
    info = sim.pipeline_info(c["runs"])
    print(f"{name}: {info}")
    assert info["uses_pipeline"] == 1, info
    _, _, ok, _ = host(c["weights"], c["delays"], c["duration"], c["runs"], c["base"], nseg=info["segments"],
                       seg=info["segment_blocks"])
    out = _launch(sim, c["runs"])
    print(f"{name}: status {out[3].tolist()}, host flags {int((~ok).sum())}, run 0 found {out[1][0, :, 0].tolist()} "
          f"expected {long_runs.expected(name)[0][0].tolist()}")
    assert info["segment_blocks"] <= U16, info
    _exact(out, long_runs.expected(name), name)
    assert out[3][0] == int((~ok).sum()) == 0, out[3]


def test_pipeline_launches_in_flight(msim):
    """honest_70_30 at the device's own wave slots planned for one, two and four launches in flight: three
    geometries, the same records byte for byte."""
    c = CASES["honest_70_30"]
    outs = []
    for jobs in (1, 2, 4):
        sim = _sim(msim, "honest_70_30")
        sim.set_concurrent_launches(jobs)
        info = sim.pipeline_info(c["runs"])
        print(f"{jobs} in flight: {info}")
        assert info["uses_pipeline"] == 1 and info["segment_blocks"] <= U16, info
        out = _launch(sim, c["runs"])
        _exact(out, long_runs.expected("honest_70_30"), jobs)
        outs.append(out)
    for out in outs[1:]:
        assert out[1].tobytes() == outs[0][1].tobytes() and out[2].tobytes() == outs[0][2].tobytes()


def test_per_lane_kernel(msim, monkeypatch):
    monkeypatch.setenv("MSIM_NO_PIPELINE", "1")  # read when the config is created
    sim = _sim(msim, "honest_70_30")
    assert sim.pipeline_info(64)["uses_pipeline"] == 0
    _exact(_launch(sim, 64), long_runs.expected("honest_70_30", 64), "per-lane")


def test_shared_draw_sweep(msim, monkeypatch):
    """propagation_sweep([70, 30], (10 s, 100 ms)) at 2 years: each point against the same network run alone."""
    monkeypatch.setenv("MSIM_K1_SLOTS", "1")
    c = CASES["honest_70_30"]
    sw = msim.propagation_sweep(long_runs.miners(msim, c), (10_000, 100), c["duration"])
    plan = sw.plan(64)
    assert plan["engine"] == 1 and plan["draw_groups"] == 1 and plan["largest_group"] == 2, plan
    sums, rec, bh, st = _launch(sw, 64, points=2)
    for p, name in enumerate(("honest_70_30_10s", "honest_70_30")):
        _exact((sums[p], rec[p], bh[p], st), long_runs.expected(name, 64), name)


# ------------------------------------------------------------------ E1 and E2
@pytest.mark.parametrize("name", long_runs.SELFISH)
def test_entity_engine(msim, monkeypatch, name):
    """E1 (settled form, in-lane draws, engine phases) past the 16-bit guards, then every run on E2: the same records.
    The host build's mixed run reported no error for any of these runs (tests/test_long_runs_host.py), so E1 retries
    nothing."""
    c = CASES[name]
    want = long_runs.expected(name)
    sim = _sim(msim, name)
    assert sim.pipeline_info(c["runs"])["uses_pipeline"] == 3
    plain = _launch(sim, c["runs"])
    _exact(plain, want, name)
    assert plain[3].tolist() == [0, 0], plain[3]
    monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")  # read at every launch
    e2 = _launch(sim, c["runs"])
    _exact(e2, want, name + " on E2")
    assert e2[3].tolist() == [c["runs"], 0], e2[3]
    assert e2[1].tobytes() == plain[1].tobytes() and e2[2].tobytes() == plain[2].tobytes()
    monkeypatch.delenv("MSIM_SEL_FORCE_RETRY")
    if name == "selfish_flush":
        monkeypatch.setenv("MSIM_SEL_NO_MACRO", "1")  # read when the config is created: the engine for every find
        alone = _launch(_sim(msim, name), 16)
        _exact(alone, long_runs.expected(name, 16), name + " without the settled form")
        assert alone[1].tobytes() == plain[1][:16].tobytes()


# ------------------------------------------------------------------ the large-network pipeline
def test_wide_pools_at_10s_goes_to_the_general_engine(msim):
    """The candidates of a 4-year run at 10 s outgrow W3's LDS: the library serves the case on the general engine (one
    lane walks 34 chains at every event for 210 000 blocks: minutes, so it is not launched here). The same network runs
    on W1-W3 at 5 s below, and at 10 s through their host bodies (tests/test_long_runs_host.py)."""
    assert _sim(msim, "wide_pools").pipeline_info(32)["uses_pipeline"] == 4


@pytest.mark.parametrize("name", long_runs.WIDE_ON_DEVICE + ("honest_70_30",))
def test_wide_pipeline(msim, monkeypatch, name):
    """W1-W3; wide_pools_5s and honest_70_30 (MSIM_FORCE_WIDE) give one miner more than 65 535 blocks."""
    c = CASES[name]
    if name == "honest_70_30":
        monkeypatch.setenv("MSIM_FORCE_WIDE", "1")  # read when the config is created
    sim = _sim(msim, name)
    assert sim.pipeline_info(c["runs"])["uses_pipeline"] == 2 and sim.wide
    _exact(_launch(sim, c["runs"]), long_runs.expected(name), name)


# ------------------------------------------------------------------ the general engine
def _oracle(oracle, c, n):
    return long_runs.oracle_counters(oracle, c, runs=n)


def test_general_engine_three_years(msim, oracle, monkeypatch):
    """[70, 30] at 100 ms on G for 3 years (G accepts any duration whose last window it can hold: the longest of the
    three asked for), 16 runs, against the oracle."""
    monkeypatch.setenv("MSIM_FORCE_GENERAL", "1")  # read when the config is created
    c = dict(CASES["honest_70_30"], duration=3 * Y)
    sim = msim.Simulation(long_runs.miners(msim, c), c["duration"])
    assert sim.pipeline_info(16)["uses_pipeline"] == 4
    _exact(_launch(sim, 16), _oracle(oracle, c, 16), "G, 3 years")


def test_general_engine_refuses_what_it_cannot_hold(msim, monkeypatch):
    """A selfish network's last window holds every block of a run: past 96 GiB of chains for one lane
    msim_config_create returns MSIM_E_MINERS and there is nothing to launch."""
    from miningsimulation_amd import _lib

    monkeypatch.setenv("MSIM_FORCE_GENERAL", "1")
    with pytest.raises(msim.MsimError) as e:
        msim.Simulation(long_runs.miners(msim, CASES["selfish_majority"]), 2 * 10**15)
    assert e.value.code == _lib.MSIM_E_MINERS


def test_general_engine_behind_e2(msim, oracle, monkeypatch):
    """selfish_majority's network, every run handed from E2 to G, 8 runs of 30 days: a run is exact, or it is counted
    in status[1] and its record is untouched."""
    monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")
    monkeypatch.setenv("MSIM_SEL_FORCE_GEN", "1")
    c = dict(CASES["selfish_majority"], duration=30 * DAY)
    sim = msim.Simulation(long_runs.miners(msim, c), c["duration"])
    assert sim.pipeline_info(8)["uses_pipeline"] == 3
    f, s, L = _oracle(oracle, c, 8)
    sums, rec, bh, st = _launch(sim, 8)
    untouched = (rec == 0xFFFFFFFF).all(axis=(1, 2))
    assert int(untouched.sum()) == st[1], (st, untouched)
    done = ~untouched
    assert np.array_equal(rec[done, :, 0], f[done]) and np.array_equal(rec[done, :, 1], s[done])
    assert np.array_equal(bh[done], L[done])
    if st[1] == 0:
        _exact((sums, rec, bh, st), (f, s, L), "G behind E2")


# ------------------------------------------------------------------ error bars
def test_error_bars_on_a_long_run(msim):
    """found above 2^16 in the second moments and in the radix keys: run_moments and run_quantiles on honest_70_30."""
    c = CASES["honest_70_30"]
    f, s, L = long_runs.expected("honest_70_30")
    assert f.max() > 1 << 16
    sim = _sim(msim, "honest_70_30")
    res = sim.run_moments(c["runs"], 0, c["base"], 0)
    bad = moments_reference.diff(res.moments, moments_reference.expected(f, s, L))
    assert not bad, bad[:8]
    q = sim.run_quantiles(c["runs"], ranks=rank_reference.rank_lists(c["runs"])[32], run_begin=0, seed_base=c["base"])
    got = [[[list(o) for o in row] for row in col] for col in q.order[0]]
    bad = rank_reference.diff(got, rank_reference.select(f, s, L, q.ranks))
    assert not bad, bad[:8]

"""The entity engine's capacity flags and its E1 -> E2 -> G hand-over on the device (msim_sel.h, msim_sel_kernels.hip,
msim_sel_launch.h), reached by natural networks at the shipped capacities: no switch forces a flag. The cases and the
host prediction are tests/sel_flag_cases.py (tests/test_sel_host.py checks that prediction against the oracle and each
case's preconditions on the CPU; every test here asserts them again before it touches the device).

Every case asserts: the launch is the entity engine's (uses_pipeline 3); found, stale and best height of every run equal
the oracle's; stats_total is the oracle's run-order sums; a second launch into a workspace and outputs of 0xFF bytes
writes every record, and its Q32.32 sums are byte for byte the first launch's; nothing fails; status[0] and counts[0]
are the number of runs the host build flags at E1's class, counts[GEN_C_L1] the number it also flags at E2's class, and
G's second list holds the runs that outgrow its first window on the host build of G (launches this short have no third
tier). The three count equalities hold because a capacity flag (SERR_ACT, SERR_GRP, SERR_QUE) is a function of the run's
own sequence of finds and arrivals: neither the wave's schedule nor its early folds touch a slot count."""
import ctypes

import numpy as np
import pytest

import moments_reference as mref
import rank_reference as rr
import sel_flag_cases as fc

pytestmark = pytest.mark.gpu

C_FLAG, C_FAIL, C_L1, C_L2, C_L3 = range(5)  # msim_general_launch.h GEN_C_*: the head of the workspace
FF = 0xFFFFFFFF
SWITCHES = ("MSIM_FORCE_GENERAL", "MSIM_SEL_FORCE_RETRY", "MSIM_SEL_FORCE_GEN", "MSIM_MAX_SLICE_RUNS", "MSIM_SEL_NO_MACRO",
            "MSIM_SEL_XTH", "MSIM_SELSEG", "MSIM_GEN_TEST_LANES", "MSIM_GEN_TEST_CAP1", "MSIM_GEN_TEST_CAP2",
            "MSIM_GEN_TEST_CAP3", "MSIM_GEN_TEST_LIST_CAP")


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


@pytest.fixture(scope="module")
def flag_run(native_tests):
    return fc.load(native_tests["sel_host"])


@pytest.fixture(scope="module")
def gen(native_tests):
    """fails(case, r, window): run r of the case outgrows a window of G on the host build (GERR_CAP)."""
    lib = ctypes.CDLL(native_tests["general_host"])
    lib.gen_run.restype = ctypes.c_uint32
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.gen_run.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8),
                            u32p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32,
                            ctypes.c_uint32, u32p, u32p, u32p, u32p]

    def fails(case, r, window):
        m = len(case.weights)
        f, s = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        bh, base = ctypes.c_uint32(), ctypes.c_uint32()
        err = lib.gen_run((ctypes.c_uint64 * m)(*case.weights), (ctypes.c_int64 * m)(*case.props),
                          (ctypes.c_uint8 * m)(*[1 if x else 0 for x in case.selfish]), None, m, case.W, case.duration,
                          fc.BASE + 2 * r, fc.BASE + 2 * r + 1, window, f, s, ctypes.byref(bh), ctypes.byref(base))
        assert err in (0, 1), (case.name, r, window, err)
        return err == 1

    return fails


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _miners(msim, case):
    return [msim.Miner(k, case.weights[k], case.props[k], case.selfish[k]) for k in range(len(case.weights))]


def _sim(msim, case, n):
    sim = msim.Simulation(_miners(msim, case), case.duration, total_weight=case.W)
    assert sim.pipeline_info(n)["uses_pipeline"] == 3, sim.pipeline_info(n)
    return sim


def _launch(obj, n, points):
    """One launch of a Simulation (points = 0) or a Sweep into a workspace and output buffers of 0xFF bytes: sums,
    records, best heights, status, and the five counter words at the head of the workspace."""
    import torch

    m = obj.m if points else len(obj.miners)
    lead = (points,) if points else ()
    ws = torch.full((obj.workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")
    sums = torch.full(lead + (m, 6), -1, dtype=torch.int64, device="cuda")
    rec = torch.full(lead + (n, m, 2), -1, dtype=torch.int32, device="cuda")
    bh = torch.full(lead + (n,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    obj.launch(n, 0, fc.BASE, sums, ws, st, rec, bh)
    torch.cuda.synchronize()
    counts = ws[:20].cpu().numpy().view(np.uint32).astype(np.int64)
    sums, rec, bh, st = [t.cpu().numpy() for t in (sums, rec, bh, st)]
    return sums, rec.view(np.uint32).astype(np.int64), bh.view(np.uint32).astype(np.int64), st.view(np.uint32).astype(np.int64), counts


def _sums_bytes(res):
    return np.array([[getattr(x, f) for f, _ in x._fields_] for x in res.sums], dtype=np.int64).tobytes()


def _records_equal(found, stale, best, oracle_out, what):
    f, s, _, _ = oracle_out
    bad = np.flatnonzero((found != f).any(axis=1) | (stale != s).any(axis=1) | (best != f.sum(axis=1)))
    assert bad.size == 0, (what, "runs that differ from the oracle", bad[:8].tolist(), int(bad.size))


def _g_lists(gen, case, p):
    """(runs in G's second list, runs that fail): G's windows behind the entity engine are 256 and 4 096 blocks for
    runs this short (msim_general_launch.h gen_tiers: the last window is no larger than the second)."""
    to_g = np.flatnonzero(p.e2 != 0)
    l2 = [r for r in to_g if gen(case, int(r), 256)]
    return len(l2), sum(gen(case, int(r), 4096) for r in l2)


def _counters(out, p, gen, case, what):
    _, _, _, st, counts = out
    e1, e2 = int((p.e1 != 0).sum()), int((p.e2 != 0).sum())
    print(f"{what}: host E1 {e1} E2 {e2}; device status {st.tolist()} counters {counts.tolist()}")
    assert st[1] == 0 and counts[C_FAIL] == 0, (what, st, counts)
    assert st[0] == counts[C_FLAG] == e1, (what, st, counts, e1)
    assert counts[C_L1] == e2, (what, counts, e2)
    l2, failed = _g_lists(gen, case, p)
    assert failed == 0
    assert counts[C_L2] == l2 and counts[C_L3] == 0, (what, counts, l2)


def _check_case(msim, oracle, flag_run, gen, case, n=fc.RUNS, no_macro=False, preconditions=True):
    """Everything the module's head lists, for n runs of one network; returns (sim, first result, second launch)."""
    p = fc.predict(flag_run, case, n, no_macro)
    if preconditions:
        fc.check_preconditions(case, p)
    want = fc.oracle_runs(oracle, case, n)
    f, s, sh, rt = want
    sim = _sim(msim, case, n)
    res = sim.run(n, 0, fc.BASE, 0, per_run=True)
    what = (case.name, n, no_macro)
    _records_equal(res.found.astype(np.int64), res.stale.astype(np.int64), res.best_height.astype(np.int64), want, what)
    for k in range(len(case.weights)):  # MinerStats summed in run order (main.cpp:211-217)
        assert res.stats_total[k].blocks_found == int(f[:, k].sum())
        assert res.stats_total[k].blocks_share == sum(sh[:, k].tolist())
        assert res.stats_total[k].stale_rate == sum(rt[:, k].tolist())
    out = _launch(sim, n, 0)
    _records_equal(out[1][:, :, 0], out[1][:, :, 1], out[2], want, what + ("0xFF buffers",))
    assert out[0].tobytes() == _sums_bytes(res), (what, "Q32.32 sums of the two launches differ")
    _counters(out, p, gen, case, what)
    return sim, res, out


# (a) mixed waves, nothing to G; (b) all three stages; (c) heterogeneous delays; (d) several selfish miners
@pytest.mark.parametrize("name", [n for n, c in fc.CASES.items() if "quiet" not in c.want])
def test_flag_case(msim, oracle, flag_run, gen, name):
    _check_case(msim, oracle, flag_run, gen, fc.CASES[name])


def test_quiet_network_flags_nothing(msim, oracle, flag_run, gen):
    """C3 at 1 s (the sweep's first point): every counter word stays 0."""
    _, _, out = _check_case(msim, oracle, flag_run, gen, fc.CASES["c3_1"])
    assert out[3].tolist() == [0, 0] and out[4].tolist() == [0] * 5


# (e) the engine for every find: E1 <1, 4, 1> engine alone, E2 engine alone
@pytest.mark.parametrize("name", ["c3_900", "c3_1800"])
def test_engine_for_every_find(msim, oracle, flag_run, gen, monkeypatch, name):
    monkeypatch.setenv("MSIM_SEL_NO_MACRO", "1")  # read when the config is created
    _check_case(msim, oracle, flag_run, gen, fc.CASES[name], no_macro=True)


# (f) run-count edges: the last ragged wave and workgroup of E1; at 513 runs more than one workgroup of E2
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 513])
def test_run_count_edges(msim, oracle, flag_run, gen, n):
    case = fc.CASES["c3_2400"]
    p = fc.predict(flag_run, case, n)
    if n == 513:
        assert (p.e1 != 0).sum() > 256 and (p.e2 != 0).any() and (p.e1 == 0).any()
    _check_case(msim, oracle, flag_run, gen, case, n=n, preconditions=False)


# (g) slices: later slices reuse the cold slots the earlier ones dirtied; the lists hold launch-relative codes
def test_slices(msim, oracle, flag_run, gen, monkeypatch):
    case, n = fc.CASES["f15_900"], 600
    p = fc.predict(flag_run, case, n)
    for lo in (0, 256, 512):  # every slice flags runs, finishes runs and sends runs to G or at least to E2
        assert (p.e1[lo:lo + 256] != 0).any() and (p.e1[lo:lo + 256] == 0).any(), lo
    assert (p.e2[256:] != 0).any()
    sim = _sim(msim, case, n)
    whole = _launch(sim, n, 0)
    assert sim.pipeline_info(n)["slice_runs"] >= n
    monkeypatch.setenv("MSIM_MAX_SLICE_RUNS", "256")  # read at every sizing and launch
    assert sim.pipeline_info(n)["slice_runs"] == 256
    _, _, sliced = _check_case(msim, oracle, flag_run, gen, case, n=n, preconditions=False)
    assert sliced[0].tobytes() == whole[0].tobytes(), "Q32.32 sums differ from the single-slice launch"
    assert sliced[3].tolist() == whole[3].tolist() and sliced[4].tolist() == whole[4].tolist()


# (h) a sweep whose groups have different selfish classes: E2 runs every point at the largest class
def test_sweep_of_three_classes(msim, oracle, flag_run, gen):
    names, n = ("c3_1", "c3_1800", "c3_three"), 100
    cases = [fc.CASES[x] for x in names]
    preds = [fc.predict(flag_run, c, n, e2=fc.E2_ENGINE_NS4) for c in cases]
    e1 = [int((p.e1 != 0).sum()) for p in preds]
    e2 = [int((p.e2 != 0).sum()) for p in preds]
    assert e1[0] == 0 and 0 < e1[1] < n and 0 < e1[2] < n and e2[2] > 0, (e1, e2)
    sw = msim.Sweep([_miners(msim, c) for c in cases], cases[0].duration)
    assert sw.plan(n)["engine"] == 3, sw.plan(n)
    res = sw.run(n, 0, fc.BASE, 0, per_run=True)
    sums, rec, bh, st, counts = _launch(sw, n, 3)
    print(f"sweep: host E1 {e1} E2 {e2}; device status {st.tolist()} counters {counts.tolist()}")
    for i, c in enumerate(cases):
        want = fc.oracle_runs(oracle, c, n)
        _records_equal(res[i].found.astype(np.int64), res[i].stale.astype(np.int64), res[i].best_height.astype(np.int64),
                       want, (c.name, "sweep"))
        _records_equal(rec[i, :, :, 0], rec[i, :, :, 1], bh[i], want, (c.name, "sweep, 0xFF buffers"))
        assert sums[i].tobytes() == _sums_bytes(res[i]), c.name
        own = _launch(_sim(msim, c, n), n, 0)
        assert own[0].tobytes() == sums[i].tobytes(), (c.name, "sums differ from the network's own launch")
        assert np.array_equal(own[1], rec[i]) and np.array_equal(own[2], bh[i]), c.name
    assert st[1] == 0 and counts[C_FAIL] == 0, (st, counts)
    assert st[0] == counts[C_FLAG] == sum(e1), (st, counts, e1)
    assert counts[C_L1] == sum(e2), (counts, e2)
    assert counts[C_L1] >= counts[C_L2] >= counts[C_L3], counts


# (i) moments and order statistics over records that E1, E2 and G wrote in one launch
def test_moments_and_quantiles(msim, oracle, flag_run):
    case, n = fc.CASES["c3_2400"], fc.RUNS
    p = fc.predict(flag_run, case, n)
    fc.check_preconditions(case, p)
    f, s, _, _ = fc.oracle_runs(oracle, case, n)
    L = f.sum(axis=1)
    sim = _sim(msim, case, n)
    res = sim.run_moments(n, 0, fc.BASE, 0)
    bad = mref.diff(res.moments, mref.expected(f, s, L))
    assert not bad, bad[:8]
    q = sim.run_quantiles(n, ranks=[0, n // 2, n - 1], seed_base=fc.BASE)
    got = [[[list(o) for o in row] for row in col] for col in q.order[0]]
    bad = rr.diff(got, rr.select(f, s, L, q.ranks))
    assert not bad, bad[:8]


# (j) the opt-in segment form does not serve these networks (runs far below its 4 096 blocks): E1 does
def test_segment_form_leaves_these_to_e1(msim, oracle, flag_run, gen, monkeypatch):
    monkeypatch.setenv("MSIM_SELSEG", "1")  # read when the config is created
    _check_case(msim, oracle, flag_run, gen, fc.CASES["slow_selfish"])

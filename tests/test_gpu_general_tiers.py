"""The general engine's tiers, lane reuse and run lists on the device (msim_general.hip, msim_general_launch.h),
reached with a few hundred 3-day runs by lowering G's lanes, windows and told list length through the test switches
MSIM_GEN_TEST_* (include/msim.h). tests/native/gen_tiers_check.cpp is the same walk on the CPU under ASan + UBSan.

Every case asserts: found, stale and best height of every finished run equal the oracle's; where no run fails, the
Q32.32 sums are byte for byte those of the same launch with no switch set; status[1] and the tier counters equal what
the host build of the engine (build/libgeneral_host.so, gen_run at a given window) predicts: whether a run outgrows a
window depends on its seeds and the window alone, so counts[GEN_C_L2] is the number of runs that fail at the first
window and counts[GEN_C_L3] the number that fail at the first two. Every lowered launch runs into a workspace and
output buffers of 0xFF bytes, and exactly the failed runs' records stay 0xFF. Each test recomputes its prediction and
asserts its precondition on it before it touches the device.

Runs of 259 200 000 ms (about 432 blocks) at seed base 1000; run r has seeds (1000 + 2r, 1001 + 2r)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D3 = 259_200_000
BASE = 1000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]
# name -> (weights, uniform delay, miner 0 selfish)
NETS = {"A": ([45, 30, 25], 1000, True), "B": ([60, 25, 15], 100, True), "C": (H, 3_600_000, False),
        "D": (H, 10_000, False), "N9": ([40, 19, 12, 11, 8, 5, 3, 1, 1], 1000, True), "ONE": ([100], 0, False)}
SWITCHES = ("MSIM_GEN_TEST_LANES", "MSIM_GEN_TEST_CAP1", "MSIM_GEN_TEST_CAP2", "MSIM_GEN_TEST_CAP3",
            "MSIM_GEN_TEST_LIST_CAP")
C_FLAG, C_FAIL, C_L1, C_L2, C_L3 = range(5)  # msim_general_launch.h GEN_C_*: the head of every G workspace
LOW = (16, 64, 1024)
FF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


@pytest.fixture(scope="module")
def gen(native_tests):
    lib = ctypes.CDLL(native_tests["general_host"])
    lib.gen_run.restype = ctypes.c_uint32
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.gen_run.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8),
                            u32p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32,
                            ctypes.c_uint32, u32p, u32p, u32p, u32p]

    def run(name, r, cap):
        """(error bits, best height) of run r of a network at one window"""
        w, delay, selfish = NETS[name]
        m = len(w)
        f, s = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        bh, base = ctypes.c_uint32(), ctypes.c_uint32()
        err = lib.gen_run((ctypes.c_uint64 * m)(*w), (ctypes.c_int64 * m)(*[delay] * m),
                          (ctypes.c_uint8 * m)(*[1 if selfish and k == 0 else 0 for k in range(m)]), None, m, sum(w), D3,
                          BASE + 2 * r, BASE + 2 * r + 1, cap, f, s, ctypes.byref(bh), ctypes.byref(base))
        return err, bh.value

    return run


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in SWITCHES + ("MSIM_FORCE_GENERAL", "MSIM_SEL_FORCE_RETRY", "MSIM_SEL_FORCE_GEN", "MSIM_MAX_SLICE_RUNS"):
        monkeypatch.delenv(k, raising=False)


_PRED, _REF, _BASE = {}, {}, {}


def _predict(gen, name, n, caps):
    """tier[r]: the tier (0-based) whose window finishes run r, or -1 when every window is too small (host build)."""
    k = (name, n, tuple(caps))
    if k not in _PRED:
        tier = np.full(n, -1, dtype=np.int64)
        for r in range(n):
            for i, c in enumerate(caps):
                err, _ = gen(name, r, c)
                assert err in (0, 1), (name, r, c, err)  # finished, or GERR_CAP
                if err == 0:
                    tier[r] = i
                    break
        tier.setflags(write=False)
        _PRED[k] = tier
    return _PRED[k]


def _oracle(oracle, name, n):
    k = (name, n)
    if k not in _REF:
        w, delay, selfish = NETS[name]
        f, s, _, _ = oracle.run_batch(list(w), [delay] * len(w), [selfish and i == 0 for i in range(len(w))], D3, n, 0, BASE,
                                      threads=16)
        f.setflags(write=False)
        s.setflags(write=False)
        _REF[k] = (f, s)
    return _REF[k]


def _miners(msim, name):
    w, delay, selfish = NETS[name]
    return [msim.Miner(k, w[k], delay, selfish and k == 0) for k in range(len(w))]


def _sim(msim, monkeypatch, name, path):
    """The network on G alone (path 4) or on the entity engine whose every run E2 hands to G (path 3)."""
    if path == 4:
        monkeypatch.setenv("MSIM_FORCE_GENERAL", "1")  # read when the config is created
    else:
        monkeypatch.setenv("MSIM_SEL_FORCE_RETRY", "1")  # read at every launch
        monkeypatch.setenv("MSIM_SEL_FORCE_GEN", "1")
    sim = msim.Simulation(_miners(msim, name), D3)
    assert sim.pipeline_info(64)["uses_pipeline"] == path
    return sim


def _launch(obj, n, points, fill):
    """One launch of a Simulation (points = 0) or a Sweep into a workspace and output buffers of `fill` bytes:
    sums, records, best heights, status, and the five counter words at the head of the workspace."""
    import torch

    m = obj.m if points else len(obj.miners)
    lead = (points,) if points else ()
    ws = torch.full((obj.workspace_bytes(n),), fill, dtype=torch.uint8, device="cuda")
    v = -1 if fill else 0
    sums = torch.full(lead + (m, 6), v, dtype=torch.int64, device="cuda")
    rec = torch.full(lead + (n, m, 2), v, dtype=torch.int32, device="cuda")
    bh = torch.full(lead + (n,), v, dtype=torch.int32, device="cuda")
    st = torch.full((2,), v, dtype=torch.int32, device="cuda")
    obj.launch(n, 0, BASE, sums, ws, st, rec, bh)
    torch.cuda.synchronize()
    counts = ws[:20].cpu().numpy().view(np.uint32).astype(np.int64)
    sums, rec, bh, st = [t.cpu().numpy() for t in (sums, rec, bh, st)]
    return sums, rec.view(np.uint32).astype(np.int64), bh.view(np.uint32).astype(np.int64), st.view(np.uint32).astype(np.int64), counts


def _natural(sim, key, n):
    """The same launch with no switch set (into zeroes): its sums, and that it fails nothing."""
    if key not in _BASE:
        out = _launch(sim, n, 0, 0)
        assert out[3][1] == 0, out[3]
        _BASE[key] = out
    return _BASE[key]


def _set(monkeypatch, lanes=None, caps=None, list_cap=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if lanes:
        monkeypatch.setenv("MSIM_GEN_TEST_LANES", str(lanes))
    for i, c in enumerate(caps or ()):
        monkeypatch.setenv(f"MSIM_GEN_TEST_CAP{i + 1}", str(c))
    if list_cap:
        monkeypatch.setenv("MSIM_GEN_TEST_LIST_CAP", str(list_cap))


def _geometry(sim, n, nat, lanes=None, caps=None, tiers=None):
    """The switches took effect, and only lowered (msim_pipeline_info: tier-1 lanes, tier-1 window, tiers, last window)."""
    info = sim.pipeline_info(n)
    assert info["slice_runs"] == (min(lanes, nat["slice_runs"]) if lanes else nat["slice_runs"]), info
    if caps:
        assert info["segment_blocks"] == caps[0] <= nat["segment_blocks"], info
        assert info["segments"] == (tiers or len(caps)), info
        assert info["blocks_per_run"] == caps[info["segments"] - 1] <= nat["blocks_per_run"], info
    else:
        assert (info["segment_blocks"], info["segments"], info["blocks_per_run"]) == \
            (nat["segment_blocks"], nat["segments"], nat["blocks_per_run"]), info
    assert sim.workspace_bytes(n) <= nat["workspace_bytes"]
    return info


def _exact(oracle, name, n, out, finished):
    """Records and heights: the oracle's for every finished run, 0xFF for every other; the set is the predicted one."""
    f, s = _oracle(oracle, name, n)
    _, rec, bh, _, _ = out
    touched = bh != FF
    assert np.array_equal(touched, finished), (np.flatnonzero(touched != finished)[:8], int(touched.sum()), int(finished.sum()))
    assert np.array_equal(rec[touched, :, 0], f[touched]), np.argwhere(rec[touched, :, 0] != f[touched])[:5]
    assert np.array_equal(rec[touched, :, 1], s[touched]), np.argwhere(rec[touched, :, 1] != s[touched])[:5]
    assert np.array_equal(bh[touched], f[touched].sum(axis=1))
    assert (rec[~touched] == FF).all()


def _counters(out, tier, path, n, tiers):
    """status and the counter words against the prediction (a launch of two tiers has no third list)."""
    _, _, _, st, counts = out
    l2, l3, failed = int((tier != 0).sum()), int(((tier != 0) & (tier != 1)).sum()), int((tier < 0).sum())
    assert counts[C_L2] == l2 and counts[C_FAIL] == failed, (counts, l2, l3, failed)
    assert counts[C_L3] == (l3 if tiers == 3 else 0), (counts, l2, l3, failed)
    assert st[1] == failed, st
    if path == 4:
        assert st[0] == counts[C_L2] + counts[C_L3], (st, counts)
    else:
        assert counts[C_L1] == n and st[0] == counts[C_FLAG], (st, counts)  # E2 handed over every run
    return l2, l3, failed


def _reuse_preconditions(gen, name, n, lanes, tier):
    """In tier 1 lane l serves runs l, l + lanes, ...: some lane takes a run that ends in tier 1 right after one that
    escalated (when any run escalates at these windows), and some lane a shorter chain right after a longer one."""
    after_escalated = shorter_after_longer = False
    h = [gen(name, r, 4096)[1] for r in range(n)]
    for r in range(lanes, n):
        after_escalated |= tier[r - lanes] != 0 and tier[r] == 0
        shorter_after_longer |= h[r] < h[r - lanes]
    assert n > lanes and shorter_after_longer, (name, n, lanes)
    if (tier != 0).any():
        assert after_escalated, (name, n, lanes, tier.tolist())


# ------------------------------------------------------------------ the switches themselves
def test_switches_only_lower(msim, monkeypatch):
    """Far above the natural value, or outside its range, a switch changes no size and no geometry; a lower one shows
    in msim_pipeline_info and never grows the workspace."""
    sims = [(_sim(msim, monkeypatch, "A", 4), 64), (_sim(msim, monkeypatch, "C", 4), 64)]
    monkeypatch.delenv("MSIM_FORCE_GENERAL")
    sims.append((msim.Simulation(_miners(msim, "A"), D3), 64))  # the entity engine with G behind it
    nat = [(s.workspace_bytes(n), s.pipeline_info(n)) for s, n in sims]
    assert [i["uses_pipeline"] for _, i in nat] == [4, 4, 3]
    for value in (str(2**31), "0", "-5"):
        for k in SWITCHES:
            monkeypatch.setenv(k, value)
        assert [(s.workspace_bytes(n), s.pipeline_info(n)) for s, n in sims] == nat, value
    for k in SWITCHES[1:4]:
        monkeypatch.setenv(k, "7")  # below the least window
    monkeypatch.setenv("MSIM_GEN_TEST_LANES", "x")
    monkeypatch.setenv("MSIM_GEN_TEST_LIST_CAP", "")
    assert [(s.workspace_bytes(n), s.pipeline_info(n)) for s, n in sims] == nat
    _set(monkeypatch, lanes=3, caps=LOW)
    for (s, n), (wsb, info) in zip(sims[:2], nat):
        low = s.pipeline_info(n)
        assert s.workspace_bytes(n) < wsb
        assert (low["slice_runs"], low["segment_blocks"]) == (3, 16)
        assert low["segments"] == (3 if s is sims[0][0] else 2) and low["blocks_per_run"] == (1024 if s is sims[0][0] else 64)
    assert sims[2][0].workspace_bytes(64) < nat[2][0]
    _set(monkeypatch, list_cap=1)  # the lists keep their allocation
    assert [(s.workspace_bytes(n), s.pipeline_info(n)) for s, n in sims] == nat


# ------------------------------------------------------------------ lane reuse
@pytest.mark.parametrize("caps", [None, LOW], ids=["natural", "16-64-1024"])
@pytest.mark.parametrize("lanes,n", [(1, 17), (3, 17), (64, 200), (300, 700)])
@pytest.mark.parametrize("name", ["A", "N9"])
def test_lane_reuse(msim, oracle, gen, monkeypatch, name, lanes, n, caps):
    """A lane serves its runs in turn over the chains, sizes, stale and folded-prefix counters its last run left:
    one lane, three (a ragged last round), a full wave, 300 (two workgroups, the second partial)."""
    tier = _predict(gen, name, n, caps or (256, 4096))
    assert (tier >= 0).all()
    _reuse_preconditions(gen, name, n, lanes, tier)
    sim = _sim(msim, monkeypatch, name, 4)
    nat = sim.pipeline_info(n)
    base = _natural(sim, (name, n, 4), n)
    _set(monkeypatch, lanes=lanes, caps=caps)
    _geometry(sim, n, nat, lanes, caps)
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, name, n, out, tier >= 0)
    _counters(out, tier, 4, n, 3 if caps else 2)
    assert out[0].tobytes() == base[0].tobytes(), "Q32.32 sums differ from the launch with no switch set"


@pytest.mark.parametrize("caps", [None, LOW], ids=["natural", "16-64-1024"])
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("name", ["A", "N9"])
def test_lane_reuse_as_e2_fallback(msim, oracle, gen, monkeypatch, name, lanes, caps):
    """The same through the lists: E1 flags every run, E2 hands every run to G (512 MiB of windows)."""
    n = 17
    tier = _predict(gen, name, n, caps or (256, 4096))
    assert (tier >= 0).all() and n > lanes
    sim = _sim(msim, monkeypatch, name, 3)
    base = _natural(sim, (name, n, 3), n)
    ws_nat = sim.workspace_bytes(n)
    _set(monkeypatch, lanes=lanes, caps=caps)
    assert sim.workspace_bytes(n) < ws_nat
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, name, n, out, tier >= 0)
    _counters(out, tier, 3, n, 3 if caps else 2)
    assert out[0].tobytes() == base[0].tobytes(), "Q32.32 sums differ from the launch with no switch set"


def test_lane_reuse_across_points(msim, oracle, monkeypatch):
    """Seven lanes over 3 x 30 runs of a sweep on G: a lane takes runs of different networks in turn."""
    rpp = 30
    pts = [[msim.Miner(k, w, 1000, k < 5) for k, w in enumerate([10] * 7 + [15, 15])], msim.PRESETS["c3"](), msim.PRESETS["c2"]()]
    sw = msim.Sweep(pts, D3)
    assert sw.plan(rpp)["engine"] == 4
    ws_nat = sw.workspace_bytes(rpp)
    base = _launch(sw, rpp, 3, 0)
    _set(monkeypatch, lanes=7)
    assert sw.workspace_bytes(rpp) < ws_nat
    sums, rec, bh, st, counts = _launch(sw, rpp, 3, 0xFF)
    for i, miners in enumerate(pts):
        f, s, _, _ = oracle.run_batch([mm.perc for mm in miners], [mm.propagation_ms for mm in miners],
                                      [mm.is_selfish for mm in miners], D3, rpp, 0, BASE, threads=16)
        assert np.array_equal(rec[i, :, :, 0], f) and np.array_equal(rec[i, :, :, 1], s), i
        assert np.array_equal(bh[i], f.sum(axis=1)), i
    assert st[1] == 0 and st[0] == counts[C_L2] + counts[C_L3], (st, counts)
    assert sums.tobytes() == base[0].tobytes() and base[3].tolist() == st.tolist()


# ------------------------------------------------------------------ all three tiers
@pytest.mark.parametrize("path", [4, 3], ids=["alone", "fallback"])
def test_all_three_tiers(msim, oracle, gen, monkeypatch, path):
    """Network A at windows of 16 / 64 / 1 024 blocks: every tier finishes runs, none fails."""
    n = 64
    tier = _predict(gen, "A", n, LOW)
    assert all((tier == i).any() for i in range(3)) and (tier >= 0).all()
    sim = _sim(msim, monkeypatch, "A", path)
    nat = sim.pipeline_info(n)
    base = _natural(sim, ("A", n, path), n)
    _set(monkeypatch, caps=LOW)
    if path == 4:
        _geometry(sim, n, nat, None, LOW)
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, "A", n, out, tier >= 0)
    l2, l3, _ = _counters(out, tier, path, n, 3)
    assert (l2, l3) == (60, 16)
    assert out[0].tobytes() == base[0].tobytes(), "Q32.32 sums differ from the launch with no switch set"


def test_every_run_reaches_tier_3(msim, oracle, gen, monkeypatch):
    """Network B (a 60 % selfish miner, 100 ms): no run ends below the third window."""
    n = 64
    tier = _predict(gen, "B", n, LOW)
    assert (tier == 2).all()
    sim = _sim(msim, monkeypatch, "B", 4)
    base = _natural(sim, ("B", n, 4), n)
    _set(monkeypatch, caps=LOW)
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, "B", n, out, tier >= 0)
    _counters(out, tier, 4, n, 3)
    assert out[4][C_L3] == n and out[3].tolist() == [2 * n, 0]
    assert out[0].tobytes() == base[0].tobytes()


@pytest.mark.parametrize("name", ["D", "ONE"])
def test_folds_every_few_blocks_in_tier_1(msim, oracle, gen, monkeypatch, name):
    """A 16-block window that every run folds again and again (honest, 10 s; one miner with zero delay, whose
    window-relative best-chain size goes negative): all in tier 1, nothing escalates."""
    n = 64
    tier = _predict(gen, name, n, (16, 4096))
    assert (tier == 0).all()
    sim = _sim(msim, monkeypatch, name, 4)
    nat = sim.pipeline_info(n)
    base = _natural(sim, (name, n, 4), n)
    _set(monkeypatch, caps=(16,))
    info = sim.pipeline_info(n)
    assert info["segment_blocks"] == 16 and info["segments"] == nat["segments"] == 2
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, name, n, out, tier >= 0)
    _counters(out, tier, 4, n, 2)
    assert out[3].tolist() == [0, 0]
    assert out[0].tobytes() == base[0].tobytes()


# ------------------------------------------------------------------ a last tier that is too small
@pytest.mark.parametrize("name,caps,failures", [("B", (16, 64, 256), 38), ("C", (8, 16), 39)])
def test_last_tier_too_small(msim, oracle, gen, monkeypatch, name, caps, failures):
    """The last window gives up: no next list, the run is counted failed, its records stay unwritten, msim_run
    returns MSIM_E_CAPACITY (B: three tiers; C: an honest network, two)."""
    from miningsimulation_amd import _lib

    n = 64
    tier = _predict(gen, name, n, caps)
    assert int((tier < 0).sum()) == failures and 0 < failures < n
    sim = _sim(msim, monkeypatch, name, 4)
    nat = sim.pipeline_info(n)
    _set(monkeypatch, caps=caps)
    _geometry(sim, n, nat, None, caps)
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, name, n, out, tier >= 0)
    _, _, failed = _counters(out, tier, 4, n, len(caps))
    assert failed == failures
    with pytest.raises(_lib.MsimError) as e:
        sim.run(n, 0, BASE, 0, per_run=True)
    assert e.value.code == _lib.MSIM_E_CAPACITY


# ------------------------------------------------------------------ the list bounds
def test_list_holds_half_of_what_leaves_tier_1(msim, oracle, gen, monkeypatch):
    """LIST_CAP = E / 2 on G alone: tier 1's appends past the list's end are dropped and counted once. Which runs are
    kept depends on the order of the atomics, so only counts are equalities."""
    n = 64
    tier = _predict(gen, "A", n, LOW)
    E = int((tier != 0).sum())
    assert E == 60 and (tier >= 0).all()
    cap = E // 2
    sim = _sim(msim, monkeypatch, "A", 4)
    _set(monkeypatch, caps=LOW, list_cap=cap)
    out = _launch(sim, n, 0, 0xFF)
    _, rec, bh, st, counts = out
    # tier 2 serves `cap` runs; those of them that need tier 3 are at most cap, so its list overflows by
    # max(0, that number - cap) = 0 whichever runs were kept
    overflow3 = 0
    assert counts[C_L2] == E and counts[C_L3] <= cap
    assert st[1] == counts[C_FAIL] == E - cap + overflow3, (st, counts)
    assert st[0] == counts[C_L2] + counts[C_L3]
    touched = bh != FF
    assert int((~touched).sum()) == st[1] and touched[tier == 0].all()
    f, s = _oracle(oracle, "A", n)
    assert np.array_equal(rec[touched, :, 0], f[touched]) and np.array_equal(rec[touched, :, 1], s[touched])
    assert np.array_equal(bh[touched], f[touched].sum(axis=1)) and (rec[~touched] == FF).all()


def test_list_clamp_on_the_fallback_path(msim, oracle, gen, monkeypatch):
    """LIST_CAP = 10 with 64 forced runs: E2's list holds 64 codes, tier 1 reads 10 and counts 54 failed."""
    n = 64
    sim = _sim(msim, monkeypatch, "A", 3)
    _set(monkeypatch, caps=LOW, list_cap=10)
    _, rec, bh, st, counts = _launch(sim, n, 0, 0xFF)
    assert counts[C_L1] == n and counts[C_L2] <= 10 and counts[C_L3] <= counts[C_L2]
    assert st[1] == counts[C_FAIL] == n - 10, (st, counts)
    touched = bh != FF
    assert int(touched.sum()) == 10
    f, s = _oracle(oracle, "A", n)
    assert np.array_equal(rec[touched, :, 0], f[touched]) and np.array_equal(rec[touched, :, 1], s[touched])
    assert np.array_equal(bh[touched], f[touched].sum(axis=1)) and (rec[~touched] == FF).all()
    # every kept run went the predicted way
    tier = _predict(gen, "A", n, LOW)
    assert counts[C_L2] == int((tier[touched] != 0).sum()) and counts[C_L3] == int((tier[touched] == 2).sum())


def test_list_of_exactly_what_leaves_tier_1(msim, oracle, gen, monkeypatch):
    """LIST_CAP = E changes nothing."""
    n = 64
    tier = _predict(gen, "A", n, LOW)
    E = int((tier != 0).sum())
    assert 0 < E < n
    sim = _sim(msim, monkeypatch, "A", 4)
    base = _natural(sim, ("A", n, 4), n)
    _set(monkeypatch, caps=LOW, list_cap=E)
    out = _launch(sim, n, 0, 0xFF)
    _exact(oracle, "A", n, out, tier >= 0)
    _, _, failed = _counters(out, tier, 4, n, 3)
    assert failed == 0
    assert out[0].tobytes() == base[0].tobytes()

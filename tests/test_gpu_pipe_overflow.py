"""The honest pipeline's capacity overflows on the device: K1's guarded appends (msim_drawgen.hip DevCtx::slow and
holes), S1's overflow rules (msim_sweepsplit.h), K2's REC_ERR and K3's guards (msim_pipeline.h combine_run), reached
with a few hundred runs by lowering the capacities through the test switches MSIM_PIPE_TEST_* (include/msim.h).

Every case asserts: found, stale and best height of every run equal the oracle's; the Q32.32 sums are byte for byte
those of the same launch with no switch set; status[1] == 0; and the stated condition on status[0], the number of
runs the retry kernel recomputed. Where the flagged set is a function of the draws and the geometry alone (slot
capacities, K2's kind), status[0] must equal the count of the host execution of the same lane bodies
(tests/native/pipeline_host.cpp) at the device's geometry (msim_pipeline_info). Every lowered launch runs into a
workspace of 0xFF bytes. 257 runs (one full workgroup plus one lane) of 10^9 ms at seed base 1000 unless stated; the
oracle's counters are computed once per network and shared."""
import numpy as np
import pytest

import pipeline_host_lib

pytestmark = pytest.mark.gpu

D = 10**9
N = 257
BASE = 1000
W = {1: [100], 2: [70, 30], 9: [30, 29, 12, 11, 8, 5, 3, 1, 1],
     15: [20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1]}
SWITCHES = ("MSIM_PIPE_TEST_CAP", "MSIM_PIPE_TEST_LCAP", "MSIM_PIPE_TEST_POINT_CAP", "MSIM_PIPE_TEST_POINT_LCAP",
            "MSIM_PIPE_TEST_K2_KIND")


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
    for k in SWITCHES + ("MSIM_MAX_SLICE_RUNS", "MSIM_SWEEP_SHARED_MAX_GROUP", "MSIM_PIPE_FORCE_RETRY"):
        monkeypatch.delenv(k, raising=False)


_REF = {}


def _oracle(oracle, percs, delay, duration, n):
    k = (tuple(percs), delay, duration, n)
    if k not in _REF:
        f, s, _, _ = oracle.run_batch(list(percs), [delay] * len(percs), [False] * len(percs), duration, n, 0, BASE, threads=16)
        f.setflags(write=False)
        s.setflags(write=False)
        _REF[k] = (f, s)
    return _REF[k]


def _net(msim, percs, delay):
    return [msim.Miner(k, percs[k], delay) for k in range(len(percs))]


def _launch(obj, n, points, fill, ws=None):
    """One launch of a Simulation (points = 0) or a Sweep into output buffers of `fill` bytes and a workspace of
    `fill` bytes (or the given one): sums, records, best heights, status as NumPy arrays, and the workspace."""
    import torch

    m = obj.m if points else len(obj.miners)
    lead = (points,) if points else ()
    if ws is None:
        ws = torch.full((obj.workspace_bytes(n),), fill, dtype=torch.uint8, device="cuda")
    sums = torch.full(lead + (m, 6), -1 if fill else 0, dtype=torch.int64, device="cuda")
    rec = torch.full(lead + (n, m, 2), -1 if fill else 0, dtype=torch.int32, device="cuda")
    bh = torch.full(lead + (n,), -1 if fill else 0, dtype=torch.int32, device="cuda")
    st = torch.full((2,), -1 if fill else 0, dtype=torch.int32, device="cuda")
    obj.launch(n, 0, BASE, sums, ws, st, rec, bh)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (sums, rec, bh, st)], ws


def _exact(oracle, out, percs, delays, duration, n):
    """Records and best heights of a launch (one network: delays is one value) against the oracle."""
    sums, rec, bh, st = out
    if len(delays) == 1:
        rec, bh = rec[None], bh[None]
    for p, delay in enumerate(delays):
        f, s = _oracle(oracle, percs, delay, duration, n)
        assert np.array_equal(rec[p, :, :, 0].astype(np.int64), f), (p, np.argwhere(rec[p, :, :, 0] != f)[:5])
        assert np.array_equal(rec[p, :, :, 1].astype(np.int64), s), (p, np.argwhere(rec[p, :, :, 1] != s)[:5])
        assert np.array_equal(bh[p].astype(np.int64), f.sum(axis=1)), p
    assert st[1] == 0, st


class Plain:
    """One network on the plain pipeline: its launch with no switch set, the device's geometry, the host's counts."""

    def __init__(self, msim, oracle, host, percs, delay, duration=D, n=N):
        self.percs, self.delay, self.duration, self.n = percs, delay, duration, n
        self.oracle, self.host = oracle, host
        self.sim = msim.Simulation(_net(msim, percs, delay), duration)
        info = self.sim.pipeline_info(n)
        assert info["uses_pipeline"] == 1, info
        self.info = info
        self.nseg, self.seg = info["segments"], info["segment_blocks"]
        self.lam = info["rho"] * self.seg  # mean listed blocks per (run, segment)
        self.ws_bytes = self.sim.workspace_bytes(n)
        self.base, _ = _launch(self.sim, n, 0, 0)
        _exact(oracle, self.base, percs, [delay], duration, n)
        assert self.base[3].tolist() == [0, 0], "the natural capacities retry nothing"

    def host_run(self, **over):
        f, s, ok, ne, listed, onepath = self.host(self.percs, [self.delay] * len(self.percs), self.duration, self.n,
                                                  nseg=self.nseg, seg=self.seg, detail=True, **over)
        of, os_ = _oracle(self.oracle, self.percs, self.delay, self.duration, self.n)
        assert np.array_equal(f[ok], of[ok]) and np.array_equal(s[ok], os_[ok]), "host: an unflagged run is not exact"
        return ok, ne, listed, onepath

    def lowered(self, ws=None):
        """A launch under the switches now set, into 0xFF bytes: exact, and the sums byte for byte the natural ones."""
        info = self.sim.pipeline_info(self.n)  # a switch changes no geometry, only sizes
        assert {**info, "workspace_bytes": 0} == {**self.info, "workspace_bytes": 0}
        assert self.sim.workspace_bytes(self.n) <= self.ws_bytes
        out, ws = _launch(self.sim, self.n, 0, 0xFF, ws)
        _exact(self.oracle, out, self.percs, [self.delay], self.duration, self.n)
        assert out[0].tobytes() == self.base[0].tobytes(), "Q32.32 sums differ from the launch with no switch set"
        assert out[1].tobytes() == self.base[1].tobytes() and out[2].tobytes() == self.base[2].tobytes()
        return out, ws


_PLAIN = {}


def _plain(msim, oracle, host, percs, delay, duration=D, n=N):
    k = (tuple(percs), delay, duration, n)
    if k not in _PLAIN:
        _PLAIN[k] = Plain(msim, oracle, host, percs, delay, duration, n)
    return _PLAIN[k]


# ------------------------------------------------------------------ the switches themselves
def test_switches_only_lower(msim, monkeypatch):
    """A value at or above the natural capacity changes no size; a lower one shrinks the workspace (the buffers are
    laid out from the lowered values); a K2 kind other than 0 or 1 is ignored."""
    sim = msim.Simulation(_net(msim, W[9], 10_000), D)
    pts = [_net(msim, W[9], d) for d in (10_000, 1_000, 100)]
    sw = msim.Sweep(pts, D, shared_draws=True)
    nat = (sim.workspace_bytes(N), sim.pipeline_info(N), sw.plan(N))
    assert nat[2]["engine"] == 1
    for k in SWITCHES[:4]:
        monkeypatch.setenv(k, str(2**31))
    monkeypatch.setenv("MSIM_PIPE_TEST_K2_KIND", "2")
    assert (sim.workspace_bytes(N), sim.pipeline_info(N), sw.plan(N)) == nat
    for k in SWITCHES[:4]:
        monkeypatch.setenv(k, "0")
    assert (sim.workspace_bytes(N), sim.pipeline_info(N), sw.plan(N)) == nat
    for k in SWITCHES[:4]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("MSIM_PIPE_TEST_K2_KIND", "0")  # the kind sizes nothing
    assert (sim.workspace_bytes(N), sim.pipeline_info(N), sw.plan(N)) == nat
    monkeypatch.delenv("MSIM_PIPE_TEST_K2_KIND")
    for k in SWITCHES[:4]:
        monkeypatch.setenv(k, "1")
        point = "POINT" in k
        assert (sim.workspace_bytes(N) < nat[0]) == (not point), k
        assert sw.plan(N)["workspace_bytes"] < nat[2]["workspace_bytes"], k
        monkeypatch.delenv(k)


# ------------------------------------------------------------------ K1: slot capacity
@pytest.mark.parametrize("which", ["one", "1.3 sigma", "2.3 sigma"])
def test_k1_slot_capacity(msim, oracle, host, monkeypatch, which):
    """K1 keeps counting past cap and stores no slot there; K3 flags the run at `v > cap`."""
    P = _plain(msim, oracle, host, W[9], 10_000)
    cap = {"one": 1, "1.3 sigma": pipeline_host_lib.sigma_cap(P.lam, 1.3), "2.3 sigma": pipeline_host_lib.sigma_cap(P.lam, 2.3)}[which]
    ok, _, _, _ = P.host_run(cap=cap)
    expected = int((~ok).sum())
    monkeypatch.setenv("MSIM_PIPE_TEST_CAP", str(cap))
    out, _ = P.lowered()
    print(f"K1 cap {cap} (lambda {P.lam:.3f}, nseg {P.nseg}, seg {P.seg}): host flags {expected}, status {out[3].tolist()}")
    assert out[3][0] == expected
    if which != "one":
        assert 0 < out[3][0] < N


# ------------------------------------------------------------------ K1: list capacity
@pytest.mark.parametrize("which", ["one", "half", "count"])
def test_k1_list_capacity(msim, oracle, host, monkeypatch, which):
    """K1 stores no entry at an index >= lcap (DevCtx::slow) and marks no hole there (DevCtx::holes); K2 runs
    min(count, lcap) entries; K3 flags a run whose slot holds such an index. Which runs lose entries depends on the
    order of K1's atomics; the results do not. The device's list also holds the unused tails of the waves' chunks, so
    half the host's count cuts well over half of it (measured: every run loses an entry); at the host's full count
    only the entries a hole displaced past it are lost (measured below: some runs, or none)."""
    P = _plain(msim, oracle, host, W[9], 10_000)
    _, ne, listed, _ = P.host_run()
    lcap = {"one": 1, "half": ne // 2, "count": ne}[which]
    monkeypatch.setenv("MSIM_PIPE_TEST_LCAP", str(lcap))
    out, ws = P.lowered()
    again, _ = P.lowered(ws)  # the same workspace, now holding the first launch's list, slots and records
    for a, b in zip(out[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    print(f"K1 lcap {lcap} (host list count {ne}): status {out[3].tolist()}, again {again[3].tolist()}")
    for st in (out[3], again[3]):
        if which == "one":
            # index 0 is the one entry kept; its run lists further blocks (every run lists at least two), so every
            # run that lists a block holds an index >= 1
            assert listed.min() >= 2 and st[0] == int((listed > 0).sum()) == N
        elif which == "half":
            assert 0 < st[0] <= N
        else:
            assert 0 <= st[0] <= N


# ------------------------------------------------------------------ K2: REC_ERR, K3's two episode paths
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("duration,path", [(5 * D, "one-read"), (D, "one-read"), (D // 10, "batched")])
def test_k2_lean_errors(msim, oracle, host, monkeypatch, m, duration, path):
    """45 s delays on K2's lean machine (two in-flight blocks): an episode that outgrows it sets REC_ERR, and K3 must
    flag the run where it applies that episode: `f0 & (REC_ERR | REC_SKIP)` on the one-read path (more than 32 listed
    blocks up to the end of the run: every run at 5*10^9 ms and at 10^9 ms, which list 93 or more) and
    `if (x & 1u) return false` on the batched path (every flagged run at 10^8 ms). An applied episode's error does not
    depend on the geometry, so status[0] is the host's count."""
    P = _plain(msim, oracle, host, W[m], 45_000, duration)
    ok, _, listed, onepath = P.host_run(kind=0)
    assert P.host_run()[0].all(), "the network's own mid machine flags nothing"
    expected = int((~ok).sum())
    assert expected > 0
    assert np.array_equal(onepath, listed > 32)
    if path == "one-read":
        assert onepath.all()
    else:
        assert not onepath[~ok].any()
    monkeypatch.setenv("MSIM_PIPE_TEST_K2_KIND", "0")
    out, _ = P.lowered()
    print(f"K2 lean, M {m}, D {duration}: host flags {expected} ({int(onepath[~ok].sum())} on the one-read path), "
          f"listed {listed.min()}..{listed.max()}, status {out[3].tolist()}")
    assert out[3][0] == expected


# ------------------------------------------------------------------ other instantiations of K2 and K3
@pytest.mark.parametrize("m", [1, 2, 15])
def test_other_miner_counts(msim, oracle, host, monkeypatch, m):
    P = _plain(msim, oracle, host, W[m], 10_000)
    cap = pipeline_host_lib.sigma_cap(P.lam, 1.3)
    ok, ne, _, _ = P.host_run(cap=cap)
    monkeypatch.setenv("MSIM_PIPE_TEST_CAP", str(cap))
    out, _ = P.lowered()
    print(f"M {m} cap {cap}: host flags {int((~ok).sum())}, status {out[3].tolist()}")
    assert 0 < out[3][0] == int((~ok).sum()) < N
    monkeypatch.delenv("MSIM_PIPE_TEST_CAP")
    monkeypatch.setenv("MSIM_PIPE_TEST_LCAP", str(ne // 2))
    out, _ = P.lowered()
    print(f"M {m} lcap {ne // 2}: status {out[3].tolist()}")
    assert 0 < out[3][0] <= N


# ------------------------------------------------------------------ S1: the shared-draw sweep
DELAYS = (10_000, 1_000, 100)


class Shared:
    def __init__(self, msim, oracle, n):
        self.n, self.oracle = n, oracle
        self.sw = msim.Sweep([_net(msim, W[9], d) for d in DELAYS], D, shared_draws=True)
        plan = self.sw.plan(n)
        assert plan["engine"] == 1 and plan["draw_groups"] == 1 and plan["largest_group"] == 3, plan
        self.plan = plan
        self.base, _ = _launch(self.sw, n, 3, 0)
        _exact(oracle, self.base, W[9], DELAYS, D, n)
        assert self.base[3].tolist() == [0, 0]

    def lowered(self):
        plan = self.sw.plan(self.n)
        assert plan["workspace_bytes"] <= self.plan["workspace_bytes"]
        out, _ = _launch(self.sw, self.n, 3, 0xFF)
        _exact(self.oracle, out, W[9], DELAYS, D, self.n)
        for a, b in zip(out[:3], self.base[:3]):
            assert a.tobytes() == b.tobytes(), "sums, records or best heights differ from the launch with no switch set"
        return out


_SHARED = {}


def _shared(msim, oracle, n=N):
    if n not in _SHARED:
        _SHARED[n] = Shared(msim, oracle, n)
    return _SHARED[n]


def _envelope_cap(msim, oracle, host, n=N):
    """c = ceil(lambda + 1.3 sqrt(lambda)) of the envelope (the 10 s network: uniform delays, so the envelope is the
    slowest point) and k_c, the host's flagged count for that network at the geometry now in force."""
    sim = msim.Simulation(_net(msim, W[9], 10_000), D)
    info = sim.pipeline_info(n)
    c = pipeline_host_lib.sigma_cap(info["rho"] * info["segment_blocks"], 1.3)
    f, s, ok, _ = host(W[9], [10_000] * 9, D, n, nseg=info["segments"], seg=info["segment_blocks"], cap=c)
    of, os_ = _oracle(oracle, W[9], 10_000, D, n)
    assert np.array_equal(f[ok], of[ok]) and np.array_equal(s[ok], os_[ok])
    return c, int((~ok).sum())


@pytest.mark.parametrize("form", ["plain", "passes of 2", "slices of 256"])
def test_shared_envelope_slot_capacity(msim, oracle, host, monkeypatch, form):
    """(a) An envelope overflow stores cap_p + 1 at every point: every point retries the same runs."""
    n = 600 if form == "slices of 256" else N
    S = _shared(msim, oracle, n)
    if form == "passes of 2":
        monkeypatch.setenv("MSIM_SWEEP_SHARED_MAX_GROUP", "2")
    if form == "slices of 256":
        monkeypatch.setenv("MSIM_MAX_SLICE_RUNS", "256")
        assert S.sw.plan(n)["slice_runs"] == 256
    c, k_c = _envelope_cap(msim, oracle, host, n)
    monkeypatch.setenv("MSIM_PIPE_TEST_CAP", str(c))
    out = S.lowered()
    print(f"shared (a) {form}: c {c}, k_c {k_c}, status {out[3].tolist()}")
    assert 0 < k_c < n and out[3][0] == 3 * k_c


def test_shared_point_slot_capacity(msim, oracle, host, monkeypatch):
    """(b) A point's own overflow flags that point only: the 10 s point retries its k_c runs; the 1 s and 100 ms
    points (lambda_p < 1 per segment) never list c blocks in a segment."""
    S = _shared(msim, oracle)
    c, k_c = _envelope_cap(msim, oracle, host)
    for d in DELAYS[1:]:
        _, _, listed, _ = _plain(msim, oracle, host, W[9], d).host_run()
        assert listed.max() < c  # not even a whole run of theirs lists c blocks
    monkeypatch.setenv("MSIM_PIPE_TEST_POINT_CAP", str(c))
    out = S.lowered()
    print(f"shared (b): c {c}, k_c {k_c}, status {out[3].tolist()}")
    assert 0 < k_c < N and out[3][0] == k_c


@pytest.mark.parametrize("point", [0, 1, 2])
def test_shared_list_capacities(msim, oracle, host, monkeypatch, point):
    """(c) The envelope's list at half its count (S1 flags the run at every point), and every point's index list at
    half the count of point `point`'s own list (a position >= lcap_p goes to slots_p, not to sel_p)."""
    S = _shared(msim, oracle)
    counts = [_plain(msim, oracle, host, W[9], d).host_run()[1] for d in DELAYS]
    monkeypatch.setenv("MSIM_PIPE_TEST_LCAP", str(counts[0] // 2))
    monkeypatch.setenv("MSIM_PIPE_TEST_POINT_LCAP", str(counts[point] // 2))
    out = S.lowered()
    print(f"shared (c): lcap {counts[0] // 2}, lcap_p {counts[point] // 2} (host list counts {counts}), status {out[3].tolist()}")
    assert 0 < out[3][0] <= 3 * N

"""Error bars without a GPU: the struct layouts, msim_moments.h's host accumulation (the lines the gfx950 kernel
runs) against tests/moments_reference.py, msim_moments_to_errors against fractions, the histogram helpers, the
sharded path under gloo, and the stand-alone sanitizer build of the wide-integer helper."""
import ctypes
import fcntl
import math
import os
import socket
import struct
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import moments_cases
import moments_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "libmoments_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "moments_check")
SPEC = (8, 29, 30, 1 << 20, 0)  # bins, share_shift, rate_shift, share_lo, rate_lo


def _built():
    """build/libmoments_host.so and build/moments_check, built here when missing or older than their sources."""
    import __graft_entry__ as ge

    srcs = [os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_moments.h"),
            os.path.join(ROOT, "include", "msim.h"),
            os.path.join(ROOT, "tests", "native", "moments_host.cpp"),
            os.path.join(ROOT, "tests", "native", "moments_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".moments_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_moments_tests()
    return HOST_LIB


def host_accumulate(found, stale, best_height, spec=None):
    """(words [M, 20] uint64, hist [M, 2, bins + 2] uint64 or None) from libmoments_host.so."""
    from miningsimulation_amd import _lib

    h = ctypes.CDLL(_built())
    rec = moments_cases.records(found, stale)
    n, m = found.shape
    bh = np.ascontiguousarray(best_height, dtype=np.uint32)
    words = np.zeros((m, 20), dtype=np.uint64)
    hist = np.zeros((m, 2, spec[0] + 2), dtype=np.uint64) if spec else None
    sp = _lib.MsimHistSpec(*spec) if spec else None
    rc = h.moments_host_accumulate(ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(bh.ctypes.data),
                                   ctypes.c_uint64(n), ctypes.c_uint32(m), ctypes.byref(sp) if sp else None,
                                   ctypes.c_void_p(words.ctypes.data),
                                   ctypes.c_void_p(hist.ctypes.data) if spec else None)
    assert rc == 0
    return words, hist


def test_struct_sizes(msim_lib_path):
    from miningsimulation_amd import _lib

    assert ctypes.sizeof(_lib.MsimMoments) == 160
    assert ctypes.sizeof(_lib.MsimErrors) == 64
    assert ctypes.sizeof(_lib.MsimHistSpec) == 32


def test_cases_hold_every_extreme():
    f, s, L = (a.astype(np.int64) for a in moments_cases.synthetic(40, 5))
    st, rt = ref.terms(f, s, L)
    flat_s, flat_r = st.ravel().tolist(), rt.ravel().tolist()
    assert (f == 0).any() and ((L == 0)[:, None] & (f > 0)).any() and (f == L[:, None]).any()
    assert (f == L[:, None] + 1).any() and (s > f).any() and ((f == 1) & (s == 2**32 - 1)).any()
    assert (f[6] == f[7]).all() and (f[7] == f[8]).all() and L[6] == L[7] == L[8]
    assert 1 << 32 in flat_s and max(flat_s) == 2**64 - 2**32 and max(flat_r) == 2**64 - 2**32
    # one uint64 per square would be wrong: the largest squares need all 128 bits
    assert max(flat_r) ** 2 >= 1 << 127


@pytest.mark.parametrize("n_runs,m", [(1, 1), (9, 3), (40, 5), (200, 17)])
def test_host_accumulation_equals_reference(msim_lib_path, n_runs, m):
    from miningsimulation_amd.moments import moments_from_words

    f, s, L = moments_cases.synthetic(n_runs, m, seed=n_runs)
    words, hist = host_accumulate(f, s, L, SPEC)
    bad = ref.diff(moments_from_words(words), ref.expected(f, s, L))
    assert not bad, "\n".join(bad[:10])
    want = ref.expected_hist(f, s, L, *SPEC)
    assert np.array_equal(hist, want)
    assert (hist.sum(axis=2) == n_runs).all()


def _bits(x):
    return struct.pack("<d", x)


def test_errors_against_fractions(msim_lib_path):
    """Exact numerators, then fewer than eight f64 roundings: relative error below 2^-50, bound 1e-13."""
    from miningsimulation_amd import _lib
    from miningsimulation_amd.moments import ERROR_FIELDS, errors_from_moments, moments_from_words

    for n_runs, m, seed in ((40, 5, 1), (200, 17, 2), (2, 3, 3)):
        f, s, L = moments_cases.synthetic(n_runs, m, seed=seed)
        words, _ = host_accumulate(f, s, L)
        mo = moments_from_words(words)
        got = errors_from_moments(mo, n_runs)
        for k in range(m):
            want = ref.errors(mo[k], n_runs)
            for name in ERROR_FIELDS:
                err = ref.rel_error(got[k][name], want[name], squared=name.endswith("_se"))
                assert err <= 1e-13, (n_runs, k, name, got[k][name], err)
        # the device's limbs (not normalised) and the normalised ones errors_from_moments built: the same bits
        raw = (_lib.MsimMoments * m)()
        ctypes.memmove(raw, words.ctypes.data, 160 * m)
        out = (_lib.MsimErrors * m)()
        _lib.lib.msim_moments_to_errors(raw, m, n_runs, out)
        for k in range(m):
            for name in ERROR_FIELDS:
                assert _bits(getattr(out[k], name)) == _bits(got[k][name]), (k, name)
        if n_runs >= 40:
            assert any(int(w) >> 32 for w in words[:, 12])  # a limb that normalising does change


def test_errors_constant_series_and_single_run(msim_lib_path):
    from miningsimulation_amd.moments import errors_from_moments, moments_from_words

    n = 37
    f = np.full((n, 2), 6, dtype=np.uint32)
    s = np.full((n, 2), 2, dtype=np.uint32)
    L = np.full(n, 18, dtype=np.uint32)
    words, _ = host_accumulate(f, s, L)
    for e in errors_from_moments(moments_from_words(words), n):
        assert e["found_se"] == 0.0 and e["share_se"] == 0.0 and e["rate_se"] == 0.0 and e["pooled_rate_se"] == 0.0
        assert e["found_mean"] == 6.0 and e["pooled_rate"] == 2.0 / 6.0
    words, _ = host_accumulate(f[:1], s[:1], L[:1])
    for e in errors_from_moments(moments_from_words(words), 1):
        assert all(math.isnan(e[k]) for k in ("found_se", "share_se", "rate_se", "pooled_rate_se"))
        assert e["found_mean"] == 6.0


def test_limb_round_trip():
    from miningsimulation_amd.moments import join_limbs, split_limbs

    f, s, L = moments_cases.synthetic(40, 3)
    words, _ = host_accumulate(f, s, L)
    for row in words.tolist():
        assert join_limbs(split_limbs(join_limbs(row))) == join_limbs(row)


def test_hist_spec_covering():
    from miningsimulation_amd import HistSpec

    sp = HistSpec.covering(0.25, 0.5, 256)
    assert sp.share_lo == 1 << 30 and sp.share_shift == 23      # 2^30 / 256 = 2^22 per bin would end AT hi
    assert sp.bin_of(1 << 31) == 129 and sp.bin_of((1 << 30) - 1) == 0
    assert ((1 << 31) - (1 << 30)) >> (sp.share_shift - 1) >= 256   # one less does not reach hi
    assert HistSpec.covering(0.0, 1.0, 1024).share_shift == 23     # 2^32 >> 22 = 1024: still outside
    assert HistSpec.covering(0.0, 0.0, 1).share_shift == 0
    sp = HistSpec.covering(0.0, 0.5, 64, rate_lo=0.0, rate_hi=4.0)
    assert (sp.share_shift, sp.rate_shift) == (26, 29)
    assert sp.bin_of(4 << 32, "rate") == 33 and sp.bin_of((4 << 32) + (1 << 34), "rate") == 65
    with pytest.raises(ValueError):
        HistSpec(0)
    with pytest.raises(ValueError):
        HistSpec(1025)


def test_hist_quantile_hand_made():
    from miningsimulation_amd import HistSpec, hist_quantile

    sp = HistSpec(4, share_shift=30, share_lo=1 << 30)   # bins of 0.25 from 0.25
    counts = [1, 2, 0, 3, 1, 1]                          # under, 4 bins, over: 8 values
    assert hist_quantile(counts, sp, 0.0) == (0.0, 0.25)
    assert hist_quantile(counts, sp, 0.125) == (0.0, 0.25)
    assert hist_quantile(counts, sp, 0.25) == (0.25, 0.5)
    assert hist_quantile(counts, sp, 0.5) == (0.75, 1.0)      # the 4th value: bin 2 is empty
    assert hist_quantile(counts, sp, 0.875) == (1.0, 1.25)
    assert hist_quantile(counts, sp, 1.0) == (1.25, math.inf)
    with pytest.raises(ValueError):
        hist_quantile(counts[:-1], sp, 0.5)


def test_report_with_errors_format(msim_lib_path):
    from miningsimulation_amd import MinerStats, SimulationResult, report, report_with_errors, setup_miners
    from miningsimulation_amd.moments import moments_from_words

    miners = setup_miners(1000)[:2]
    f = np.array([[4, 0], [6, 0], [8, 0], [6, 0]], dtype=np.uint32)
    s = np.array([[1, 0], [0, 0], [2, 0], [1, 0]], dtype=np.uint32)
    L = np.array([8, 12, 16, 12], dtype=np.uint32)
    words, _ = host_accumulate(f, s, L)
    st = [MinerStats(24, 2.0, 0.25 + 0.25 + 1 / 6), MinerStats()]
    res = SimulationResult(stats_total=st, sums=[], n_runs=4, moments=moments_from_words(words))
    plain = report(miners, st, 4).splitlines()
    out = report_with_errors(miners, res).splitlines()
    assert out[0] == plain[0] and len(out) == 3
    # found 4, 6, 8, 6: se = sqrt(8/3 / 4); share 0.5 in every run; rate 1/4, 0, 1/4, 1/6
    assert out[1].startswith(plain[1] + " ± 0.816497 blocks, ± 0% of blocks, stale rate ± ")
    assert out[2] == plain[2] + " ± 0 blocks, ± 0% of blocks, stale rate ± 0%"
    one = SimulationResult(stats_total=st, sums=[], n_runs=1, moments=moments_from_words(host_accumulate(f[:1], s[:1], L[:1])[0]))
    assert report_with_errors(miners, one).splitlines()[1].endswith(" ± n/a blocks, ± n/a of blocks, stale rate ± n/a")


def test_moments_check_under_sanitizers():
    """The wide-integer helper and the host accumulation, built stand-alone with ASan + UBSan, on the extreme
    records: a child process on the CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "moments_check: ok" in r.stdout


# ---------------------------------------------------------------- sharded path under gloo
N_TOTAL, M_SH, CHUNK = 29, 4, 6
HSPEC = dict(bins=8, share_shift=29, rate_shift=30, share_lo=1 << 20, rate_lo=0)


class _FakeSim:
    """Stands in for Simulation on a CPU rank: launch fills the records of runs [begin, begin + n) of one fixed
    synthetic data set (and their first sums), launch_moments is msim_moments.h's host accumulation."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = moments_cases.synthetic(N_TOTAL, M_SH, seed=7)

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        assert ws is None and n <= CHUNK
        f, s, L = self.f[begin:begin + n], self.s[begin:begin + n], self.L[begin:begin + n]
        d_per_run[:n] = torch.from_numpy(moments_cases.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        words, _ = host_accumulate(f, s, L)
        sums.copy_(torch.from_numpy(words[:, :6].copy().view(np.int64)))
        status.zero_()

    def launch_moments(self, n, d_per_run, d_best_height, d_moments, hist_spec, d_hist, stream=None):
        import torch

        rec = d_per_run[:n].numpy().view(np.uint32)
        spec = (hist_spec.bins, hist_spec.share_shift, hist_spec.rate_shift, hist_spec.share_lo, hist_spec.rate_lo)
        words, hist = host_accumulate(rec[:, :, 0], rec[:, :, 1], d_best_height[:n].numpy().view(np.uint32), spec)
        d_moments.copy_(torch.from_numpy(words.view(np.int64)))
        d_hist.copy_(torch.from_numpy(hist.view(np.int64)))


def _run_fake():
    import torch

    from miningsimulation_amd import HistSpec
    from miningsimulation_amd.distributed import run_sharded_moments

    sim = _FakeSim()
    res = run_sharded_moments(sim, N_TOTAL, 1000, launch=sim.launch, launch_moments=sim.launch_moments,
                              device=torch.device("cpu"), max_chunk=CHUNK, hist=HistSpec(**HSPEC))
    sums = [[getattr(x, f) for f, _ in x._fields_] for x in res.sums]
    return {"moments": res.moments, "hist": res.hist.tolist(), "sums": sums, "n_runs": res.n_runs,
            "share": [s.blocks_share for s in res.stats_total]}


def _worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce

    def counted(t, *a, **kw):
        calls.append(t.numel())
        return real(t, *a, **kw)

    dist.all_reduce = counted
    try:
        res = _run_fake()
    finally:
        dist.all_reduce = real
    out_q.put((rank, res, calls))
    dist.destroy_process_group()


def test_gloo_world2_run_sharded_moments_matches_world1(msim_lib_path):
    _built()
    want = _run_fake()  # no process group: world 1
    f, s, L = moments_cases.synthetic(N_TOTAL, M_SH, seed=7)
    assert not ref.diff(want["moments"], ref.expected(f, s, L))
    assert want["hist"] == ref.expected_hist(f, s, L, *HSPEC.values()).tolist()
    # the first moments are the launches' own sums, limbs joined
    for mo, row in zip(want["moments"], want["sums"]):
        assert (mo["found"], mo["stale"]) == (row[0], row[1])
        assert mo["share"] == (row[2] << 32) + row[3] and mo["rate"] == (row[4] << 32) + row[5]

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res, calls in got:
        assert res == want, rank
        # ONE all-reduce of sums + status + moments + histogram
        assert calls == [6 * M_SH + 2 + 20 * M_SH + 2 * (HSPEC["bins"] + 2) * M_SH], (rank, calls)

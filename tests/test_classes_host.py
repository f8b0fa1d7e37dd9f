"""Miner classes without a GPU: msim_fold.h's host-executed lane body (the lines the gfx950 fold kernel runs) against
tests/classes_reference.py, its stand-alone sanitizer build, msim_classes_check, the Python helpers, and the sharded
path under gloo."""
import ctypes
import fcntl
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import classes_reference as cls
import cross_reference as cref
import moments_cases
import moments_reference as ref
from test_moments_host import host_accumulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "libfold_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "fold_check")
U32 = 0xFFFFFFFF


def _built():
    """build/libfold_host.so and build/fold_check, built here when missing or older than their sources."""
    import __graft_entry__ as ge

    srcs = [os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_fold.h"),
            os.path.join(ROOT, "include", "msim.h"),
            os.path.join(ROOT, "tests", "native", "fold_host.cpp"),
            os.path.join(ROOT, "tests", "native", "fold_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".fold_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_fold_tests()
    return HOST_LIB


def host_fold(found, stale, class_of, n_classes, tc=0, gw=0):
    """(found [n, C], stale [n, C]) from libfold_host.so into a 0xFF-filled output; tc = gw = 0: the launch's shape."""
    h = ctypes.CDLL(_built())
    rec = cls.records(found, stale)
    n, m = found.shape
    cmap = np.asarray(class_of, dtype=np.uint32)
    out = np.full((n, n_classes, 2), U32, dtype=np.uint32)
    rc = h.fold_host_run(ctypes.c_void_p(rec.ctypes.data), ctypes.c_uint64(n), ctypes.c_uint32(m),
                         ctypes.c_void_p(cmap.ctypes.data), ctypes.c_uint32(n_classes),
                         ctypes.c_void_p(out.ctypes.data), ctypes.c_uint32(tc), ctypes.c_uint32(gw))
    assert rc == 0
    return out[:, :, 0].copy(), out[:, :, 1].copy()


def _plan(m, n_classes, n_runs):
    h = ctypes.CDLL(_built())
    tc, gw = ctypes.c_uint32(), ctypes.c_uint32()
    h.fold_host_plan(ctypes.c_uint32(m), ctypes.c_uint32(n_classes), ctypes.c_uint64(n_runs), ctypes.byref(tc),
                     ctypes.byref(gw))
    return tc.value, gw.value


@pytest.mark.parametrize("m", [1, 2, 9, 64, 65, 257, 1026])
def test_host_fold_equals_reference(m):
    """Random records with full-range counters (the sums wrap) under every named map, at the launch's tile shape
    and at forced ones: several class tiles with a partial last one, segments of several runs."""
    n = 37
    rng = np.random.default_rng(m)
    f = rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64).astype(np.uint32)
    s = rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64).astype(np.uint32)
    for name, (cmap, nc) in cls.maps(m).items():
        want = cls.fold(f, s, cmap, nc)
        for tc, gw in ((0, 0), (max(1, nc // 2), 1), (nc, 3), (1 if nc <= 9 else nc, 2)):
            got = host_fold(f, s, cmap, nc, tc, gw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, tc, gw)
        if name == "identity":  # the output bytes are the input's
            assert np.array_equal(want[0], f) and np.array_equal(want[1], s)
        if name == "all_none":
            assert not want[0].any() and not want[1].any()
        if name == "one_empty":
            assert not want[0][:, 1].any() and want[0][:, 0].any()


def test_host_fold_wraps_modulo_2_32():
    """A class sum of exactly 2^32 - 1 stays; one of 2^32 + 5 comes out as 5."""
    m = 130
    f = np.zeros((2, m), dtype=np.uint32)
    s = np.zeros((2, m), dtype=np.uint32)
    f[0, 0], f[0, 64], f[0, 65] = 0xFFFFFF00, 0xFE, 1          # 2^32 - 1: lanes 0, 0 and 1
    s[0, 0], s[0, 64], s[0, 65] = U32, 3, 3                    # 2^32 + 5
    f[1, :] = 0x02000000                                       # 128 members of 2^25 each: 2^32, i.e. 0
    cmap = [0] * m
    cmap[7], cmap[129] = cls.NONE, 1
    f[0, 7] = s[0, 7] = 9
    for tc, gw in ((0, 0), (1, 2)):
        cf, cs = host_fold(f, s, cmap, 2, tc, gw)
        assert (int(cf[0, 0]), int(cs[0, 0])) == (U32, 5) and (int(cf[0, 1]), int(cs[0, 1])) == (0, 0)
        assert int(cf[1, 0]) == 0 and int(cf[1, 1]) == 0x02000000
    assert np.array_equal(cls.fold(f, s, cmap, 2)[0], cf)


def test_plan_keeps_the_tile_within_its_cells():
    for m, nc, runs in ((1, 1, 1), (9, 8, 65536), (9, 8, 300), (1026, 3, 65536), (1026, 1026, 65536),
                        (4100, 4100, 257), (4100, 2, 1000), (2048, 1, 10**6), (2049, 1, 10**6), (64, 64, 10**9)):
        tc, gw = _plan(m, nc, runs)
        assert 1 <= tc <= nc and gw >= 1 and 4 * gw * tc <= 4608, (m, nc, runs, tc, gw)
        assert gw == 1 or gw * m <= 2048, (m, nc, runs, tc, gw)
    assert _plan(1026, 1026, 65536) == (1026, 1) and _plan(4100, 4100, 257)[0] == 1152


def test_fold_feeds_the_moments_reference():
    """The folded counters through the existing host accumulation (msim_moments.h) and references: a class is one
    miner to them, and a class holding the single miner k gives miner k's sums."""
    from miningsimulation_amd.moments import moments_from_words

    f, s, L = moments_cases.synthetic(40, 5, seed=3)
    cmap, nc = [0, 1, 1, cls.NONE, 0], 3  # class 2 is empty
    cf, cs = host_fold(f, s, cmap, nc)
    assert np.array_equal(cf, cls.fold(f, s, cmap, nc)[0])
    words, _ = host_accumulate(cf, cs, L)
    assert not ref.diff(moments_from_words(words), ref.expected(cf, cs, L))
    single = host_fold(f, s, [cls.NONE, cls.NONE, 0, cls.NONE, cls.NONE], 1)
    assert ref.expected(single[0], single[1], L)[0] == ref.expected(f, s, L)[2]


def test_fold_check_under_sanitizers():
    """The lane body built stand-alone with ASan + UBSan on random and extreme records: a child process on the CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fold_check: ok" in r.stdout


def test_classes_check_validation(msim_lib_path):
    from miningsimulation_amd import _lib

    u32 = ctypes.c_uint32
    chk = _lib.lib.msim_classes_check
    ok = (u32 * 4)(0, _lib.MSIM_CLASS_NONE, 1, 0)
    assert chk(4, ok, 2) == _lib.MSIM_OK and chk(4, ok, 4) == _lib.MSIM_OK
    assert chk(4, (u32 * 4)(*[_lib.MSIM_CLASS_NONE] * 4), 1) == _lib.MSIM_OK     # all NONE
    assert chk(4, (u32 * 4)(0, 2, 1, 0), 2) == _lib.MSIM_E_INVALID                # a class == n_classes
    assert chk(4, ok, 0) == _lib.MSIM_E_INVALID                                   # no classes
    assert chk(4, ok, 5) == _lib.MSIM_E_INVALID                                   # m + 1 classes
    assert chk(4, None, 2) == _lib.MSIM_E_INVALID                                 # a null map
    assert chk(0, ok, 1) == _lib.MSIM_E_INVALID
    assert ctypes.CDLL(_built()).fold_host_map_ok(u32(4), ok, u32(2)) == 1


def test_fold_launch_rejects_bad_arguments_without_a_device(msim_lib_path):
    """The domain errors are decided before anything touches the device."""
    from miningsimulation_amd import _lib

    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused
    ok = dict(m=3, points=1, runs=2, rec=p, cmap=p, nc=2, out=p)
    for change in (dict(m=0), dict(points=0), dict(points=65536), dict(runs=0), dict(runs=1 << 32), dict(nc=0),
                   dict(nc=4), dict(rec=None), dict(cmap=None), dict(out=None)):
        a = dict(ok, **change)
        rc = _lib.lib.msim_fold_launch(a["m"], a["points"], a["runs"], a["rec"], a["cmap"], a["nc"], a["out"], None)
        assert rc == _lib.MSIM_E_INVALID, change


def test_classes_of_and_from_groups(msim_lib_path):
    import miningsimulation_amd as msim
    from miningsimulation_amd.classes import NONE, class_count, class_map_struct, members_of

    cmap, members = msim.classes_of(msim.c5_network())
    assert [len(g) for g in members] == [1, 1, 1024] and cmap[:3] == [0, 1, 2] and set(cmap[2:]) == {2}
    cmap, members = msim.classes_of(msim.setup_miners())
    assert [len(g) for g in members] == [1, 1, 1, 1, 1, 1, 1, 2] and members[7] == [7, 8] and cmap[8] == 7
    sel = msim.setup_miners(1000, selfish_perc=40)
    cmap, members = msim.classes_of(sel)
    assert members[0] == [0] and len(members) == 8            # 40 and 19 are alone; the two 1 % miners share
    twin = [msim.Miner(0, 50, 1000, True), msim.Miner(1, 50, 1000, False)]
    assert msim.classes_of(twin)[0] == [0, 1]                 # the strategy separates equal hashrates
    assert members_of(cmap, len(members)) == members and class_count(cmap) == 8

    cmap, members = msim.classes_from_groups(9, [[0], [8, 7], []])
    assert cmap == [0, NONE, NONE, NONE, NONE, NONE, NONE, 1, 1] and members == [[0], [7, 8], []]
    assert class_count(cmap) == 2 and class_count([NONE] * 3) == 1
    class_map_struct(cmap, 9, 3)                              # an empty last class is a valid map
    for bad in ([[0], [0]], [[9]], [[-1]], [], [[k] for k in range(9)] + [[]]):
        with pytest.raises(ValueError):
            msim.classes_from_groups(9, bad)
    for bad_map, nc in (([0, 2, 1], 2), ([0, 1], 2), ([0, 0, 0], 0), ([0, 0, 0], 4), ([0, -1, 0], 1)):
        with pytest.raises(ValueError):
            class_map_struct(bad_map, 3, nc)


def test_report_classes_hand_made(msim_lib_path):
    import miningsimulation_amd as msim
    from miningsimulation_amd.moments import moments_from_words

    miners = msim.setup_miners(1000)
    cmap, members = msim.classes_from_groups(9, [[0, 1], [7, 8], []])
    f = np.array([[4, 0, 0], [6, 0, 0], [8, 0, 0], [6, 0, 0]], dtype=np.uint32)   # per class, as folded
    s = np.array([[1, 0, 0], [0, 0, 0], [2, 0, 0], [1, 0, 0]], dtype=np.uint32)
    L = np.array([8, 12, 16, 12], dtype=np.uint32)
    words, _ = host_accumulate(f, s, L)
    res = msim.SimulationResult(stats_total=[], sums=[], n_runs=4, moments=moments_from_words(words))
    out = msim.report_classes(miners, members, res).splitlines()
    # found 4, 6, 8, 6: mean 6, se sqrt(8/3 / 4); share 0.5 in every run; rate 1/4, 0, 1/4, 1/6
    assert out[0].startswith("  - Class 0 (2 miners, 59% of network hashrate) found 6 ± 0.816497 blocks i.e. "
                             "50% ± 0% of blocks. Stale rate: 16.6667% ± ")
    assert out[1] == ("  - Class 1 (2 miners, 2% of network hashrate) found 0 ± 0 blocks i.e. 0% ± 0% of blocks. "
                      "Stale rate: 0% ± 0%.")
    assert out[2].startswith("  - Class 2 (0 miners, 0% of network hashrate) found 0 ± 0 blocks") and len(out) == 3
    with pytest.raises(ValueError):
        msim.report_classes(miners, members[:2], res)


# ---------------------------------------------------------------- sharded path under gloo
N_TOTAL, M_SH, CHUNK = 29, 5, 6
CMAP, NC = [1, 0, cls.NONE, 1, 0], 3   # class 2 is empty
PAIRS = [(0, 0, 0, 1), (0, 1, 0, 1), (0, 2, 0, 0)]
HSPEC = dict(bins=8, share_shift=29, rate_shift=30, share_lo=1 << 20, rate_lo=0)


class _FakeSim:
    """Stands in for Simulation on a CPU rank, as tests/test_moments_host.py's: launch fills the records of one fixed
    synthetic data set, launch_fold is msim_fold.h's host body, the moments and cross launches are the host
    accumulations of msim_moments.h and msim_cross.h."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = moments_cases.synthetic(N_TOTAL, M_SH, seed=11)

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        assert ws is None and n <= CHUNK
        f, s, L = self.f[begin:begin + n], self.s[begin:begin + n], self.L[begin:begin + n]
        d_per_run[:n] = torch.from_numpy(moments_cases.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        words, _ = host_accumulate(f, s, L)
        sums.copy_(torch.from_numpy(words[:, :6].copy().view(np.int64)))
        status.zero_()

    def launch_fold(self, n, d_per_run, d_class_of, n_classes, d_class_run, stream=None):
        import torch

        rec = d_per_run[:n].numpy().view(np.uint32)
        cf, cs = host_fold(rec[:, :, 0], rec[:, :, 1], d_class_of.numpy().view(np.uint32), n_classes)
        d_class_run.view(torch.uint8).fill_(0xFF)
        d_class_run[:n] = torch.from_numpy(cls.records(cf, cs).view(np.int32))

    def launch_moments(self, n, d_per_run, d_best_height, d_moments, hist_spec, d_hist, stream=None):
        import torch

        rec = d_per_run[:n].numpy().view(np.uint32)
        assert rec.shape[1] == NC
        spec = (hist_spec.bins, hist_spec.share_shift, hist_spec.rate_shift, hist_spec.share_lo, hist_spec.rate_lo)
        words, hist = host_accumulate(rec[:, :, 0], rec[:, :, 1], d_best_height[:n].numpy().view(np.uint32), spec)
        d_moments.copy_(torch.from_numpy(words.view(np.int64)))
        d_hist.copy_(torch.from_numpy(hist.view(np.int64)))

    def launch_cross(self, n, d_per_run, d_best_height, d_pairs, n_pairs, d_cross, stream=None):
        import torch

        from miningsimulation_amd.contrasts import split_cross

        rec = d_per_run[:n].numpy().view(np.uint32)
        cols = cref.columns([(rec[:, :, 0], rec[:, :, 1], d_best_height[:n].numpy().view(np.uint32))])
        pairs = [tuple(int(x) for x in q) for q in d_pairs.numpy().view(np.uint32)[:n_pairs]]
        words = np.array([split_cross(c) for c in cref.expected(cols, pairs)], dtype=np.uint64)
        d_cross.copy_(torch.from_numpy(words.view(np.int64)))


def _run_fake():
    import torch

    from miningsimulation_amd import HistSpec
    from miningsimulation_amd.distributed import run_sharded_classes

    sim = _FakeSim()
    res = run_sharded_classes(sim, N_TOTAL, 1000, CMAP, NC, pairs=PAIRS, hist=HistSpec(**HSPEC), launch=sim.launch,
                              launch_fold=sim.launch_fold, launch_moments=sim.launch_moments,
                              launch_cross=sim.launch_cross, device=torch.device("cpu"), max_chunk=CHUNK)
    pt = res.points[0]
    sums = [[getattr(x, f) for f, _ in x._fields_] for x in pt.sums]
    return {"moments": pt.moments, "hist": pt.hist.tolist(), "sums": sums, "n_runs": res.n_runs, "cross": res.cross,
            "pairs": [tuple(q) for q in res.pairs]}


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


def test_gloo_world2_run_sharded_classes_matches_world1(msim_lib_path):
    _built()
    want = _run_fake()  # no process group: world 1
    f, s, L = moments_cases.synthetic(N_TOTAL, M_SH, seed=11)
    cf, cs = cls.fold(f, s, CMAP, NC)
    assert not ref.diff(want["moments"], ref.expected(cf, cs, L))
    assert want["hist"] == ref.expected_hist(cf, cs, L, *HSPEC.values()).tolist()
    assert not cref.diff(want["cross"], cref.expected(cref.columns([(cf, cs, L)]), PAIRS))
    assert len(want["sums"]) == M_SH and len(want["moments"]) == NC   # sums per miner, moments per class
    assert [r[0] for r in want["sums"]] == [int(x) for x in f.astype(np.int64).sum(axis=0)]

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
        # ONE all-reduce of sums + status + class moments + class histogram + cross words
        assert calls == [6 * M_SH + 2 + 20 * NC + 2 * (HSPEC["bins"] + 2) * NC + 12 * len(PAIRS)], (rank, calls)

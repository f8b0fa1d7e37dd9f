"""Paired contrasts without a GPU: the struct layouts, msim_cross.h's host accumulation (the lines the gfx950
kernel runs) against tests/cross_reference.py, msim_cross_to_contrasts against fractions, msim_pairs_check, the
pair builders and the report, the sharded path under gloo, and the stand-alone sanitizer build."""
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

import cross_reference as cref
import moments_cases
import moments_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "libcross_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "cross_check")
U32 = 0xFFFFFFFF


def _built():
    """build/libcross_host.so and build/cross_check, built here when missing or older than their sources."""
    import __graft_entry__ as ge

    srcs = [os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_cross.h"),
            os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_moments.h"),
            os.path.join(ROOT, "include", "msim.h"),
            os.path.join(ROOT, "tests", "native", "cross_host.cpp"),
            os.path.join(ROOT, "tests", "native", "cross_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".cross_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_cross_tests()
    return HOST_LIB


def make_data(n_runs, m, points, seed=0):
    """Per point (found, stale, best_height), a different seed per point."""
    return [moments_cases.synthetic(n_runs, m, seed=31 * p + seed) for p in range(points)]


def mixed_pairs(points, m):
    """Pairs across points, across miners of one point, self pairs, a swapped pair and a duplicate."""
    last = points - 1
    pairs = [(last, k, 0, k) for k in range(m)]                     # against a baseline
    pairs += [(0, i, 0, j) for i in range(m) for j in range(i + 1, m)][:7]  # between miners
    pairs += [(p, k, p, k) for p in range(points) for k in range(m)]  # self pairs
    pairs += [(0, 0, last, m - 1), (last, m - 1, 0, 0), (0, 0, last, m - 1)]  # swapped, duplicate
    return pairs


def host_cross(data, pairs):
    """words [n_pairs, 12] uint64 from libcross_host.so over the stacked records of the points."""
    h = ctypes.CDLL(_built())
    rec = np.ascontiguousarray(np.stack([moments_cases.records(f, s) for f, s, _ in data]))
    bh = np.ascontiguousarray(np.stack([L for _, _, L in data]), dtype=np.uint32)
    points, n, m = rec.shape[:3]
    pa = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 4))
    words = np.full((len(pairs), 12), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rc = h.cross_host_accumulate(ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(bh.ctypes.data),
                                 ctypes.c_uint32(points), ctypes.c_uint64(n), ctypes.c_uint32(m),
                                 ctypes.c_void_p(pa.ctypes.data), ctypes.c_uint32(len(pairs)),
                                 ctypes.c_void_p(words.ctypes.data))
    assert rc == 0
    return words


def test_struct_sizes(msim_lib_path):
    from miningsimulation_amd import _lib

    assert ctypes.sizeof(_lib.MsimPair) == 16
    assert ctypes.sizeof(_lib.MsimCross) == 96
    assert ctypes.sizeof(_lib.MsimContrast) == 128
    with open(os.path.join(ROOT, "include", "msim.h")) as f:
        src = f.read()
    # the header's own fields, in order: four uint32, twelve uint64 words, sixteen doubles
    assert "uint32_t point_a, miner_a, point_b, miner_b;" in src
    assert [n for n, _ in _lib.MsimCross._fields_] == ["found_found", "stale_stale", "share_share", "rate_rate"]
    assert [n for n, _ in _lib.MsimContrast._fields_] == list(cref.FIELDS)
    body = src[src.index("typedef struct msim_contrast {"):src.index("} msim_contrast;")]
    assert [w.strip(",;") for ln in body.splitlines()[1:] for w in ln.split()[1:]] == list(cref.FIELDS)


def test_product_is_the_square_for_equal_factors():
    h = ctypes.CDLL(_built())
    vals = [0, 1, U32, 1 << 32, (1 << 64) - (1 << 32), (1 << 64) - 1, 0x123456789ABCDEF, 3 << 40]
    for a in vals:
        for b in vals:
            p = (ctypes.c_uint64 * 4)()
            q = (ctypes.c_uint64 * 4)()
            h.cross_host_pieces(ctypes.c_uint64(a), ctypes.c_uint64(b), p, q)
            assert sum(int(p[i]) << (32 * i) for i in range(4)) == a * b and all(int(x) <= U32 for x in p)
            if a == b:
                assert list(p) == list(q)


@pytest.mark.parametrize("points", [2, 3])
@pytest.mark.parametrize("n_runs", [1, 2, 40, 257])
def test_host_accumulation_equals_reference(msim_lib_path, n_runs, points):
    from miningsimulation_amd.contrasts import cross_from_words

    m = 5
    data = make_data(n_runs, m, points, seed=n_runs)
    pairs = mixed_pairs(points, m)
    words = host_cross(data, pairs)
    want = cref.expected(cref.columns(data), pairs)
    bad = cref.diff(cross_from_words(words), want)
    assert not bad, "\n".join(bad[:10])
    if n_runs >= 40:
        assert max(w["rate_rate"] for w in want) >= 1 << 127  # the 2^128-edge products are in


def test_self_pairs_are_the_square_sums_and_pairs_commute(msim_lib_path):
    """A self pair's cross words equal msim_moments' four square sums word by word (moments_cases' patterns 4 and
    5 put products at the 2^128 edge into them); (a, b) and (b, a) give the same words."""
    from test_moments_host import host_accumulate

    n, m, points = 40, 5, 2
    data = make_data(n, m, points, seed=3)
    pairs = [(p, k, p, k) for p in range(points) for k in range(m)]
    words = host_cross(data, pairs).reshape(points, m, 12)
    for p, (f, s, L) in enumerate(data):
        mom, _ = host_accumulate(f, s, L)
        assert np.array_equal(words[p][:, 0:2], mom[:, 6:8])     # found_sq
        assert np.array_equal(words[p][:, 2:4], mom[:, 8:10])    # stale_sq
        assert np.array_equal(words[p][:, 4:8], mom[:, 12:16])   # share_sq
        assert np.array_equal(words[p][:, 8:12], mom[:, 16:20])  # rate_sq
    ab = [(0, i, 1, j) for i in range(m) for j in range(m)]
    ba = [(1, j, 0, i) for i in range(m) for j in range(m)]
    assert np.array_equal(host_cross(data, ab), host_cross(data, ba))


def test_out_of_range_pairs_contribute_nothing(msim_lib_path):
    data = make_data(9, 3, 2)
    good = [(1, 0, 0, 0), (0, 1, 0, 2), (1, 2, 1, 2)]
    bad = [(2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3), (U32, 0, 0, 0), (0, 0, 0, U32)]
    pairs = [bad[0], good[0], bad[1], bad[2], good[1], bad[3], bad[4], good[2], bad[5]]
    words = host_cross(data, pairs)
    alone = host_cross(data, good)
    assert np.array_equal(words[[1, 4, 7]], alone) and alone.any()
    assert not words[[0, 2, 3, 5, 6, 8]].any()


def _bits(x):
    return struct.pack("<d", x)


def _moments(data):
    return [ref.expected(*d) for d in data]


def test_contrasts_against_fractions(msim_lib_path):
    """Exact numerators, then fewer than eight f64 roundings per field: relative error below 2^-50, bound 1e-13
    (as tests/test_moments_host.py). The synthetic terms reach 2^64 - 2^32, so the ratio's numerator needs the
    full width msim_cross.h derives; a narrower integer type fails here."""
    from miningsimulation_amd import _lib
    from miningsimulation_amd.contrasts import contrasts_from_sums, cross_from_words

    widest = 0
    for n_runs, m, points, seed in ((40, 5, 2, 1), (257, 5, 3, 2), (2, 3, 2, 3)):
        data = make_data(n_runs, m, points, seed=seed)
        pairs = mixed_pairs(points, m)
        words = host_cross(data, pairs)
        mo = _moments(data)
        cross = cross_from_words(words)
        got = contrasts_from_sums(mo, pairs, cross, n_runs)
        for i, q in enumerate(pairs):
            a, b = mo[q[0]][q[1]], mo[q[2]][q[3]]
            want = cref.contrast(a, b, cross[i], n_runs)
            for name in cref.FIELDS:
                err = cref.field_error(name, got[i][name], want[name])
                assert err <= 1e-13, (n_runs, q, name, got[i][name], want[name], err)
            widest = max(widest, (n_runs * (b["share"] ** 2 * a["share_sq"] + a["share"] ** 2 * b["share_sq"])).bit_length())
        # the unnormalised limbs of the accumulation and the normalised ones contrasts_from_sums built: the same bits
        from miningsimulation_amd.moments import split_limbs
        from test_moments_host import host_accumulate

        raw_m = np.concatenate([host_accumulate(*d)[0] for d in data])
        arr = (_lib.MsimMoments * (points * m))()
        ctypes.memmove(arr, raw_m.ctypes.data, 160 * points * m)
        cr = (_lib.MsimCross * len(pairs))()
        ctypes.memmove(cr, words.ctypes.data, 96 * len(pairs))
        pa = (_lib.MsimPair * len(pairs))(*[_lib.MsimPair(*q) for q in pairs])
        out = (_lib.MsimContrast * len(pairs))()
        _lib.lib.msim_cross_to_contrasts(arr, m, pa, cr, len(pairs), n_runs, out)
        for i in range(len(pairs)):
            for name in cref.FIELDS:
                assert _bits(getattr(out[i], name)) == _bits(got[i][name]), (i, name)
        if n_runs >= 40:
            assert any(int(w) >> 32 for w in words[:, 4])  # a limb that normalising does change
            assert any(split_limbs(mo[0][k]) != [int(x) for x in raw_m[k]] for k in range(m))
    assert widest > 256  # the numerators here are far past four 64-bit words


def _two_columns(fa, sa, fb, sb, L):
    """One point, two miners, from hand-made per-run lists."""
    f = np.array([fa, fb], dtype=np.uint32).T.copy()
    s = np.array([sa, sb], dtype=np.uint32).T.copy()
    return [(f, s, np.array(L, dtype=np.uint32))]


def _contrast_of(data, pair=(0, 0, 0, 1)):
    from miningsimulation_amd.contrasts import contrasts_from_sums, cross_from_words

    n = data[0][0].shape[0]
    return contrasts_from_sums(_moments(data), [pair], cross_from_words(host_cross(data, [pair])), n)[0]


def test_contrasts_special_cases(msim_lib_path):
    # N == 1: every error and correlation is NaN, differences and ratios are not
    c = _contrast_of(_two_columns([10], [3], [6], [2], [16]))
    assert all(math.isnan(c[k]) for k in cref.FIELDS if k.endswith("_se") or k.endswith("_corr"))
    assert c["found_diff"] == 4.0 and c["found_ratio"] == 10.0 / 6.0 and c["share_diff"] == 0.25
    # a constant difference between two varying columns: diff_se == 0 exactly, correlation 1
    c = _contrast_of(_two_columns([4, 6, 8, 6], [3, 1, 2, 1], [1, 3, 5, 3], [2, 0, 1, 0], [16, 16, 16, 16]))
    assert c["found_diff"] == 3.0 and c["found_diff_se"] == 0.0 and c["stale_diff_se"] == 0.0
    assert c["share_diff"] == 3.0 / 16.0 and c["share_diff_se"] == 0.0
    assert abs(c["found_corr"] - 1.0) < 1e-15 and c["found_ratio_se"] > 0.0
    # a constant series: no correlation, and against itself no error at all
    c = _contrast_of(_two_columns([6] * 5, [2] * 5, [6] * 5, [2] * 5, [18] * 5))
    assert c["found_diff"] == 0.0 and c["found_diff_se"] == 0.0 and math.isnan(c["found_corr"])
    assert c["found_ratio"] == 1.0 and c["found_ratio_se"] == 0.0 and c["rate_diff_se"] == 0.0
    # B == 0: no ratio (and a zero column does not vary: no correlation)
    c = _contrast_of(_two_columns([4, 6, 8], [1, 0, 2], [0, 0, 0], [0, 0, 0], [12, 12, 12]))
    assert math.isnan(c["found_ratio"]) and math.isnan(c["found_ratio_se"])
    assert math.isnan(c["share_ratio"]) and math.isnan(c["share_ratio_se"]) and math.isnan(c["found_corr"])
    assert c["found_diff"] == 6.0 and c["found_diff_se"] > 0.0
    # perfectly opposed columns: correlation -1 and a difference noisier than either side
    c = _contrast_of(_two_columns([2, 8, 4, 6], [0] * 4, [8, 2, 6, 4], [0] * 4, [10] * 4))
    assert abs(c["found_corr"] + 1.0) < 1e-15 and c["found_diff"] == 0.0
    assert abs(c["found_diff_se"] - math.sqrt(4 * (36 + 36 + 4 + 4) / (16 * 3))) < 1e-14


def test_pairs_check(msim_lib_path):
    from miningsimulation_amd import _lib

    def rc(m, points, pairs):
        arr = (_lib.MsimPair * max(len(pairs), 1))(*[_lib.MsimPair(*q) for q in pairs])
        return _lib.lib.msim_pairs_check(m, points, arr, len(pairs))

    assert rc(3, 2, [(0, 0, 1, 2), (1, 2, 0, 0), (1, 1, 1, 1)]) == _lib.MSIM_OK
    for bad in ((2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3), (U32, 0, 0, 0)):
        assert rc(3, 2, [(0, 0, 1, 2), bad]) == _lib.MSIM_E_INVALID, bad
    assert rc(3, 2, []) == _lib.MSIM_E_INVALID
    assert _lib.lib.msim_pairs_check(3, 2, None, 1) == _lib.MSIM_E_INVALID
    assert rc(0, 2, [(0, 0, 0, 0)]) == _lib.MSIM_E_INVALID and rc(3, 0, [(0, 0, 0, 0)]) == _lib.MSIM_E_INVALID


def test_pair_builders(msim_lib_path):
    from miningsimulation_amd import Pair, pairs_between_miners, pairs_vs_baseline
    from miningsimulation_amd.contrasts import pairs_struct

    assert pairs_vs_baseline(3, 2) == [Pair(1, 0, 0, 0), Pair(1, 1, 0, 1), Pair(2, 0, 0, 0), Pair(2, 1, 0, 1)]
    assert pairs_vs_baseline(3, 2, baseline=1) == [Pair(0, 0, 1, 0), Pair(0, 1, 1, 1), Pair(2, 0, 1, 0), Pair(2, 1, 1, 1)]
    assert pairs_vs_baseline(1, 4) == []
    assert len(pairs_vs_baseline(360, 9)) == 3231
    assert pairs_between_miners(3) == [Pair(0, 0, 0, 1), Pair(0, 0, 0, 2), Pair(0, 1, 0, 2)]
    assert pairs_between_miners(2, point=4) == [Pair(4, 0, 4, 1)]
    assert len(pairs_between_miners(9)) == 36
    with pytest.raises(ValueError):
        pairs_vs_baseline(3, 2, baseline=3)
    arr = pairs_struct(pairs_vs_baseline(3, 2), 3, 2)
    assert (arr[3].point_a, arr[3].miner_a, arr[3].point_b, arr[3].miner_b) == (2, 1, 0, 1)
    for bad in ([], [(3, 0, 0, 0)], [(0, 0, 0, 2)], [(-1, 0, 0, 0)]):
        with pytest.raises(ValueError):
            pairs_struct(bad, 3, 2)


def test_cross_limb_round_trip(msim_lib_path):
    from miningsimulation_amd import join_cross, split_cross

    words = host_cross(make_data(40, 3, 2), mixed_pairs(2, 3))
    for row in words.tolist():
        assert join_cross(split_cross(join_cross(row))) == join_cross(row)
    assert split_cross({"found_found": (5 << 32) + 7, "stale_stale": 1, "share_share": (1 << 130) + 3,
                        "rate_rate": 0}) == [7, 5, 1, 0, 3, 0, 0, 1 << 34, 0, 0, 0, 0]


def test_report_contrasts_hand_made(msim_lib_path):
    from miningsimulation_amd import ContrastResult, Pair, SimulationResult, contrasts, report_contrasts
    from miningsimulation_amd.contrasts import cross_from_words

    # two points of one miner each: found 4, 6, 8, 6 against 2, 4, 8, 2 at L = 16
    data = [(np.array([[4], [6], [8], [6]], dtype=np.uint32), np.array([[1], [0], [2], [1]], dtype=np.uint32),
             np.array([16] * 4, dtype=np.uint32)),
            (np.array([[2], [4], [8], [2]], dtype=np.uint32), np.array([[1], [0], [2], [1]], dtype=np.uint32),
             np.array([16] * 4, dtype=np.uint32))]
    pairs = [Pair(0, 0, 1, 0), Pair(0, 0, 0, 0)]
    mo = _moments(data)

    def result(n):
        cut = [(f[:n], s[:n], L[:n]) for f, s, L in data]
        return ContrastResult(points=[SimulationResult(stats_total=[], sums=[], n_runs=n, moments=m_) for m_ in _moments(cut)],
                              pairs=pairs, cross=cross_from_words(host_cross(cut, pairs)), n_runs=n)

    res = result(4)
    assert res.points[0].moments == mo[0]
    c = contrasts(res)[0]
    # differences 2, 2, 0, 4: mean 2, se = sqrt(8 / 3 / 4); shares differ by the same over 16
    assert c["found_diff"] == 2.0 and abs(c["found_diff_se"] - math.sqrt(8 / 3 / 4)) < 1e-15
    assert c["share_diff"] == 0.125 and c["found_ratio"] == 1.5
    lines = report_contrasts(res).splitlines()
    assert len(lines) == 2
    assert lines[0].startswith("  - Miner 0 of point 0 vs point 1: found +2 ± 0.816497 blocks (corr 0.866), ×1.5 ± ")
    # corr = 12 / sqrt(8 * 24); stale rates 1/4, 0, 1/4, 1/6 against 1/2, 0, 1/4, 1/2: mean difference -7/48
    assert "; share +12.5% ± 5.1031% of blocks (corr 0.866), ×1.5 ± " in lines[0]
    assert "; stale rate -14.5833% ± " in lines[0] and lines[0].endswith(")")
    assert lines[1].startswith("  - Miner 0 of point 0 vs miner 0 of point 0: found +0 ± 0 blocks (corr 1), ×1 ± 0;")
    one = report_contrasts(result(1)).splitlines()[0]
    assert one.startswith("  - Miner 0 of point 0 vs point 1: found +2 ± n/a blocks (corr n/a), ×2 ± n/a;")
    assert one.endswith(" (corr n/a)")


def test_cross_check_under_sanitizers():
    """The product, the accumulation with out-of-range pairs and the contrasts at the extremes, built stand-alone
    with ASan + UBSan: a child process on the CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cross_check: ok" in r.stdout


# ---------------------------------------------------------------- sharded path under gloo
N_TOTAL, M_SH, CHUNK = 29, 4, 6
PAIRS_SH = [(0, i, 0, j) for i in range(M_SH) for j in range(i + 1, M_SH)] + [(0, 2, 0, 2), (0, 3, 0, 0)]


class _FakeSim:
    """Stands in for Simulation on a CPU rank, as tests/test_moments_host.py's: launch fills the records of runs
    [begin, begin + n) of one fixed synthetic data set, launch_moments and launch_cross are the host accumulations."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = moments_cases.synthetic(N_TOTAL, M_SH, seed=7)

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        from test_moments_host import host_accumulate

        assert ws is None and n <= CHUNK
        f, s, L = self.f[begin:begin + n], self.s[begin:begin + n], self.L[begin:begin + n]
        d_per_run[:n] = torch.from_numpy(moments_cases.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        words, _ = host_accumulate(f, s, L)
        sums.copy_(torch.from_numpy(words[:, :6].copy().view(np.int64)))
        status.zero_()

    @staticmethod
    def _chunk(n, d_per_run, d_best_height):
        rec = d_per_run[:n].numpy().view(np.uint32)
        return rec[:, :, 0], rec[:, :, 1], d_best_height[:n].numpy().view(np.uint32)

    def launch_moments(self, n, d_per_run, d_best_height, d_moments, hist_spec, d_hist, stream=None):
        import torch

        from test_moments_host import host_accumulate

        assert hist_spec is None and d_hist is None
        words, _ = host_accumulate(*self._chunk(n, d_per_run, d_best_height))
        d_moments.copy_(torch.from_numpy(words.view(np.int64)))

    def launch_cross(self, n, d_per_run, d_best_height, d_pairs, n_pairs, d_cross, stream=None):
        import torch

        pairs = d_pairs.numpy().view(np.uint32).reshape(-1, 4)
        assert n_pairs == len(PAIRS_SH) and pairs.tolist() == [list(q) for q in PAIRS_SH]
        words = host_cross([self._chunk(n, d_per_run, d_best_height)], pairs)
        d_cross.copy_(torch.from_numpy(words.view(np.int64)))


def _run_fake():
    import torch

    from miningsimulation_amd.distributed import run_sharded_contrasts

    sim = _FakeSim()
    res = run_sharded_contrasts(sim, N_TOTAL, 1000, PAIRS_SH, launch=sim.launch, launch_moments=sim.launch_moments,
                                launch_cross=sim.launch_cross, device=torch.device("cpu"), max_chunk=CHUNK)
    return {"moments": res.points[0].moments, "cross": res.cross, "pairs": [tuple(q) for q in res.pairs],
            "n_runs": (res.n_runs, res.points[0].n_runs)}


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


def test_gloo_world2_run_sharded_contrasts_matches_world1(msim_lib_path):
    _built()
    want = _run_fake()  # no process group: world 1, five chunks
    data = [moments_cases.synthetic(N_TOTAL, M_SH, seed=7)]
    assert not ref.diff(want["moments"], ref.expected(*data[0]))
    assert not cref.diff(want["cross"], cref.expected(cref.columns(data), PAIRS_SH))
    assert want["pairs"] == PAIRS_SH and want["n_runs"] == (N_TOTAL, N_TOTAL)
    with pytest.raises(ValueError):
        from miningsimulation_amd.distributed import run_sharded_contrasts

        run_sharded_contrasts(_FakeSim(), N_TOTAL, 1000, [(1, 0, 0, 0)], device="cpu")  # a sim has one point

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]  # 15 + 14 runs
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res, calls in got:
        assert res == want, rank
        # ONE all-reduce of sums + status + moments + cross words
        assert calls == [6 * M_SH + 2 + 20 * M_SH + 12 * len(PAIRS_SH)], (rank, calls)

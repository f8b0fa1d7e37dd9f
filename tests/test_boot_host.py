"""The bootstrap without a GPU: msim_boot.h's weight function, sequential selection and launch mirrors (the lines the
gfx950 kernels run) against tests/boot_reference.py, the identities with the rank selection and msim_tail_means, split
independence, the ABI's argument checks, the stand-alone sanitizer build and the Python layer's statistics. Every
comparison is exact."""
import ctypes
import fcntl
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import boot_reference as br
import rank_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "libboot_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "boot_check")
U64 = 2**64 - 1
QS = (1e-9, 0.05, 0.5, 1.0)
SEED = 0x5EEDB007


def _built():
    """build/libboot_host.so and build/boot_check (and the rank and tail host libraries the identities use), built
    here when missing or older than their sources."""
    import __graft_entry__ as ge

    csrc = os.path.join(ROOT, "miningsimulation_amd", "csrc")
    srcs = [os.path.join(csrc, h) for h in ("msim_boot.h", "msim_rank.h", "msim_moments.h", "msim_draws.h")] + \
           [os.path.join(ROOT, "include", "msim.h"), os.path.join(ROOT, "tests", "native", "boot_host.cpp"),
            os.path.join(ROOT, "tests", "native", "boot_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".boot_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_boot_tests()
        if not os.path.exists(os.path.join(ROOT, "build", "librank_host.so")):
            ge.build_rank_tests()
        if not os.path.exists(os.path.join(ROOT, "build", "libtail_host.so")):
            ge.build_tail_tests()
    return HOST_LIB


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _host():
    h = ctypes.CDLL(_built())
    h.boot_host_weight.restype = ctypes.c_uint32
    h.boot_host_weight.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    h.boot_host_weight_sum.restype = ctypes.c_uint64
    h.boot_host_weight_sum.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    h.boot_host_threshold_weight.restype = ctypes.c_uint32
    h.boot_host_threshold_weight.argtypes = [ctypes.c_uint32]
    h.boot_host_rank.restype = ctypes.c_uint64
    h.boot_host_rank.argtypes = [ctypes.c_uint64, ctypes.c_double]
    h.boot_host_workspace_words.restype = ctypes.c_uint64
    for fn in (h.boot_host_select, h.boot_host_select_keys, h.boot_host_select_split):
        fn.restype = ctypes.c_longlong
    return h


def synthetic_points(p, n, m, seed=0):
    """f, s [P, n, M] and L [P, n]: rank_reference.synthetic per point, the patterns shifted from point to point."""
    pts = [rr.synthetic(n, m, shift=(3 * k + seed) % 9 if m < 9 else k, seed=seed + k) for k in range(p)]
    return (np.stack([x[0] for x in pts]), np.stack([x[1] for x in pts]), np.stack([x[2] for x in pts]))


def all_items(p, m):
    """Every (point, column, quantity), the quantile index cycling over QS."""
    return [(pt, k, q, (pt + k + q) % len(QS)) for pt in range(p) for k in range(m) for q in range(4)]


def item_words(items):
    return np.ascontiguousarray(np.asarray(items, dtype=np.uint32).reshape(-1, 4))


def host_select(f, s, L, items, B, seed=SEED, run_begin=0, qs=QS):
    """(W list, rows [n_items][B] of 5-tuples) from libboot_host.so; the outputs start 0xFF-filled."""
    h = _host()
    p, n, m = f.shape
    rec = np.ascontiguousarray(np.stack([f, s], axis=-1).astype(np.uint32))
    bh = np.ascontiguousarray(L, dtype=np.uint32)
    iw, q = item_words(items), np.asarray(qs, dtype=np.float64)
    W = np.full(B, U64, dtype=np.uint64)
    rows = np.full((len(items), B, 5), U64, dtype=np.uint64)
    rc = h.boot_host_select(_vp(rec), _vp(bh), ctypes.c_uint32(p), ctypes.c_uint64(run_begin), ctypes.c_uint64(n),
                            ctypes.c_uint32(m), _vp(iw), ctypes.c_uint32(len(items)), _vp(q), ctypes.c_uint32(len(qs)),
                            ctypes.c_uint32(B), ctypes.c_uint64(seed), _vp(W), _vp(rows))
    assert rc == 0, rc
    return W.tolist(), rows.tolist()


def reference(f, s, L, items, B, seed=SEED, run_begin=0, qs=QS):
    return br.bootstrap([br.point_keys(f[k], s[k], L[k]) for k in range(f.shape[0])], items, qs, B, seed, run_begin)


def test_thresholds_from_decimal():
    assert br.thresholds() == br.T
    h = _host()
    for k, t in enumerate(br.T):
        assert h.boot_host_threshold_weight(t) == k + 1
        assert h.boot_host_threshold_weight(t - 1) == k
    assert h.boot_host_threshold_weight(0) == 0 and h.boot_host_threshold_weight(2**32 - 1) == 13


def test_weight_function_equals_reference():
    h = _host()
    for seed in (0, 1, SEED, U64, 0x0123456789ABCDEF):
        for b in (0, 1, 2, 3, 10, 11, 4095):  # 2/3 and 10/11 are odd/even pairs sharing b >> 1
            for run in (0, 1, 2**32 - 1, 2**32, 2**63, U64) + tuple(range(100, 140)):
                assert h.boot_host_weight(seed, b, run) == br.weight(seed, b, run), (seed, b, run)
    assert all(h.boot_host_weight(SEED, 0, r) == 1 for r in range(50))
    # a pair draws the two halves of one word: the same constant, different weights somewhere
    assert any(br.weight(SEED, 10, r) != br.weight(SEED, 11, r) for r in range(50))


def test_weight_mean_is_one():
    """2^20 weights of one replicate: Poisson(1) has variance 1, so the mean lies within 6 / sqrt(n) of 1. The
    outcome is deterministic (checked on the CPU: the sum is within a few hundred of 2^20)."""
    n = 1 << 20
    total = _host().boot_host_weight_sum(SEED, 5, n)
    assert abs(total / n - 1.0) < 6.0 / n ** 0.5, total
    assert sum(br.weight(SEED, 5, r) for r in range(4096)) == _host().boot_host_weight_sum(SEED, 5, 4096)


def test_rank_is_quantile_rank(msim_lib_path):
    from miningsimulation_amd import quantile_rank
    from miningsimulation_amd.bootstrap import BOOT_EMPTY, boot_rank

    h = _host()
    for W in list(range(1, 60)) + [257, 13 << 20, (13 << 28) - 1]:
        for q in (0.0, 1e-9, 0.05, 0.5, 0.95, 1.0):
            assert h.boot_host_rank(W, q) == quantile_rank(W, q) == br.quantile_rank(W, q) == boot_rank(W, q), (W, q)
    assert h.boot_host_rank(0, 0.5) == BOOT_EMPTY == boot_rank(0, 0.5) == U64


SHAPES = [(1, 1, 1, 65), (2, 2, 1, 33), (3, 3, 3, 65), (3, 8, 1, 33), (64, 5, 1, 2), (64, 9, 3, 1), (64, 7, 1, 65),
          (257, 9, 1, 33), (257, 4, 3, 65), (257, 6, 1, 2)]
_CASES = {}


def case(n, m, p, B):
    if (n, m, p, B) not in _CASES:
        f, s, L = synthetic_points(p, n, m, seed=n + m)
        items = all_items(p, m)
        _CASES[(n, m, p, B)] = (f, s, L, items, host_select(f, s, L, items, B), reference(f, s, L, items, B))
    return _CASES[(n, m, p, B)]


@pytest.mark.parametrize("n,m,p,B", SHAPES)
def test_host_selection_equals_reference(n, m, p, B):
    f, s, L, items, (W, rows), (W_ref, rows_ref) = case(n, m, p, B)
    assert W == W_ref and W[0] == n
    miss = br.diff_rows(rows, rows_ref)
    assert not miss, miss[:8]
    for i, it in enumerate(items):
        for b in range(B):
            v, below, equal, _, _ = rows[i][b]
            if W[b]:
                assert below <= br.quantile_rank(W[b], QS[it[3]]) < below + equal


@pytest.mark.parametrize("n,m,p,B", [c for c in SHAPES if c[0] <= 3])
def test_empty_replicates_are_exactly_the_references(n, m, p, B):
    _, _, _, items, (W, rows), (W_ref, rows_ref) = case(n, m, p, B)
    empty = {(i, b) for i in range(len(items)) for b in range(B) if rows[i][b][2] == 0}
    assert empty == {(i, b) for i in range(len(items)) for b in range(B) if W_ref[b] == 0}
    assert empty, "the fixed seed gives empty replicates at 1 to 3 runs"
    assert all(rows[i][b] == [0, 0, 0, 0, 0] for i, b in empty)
    assert all(b != 0 for _, b in empty)


def test_all_equal_column():
    """Pattern 1 of rank_reference.synthetic is (6, 2) in every run: below = 0 and equal = W_b on found, stale, rate."""
    f, s, L, items, (W, rows), _ = case(257, 9, 1, 33)
    assert (f[0, :, 1] == 6).all() and (s[0, :, 1] == 2).all()
    for i, it in enumerate(items):
        if it[1] == 1 and it[2] in (0, 1, 3):
            for b in range(33):
                assert rows[i][b][1] == 0 and rows[i][b][2] == W[b] and rows[i][b][3:] == [0, 0]


def test_extreme_keys():
    """Raw keys 0 and 2^64 - 1 through the header's selection, and the largest key a record gives."""
    h = _host()
    n, B = 65, 33
    keys = np.where(np.arange(n) % 2 == 0, 0, U64).astype(np.uint64)
    q = np.asarray(QS, dtype=np.float64)
    W = np.zeros(B, dtype=np.uint64)
    rows = np.full((len(QS), B, 5), U64, dtype=np.uint64)
    assert h.boot_host_select_keys(_vp(keys), ctypes.c_uint64(n), ctypes.c_uint32(3), _vp(q), ctypes.c_uint32(len(QS)),
                                   ctypes.c_uint32(B), ctypes.c_uint64(SEED), _vp(W), _vp(rows)) == 0
    want = []
    for j in range(len(QS)):
        wts = [br.weights(SEED, b, 0, n) for b in range(B)]
        want.append([br.select_weighted(keys.tolist(), wts[b], br.quantile_rank(sum(wts[b]), QS[j])) for b in range(B)])
    assert not br.diff_rows(rows.tolist(), want)
    assert {r[0] for r in rows[3].tolist()} == {U64} and {r[0] for r in rows[0].tolist()} == {0}
    assert all(r[3] == 0 and r[4] == 0 for r in rows[3].tolist())  # only zeros lie below 2^64 - 1
    f, s, L = br.extreme_columns(65)
    items = [(0, k, qu, 3) for k in range(3) for qu in range(4)]
    Wh, rh = host_select(f[None], s[None], L[None], items, 33)
    Wr, rf = reference(f[None], s[None], L[None], items, 33)
    assert Wh == Wr and not br.diff_rows(rh, rf)
    assert rh[2 * 4 + 3][0][0] == 2**64 - 2**32 and rh[1 * 4 + 0][0][0] == 2**32 - 1


def test_replicate_zero_is_the_order_statistic_and_the_tail_mean():
    """Replicate 0 against librank_host.so's selection and libtail_host.so's msim_tail_means on the same records."""
    n, m = 257, 9
    f, s, L, items, (W, rows), _ = case(n, m, 1, 33)
    hr = ctypes.CDLL(os.path.join(ROOT, "build", "librank_host.so"))
    hr.rank_host_select.restype = ctypes.c_longlong
    ht = ctypes.CDLL(os.path.join(ROOT, "build", "libtail_host.so"))
    rec = rr.records(f[0], s[0])
    bh = np.ascontiguousarray(L[0], dtype=np.uint32)
    ranks = np.asarray([br.quantile_rank(n, q) for q in QS], dtype=np.uint64)
    order = np.zeros((m, 4, len(QS), 3), dtype=np.uint64)
    assert hr.rank_host_select(_vp(rec), _vp(bh), ctypes.c_uint64(n), ctypes.c_uint32(m), _vp(ranks),
                               ctypes.c_uint32(len(QS)), _vp(order)) == 0
    tail_items = np.zeros((len(items), 8), dtype=np.uint32)
    for i, (_, k, qu, qi) in enumerate(items):
        v = rows[i][0][0]
        assert rows[i][0][:3] == order[k, qu, qi].tolist()
        tail_items[i] = (0, k, qu, 0, k, 0, v & 0xFFFFFFFF, v >> 32)
    tails = np.zeros((len(items), 42), dtype=np.uint64)
    assert ht.tail_host_accumulate(_vp(rec[None].copy()), _vp(bh), ctypes.c_uint32(1), ctypes.c_uint64(n),
                                   ctypes.c_uint32(m), _vp(tail_items), ctypes.c_uint32(len(items)), _vp(tails)) == 0
    ht.tail_host_means.restype = ctypes.c_int
    for i, (_, k, qu, qi) in enumerate(items):
        out = (ctypes.c_double * 4)()
        kk = int(ranks[qi]) + 1
        assert ht.tail_host_means(ctypes.c_void_p(tails[i].ctypes.data), None, ctypes.c_uint64(n), ctypes.c_uint64(kk), 0,
                                  out) == 0
        es = br.shortfall(tuple(rows[i][0]), W[0], QS[qi])
        assert float(es) * (1.0 if qu < 2 else 2.0 ** -32) == out[qu], (i, es, out[qu])


@pytest.mark.parametrize("n,m,p,B,cut", [(257, 5, 1, 33, 100), (64, 3, 3, 65, 1), (3, 2, 1, 33, 2)])
def test_split_independence_from_a_dirty_workspace(n, m, p, B, cut):
    """The mirrors of begin, count, step and below over two buffers, from a 0xFF-filled workspace, equal one buffer's
    selection, and a run_begin past 2^32 shifts nothing but the weights."""
    h = _host()
    f, s, L = synthetic_points(p, n, m, seed=cut)
    items = all_items(p, m)
    for run_begin in (0, 2**40 + 7):
        W1, rows1 = host_select(f, s, L, items, B, run_begin=run_begin)
        recs = [np.ascontiguousarray(np.stack([f[:, a:b], s[:, a:b]], axis=-1).astype(np.uint32))
                for a, b in ((0, cut), (cut, n))]
        bhs = [np.ascontiguousarray(L[:, a:b], dtype=np.uint32) for a, b in ((0, cut), (cut, n))]
        ws = np.full(int(h.boot_host_workspace_words(len(items), B)), U64, dtype=np.uint64)
        W = np.full(B, U64, dtype=np.uint64)
        rows = np.full((len(items), B, 5), U64, dtype=np.uint64)
        iw, q = item_words(items), np.asarray(QS, dtype=np.float64)
        rc = h.boot_host_select_split(_vp(recs[0]), _vp(bhs[0]), ctypes.c_uint64(cut), _vp(recs[1]), _vp(bhs[1]),
                                      ctypes.c_uint64(n - cut), ctypes.c_uint32(p), ctypes.c_uint64(run_begin),
                                      ctypes.c_uint32(m), _vp(iw), ctypes.c_uint32(len(items)), _vp(q),
                                      ctypes.c_uint32(len(QS)), ctypes.c_uint32(B), ctypes.c_uint64(SEED), _vp(ws), _vp(W),
                                      _vp(rows))
        assert rc == 0
        assert W.tolist() == W1 and rows.tolist() == rows1
        Wr, rr_ = reference(f, s, L, items, B, run_begin=run_begin)
        assert W1 == Wr and not br.diff_rows(rows1, rr_)
    rec = recs[0]
    assert h.boot_host_unprepared_is_noop(_vp(rec), _vp(bhs[0]), ctypes.c_uint64(cut), ctypes.c_uint32(m),
                                          ctypes.c_uint32(len(items)), ctypes.c_uint32(B), ctypes.c_uint64(U64)) == 1
    assert h.boot_host_unprepared_is_noop(_vp(rec), _vp(bhs[0]), ctypes.c_uint64(cut), ctypes.c_uint32(m),
                                          ctypes.c_uint32(len(items)), ctypes.c_uint32(B), ctypes.c_uint64(0)) == 1


def test_boot_check_under_sanitizers():
    """The weight, rank, layout, selection and mirrors built stand-alone with ASan + UBSan: a child process on the
    CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boot_check: ok" in r.stdout


def test_struct_and_constants(msim_lib_path):
    from miningsimulation_amd import _lib, bootstrap

    assert ctypes.sizeof(_lib.MsimBootItem) == 16 and ctypes.sizeof(_lib.MsimBootRow) == 40
    assert (bootstrap.MAX_BOOT_REPLICATES, bootstrap.MAX_BOOT_ITEMS, bootstrap.BOOT_MAX_RUNS) == (4096, 65535, 1 << 28)
    with open(os.path.join(ROOT, "include", "msim.h")) as fh:
        src = fh.read()
    assert "#define MSIM_MAX_BOOT_REPLICATES 4096u" in src and "#define MSIM_MAX_BOOT_ITEMS 65535u" in src
    assert "#define MSIM_BOOT_MAX_RUNS (1ull << 28)" in src and "MSIM_BOOT_TEST_WG_RUNS" in src
    words = int(_host().boot_host_workspace_words(37, 65))
    assert bootstrap.boot_workspace_bytes(37, 65) == 8 * words
    off, cnt = bootstrap.boot_counts_view(37, 65)
    assert off % 256 == 0 and cnt == 37 * 65 * 256 and off + 8 * cnt == 8 * words


def test_argument_checks(msim_lib_path):
    """Every refusal of the new ABI returns MSIM_E_INVALID before anything touches a device."""
    from miningsimulation_amd import Simulation, _lib, setup_miners
    from miningsimulation_amd._lib import MsimBootItem, lib

    INV = _lib.MSIM_E_INVALID
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused first
    item = (MsimBootItem * 1)(MsimBootItem(0, 0, 2, 0))
    ranks = (ctypes.c_uint64 * 2)(0, 0)
    big = 1 << 40
    assert lib.msim_boot_workspace_bytes(0, 1) == 0 and lib.msim_boot_workspace_bytes(1, 0) == 0
    assert lib.msim_boot_workspace_bytes(65536, 1) == 0 and lib.msim_boot_workspace_bytes(1, 4097) == 0
    assert lib.msim_boot_workspace_bytes(65535, 4096) > 0
    off, words = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.msim_boot_counts_view(0, 1, ctypes.byref(off), ctypes.byref(words)) == INV
    assert lib.msim_boot_counts_view(1, 1, None, ctypes.byref(words)) == INV
    assert lib.msim_boot_counts_view(1, 1, ctypes.byref(off), None) == INV
    # items
    assert lib.msim_boot_items_check(3, 2, 1, item, 1) == 0
    assert lib.msim_boot_items_check(3, 2, 1, None, 1) == INV and lib.msim_boot_items_check(3, 2, 1, item, 0) == INV
    assert lib.msim_boot_items_check(3, 2, 0, item, 1) == INV and lib.msim_boot_items_check(3, 2, 33, item, 1) == INV
    for bad in ((2, 0, 2, 0), (0, 3, 2, 0), (0, 0, 4, 0), (0, 0, 2, 1)):
        assert lib.msim_boot_items_check(3, 2, 1, (MsimBootItem * 1)(MsimBootItem(*bad)), 1) == INV, bad
    # weights
    for seed, rb, runs, B, w in ((1, 0, 0, 2, one), (1, 0, 1 << 32, 2, one), (1, 0, 5, 0, one), (1, 0, 5, 4097, one),
                                 (1, 0, 5, 2, None)):
        assert lib.msim_boot_weights_launch(seed, rb, runs, B, w, None) == INV
    # begin
    for m, np_, it, ni, B, rk, nq, ws, wsb in (
            (0, 1, item, 1, 2, ranks, 1, one, big), (3, 0, item, 1, 2, ranks, 1, one, big),
            (3, 65536, item, 1, 2, ranks, 1, one, big), (3, 1, None, 1, 2, ranks, 1, one, big),
            (3, 1, item, 0, 2, ranks, 1, one, big), (3, 1, item, 1, 0, ranks, 1, one, big),
            (3, 1, item, 1, 4097, ranks, 1, one, big), (3, 1, item, 1, 2, None, 1, one, big),
            (3, 1, item, 1, 2, ranks, 0, one, big), (3, 1, item, 1, 2, ranks, 33, one, big),
            (3, 1, item, 1, 2, ranks, 1, None, big),
            (3, 1, item, 1, 2, ranks, 1, one, lib.msim_boot_workspace_bytes(1, 2) - 1),
            (1, 1, (MsimBootItem * 1)(MsimBootItem(0, 1, 2, 0)), 1, 2, ranks, 1, one, big)):
        assert lib.msim_boot_begin_launch(m, np_, it, ni, B, rk, nq, ws, wsb, None) == INV
    # count and below
    ok = dict(m=3, np_=1, runs=5, rec=one, bh=one, ni=1, B=2, p=0, ws=one, wsb=big, rows=one)
    for k, v in (("m", 0), ("np_", 0), ("np_", 65536), ("runs", 0), ("runs", 1 << 32), ("rec", None), ("bh", None),
                 ("ni", 0), ("ni", 65536), ("B", 0), ("B", 4097), ("p", 8), ("ws", None),
                 ("wsb", lib.msim_boot_workspace_bytes(1, 2) - 1), ("rows", None)):
        a = dict(ok, **{k: v})
        if k != "rows":
            assert lib.msim_boot_count_launch(a["m"], a["np_"], 1, 0, a["runs"], a["rec"], a["bh"], a["ni"], a["B"], a["p"],
                                              a["ws"], a["wsb"], None) == INV, (k, v)
        if k != "p":
            assert lib.msim_boot_below_launch(a["m"], a["np_"], 1, 0, a["runs"], a["rec"], a["bh"], a["ni"], a["B"], a["ws"],
                                              a["wsb"], a["rows"], None) == INV, (k, v)
    # step
    for ni, B, p, ws, wsb, out, st in ((0, 2, 0, one, big, one, one), (1, 0, 0, one, big, one, one),
                                       (1, 2, 8, one, big, one, one), (1, 2, 0, None, big, one, one),
                                       (1, 2, 0, one, 8, one, one), (1, 2, 7, one, big, None, one),
                                       (1, 2, 0, one, big, one, None)):
        assert lib.msim_boot_step_launch(ni, B, p, ws, wsb, out, st, None) == INV
    # the drivers: 2^28 runs, and everything else they validate, before a device is chosen
    sim = Simulation(setup_miners())
    m = len(sim.miners)
    st, su = (_lib.MsimStats * m)(), (_lib.MsimSums * m)()
    order, W, rows = (_lib.MsimOrderStat * (m * 4))(), (ctypes.c_uint64 * 2)(), (_lib.MsimBootRow * 2)()
    q, r0 = (ctypes.c_double * 1)(0.05), (ctypes.c_uint64 * 1)(0)

    def run(n_runs=100, items=item, ni=1, qs=q, nq=1, B=2, W_=W, rows_=rows):
        return lib.msim_run_bootstrap(sim._h, 0, n_runs, 1, 0, None, 0, r0, 1, items, ni, qs, nq, B, 7, st, su, order, W_,
                                      rows_)

    assert run(n_runs=1 << 28) == INV and run(n_runs=(1 << 28) + 5) == INV
    assert run(items=None) == INV and run(ni=0) == INV and run(qs=None) == INV and run(nq=0) == INV
    assert run(B=0) == INV and run(B=4097) == INV and run(W_=None) == INV and run(rows_=None) == INV
    assert run(qs=(ctypes.c_double * 1)(1.5)) == INV and run(qs=(ctypes.c_double * 1)(float("nan"))) == INV
    assert run(items=(MsimBootItem * 1)(MsimBootItem(0, m, 2, 0))) == INV
    assert lib.msim_run_bootstrap(None, 0, 100, 1, 0, None, 0, r0, 1, item, 1, q, 1, 2, 7, st, su, order, W, rows) == INV
    assert lib.msim_sweep_run_bootstrap(None, 0, 100, 1, 0, None, 0, r0, 1, item, 1, q, 1, 2, 7, st, su, order, W, rows) == INV
    with pytest.raises(ValueError):
        sim.run_bootstrap(1 << 28)
    with pytest.raises(ValueError):
        sim.run_bootstrap(100, replicates=4097)
    with pytest.raises(ValueError):
        sim.run_bootstrap(100, qs=(1.5,))
    with pytest.raises(ValueError):
        sim.run_bootstrap(100, items=[(0, m, 2, 0)])


def test_python_statistics_equal_reference(msim_lib_path):
    """se, shortfall_se, interval and difference of BootstrapResult against the reference; the squared standard errors
    are compared exactly as Fractions."""
    import math

    from miningsimulation_amd import bootstrap

    for (n, m, p, B) in ((257, 4, 3, 65), (3, 3, 3, 65)):
        f, s, L, items, (W, rows), _ = case(n, m, p, B)
        res = bootstrap.make_result([None] * p, [br.quantile_rank(n, q) for q in QS], QS, [[]] * p, n,
                                    [bootstrap.BootItem(*it) for it in items], B, SEED, W,
                                    np.asarray(rows, dtype=np.uint64))
        assert res.W == W and res.rows.shape == (len(items), B, 5)
        for i, it in enumerate(items):
            vals = [None if r[2] == 0 else r[0] for r in rows[i]]
            es = [br.shortfall(tuple(r), W[b], QS[it[3]]) for b, r in enumerate(rows[i])]
            assert res.values(i) == vals and res.shortfalls(i) == es
            assert res.n_empty(i) == sum(1 for w in W if w == 0)
            assert res.variance(i) == br.variance(vals) and res.variance(i, shortfall=True) == br.variance(es)
            assert res.se(i) == math.sqrt(float(br.variance(vals)))
            assert res.shortfall_se(i) == math.sqrt(float(br.variance(es)))
            for level in (0.5, 0.9, 0.95):
                assert res.interval(i, level) == br.interval(vals, level)
                assert res.interval(i, level, shortfall=True) == br.interval(es, level)
        # the same column and quantity at two points: paired replicates
        i = items.index((0, 1, 2, (0 + 1 + 2) % 4))
        j = items.index((2, 1, 2, (2 + 1 + 2) % 4))
        for sf in (False, True):
            xs = res.shortfalls(i) if sf else res.values(i)
            ys = res.shortfalls(j) if sf else res.values(j)
            d = res.difference(i, j, 0.9, shortfall=sf)
            d0, diffs, var, iv = br.difference(xs, ys, 0.9)
            assert (d.data, d.diffs, d.variance, d.interval) == (d0, diffs, var, iv)
            assert d.se == math.sqrt(float(var)) and len(diffs) == B - 1 - sum(1 for w in W[1:] if w == 0)
    assert bootstrap.own_bootstrap(2, 3, "rate", 1) == [bootstrap.BootItem(pt, k, 3, 1) for pt in range(2) for k in range(3)]
    assert bootstrap.across_points(4, [0, 2]) == [bootstrap.BootItem(0, 4, 2, 0), bootstrap.BootItem(2, 4, 2, 0)]
    with pytest.raises(ValueError):
        bootstrap.sample_variance([1])

"""Tail statistics without a GPU: msim_tail.h's sequential host accumulation (the lines the gfx950 kernel runs), the
sides and the means against tests/tail_reference.py on rank_reference.synthetic records, the identities between them,
the ABI's argument checks and the stand-alone sanitizer build. Every comparison is exact unless said otherwise."""
import ctypes
import fcntl
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import moments_reference as ref
import tail_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "libtail_host.so")
CHECK_BIN = os.path.join(ROOT, "build", "tail_check")
U64 = 2**64 - 1


def _built():
    """build/libtail_host.so and build/tail_check, built here when missing or older than their sources."""
    import __graft_entry__ as ge

    srcs = [os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_tail.h"),
            os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_moments.h"),
            os.path.join(ROOT, "include", "msim.h"),
            os.path.join(ROOT, "tests", "native", "tail_host.cpp"),
            os.path.join(ROOT, "tests", "native", "tail_check.cpp")]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".tail_tests.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (HOST_LIB, CHECK_BIN)
        if not all(os.path.exists(p) for p in outs) or \
                min(os.path.getmtime(p) for p in outs) < max(os.path.getmtime(p) for p in srcs):
            ge.build_tail_tests()
    return HOST_LIB


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _host():
    h = ctypes.CDLL(_built())
    for fn in (h.tail_host_accumulate, h.tail_host_accumulate_add, h.tail_host_items_check, h.tail_host_side,
               h.tail_host_means):
        fn.restype = ctypes.c_int
    h.tail_host_div.restype = ctypes.c_double
    h.tail_host_div.argtypes = [ctypes.c_uint64] * 4
    return h


def host_tails(f, s, L, items, fn="tail_host_accumulate", out=None):
    """[n_items, 42] uint64 from libtail_host.so; f, s [P, n, M], L [P, n]."""
    h = _host()
    p, n, m = f.shape
    rec = np.ascontiguousarray(np.stack([f, s], axis=-1).astype(np.uint32))
    bh = np.ascontiguousarray(L, dtype=np.uint32)
    iw = tr.item_words(items)
    if out is None:
        out = np.full((len(items), tr.WORDS), U64, dtype=np.uint64)
    rc = getattr(h, fn)(_vp(rec), _vp(bh), ctypes.c_uint32(p), ctypes.c_uint64(n), ctypes.c_uint32(m), _vp(iw),
                        ctypes.c_uint32(len(items)), _vp(out))
    assert rc == 0
    return out


make_items = tr.make_items


SHAPES = [(n, m, p) for n in (1, 2, 65, 257) for m in (1, 3, 9) for p in (1, 3)]
_CASES = {}


def case(n, m, p):
    """(f, s, L, reference, items, host words) of one shape, computed once."""
    if (n, m, p) not in _CASES:
        f, s, L = tr.synthetic_points(p, n, m, shift=(n + 2 * m) % 9 if m < 9 else 0, seed=n + m)
        r = tr.Reference(f, s, L)
        items = make_items(r)
        got = host_tails(f, s, L, items)
        got.setflags(write=False)
        _CASES[(n, m, p)] = (f, s, L, r, items, got)
    return _CASES[(n, m, p)]


def test_struct_and_constants(msim_lib_path):
    from miningsimulation_amd import _lib, tails

    assert ctypes.sizeof(_lib.MsimTailItem) == 32 and ctypes.sizeof(_lib.MsimTail) == 42 * 8
    assert ctypes.sizeof(_lib.MsimTailSpec) == 24 and _lib.MsimTailItem.value.offset == 24
    assert tails.TAIL_WORDS == 42 and tails.MAX_TAIL_ITEMS == 65535 * 128
    with open(os.path.join(ROOT, "include", "msim.h")) as fh:
        src = fh.read()
    assert "#define MSIM_MAX_TAIL_ITEMS 8388480u" in src and "MSIM_TAIL_TEST_WG_RUNS" in src
    assert "enum { MSIM_TAIL_BELOW, MSIM_TAIL_AT_MOST, MSIM_TAIL_ABOVE, MSIM_TAIL_AT_LEAST }" in src


def test_cases_hold_every_extreme():
    f, s, L, r, items, _ = case(257, 9, 3)
    assert (f[0, :, 1] == 6).all() and len(set(r.keys[0][3][:, 1].tolist())) == 1          # the all-equal column
    assert (L[0] == 0).sum() == 51 and (f[0, L[0] == 0, 4] == 5).all()                      # L == 0 with f > 0
    assert int(r.keys[0][3][:, 3].max()) == 2**64 - 2**32
    med = tr.thresholds(r.keys[0][0][:, 4])[2]                                              # a heavily tied median
    assert int((r.keys[0][0][:, 4] == med).sum()) == 257
    assert any(it[0] != it[3] for it in items) and any(it[6] == U64 for it in items) and any(it[6] == 0 for it in items)
    assert {it[2] for it in items if tr.item_ok(it, 3, 9)} == {0, 1, 2, 3}


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_host_accumulation_equals_reference(n, m, p):
    f, s, L, r, items, got = case(n, m, p)
    bad = tr.diff(got.tolist(), r.all_words(items))
    assert not bad, bad[:8]
    for it, row in zip(items, got.tolist()):
        if not tr.item_ok(it, p, m):
            assert row == [0] * 42, it
        elif it[6] == 0:
            assert row[0] == 0 and row[2:22] == [0] * 20                   # nothing lies below 0
        elif it[6] == U64:
            assert row[0] + row[1] == n


def test_items_check(msim_lib_path):
    from miningsimulation_amd import _lib

    h = _host()
    _, _, _, r, items, _ = case(65, 3, 3)
    good = [it for it in items if tr.item_ok(it, 3, 3)]
    as_ptr = (lambda w: ctypes.cast(_vp(w), ctypes.POINTER(_lib.MsimTailItem)))
    w = tr.item_words(good)
    assert _lib.lib.msim_tail_items_check(3, 3, as_ptr(w), len(good)) == _lib.MSIM_OK
    assert h.tail_host_items_check(ctypes.c_uint32(3), ctypes.c_uint32(3), _vp(w), ctypes.c_uint32(len(good))) == 0
    assert _lib.lib.msim_tail_items_check(3, 3, as_ptr(w), 0) == _lib.MSIM_E_INVALID
    assert _lib.lib.msim_tail_items_check(3, 3, None, 1) == _lib.MSIM_E_INVALID
    assert _lib.lib.msim_tail_items_check(3, 3, as_ptr(w), 65535 * 128 + 1) == _lib.MSIM_E_INVALID
    for it in (x for x in items if not tr.item_ok(x, 3, 3)):
        w = tr.item_words(good[:2] + [it] + good[2:4])
        assert _lib.lib.msim_tail_items_check(3, 3, as_ptr(w), 5) == _lib.MSIM_E_INVALID, it
        assert h.tail_host_items_check(ctypes.c_uint32(3), ctypes.c_uint32(3), _vp(w), ctypes.c_uint32(5)) == -1


def _c_side(fn, row, total, n, side):
    """(20 words, count) from msim_tail_side / tail_host_side, or the error code."""
    t = np.asarray(row, dtype=np.uint64)
    tot = np.asarray(total, dtype=np.uint64) if total is not None else None
    out, cnt = np.zeros(20, dtype=np.uint64), ctypes.c_uint64(7)
    rc = fn(_vp(t), _vp(tot) if tot is not None else None, ctypes.c_uint64(n), ctypes.c_int(side), _vp(out),
            ctypes.byref(cnt))
    return (out.tolist(), int(cnt.value)) if rc == 0 else rc


def _c_means(fn, row, total, n, k, upper):
    t, tot = np.asarray(row, dtype=np.uint64), np.asarray(total, dtype=np.uint64)
    out = np.zeros(4, dtype=np.float64)
    rc = fn(_vp(t), _vp(tot), ctypes.c_uint64(n), ctypes.c_uint64(k), ctypes.c_int(int(upper)), _vp(out))
    return out.tolist() if rc == 0 else rc


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_sides_and_means(msim_lib_path, n, m, p):
    """msim_tail_side and msim_tail_means (libmsim.so, host only) and the same functions of libtail_host.so against
    the reference; below + equal + above is the total; the own-column mean is the expected shortfall; k outside the
    tie range is refused."""
    lib = ctypes.CDLL(msim_lib_path)
    lib.msim_tail_side.restype = lib.msim_tail_means.restype = ctypes.c_int
    h = _host()
    f, s, L, r, items, got = case(n, m, p)
    rows = got.tolist()
    step = 1 if n * m * p < 400 else 7  # every item of the small shapes, a spread of the large ones
    for it, row in list(zip(items, rows))[::step]:
        if not tr.item_ok(it, p, m):
            continue
        total = r.total(it[3], it[4])
        want = tr.sides(row, total, n)
        for side, name in enumerate(tr.SIDES):
            for fn in (lib.msim_tail_side, h.tail_host_side):
                assert _c_side(fn, row, total, n, side) == (want[name][0], want[name][1]), (it, name)
        b, e, a = tr.join(want["below"][0]), tr.join(row[22:42]), tr.join(want["above"][0])
        assert {k: b[k] + e[k] + a[k] for k in b} == tr.join(total)
        assert want["below"][1] + row[1] + want["above"][1] == n
        assert _c_side(lib.msim_tail_side, row, None, n, 2) == -1 and _c_side(lib.msim_tail_side, row, None, n, 0) != -1
        assert _c_side(lib.msim_tail_side, row, total, n, 4) == -1
        nb, ne = row[0], row[1]
        for upper in (False, True):
            n_strict = n - nb - ne if upper else nb
            for k in ({n_strict + 1, n_strict + (ne + 1) // 2, n_strict + ne} if ne else ()):
                wantk = tr.mean_k(row, total, n, k, upper)
                for fn in (lib.msim_tail_means, h.tail_host_means):
                    assert _c_means(fn, row, total, n, k, upper) == [float(x) for x in wantk], (it, k, upper)
                if not upper and it[:2] == it[3:5]:  # the target is the condition's own column: expected shortfall
                    q, scale = it[2], (1, 1, 1 << 32, 1 << 32)[it[2]]
                    s_below = tr.join(row[2:22])[("found", "stale", "share", "rate")[q]]
                    es = Fraction(s_below + (k - nb) * it[6], k * scale)
                    assert wantk[q] == es
                    assert _c_means(lib.msim_tail_means, row, total, n, k, False)[q] == float(es)
            for k in (n_strict, n_strict + ne + 1):
                assert tr.mean_k(row, total, n, k, upper) is None
                assert _c_means(lib.msim_tail_means, row, total, n, k, upper) == -1
                assert _c_means(h.tail_host_means, row, total, n, k, upper) == -1


def test_division_is_correctly_rounded():
    """The one division behind msim_tail_means against float(Fraction) (CPython's int / int is correctly rounded)."""
    h = _host()
    rng = np.random.default_rng(5)
    cases = [(1, 3), (2**53 + 1, 1), (2**54 + 2, 2), (2**54 + 6, 2), (2**55 + 5, 4), (2**128 - 1, 2**64 - 1), (0, 9),
             (2**127 + 2**74, 2**64), (2**127 + 2**74 + 1, 2**64), (3, 2**128 - 1)]
    for _ in range(300):
        nb, db = int(rng.integers(1, 129)), int(rng.integers(1, 129))
        cases.append((int(rng.integers(0, 2**63)) ** 3 % (1 << nb), 1 + int(rng.integers(0, 2**63)) ** 3 % (1 << db)))
    for num, den in cases:
        got = h.tail_host_div(num & U64, num >> 64, den & U64, den >> 64)
        assert got == num / den, (num, den)


def test_side_moments_to_errors(msim_lib_path):
    """msim_tail_side's moments through msim_moments_to_errors equal moments_reference.errors on the subset (exact
    numerators, then fewer than eight f64 roundings: bound 1e-13, as tests/test_moments_host.py)."""
    from miningsimulation_amd import _lib

    f, s, L, r, items, got = case(257, 9, 1)
    lib = _lib.lib
    checked = 0
    for it, row in list(zip(items, got.tolist()))[::5]:
        if not tr.item_ok(it, 1, 9):
            continue
        total = r.total(it[3], it[4])
        key = r.keys[it[0]][it[2]][:, it[1]]
        masks = {"below": key < np.uint64(it[6]), "at_most": key <= np.uint64(it[6]), "above": key > np.uint64(it[6]),
                 "at_least": key >= np.uint64(it[6])}
        for side, name in enumerate(tr.SIDES):
            words, cnt = _c_side(ctypes.CDLL(msim_lib_path).msim_tail_side, row, total, 257, side)
            sel = masks[name]
            assert cnt == int(sel.sum())
            if cnt == 0:
                continue
            want_mo = ref.expected(f[it[3]][sel][:, it[4]:it[4] + 1], s[it[3]][sel][:, it[4]:it[4] + 1], L[it[3]][sel])[0]
            assert tr.join(words) == want_mo
            mo = (_lib.MsimMoments * 1)()
            ctypes.memmove(mo, np.asarray(words, dtype=np.uint64).ctypes.data, 160)
            out = (_lib.MsimErrors * 1)()
            lib.msim_moments_to_errors(mo, 1, cnt, out)
            want = ref.errors(want_mo, cnt)
            for fname, _ in _lib.MsimErrors._fields_:
                g = getattr(out[0], fname)
                if want[fname] is None:
                    assert np.isnan(g)
                else:
                    assert ref.rel_error(g, want[fname], squared=fname.endswith("_se")) <= 1e-13, (it, name, fname)
            checked += 1
    assert checked > 50


def test_two_buffers_add_to_one():
    """100 + 157 runs accumulated into the same words equal the 257 runs in one buffer."""
    f, s, L, r, items, got = case(257, 9, 3)
    out = np.zeros((len(items), tr.WORDS), dtype=np.uint64)
    host_tails(f[:, :100], s[:, :100], L[:, :100], items, "tail_host_accumulate_add", out)
    host_tails(f[:, 100:], s[:, 100:], L[:, 100:], items, "tail_host_accumulate_add", out)
    assert (out == got).all()


def test_tail_check_under_sanitizers():
    """The guard, the key, the per-run add, the accumulation, the sides, the means and the division, built
    stand-alone with ASan + UBSan on the extreme records: a child process on the CPU."""
    _built()
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tail_check: ok" in r.stdout


def test_python_layer_without_gpu(msim_lib_path):
    """Spec builders, the words of items, TailResult's arithmetic and report_tails on a result built from the
    reference's words."""
    import miningsimulation_amd as msim
    from miningsimulation_amd import tails
    from miningsimulation_amd.quantiles import OrderStat

    assert msim.own_tails(2, 3, "found", 1) == [msim.TailSpec(p, k, 0, 1, p, k) for p in range(2) for k in range(3)]
    given = msim.tails_given(0, 2, "share", 3, target_point=1)
    assert given == [msim.TailSpec(0, 2, 2, 0, 1, k) for k in range(3)]
    items = [msim.TailItem(1, 2, 3, 0, 1, 2**64 - 2**32)]
    assert msim.items_words(items).tolist() == tr.item_words([(1, 2, 3, 0, 1, 0, 2**64 - 2**32)]).tolist()
    assert tails.items_check(items, 2, 3) and not tails.items_check(items, 1, 3) and not tails.items_check([], 2, 3)
    with pytest.raises(ValueError):
        tails.specs_struct([msim.TailSpec(0, 0, 2, 1, 0, 0)], 1, 3, 1)       # rank index 1 of one rank
    with pytest.raises(ValueError):
        tails.specs_struct([], 1, 3, 1)

    f, s, L, r, _, _ = case(65, 3, 1)
    n, rank = 65, 3
    order = [[[[None] for _ in range(4)] for _ in range(3)]]
    for k in range(3):
        for q in range(4):
            srt = np.sort(r.keys[0][q][:, k])
            v = int(srt[rank])
            order[0][k][q][0] = OrderStat(v, int((srt < v).sum()), int((srt == v).sum()))
    specs = msim.own_tails(1, 3) + msim.tails_given(0, 1, "found", 3)
    its = tails.items_from_specs(specs, order)
    words = r.all_words([(i.cond_point, i.cond_column, i.quantity, i.target_point, i.target_column, 0, i.value) for i in its])
    totals = [r.total(0, k) for k in range(3)]
    res = tails.make_result([None], [rank], [0.05], order, n, specs, np.array(totals, dtype=np.uint64),
                            np.array(words, dtype=np.uint64))
    assert quantile_ok(msim, n, rank)
    for i, (sp, w) in enumerate(zip(specs, words)):
        o = order[0][sp.cond_column][sp.quantity][0]
        assert (res.tails[i]["n_below"], res.tails[i]["n_equal"]) == (o.below, o.equal) == (w[0], w[1])
        sd = tr.sides(w, totals[sp.target_column], n)
        for name in tr.SIDES:
            assert res.side(i, name) == (tr.join(sd[name][0]), sd[name][1])
        for upper in (False, True):
            want = tr.mean_k(w, totals[sp.target_column], n, res.k(i, upper), upper)
            assert list(res.means(i, upper).values()) == [float(x) for x in want]
        assert res.errors(i, "at_most")["found_mean"] == pytest.approx(float(Fraction(tr.join(sd["at_most"][0])["found"],
                                                                                      sd["at_most"][1])))
    for k in range(3):
        assert res.expected_shortfall(k) * Fraction(1, 1 << 32) == tr.mean_k(words[k], totals[k], n, rank + 1)[2]
    lines = msim.report_tails(list(msim.setup_miners()[:3]), res).splitlines()
    assert len(lines) == 3 and lines[0].startswith("  - Miner 0 (30% of network hashrate) in its worst 4 of 65 runs found ")
    assert " blocks (all runs: " in lines[0] and lines[0].endswith("%).")


def quantile_ok(msim, n, rank):
    return msim.quantile_rank(n, 0.05) == rank


def test_run_tails_rejects_bad_arguments(msim_lib_path):
    from miningsimulation_amd import Simulation, _lib, setup_miners

    sim = Simulation(setup_miners())
    lib = _lib.lib
    stats, sums = (_lib.MsimStats * 9)(), (_lib.MsimSums * 9)()
    order = (_lib.MsimOrderStat * (9 * 4))()
    mom, tails = (_lib.MsimMoments * 9)(), (_lib.MsimTail * 2)()
    ranks = (ctypes.c_uint64 * 1)(3)
    spec = (lambda *a: (_lib.MsimTailSpec * 2)(_lib.MsimTailSpec(0, 0, 2, 0, 0, 0), _lib.MsimTailSpec(*a)))
    ok = spec(0, 8, 3, 0, 0, 8)
    call = (lambda h, n, sp, ns, o, mo, t: lib.msim_run_tails(h, 0, n, 1000, 0, None, 0, ranks, 1, sp, ns, stats, sums, o,
                                                              mo, t))
    E = _lib.MSIM_E_INVALID
    assert call(None, 16, ok, 2, order, mom, tails) == E
    assert call(sim.handle, 3, ok, 2, order, mom, tails) == E                 # rank 3 of 3 runs
    assert call(sim.handle, 16, None, 2, order, mom, tails) == E
    assert call(sim.handle, 16, ok, 0, order, mom, tails) == E
    assert call(sim.handle, 16, ok, 2, None, mom, tails) == E
    assert call(sim.handle, 16, ok, 2, order, None, tails) == E
    assert call(sim.handle, 16, ok, 2, order, mom, None) == E
    for bad in ((1, 0, 0, 0, 0, 0), (0, 9, 0, 0, 0, 0), (0, 0, 4, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0),
                (0, 0, 0, 0, 0, 9)):
        assert call(sim.handle, 16, spec(*bad), 2, order, mom, tails) == E, bad
    assert lib.msim_sweep_run_tails(None, 0, 16, 1000, 0, None, 0, ranks, 1, ok, 2, stats, sums, order, mom, tails) == E
    with pytest.raises(ValueError):
        sim.run_tails(16, ranks=[16])
    with pytest.raises(ValueError):
        sim.run_tails(16, specs=[(0, 9, 2, 0, 0, 0)])


def test_launch_rejects_bad_arguments(msim_lib_path):
    """Every refusal comes before any HIP call; the pointers are never dereferenced."""
    from miningsimulation_amd import _lib

    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    ok = dict(m=9, points=1, runs=100, rec=p, bh=p, items=p, n=3, out=p)
    for ch in (dict(m=0), dict(points=0), dict(runs=0), dict(runs=1 << 32), dict(rec=None), dict(bh=None),
               dict(items=None), dict(n=0), dict(n=65535 * 128 + 1), dict(out=None)):
        a = dict(ok, **ch)
        assert lib.msim_tail_launch(a["m"], a["points"], a["runs"], a["rec"], a["bh"], a["items"], a["n"], a["out"],
                                    None) == _lib.MSIM_E_INVALID, ch

"""Networks that reach the entity engine's capacity flags at the device's shipped capacities, and the host prediction
of what the device flags on them (tests/native/sel_host.cpp at the device's classes). Shared by tests/test_sel_host.py
(the prediction against the oracle, and each case's preconditions) and tests/test_gpu_selfish_flags.py (the device's
counters against the prediction).

A case is 257 runs from run 0 at seed base 1000 (run r has seeds 1000 + 2r and 1001 + 2r) unless a test says otherwise.
E1 is the first kernel (one lane per run), E2 the retry kernel over the runs E1 flagged, G the general engine over the
runs E2 flagged too (msim_sel_launch.h). `want` names what the case is for:
  "mixed"  E1 flags some runs and finishes others, and both kinds meet among the first 64 runs (one wave)
  "e2"     E2 finishes every run E1 flagged: nothing reaches G
  "g"      at least one run reaches G
  "e1"     at least one run is finished by E1 (with "g": all three stages write records in one launch)"""
import ctypes
from collections import namedtuple

import numpy as np

BASE = 1000
RUNS = 257
SERR_WIN, SERR_ACT, SERR_GRP, SERR_QUE = 2, 16, 32, 64  # msim_sel.h

C3 = [40, 19, 12, 11, 8, 5, 3, 1, 1]
F15 = [30] + [5] * 14
T15 = [15, 15] + [5] * 12 + [10]
S = 1000  # ms

Case = namedtuple("Case", "name weights props selfish duration W want")


def _case(name, weights, props, selfish, duration, want, W=100):
    props = [props] * len(weights) if isinstance(props, int) else list(props)
    return Case(name, tuple(weights), tuple(props), tuple(k in selfish for k in range(len(weights))), duration, W,
                tuple(want.split()))


CASES = {c.name: c for c in [
    # (a) one selfish miner, mixed waves, nothing to G
    _case("c3_900", C3, 900 * S, (0,), 3 * 10**8, "mixed e2"),
    _case("slow_selfish", [45, 30, 25], [600 * S, S, S], (0,), 10**9, "mixed e2"),
    _case("f15_600", F15, 600 * S, (0,), 3 * 10**8, "mixed e2"),
    # (b) all three stages in one launch
    _case("c3_1800", C3, 1800 * S, (0,), 3 * 10**8, "mixed g e1"),
    _case("c3_1800_w1000", [10 * w for w in C3], 1800 * S, (0,), 3 * 10**8, "mixed g e1", W=1000),
    _case("c3_2400", C3, 2400 * S, (0,), 3 * 10**8, "mixed g e1"),
    _case("f15_900", F15, 900 * S, (0,), 3 * 10**8, "mixed g e1"),
    _case("two_5400", [49, 51], [5400 * S, 100], (0,), 10**9, "g"),
    _case("two_900", [10, 90], [S, 900 * S], (0,), 3 * 10**8, "mixed g e1"),
    # (c) heterogeneous delays: the instance that reads them from the LDS table
    _case("c3_hetero", C3, [S, 3600 * S, S, 1800 * S, S, 900 * S, S, S, 600 * S], (0,), 3 * 10**8, "mixed g e1"),
    # (d) several selfish miners: the engine alone
    _case("t15_900", T15, 900 * S, (0, 1), 3 * 10**8, "mixed g e1"),
    _case("t15_1200", T15, 1200 * S, (0, 1), 3 * 10**8, "mixed g e1"),
    _case("c3_three", C3, 1800 * S, (1, 2, 3), 3 * 10**8, "mixed g e1"),
    _case("c3_four", C3, 2400 * S, (2, 3, 4, 5), 3 * 10**8, "mixed g e1"),
    # the quiet point of the sweep: no flags
    _case("c3_1", C3, S, (0,), 3 * 10**8, "quiet"),
]}

# host classes (tests/native/sel_host.cpp run_caps)
E1_MIXED, E1_ENGINE_ONE, E1_ENGINE = 12, 20, 0
E2_DEVICE, E2_ENGINE, E2_ENGINE_NS4 = 21, 22, 23


def e1_class(case, no_macro=False):
    """The host class of what E1 runs: the mixed schedule for one selfish miner whose network's delays are all at
    least 1 ms (build_sel_params: macro), the engine alone otherwise."""
    ns = sum(case.selfish)
    if ns == 1:
        return E1_MIXED if not no_macro and min(case.props) >= 1 else E1_ENGINE_ONE
    return E1_ENGINE


def e2_class(case, no_macro=False):
    return E2_ENGINE if no_macro else E2_DEVICE


def load(path):
    """run(case, r, caps, fold_every=0) -> (err, [[found, stale]] * M, best height) of one run on the host build."""
    lib = ctypes.CDLL(path)
    lib.sel_set_fold_every.argtypes = [ctypes.c_uint32]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.sel_run.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8),
                            ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                            u32p, u32p, u32p, u32p]

    def run(case, r, caps, begin=0, fold_every=0):
        m = len(case.weights)
        f, s = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        bh, err = ctypes.c_uint32(), ctypes.c_uint32()
        lib.sel_set_fold_every(fold_every)
        try:
            rc = lib.sel_run((ctypes.c_uint64 * m)(*case.weights), (ctypes.c_int64 * m)(*case.props),
                             (ctypes.c_uint8 * m)(*[1 if x else 0 for x in case.selfish]), m, case.W, case.duration,
                             BASE + 2 * (begin + r), BASE + 2 * (begin + r) + 1, caps, f, s, ctypes.byref(bh),
                             ctypes.byref(err))
        finally:
            lib.sel_set_fold_every(0)
        assert rc == 0, rc
        return err.value, np.array([[f[k], s[k]] for k in range(m)], dtype=np.int64), bh.value

    return run


Prediction = namedtuple("Prediction", "e1 e2 rec bh")
_PRED = {}


def predict(run, case, n=RUNS, no_macro=False, e2=None):
    """The error words of every run at E1's class (e1[n]) and, for the runs E1 flags, at E2's class (e2[n], 0 for the
    others), with the records [n, M, 2] and best heights of the stage that finishes each run (-1 where it is G).
    Read-only and computed once per (case, n, classes)."""
    e2 = e2_class(case, no_macro) if e2 is None else e2
    key = (case.name, n, no_macro, e2)
    if key not in _PRED:
        m = len(case.weights)
        a1, a2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        rec, bh = np.full((n, m, 2), -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        c1 = e1_class(case, no_macro)
        for r in range(n):
            a1[r], res, h = run(case, r, c1)
            if a1[r]:
                a2[r], res, h = run(case, r, e2)
            if not a2[r]:
                rec[r], bh[r] = res, h
        for x in (a1, a2, rec, bh):
            x.setflags(write=False)
        _PRED[key] = Prediction(a1, a2, rec, bh)
    return _PRED[key]


def check_preconditions(case, p):
    """What the case is for holds on the host prediction."""
    n = len(p.e1)
    f1, f2 = p.e1 != 0, p.e2 != 0
    assert not (f2 & ~f1).any()
    # the flags asserted as equalities on the device are those no fold can move: the slot capacities
    assert not ((p.e1 | p.e2) & ~(SERR_ACT | SERR_GRP | SERR_QUE)).any(), (case.name, sorted(set((p.e1 | p.e2).tolist())))
    if "quiet" in case.want:
        assert not f1.any(), case.name
    else:
        assert f1.any(), case.name
    if "mixed" in case.want:
        assert 0 < f1.sum() < n, (case.name, int(f1.sum()))
        if n >= 64:
            assert f1[:64].any() and not f1[:64].all(), case.name
    if "e2" in case.want:
        assert not f2.any(), (case.name, int(f2.sum()))
    if "g" in case.want:
        assert f2.any(), case.name
    if "e1" in case.want:
        assert not f1.all(), case.name


_ORACLE = {}


def oracle_runs(oracle, case, n=RUNS, begin=0):
    """(found [n, M], stale [n, M], share [n, M], rate [n, M]) of the oracle, computed once, read-only."""
    key = (case.name, n, begin)
    if key not in _ORACLE:
        out = oracle.run_batch(list(case.weights), list(case.props), list(case.selfish), case.duration, n, begin, BASE,
                               threads=16, total_weight=case.W)
        for x in out:
            x.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]

"""The event-skipping pipeline on the host with the draw kernel's OWN lane body (msim_pipeline.h
draw_segment_k1 on K1's tables, tests/native/pipeline_k1_host.cpp), against the oracle: the per-finder form,
the uniform-delay form, and what launch_draws picks. tests/test_pipeline_host.py runs the same pipeline on the
general tables; tests/test_gpu_k1_forms.py checks the device build."""
import ctypes

import numpy as np
import pytest

import k1_native

D = 31_556_952_000
MONTH = 30 * 86_400_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]
GENERAL, PER_FINDER, UNIFORM, AUTO = 0, 1, 2, 3


@pytest.fixture(scope="module")
def k1pipe():
    lib = ctypes.CDLL(k1_native.ensure()["pipeline_k1_host"])
    lib.pipeline_k1_uniform.restype = ctypes.c_int64

    def run(percs, props, duration, n, form, base=1000, begin=0, slots=8192):
        m = len(percs)
        f = (ctypes.c_uint32 * (n * m))()
        s = (ctypes.c_uint32 * (n * m))()
        ok = (ctypes.c_uint8 * n)()
        ft = (ctypes.c_uint32 * n)()
        ne = ctypes.c_uint32()
        rc = lib.pipeline_k1_run((ctypes.c_uint64 * m)(*percs), (ctypes.c_int64 * m)(*props), (ctypes.c_uint8 * m)(),
                                 m, form, ctypes.c_int64(duration), ctypes.c_uint32(base), ctypes.c_uint64(begin),
                                 ctypes.c_uint32(n), ctypes.c_uint32(slots), f, s, ok, ctypes.byref(ne), ft)
        assert rc == 0, f"pipeline_k1_run rc={rc} (-60: no uniform threshold, -61: bad counter row)"
        return (np.array(f, dtype=np.int64).reshape(n, m), np.array(s, dtype=np.int64).reshape(n, m),
                np.array(ok, dtype=bool), np.array(ft, dtype=np.int64))

    def uniform(props):
        m = len(props)
        return lib.pipeline_k1_uniform((ctypes.c_int64 * m)(*props), (ctypes.c_uint8 * m)(), m)

    run.uniform = uniform
    return run


def _check(k1pipe, oracle, percs, props, duration, n, form, **kw):
    f, s, ok, _ = k1pipe(percs, props, duration, n, form, **kw)
    of, os_, _, _ = oracle.run_batch(percs, props, [0] * len(percs), duration, n, kw.get("begin", 0), kw.get("base", 1000),
                                     threads=8)
    assert ok.all(), f"{(~ok).sum()} runs flagged for retry"
    assert np.array_equal(f, of), (percs, props, duration, form)
    assert np.array_equal(s, os_), (percs, props, duration, form)


def test_uniform_choice(k1pipe):
    """launch_draws takes the uniform-delay form exactly when every miner has the same delay."""
    assert k1pipe.uniform([100] * 9) == 100
    assert k1pipe.uniform([0]) == 0
    assert k1pipe.uniform([100] * 8 + [101]) == -1
    assert k1pipe.uniform([10**7] * 3) == (1 << 18) - 1  # FTHR_CAP


@pytest.mark.parametrize("form", [PER_FINDER, UNIFORM])
@pytest.mark.parametrize("prop", [0, 100, 10_000])
def test_uniform_network_full_year(k1pipe, oracle, form, prop):
    """c2-like networks over a year (the band, every segment's jump): both instantiations of K1's body."""
    _check(k1pipe, oracle, H, [prop] * 9, D, 8, form)


def test_three_delays(k1pipe, oracle):
    """Nine miners, three different delays: no uniform threshold, so launch_draws' choice is the per-finder form."""
    props = [100, 100, 100, 1000, 1000, 1000, 10_000, 10_000, 0]
    assert k1pipe.uniform(props) == -1
    _check(k1pipe, oracle, H, props, MONTH, 64, AUTO)
    _check(k1pipe, oracle, H, props, D, 4, PER_FINDER, base=77, begin=123_456)


@pytest.mark.parametrize("form", [PER_FINDER, UNIFORM])
def test_one_and_fifteen_miners(k1pipe, oracle, form):
    _check(k1pipe, oracle, [100], [1000], MONTH, 32, form)
    _check(k1pipe, oracle, [7] * 14 + [2], [250] * 15, MONTH, 32, form)


def test_fall_through_gap_ends_in_retry(k1pipe, oracle):
    """Percentages summing to 98: PickFinder falls through for 2 % of its draws (simulation.h:220). In every form
    a run with a fall-through before its end must be flagged for the retry path (by owner 15's counter, not by the
    block's fast bit, which the uniform-delay form does not define for it), a run K1 saw no fall-through in must
    not be flagged, and an unflagged run equals the oracle's run of the network whose tenth miner takes the gap
    (same draws; that miner found nothing before the end)."""
    percs, props, dur, n = [30, 29, 12, 11, 8, 5, 1, 1, 1], [100] * 9, 24_000_000, 256
    res = {form: k1pipe(percs, props, dur, n, form) for form in (GENERAL, PER_FINDER, UNIFORM)}
    of, os_, _, _ = oracle.run_batch(percs + [2], props + [100], [0] * 10, dur, n, 0, 1000, threads=8)
    for form, (f, s, ok, ft) in res.items():
        gap_hit = (of[:, 9] + os_[:, 9]) > 0
        assert not ok[gap_hit].any(), form            # a fall-through before the end: always the retry path
        assert ok[ft == 0].all(), form                # nothing fell through anywhere: never flagged
        assert (ft[~ok] > 0).all(), form
        assert np.array_equal(f[ok], of[ok][:, :9]) and np.array_equal(s[ok], os_[ok][:, :9]), form
        assert (of[ok][:, 9] == 0).all(), form
        assert gap_hit.sum() > 32 and ok.sum() > 32   # both kinds of run are in the sample
    for form in (PER_FINDER, UNIFORM):  # the same runs flagged, the same fall-through counts
        assert np.array_equal(res[GENERAL][2], res[form][2]) and np.array_equal(res[GENERAL][3], res[form][3]), form

"""The reference side of tests/test_gpu_sums.py, checked on the CPU: the two forms of the expected sums agree on
the instantiation networks (the terms rebuilt from the integer counters are the terms of the oracle's own share and
rate doubles), and msim_sums_to_stats converts a Q32.32 limb pair with one rounding of its exact value."""
from fractions import Fraction

import numpy as np
import pytest

import instantiation_networks as nets
import sums_reference as ref


def _networks():
    seen = {}
    for name, (lo, _) in nets.CASES.items():
        for m in (2, 9, 15):
            if m >= lo:
                seen.setdefault((nets.case(name, m)["key"], m), name)
    return [(name, m) for (_, m), name in seen.items()]


def test_expected_forms_agree_on_instantiation_networks(oracle):
    """Every network of the matrix at M = 2, 9, 15 (one oracle batch per network, whatever switches its cases
    set): expected() from (found, stale, sum of found) == expected_from_doubles() from the oracle's doubles."""
    nonzero_rate_hi = False
    for name, m in _networks():
        c = nets.case(name, m)
        f, s, sh, r = oracle.run_batch(c["percs"], c["props"], c["selfish"], nets.DURATION_MS, nets.N_RUNS, 100 * m,
                                       1000, threads=16, total_weight=c["W"])
        a = ref.expected(f, s, f.sum(axis=1))
        b = ref.expected_from_doubles(f, s, sh, r)
        assert a == b, (name, m, ref.diff(a, b)[:4])
        for k in range(m):
            assert a[k][0] == int(f[:, k].sum()) and a[k][1] == int(s[:, k].sum())
            assert a[k][2] <= nets.N_RUNS << 32  # a share is at most 1
        assert s.sum() > 0, (name, m)  # stale blocks: the rate terms are not all zero
        nonzero_rate_hi = nonzero_rate_hi or bool((r >= 1.0).any())
    assert nonzero_rate_hi  # some miner lost more blocks than it kept in a run: rate_hi is exercised


def test_expected_handles_runs_without_blocks():
    """found == 0 gives share = rate = 0, also where the best height is 0 (no 0/0), and a lone miner's share is 2^32."""
    f = np.array([[0, 0], [3, 0], [0, 0], [1, 2]])
    s = np.array([[0, 0], [1, 4], [2, 0], [0, 3]])
    got = ref.expected(f, s, f.sum(axis=1))
    third = int(np.floor(np.float64(1) / np.float64(3) * 4294967296.0 + 0.5))
    two_thirds = int(np.floor(np.float64(2) / np.float64(3) * 4294967296.0 + 0.5))
    assert got[0] == (4, 3, (1 << 32) + third, third)
    assert got[1] == (2, 7, two_thirds, 3 << 31)
    sh = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [1 / 3, 2 / 3]])
    rt = np.array([[0.0, 0.0], [1 / 3, 0.0], [0.0, 0.0], [0.0, 1.5]])
    assert ref.expected_from_doubles(f, s, sh, rt) == got


class _Row:
    def __init__(self, *v):
        (self.blocks_found, self.stale_blocks, self.share_hi, self.share_lo, self.rate_hi, self.rate_lo) = v


def test_combined_joins_limbs():
    rows = [_Row(5, 1, 3, (1 << 40) + 7, 0, 1 << 63), _Row(0, 0, 0, 0, 0, 0)]
    want = [(5, 1, (3 << 32) + (1 << 40) + 7, 1 << 63), (0, 0, 0, 0)]
    assert ref.combined(rows) == want
    # the same limbs as an int64 array: uint64 limbs above 2^63 arrive negative
    arr = np.array([[5, 1, 3, (1 << 40) + 7, 0, -(1 << 63)], [0] * 6], dtype=np.int64)
    assert ref.combined(arr) == want
    assert ref.diff(want, want) == []
    assert ref.diff([(5, 1, 9, 2)], [(5, 1, 8, 2)]) == ["miner 0 share: device 9 reference 8 (device - reference 1)"]


def _splits(v):
    """Limb pairs (hi, lo) of 64 bits with (hi << 32) + lo == v: the canonical one (lo < 2^32), others with value
    moved into lo, and lo alone where v fits."""
    hi, lo = v >> 32, v & 0xFFFFFFFF
    out = [(hi - d, lo + (d << 32)) for d in (0, 1, 12345, (1 << 31) - 1, (1 << 32) - 1) if 0 <= hi - d < 1 << 64]
    if v < 1 << 64:
        out.append((0, v))
    assert out
    return out


def _adversarial_values():
    vals = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 1, ((1 << 53) + 1) << 32, ((1 << 60) + 12345) << 32 | 0xFFFFFFFF,
            ((1 << 64) - 1 << 32) + (1 << 64) - 1]  # the largest pair of limbs
    # either side of f64 rounding boundaries: with 53 bits kept, the spacing at 2^e is 2^(e - 52)
    for e in (53, 54, 60, 63, 64, 70, 85, 95):
        ulp = 1 << (e - 52)
        for base in ((1 << e), (1 << e) + ulp, (1 << e) + 5 * ulp, (1 << (e + 1)) - ulp):
            mid = base + ulp // 2
            vals += [mid - 1, mid, mid + 1]
    return vals


def test_sums_to_stats_rounds_the_exact_value_once(msim_lib_path):
    """msim_sums_to_stats against fractions.Fraction: lo far above 2^32 (up to 2^64 - 1), hi above 2^53, values one
    unit either side of an f64 rounding boundary; every split of a value into limbs gives the same double. (The
    library loads without a device; the conversion is host code.)"""
    from miningsimulation_amd import _lib, sums_to_stats

    cases = []
    for v in _adversarial_values():
        for hi, lo in _splits(v):
            assert (hi << 32) + lo == v and hi < 1 << 64 and lo < 1 << 64
            cases.append((v, hi, lo))
    assert any(lo >= 1 << 63 for _, _, lo in cases) and any(hi > 1 << 53 for _, hi, _ in cases)
    n = len(cases)
    sums = (_lib.MsimSums * n)()
    for i, (v, hi, lo) in enumerate(cases):
        # the value in the share limbs, and split the other way round in the rate limbs of the mirrored entry
        sums[i] = _lib.MsimSums(i, 2 * i, hi, lo, cases[n - 1 - i][1], cases[n - 1 - i][2])
    out = (_lib.MsimStats * n)()
    _lib.lib.msim_sums_to_stats(sums, n, out)
    for i, (v, hi, lo) in enumerate(cases):
        want = float(Fraction(v, 1 << 32))  # Fraction -> float rounds the exact quotient once, to nearest even
        assert out[i].blocks_found == i
        assert out[i].blocks_share == want, (hex(v), hex(hi), hex(lo), out[i].blocks_share, want)
        assert out[i].stale_rate == float(Fraction(cases[n - 1 - i][0], 1 << 32)), (i, hex(cases[n - 1 - i][0]))
        py = sums_to_stats([[i, 2 * i, hi, lo, 0, 0]])[0]  # the Python mirror of the same conversion
        assert py.blocks_share == want, (hex(v), hex(hi), hex(lo))
    # a tie goes to the even neighbour, one unit more goes up: the boundary cases above are real boundaries
    assert float(Fraction((1 << 60) + (1 << 7), 1 << 32)) == float(Fraction(1 << 60, 1 << 32))
    assert float(Fraction((1 << 60) + (1 << 7) + 1, 1 << 32)) > float(Fraction(1 << 60, 1 << 32))

"""Per-miner error bars: exact second moments and histograms of the per-run terms (include/msim.h: msim_moments,
msim_hist_spec, msim_errors; kernel in csrc/msim_moments.hip).

The reference prints three means per miner (main.cpp:224-234) and nothing about their spread. The device sums
the squares and cross products of the same integer terms its msim_sums add, so standard errors follow without
the per-run records ever leaving device memory, and the sums stay order-independent: identical for any split into
workgroups, launches or ranks.

Terms are Q32.32 integers: a share or stale rate x is the term t = round(x * 2^32), and HistSpec's bounds, edges
and shifts are in those units."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import MsimErrors, MsimHistSpec, MsimMoments, lib

ONE = 1 << 32  # the term of 1.0
MOMENT_WORDS = 20
MAX_BINS = 1024
# (name, first word, limbs, shift of limb 0 in bits, step per limb): msim_sums' hi/lo pairs are stored high limb
# first, the square sums low limb first
_LAYOUT = (("found", 0, 1, 0, 32), ("stale", 1, 1, 0, 32), ("share", 2, 2, 32, -32), ("rate", 4, 2, 32, -32),
           ("found_sq", 6, 2, 0, 32), ("stale_sq", 8, 2, 0, 32), ("found_stale", 10, 2, 0, 32),
           ("share_sq", 12, 4, 0, 32), ("rate_sq", 16, 4, 0, 32))
ERROR_FIELDS = tuple(n for n, _ in MsimErrors._fields_)


def join_limbs(row: Sequence[int]) -> dict:
    """One miner's 20 msim_moments words (uint64, or int64 holding the same bits) as a dict of Python ints with
    the limbs joined: found, stale, share, rate (the sums of the terms) and found_sq, stale_sq, found_stale,
    share_sq, rate_sq."""
    w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in row]
    assert len(w) == MOMENT_WORDS
    return {name: sum(w[at + i] << (sh + i * step) for i in range(n)) for name, at, n, sh, step in _LAYOUT}


def split_limbs(mo: dict) -> List[int]:
    """The inverse of join_limbs with normalised limbs (every limb but the top one below 2^32)."""
    w = [0] * MOMENT_WORDS
    for name, at, n, sh, step in _LAYOUT:
        v = int(mo[name])
        if n == 1:
            w[at] = v
            continue
        order = range(n) if step > 0 else range(n - 1, -1, -1)  # low limb first
        for j, i in enumerate(order):
            w[at + i] = v & 0xFFFFFFFF if j < n - 1 else v
            v >>= 32
    return w


def moments_from_words(words) -> List[dict]:
    """[M, 20] words -> per-miner dicts (join_limbs)."""
    return [join_limbs(r) for r in np.asarray(words).reshape(-1, MOMENT_WORDS).tolist()]


@dataclass(frozen=True)
class HistSpec:
    """msim_hist_spec: `bins` bins of width 2^shift term units from `lo`, per quantity. Row layout of the counts:
    [under, bin 1 .. bin `bins`, over]."""

    bins: int
    share_shift: int = 0
    rate_shift: int = 0
    share_lo: int = 0
    rate_lo: int = 0

    def __post_init__(self):
        if not (1 <= self.bins <= MAX_BINS and 0 <= self.share_shift <= 63 and 0 <= self.rate_shift <= 63
                and 0 <= self.share_lo < 1 << 64 and 0 <= self.rate_lo < 1 << 64):
            raise ValueError(f"invalid histogram spec {self}")

    @staticmethod
    def shift_covering(lo_t: int, hi_t: int, bins: int) -> int:
        """The smallest shift with ((hi_t - lo_t) >> shift) < bins: hi_t falls into the last bin at the latest."""
        if hi_t < lo_t:
            raise ValueError("hi below lo")
        shift = 0
        while ((hi_t - lo_t) >> shift) >= bins:
            shift += 1
        return shift

    @classmethod
    def covering(cls, lo: float, hi: float, bins: int, rate_lo: Optional[float] = None,
                 rate_hi: Optional[float] = None) -> "HistSpec":
        """Bins covering the values lo..hi (fractions: a share of 30 % is 0.3) with the smallest power-of-two bin
        width that reaches hi; the stale rate's range defaults to the share's."""
        rate_lo = lo if rate_lo is None else rate_lo
        rate_hi = hi if rate_hi is None else rate_hi
        slo, shi, rlo, rhi = (int(x * ONE) for x in (lo, hi, rate_lo, rate_hi))
        return cls(bins, cls.shift_covering(slo, shi, bins), cls.shift_covering(rlo, rhi, bins), slo, rlo)

    def struct(self) -> MsimHistSpec:
        return MsimHistSpec(self.bins, self.share_shift, self.rate_shift, self.share_lo, self.rate_lo)

    def lo_shift(self, which: str) -> Tuple[int, int]:
        if which not in ("share", "rate"):
            raise ValueError(which)
        return (self.share_lo, self.share_shift) if which == "share" else (self.rate_lo, self.rate_shift)

    def bin_of(self, t: int, which: str = "share") -> int:
        lo, shift = self.lo_shift(which)
        if t < lo:
            return 0
        q = (t - lo) >> shift
        return self.bins + 1 if q >= self.bins else 1 + q

    def edges(self, b: int, which: str = "share") -> Tuple[float, float]:
        """The values [low, high) of row index b: (0, lo) for the underflow bin, (end, inf) for the overflow bin."""
        lo, shift = self.lo_shift(which)
        if b == 0:
            return 0.0, lo / ONE
        if b == self.bins + 1:
            return (lo + (self.bins << shift)) / ONE, math.inf
        return (lo + ((b - 1) << shift)) / ONE, (lo + (b << shift)) / ONE


def hist_quantile(counts, spec: HistSpec, q: float, which: str = "share") -> Tuple[float, float]:
    """The edge interval [low, high) of the bin holding the q-quantile of one histogram row ([bins + 2] counts):
    the k-th smallest value with k = max(1, ceil(q N))."""
    c = [int(x) for x in np.asarray(counts).reshape(-1)]
    if len(c) != spec.bins + 2 or not 0.0 <= q <= 1.0:
        raise ValueError("counts must be one row of bins + 2 entries and q within [0, 1]")
    n = sum(c)
    if n == 0:
        raise ValueError("empty histogram")
    k = max(1, math.ceil(q * n))
    run = 0
    for b, x in enumerate(c):
        run += x
        if run >= k:
            return spec.edges(b, which)
    raise AssertionError("unreachable")


def errors_from_moments(moments: Sequence[dict], n_runs: int) -> List[dict]:
    """msim_moments_to_errors: per miner found_mean/se, share_mean/se, rate_mean/se, pooled_rate/se."""
    m = len(moments)
    arr = (MsimMoments * m)()
    flat = ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint64))
    for k, mo in enumerate(moments):
        for i, v in enumerate(split_limbs(mo)):
            flat[k * MOMENT_WORDS + i] = v
    out = (MsimErrors * m)()
    lib.msim_moments_to_errors(arr, m, int(n_runs), out)
    return [{f: getattr(e, f) for f in ERROR_FIELDS} for e in out]


def error_bars(result) -> List[dict]:
    """Means and standard errors per miner of a result that carries moments (run_moments, run_sharded_moments)."""
    if getattr(result, "moments", None) is None:
        raise ValueError("the result has no moments: use run_moments()")
    return errors_from_moments(result.moments, result.n_runs)


def _pm(x: float, scale: float = 1.0, unit: str = "") -> str:
    return "n/a" if math.isnan(x) else f"{x * scale:.6g}{unit}"


def error_columns(e: dict) -> str:
    """The columns report_with_errors (and host/msim_main --errors) append to a report line."""
    return (f" ± {_pm(e['found_se'])} blocks, ± {_pm(e['share_se'], 100.0, '%')} of blocks,"
            f" stale rate ± {_pm(e['rate_se'], 100.0, '%')}")


def report_with_errors(miners, result, duration_ms: Optional[int] = None) -> str:
    """report()'s lines (main.cpp:224-234) with the standard errors of the three means appended to each."""
    from .simulation import SIM_DURATION_MS, report

    lines = report(miners, result.stats_total, result.n_runs,
                   SIM_DURATION_MS if duration_ms is None else duration_ms).splitlines()
    errs = error_bars(result)
    return "\n".join([lines[0]] + [ln + error_columns(e) for ln, e in zip(lines[1:], errs)])

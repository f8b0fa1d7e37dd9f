"""Paired contrasts between sweep points and miners (include/msim.h: msim_pair, msim_cross, msim_contrast; kernel in
csrc/msim_cross.hip).

The reference compares networks by rebuilding per network (README.md:21-27) and reading two reports side by side.
A sweep runs every point on the same seeds, so the per-run difference of two points is far less noisy than either
side, and two miners of one network are negatively correlated. The device sums the per-run products of the two
sides of each pair exactly; together with each side's moments they give the difference, the ratio and the
correlation with standard errors, and the per-run records never leave device memory.

Points and miners are indices (from 0) into the launch's records."""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Sequence

import numpy as np

from ._lib import MSIM_OK, MsimContrast, MsimCross, MsimMoments, MsimPair, lib
from .moments import MOMENT_WORDS, split_limbs

CROSS_WORDS = 12
# (name, first word, limbs), low limb first
_LAYOUT = (("found_found", 0, 2), ("stale_stale", 2, 2), ("share_share", 4, 4), ("rate_rate", 8, 4))
CONTRAST_FIELDS = tuple(n for n, _ in MsimContrast._fields_)


class Pair(NamedTuple):
    """msim_pair: side a and side b, each a (point, miner) column. A contrast is a minus b, a over b."""

    point_a: int
    miner_a: int
    point_b: int
    miner_b: int


def pairs_vs_baseline(n_points: int, m: int, baseline: int = 0) -> List[Pair]:
    """Every miner of every other point against the same miner of `baseline`, point-major and miner-minor."""
    if not 0 <= baseline < n_points:
        raise ValueError(f"baseline {baseline} outside 0..{n_points - 1}")
    return [Pair(p, k, baseline, k) for p in range(n_points) if p != baseline for k in range(m)]


def pairs_between_miners(m: int, point: int = 0) -> List[Pair]:
    """All miners i < j of one point."""
    return [Pair(point, i, point, j) for i in range(m) for j in range(i + 1, m)]


def pairs_struct(pairs: Sequence[Pair], n_points: int, m: int):
    """The pairs as an msim_pair array, checked with msim_pairs_check against n_points x m."""
    arr = (MsimPair * len(pairs))()
    for i, q in enumerate(pairs):
        if min(q) < 0 or max(q) > 0xFFFFFFFF:
            raise ValueError(f"pair {i} {tuple(q)} does not fit msim_pair")
        arr[i] = MsimPair(*q)
    if lib.msim_pairs_check(m, n_points, arr, len(pairs)) != MSIM_OK:
        raise ValueError(f"no pairs, too many, or a pair outside {n_points} points x {m} miners")
    return arr


def join_cross(row: Sequence[int]) -> dict:
    """One pair's 12 msim_cross words (uint64, or int64 holding the same bits) as a dict of Python ints with the
    limbs joined: found_found, stale_stale, share_share, rate_rate."""
    w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in row]
    assert len(w) == CROSS_WORDS
    return {name: sum(w[at + i] << (32 * i) for i in range(n)) for name, at, n in _LAYOUT}


def split_cross(cr: dict) -> List[int]:
    """The inverse of join_cross with normalised limbs (every limb but the top one below 2^32)."""
    w = [0] * CROSS_WORDS
    for name, at, n in _LAYOUT:
        v = int(cr[name])
        for i in range(n):
            w[at + i] = v & 0xFFFFFFFF if i < n - 1 else v
            v >>= 32
    return w


def cross_from_words(words) -> List[dict]:
    """[n_pairs, 12] words -> per-pair dicts (join_cross)."""
    return [join_cross(r) for r in np.asarray(words).reshape(-1, CROSS_WORDS).tolist()]


def contrasts_from_sums(moments: Sequence[Sequence[dict]], pairs: Sequence[Pair], cross: Sequence[dict],
                        n_runs: int) -> List[dict]:
    """msim_cross_to_contrasts: per pair a dict of msim_contrast's fields, from the per-point lists of per-miner
    moments (moments.join_limbs dicts), the pairs and their cross sums (join_cross dicts)."""
    n_points, m = len(moments), len(moments[0])
    if len(cross) != len(pairs) or any(len(mo) != m for mo in moments):
        raise ValueError("one cross entry per pair and the same miner count at every point")
    arr = (MsimMoments * (n_points * m))()
    flat = ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint64))
    for p, mos in enumerate(moments):
        for k, mo in enumerate(mos):
            for i, v in enumerate(split_limbs(mo)):
                flat[(p * m + k) * MOMENT_WORDS + i] = v
    cr = (MsimCross * len(pairs))()
    cflat = ctypes.cast(cr, ctypes.POINTER(ctypes.c_uint64))
    for j, c in enumerate(cross):
        for i, v in enumerate(split_cross(c)):
            cflat[j * CROSS_WORDS + i] = v
    out = (MsimContrast * len(pairs))()
    lib.msim_cross_to_contrasts(arr, m, pairs_struct(pairs, n_points, m), cr, len(pairs), int(n_runs), out)
    return [{f: getattr(c, f) for f in CONTRAST_FIELDS} for c in out]


def contrasts(result) -> List[dict]:
    """Per pair of a ContrastResult (run_contrasts, run_sharded_contrasts) a dict of msim_contrast's fields."""
    return contrasts_from_sums([r.moments for r in result.points], result.pairs, result.cross, result.n_runs)


def _g(x: float, fmt: str = "g", scale: float = 1.0, unit: str = "") -> str:
    return "n/a" if math.isnan(x) else f"{format(x * scale, fmt)}{unit}"


def _head(q: Pair) -> str:
    if q.miner_a == q.miner_b and q.point_a != q.point_b:
        return f"Miner {q.miner_a} of point {q.point_a} vs point {q.point_b}"
    return f"Miner {q.miner_a} of point {q.point_a} vs miner {q.miner_b} of point {q.point_b}"


def contrast_line(q: Pair, c: dict) -> str:
    """One pair's line (host/msim_main --contrast prints the same): a minus b with the standard error of the
    per-run difference, the correlation of the sides and, for found and share, a over b."""
    return (f"  - {_head(q)}: found {_g(c['found_diff'], '+g')} ± {_g(c['found_diff_se'])} blocks"
            f" (corr {_g(c['found_corr'], '.3g')}), ×{_g(c['found_ratio'])} ± {_g(c['found_ratio_se'])};"
            f" share {_g(c['share_diff'], '+g', 100.0, '%')} ± {_g(c['share_diff_se'], 'g', 100.0, '%')} of blocks"
            f" (corr {_g(c['share_corr'], '.3g')}), ×{_g(c['share_ratio'])} ± {_g(c['share_ratio_se'])};"
            f" stale rate {_g(c['rate_diff'], '+g', 100.0, '%')} ± {_g(c['rate_diff_se'], 'g', 100.0, '%')}"
            f" (corr {_g(c['rate_corr'], '.3g')})")


def report_contrasts(result) -> str:
    """One readable line per pair of a ContrastResult, e.g.
    "  - Miner 0 of point 0 vs point 2: found ... ; share +0.0864% ± 0.0072% of blocks (corr 0.995), ×1.00288 ± 0.00024; ..."."""
    return "\n".join(contrast_line(q, c) for q, c in zip(result.pairs, contrasts(result)))

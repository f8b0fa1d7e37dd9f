"""Bootstrap: resampled quantiles and expected shortfalls, exact on the device (include/msim.h: msim_boot_item,
msim_boot_row, msim_boot_*_launch, msim_run_bootstrap; kernels in csrc/msim_boot.hip).

run_tails gives an expected shortfall whose standard error holds the threshold fixed, and quantile_ci_ranks gives each
sweep point an interval of its own. A Poisson bootstrap answers what they leave open: replicate b gives run r the
integer weight boot_weight(seed, b, r), which depends on nothing else, so a replicate's quantile is an order statistic
of a weighted multiset (exact integers, identical for any split of the runs) and replicates are paired across the
points of a sweep. Replicate 0 has weight 1 everywhere: it is the data, and its row equals run_quantiles' order
statistic and run_tails' expected shortfall.

An item names (point, column, quantity, q_index); quantities are indexed as in quantiles.QUANTITIES and q_index picks
one of the call's quantiles. Per (item, replicate) the device returns value, below, equal and the weighted sum of the
keys below the value (s_hi, s_lo); a replicate whose weights are all zero (only with a handful of runs) has no
quantile and is marked by equal == 0. Standard errors are the sample standard deviation over the non-empty replicates
b >= 1, formed exactly as a Fraction and rooted once; intervals are percentile intervals."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import (MSIM_BOOT_EMPTY, MSIM_BOOT_MAX_RUNS, MSIM_MAX_BOOT_ITEMS, MSIM_MAX_BOOT_REPLICATES, MSIM_MAX_RANKS,
                   MSIM_OK, MsimBootItem, MsimBootRow, MsimOrderStat, check, lib)
from .quantiles import QUANTITIES, QuantileResult, order_stats_from_words, quantile_rank, ranks_array

MAX_BOOT_REPLICATES = MSIM_MAX_BOOT_REPLICATES
MAX_BOOT_ITEMS = MSIM_MAX_BOOT_ITEMS
BOOT_MAX_RUNS = MSIM_BOOT_MAX_RUNS
BOOT_EMPTY = MSIM_BOOT_EMPTY
ROW_WORDS = 5
DEFAULT_BOOT_SEED = 0x626F6F7473747261  # "bootstra"
_SCALE = (1.0, 1.0, 2.0 ** -32, 2.0 ** -32)


class BootItem(NamedTuple):
    point: int
    column: int
    quantity: int
    q_index: int


def _quantity(q) -> int:
    return QUANTITIES.index(q) if isinstance(q, str) else int(q)


def _indices(x: Union[int, Iterable[int]]) -> List[int]:
    return list(range(x)) if isinstance(x, int) else [int(v) for v in x]


def own_bootstrap(points: Union[int, Iterable[int]], columns: Union[int, Iterable[int]], quantity="share",
                  q_index: int = 0) -> List[BootItem]:
    """Every column (a count, or the columns themselves) of every point, point-major and column-minor."""
    q = _quantity(quantity)
    return [BootItem(p, k, q, q_index) for p in _indices(points) for k in _indices(columns)]


def across_points(column: int, points: Union[int, Iterable[int]], quantity="share", q_index: int = 0) -> List[BootItem]:
    """One column at several points of a sweep, in the points' order: the items BootstrapResult.difference pairs."""
    q = _quantity(quantity)
    return [BootItem(p, int(column), q, q_index) for p in _indices(points)]


def items_struct(items: Sequence[BootItem], n_points: int, columns: int, n_q: int):
    """The items as an msim_boot_item array, checked with msim_boot_items_check."""
    items = [BootItem(*(int(x) for x in it)) for it in items]
    if not 1 <= len(items) <= MAX_BOOT_ITEMS or any(not 0 <= x <= 0xFFFFFFFF for it in items for x in it):
        raise ValueError(f"1..{MAX_BOOT_ITEMS} items of 32-bit fields")
    arr = (MsimBootItem * len(items))(*[MsimBootItem(*it) for it in items])
    if lib.msim_boot_items_check(columns, n_points, n_q, arr, len(items)) != MSIM_OK:
        raise ValueError(f"an item lies outside {n_points} points x {columns} columns x 4 quantities x {n_q} quantiles")
    return items, arr


def boot_rank(total_weight: int, q: float) -> int:
    """msim_boot_rank: quantile_rank(W, q), or BOOT_EMPTY for W == 0."""
    return int(lib.msim_boot_rank(int(total_weight), float(q)))


def boot_ranks(W: Sequence[int], qs: Sequence[float]) -> List[int]:
    """ranks[n_q][B], flat: what launch_boot_begin takes, from the complete W."""
    return [boot_rank(w, q) for q in qs for w in W]


def boot_workspace_bytes(n_items: int, replicates: int) -> int:
    n = int(lib.msim_boot_workspace_bytes(n_items, replicates))
    if n == 0:
        raise ValueError(f"no workspace for {n_items} items and {replicates} replicates")
    return n


def boot_counts_view(n_items: int, replicates: int) -> Tuple[int, int]:
    """(byte offset, uint64 words) of the digit counts inside the workspace, for the all-reduce of a pass."""
    off, words = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.msim_boot_counts_view(n_items, replicates, ctypes.byref(off), ctypes.byref(words)), "msim_boot_counts_view")
    return int(off.value), int(words.value)


# ---------------------------------------------------------------- launches (device tensors from torch)
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else None


def _bytes(t) -> int:
    return t.numel() * t.element_size()


def launch_boot_weights(seed: int, run_begin: int, n_runs: int, replicates: int, d_W, stream=None) -> None:
    """msim_boot_weights_launch: adds the weights of the absolute runs [run_begin, run_begin + n_runs) to d_W (int64
    [replicates], cleared by the caller before the first chunk)."""
    if d_W is None or _bytes(d_W) < replicates * 8:
        raise ValueError("d_W holds one 64-bit word per replicate")
    check(lib.msim_boot_weights_launch(seed & (2 ** 64 - 1), run_begin, n_runs, replicates, _ptr(d_W), _stream(stream)),
          "msim_boot_weights_launch")


def _launch_boot_begin(m: int, n_points: int, items: Sequence[BootItem], replicates: int, ranks: Sequence[int],
                       n_q: int, d_ws, stream) -> None:
    if len(ranks) != n_q * replicates:
        raise ValueError("ranks is [n_q][replicates]")
    arr = (MsimBootItem * len(items))(*[MsimBootItem(*(int(x) for x in it)) for it in items])
    rk = (ctypes.c_uint64 * len(ranks))(*[int(r) for r in ranks])
    check(lib.msim_boot_begin_launch(m, n_points, arr, len(items), replicates, rk, n_q, _ptr(d_ws), _bytes(d_ws),
                                     _stream(stream)), "msim_boot_begin_launch")


def _launch_boot_count(m: int, n_points: int, seed: int, run_begin: int, runs_per_point: int, d_per_run, d_best_height,
                       n_items: int, replicates: int, pass_: int, d_ws, stream) -> None:
    need = n_points * runs_per_point
    if _bytes(d_per_run) < need * m * 8 or _bytes(d_best_height) < need * 4:
        raise ValueError("a buffer is smaller than the launch reads")
    check(lib.msim_boot_count_launch(m, n_points, seed & (2 ** 64 - 1), run_begin, runs_per_point, _ptr(d_per_run),
                                     _ptr(d_best_height), n_items, replicates, pass_, _ptr(d_ws), _bytes(d_ws),
                                     _stream(stream)), "msim_boot_count_launch")


def _launch_boot_step(n_items: int, replicates: int, pass_: int, d_ws, d_rows, d_status, stream) -> None:
    if d_status is None or _bytes(d_status) < 4:
        raise ValueError("d_status is one 32-bit word")
    if d_rows is not None and _bytes(d_rows) < n_items * replicates * ROW_WORDS * 8:
        raise ValueError("d_rows is smaller than the launch writes")
    check(lib.msim_boot_step_launch(n_items, replicates, pass_, _ptr(d_ws), _bytes(d_ws), _ptr(d_rows), _ptr(d_status),
                                    _stream(stream)), "msim_boot_step_launch")


def _launch_boot_below(m: int, n_points: int, seed: int, run_begin: int, runs_per_point: int, d_per_run, d_best_height,
                       n_items: int, replicates: int, d_ws, d_rows, stream) -> None:
    need = n_points * runs_per_point
    if (_bytes(d_per_run) < need * m * 8 or _bytes(d_best_height) < need * 4 or d_rows is None or
            _bytes(d_rows) < n_items * replicates * ROW_WORDS * 8):
        raise ValueError("a buffer is smaller than the launch reads or writes")
    check(lib.msim_boot_below_launch(m, n_points, seed & (2 ** 64 - 1), run_begin, runs_per_point, _ptr(d_per_run),
                                     _ptr(d_best_height), n_items, replicates, _ptr(d_ws), _bytes(d_ws), _ptr(d_rows),
                                     _stream(stream)), "msim_boot_below_launch")


# ---------------------------------------------------------------- results
class BootDifference(NamedTuple):
    """difference(i, j): the data's difference (replicate 0; None if it is empty on a side), the paired
    per-replicate differences over the replicates b >= 1 that are non-empty in both items, their exact sample
    variance, its root and the percentile interval."""
    data: Optional[Fraction]
    diffs: List[Fraction]
    variance: Fraction
    se: float
    interval: Tuple[Fraction, Fraction]


def sample_variance(xs: Sequence) -> Fraction:
    """sum (x - mean)^2 / (n - 1) as an exact Fraction."""
    n = len(xs)
    if n < 2:
        raise ValueError("a variance needs two non-empty replicates")
    total = sum(Fraction(x) for x in xs)
    return (sum(Fraction(x) ** 2 for x in xs) - total * total / n) / (n - 1)


def percentile_interval(xs: Sequence, level: float = 0.95) -> Tuple:
    """The order statistics of xs at quantile_rank(n, (1 - level) / 2) and quantile_rank(n, 1 - (1 - level) / 2)."""
    if not xs or not 0.0 < level < 1.0:
        raise ValueError("no replicate, or a level outside (0, 1)")
    srt = sorted(xs)
    a = (1.0 - level) / 2.0
    return srt[quantile_rank(len(srt), a)], srt[quantile_rank(len(srt), 1.0 - a)]


def _sqrt_fraction(v: Fraction) -> float:
    """The one square root: of the exact variance's correctly rounded float."""
    return math.sqrt(float(v))


@dataclass
class BootstrapResult(QuantileResult):
    """What run_bootstrap returns: QuantileResult's fields (the order statistics at the quantiles over all runs), the
    items, the replicates' total weights W[b] (W[0] = n_runs) and the raw rows[item, replicate] = (value, below,
    equal, s_hi, s_lo) as uint64."""

    items: List[BootItem] = field(default_factory=list)
    replicates: int = 0
    boot_seed: int = 0
    W: List[int] = field(default_factory=list)
    rows: Optional[np.ndarray] = field(default=None, compare=False)  # [n_items, B, 5] uint64

    def row(self, i: int, b: int) -> Tuple[int, int, int, int, int]:
        return tuple(int(x) for x in self.rows[i, b])

    def empty(self, i: int, b: int) -> bool:
        return int(self.rows[i, b, 2]) == 0

    def n_empty(self, i: int) -> int:
        """How many replicates of item i have no quantile (all weights zero)."""
        return int((self.rows[i, :, 2] == 0).sum())

    def k(self, i: int, b: int) -> int:
        """rank + 1 of replicate b: how many of its weighted runs the quantile holds."""
        return quantile_rank(self.W[b], self.qs[self.items[i].q_index]) + 1

    def values(self, i: int) -> List[Optional[int]]:
        """The replicates' quantiles as keys (terms of 2^-32 for share and rate); None for an empty replicate."""
        return [None if self.empty(i, b) else int(self.rows[i, b, 0]) for b in range(self.replicates)]

    def shortfalls(self, i: int) -> List[Optional[Fraction]]:
        """The replicates' expected shortfalls (S_below + (k - below) value) / k, exact, in key units."""
        out: List[Optional[Fraction]] = []
        for b in range(self.replicates):
            if self.empty(i, b):
                out.append(None)
                continue
            v, below, _, hi, lo = self.row(i, b)
            k = self.k(i, b)
            out.append(Fraction((hi << 32) + lo + (k - below) * v, k))
        return out

    def _resampled(self, i: int, shortfall: bool) -> list:
        xs = self.shortfalls(i) if shortfall else self.values(i)
        return [x for x in xs[1:] if x is not None]

    def variance(self, i: int, shortfall: bool = False) -> Fraction:
        """The sample variance over the non-empty replicates b >= 1, exact."""
        return sample_variance(self._resampled(i, shortfall))

    def se(self, i: int) -> float:
        """The bootstrap standard error of item i's quantile, in key units."""
        return _sqrt_fraction(self.variance(i))

    def shortfall_se(self, i: int) -> float:
        """The bootstrap standard error of item i's expected shortfall: the threshold's own variability included."""
        return _sqrt_fraction(self.variance(i, shortfall=True))

    def interval(self, i: int, level: float = 0.95, shortfall: bool = False) -> Tuple:
        """The percentile interval over the non-empty replicates b >= 1: it can only name values the data hold, so
        it respects ties."""
        return percentile_interval(self._resampled(i, shortfall), level)

    def difference(self, i: int, j: int, level: float = 0.95, shortfall: bool = False) -> BootDifference:
        """Item i minus item j replicate by replicate, typically one column at two sweep points: the weights do not
        depend on the point, so the replicates are paired. A replicate empty in either item is left out."""
        a = self.shortfalls(i) if shortfall else self.values(i)
        c = self.shortfalls(j) if shortfall else self.values(j)
        d = [None if x is None or y is None else Fraction(x) - Fraction(y) for x, y in zip(a, c)]
        diffs = [x for x in d[1:] if x is not None]
        var = sample_variance(diffs)
        return BootDifference(d[0], diffs, var, _sqrt_fraction(var), percentile_interval(diffs, level))

    def scale(self, i: int) -> float:
        """What turns item i's key units into a number: 1 for found and stale, 2^-32 for share and rate."""
        return _SCALE[self.items[i].quantity]


def make_result(points, sel, qs, order, n_runs, items, replicates, boot_seed, W, rows) -> BootstrapResult:
    a = np.asarray(rows)
    a = a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)
    return BootstrapResult(points=points, ranks=sel, qs=[float(q) for q in qs], order=order, n_runs=n_runs,
                           items=list(items), replicates=replicates, boot_seed=boot_seed,
                           W=[int(w) & (2 ** 64 - 1) for w in np.asarray(W).reshape(-1).tolist()],
                           rows=np.ascontiguousarray(a.reshape(len(items), replicates, ROW_WORDS)))


def _check_call(n_runs: int, qs, replicates: int) -> List[float]:
    qs = [float(q) for q in qs]
    if not 1 <= len(qs) <= MSIM_MAX_RANKS or any(not 0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"1..{MSIM_MAX_RANKS} quantiles within [0, 1]")
    if not 1 <= replicates <= MAX_BOOT_REPLICATES:
        raise ValueError(f"1..{MAX_BOOT_REPLICATES} replicates")
    if not 1 <= n_runs < BOOT_MAX_RUNS:
        raise ValueError(f"1..{BOOT_MAX_RUNS - 1} runs per point")
    return qs


def _run_bootstrap(fn, what: str, handle, n_points: int, m: int, n_runs: int, items, qs, replicates: int,
                   boot_seed: int, class_of, n_classes, run_begin: int, seed_base: int, device: int) -> BootstrapResult:
    """msim_run_bootstrap / msim_sweep_run_bootstrap into a BootstrapResult."""
    from ._lib import MsimStats, MsimSums
    from .classes import class_count, class_map_struct
    from .simulation import MinerStats, SimulationResult

    qs = _check_call(n_runs, qs, replicates)
    sel = [quantile_rank(n_runs, q) for q in qs]
    arr = ranks_array(sel, n_runs)
    if class_of is not None:
        nc = class_count(class_of) if n_classes is None else int(n_classes)
        cmap = class_map_struct(class_of, m, nc)
    else:
        nc, cmap = 0, None
    cols = nc if class_of is not None else m
    items, iarr = items_struct(own_bootstrap(n_points, cols) if items is None else items, n_points, cols, len(qs))
    stats = (MsimStats * (n_points * m))()
    sums = (MsimSums * (n_points * m))()
    order = (MsimOrderStat * (n_points * cols * 4 * len(sel)))()
    W = (ctypes.c_uint64 * replicates)()
    rows = (MsimBootRow * (len(items) * replicates))()
    qarr = (ctypes.c_double * len(qs))(*qs)
    check(fn(handle, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, cmap, nc, arr, len(sel), iarr, len(items), qarr,
             len(qs), replicates, boot_seed & (2 ** 64 - 1), stats, sums, order, W, rows), what)
    as_words = (lambda a, n: np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy())
    points = [SimulationResult(
        stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
        sums=list(sums[p * m:(p + 1) * m]),
        n_runs=n_runs,
    ) for p in range(n_points)]
    return make_result(points, sel, qs, order_stats_from_words(as_words(order, len(order) * 3), n_points, cols, len(sel)),
                       n_runs, items, replicates, boot_seed & (2 ** 64 - 1), as_words(W, replicates),
                       as_words(rows, len(rows) * ROW_WORDS))


# ---------------------------------------------------------------- report
def bootstrap_columns(res: BootstrapResult, i: int, level: float = 0.95) -> str:
    """The text report_bootstrap puts behind a line's head: the quantile with its bootstrap SE and percentile
    interval, then the expected shortfall with its own."""
    it, sc = res.items[i], res.scale(i)
    pct = 100.0 if it.quantity >= 2 else 1.0
    unit = "%" if it.quantity >= 2 else ""
    fmt = (lambda x: f"{float(x) * sc * pct:g}{unit}")
    lo, hi = res.interval(i, level)
    slo, shi = res.interval(i, level, shortfall=True)
    return (f" {QUANTITIES[it.quantity]} q{res.qs[it.q_index]:g} = {fmt(res.values(i)[0])} (SE {fmt(res.se(i))},"
            f" {level * 100:g}% interval {fmt(lo)} to {fmt(hi)}); expected shortfall {fmt(res.shortfalls(i)[0])}"
            f" (SE {fmt(res.shortfall_se(i))}, {fmt(slo)} to {fmt(shi)}); {res.replicates - 1} replicates,"
            f" {res.n_empty(i)} empty.")


def report_bootstrap(miners, res: BootstrapResult, level: float = 0.95, members=None) -> str:
    """One line per item of a run_bootstrap result: the column (a miner, or a class with the `members` lists of a
    class map), its point when there are several, and bootstrap_columns."""
    lines = []
    total = sum(mn.perc for mn in miners)
    for i, it in enumerate(res.items):
        if members is None:
            mn = miners[it.column]
            head = f"  - Miner {mn.id} ({mn.perc}% of network hashrate)"
        else:
            g = members[it.column]
            head = (f"  - Class {it.column} ({len(g)} miners, {sum(miners[k].perc for k in g) * 100.0 / total:g}% of "
                    f"network hashrate)")
        if len(res.points) > 1:
            head += f" at point {it.point}"
        lines.append(head + bootstrap_columns(res, i, level))
    return "\n".join(lines)

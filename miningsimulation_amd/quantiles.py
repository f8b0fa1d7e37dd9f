"""Exact quantiles: order statistics of the per-run terms, selected on the device (include/msim.h: msim_order_stat,
msim_rank_launch, msim_run_order_stats; kernels in csrc/msim_rank.hip).

The reference prints three means per miner (main.cpp:224-234). What a bad year looks like for a 1 % miner is a
quantile of its per-run share, and a histogram (moments.HistSpec) only brackets it by a bin whose range has to be
guessed before the run. The device selects the r-th smallest term of every column by radix selection over the
records a launch leaves in device memory: exact integers, identical for any split of the runs into workgroups,
chunks, launches or ranks, and the per-run records never leave device memory.

Quantities are indexed 0 = found, 1 = stale, 2 = share, 3 = rate (QUANTITIES); share and rate values are Q32.32
terms (moments.ONE is 1.0). Ranks are 0-based; the q-quantile is hist_quantile's: the k-th smallest with
k = max(1, ceil(q N)), i.e. rank k - 1."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import MSIM_MAX_RANKS, MSIM_OK, MSIM_RANK_PASSES, MsimOrderStat, check, lib

QUANTITIES = ("found", "stale", "share", "rate")
MAX_RANKS = MSIM_MAX_RANKS
RANK_PASSES = MSIM_RANK_PASSES
_SCALE = (1.0, 1.0, 2.0 ** -32, 2.0 ** -32)


class OrderStat(NamedTuple):
    """value: the r-th smallest key; below: how many keys are smaller; equal: how many equal it."""
    value: int
    below: int
    equal: int


def quantile_rank(n: int, q: float) -> int:
    """The 0-based rank of the q-quantile of n values in hist_quantile's convention: k - 1 with
    k = max(1, ceil(q n)), q n being the same rounded float product hist_quantile forms, so that the selected value
    always lies in the bin hist_quantile names. (The product of the float's exact value would differ where q n
    rounds to an integer from above: Fraction(0.05) * 20 is just above 1 and would give k = 2 where hist_quantile
    has k = 1; likewise n = 40. quantile_rank_exact is that form.)"""
    if n < 1 or not 0.0 <= q <= 1.0:
        raise ValueError("n must be at least 1 and q within [0, 1]")
    return max(1, math.ceil(q * n)) - 1


def quantile_rank_exact(n: int, q: float) -> int:
    """quantile_rank from the float's exact value (fractions.Fraction, no rounding of q n): what the definition
    gives for the number the float holds, e.g. rank 1 for (20, 0.05) because the float 0.05 is above 1/20."""
    if n < 1 or not 0.0 <= q <= 1.0:
        raise ValueError("n must be at least 1 and q within [0, 1]")
    return max(1, math.ceil(Fraction(q) * n)) - 1


def quantile_ci_ranks(n: int, q: float, z: float = 1.96) -> Tuple[int, int]:
    """The two 0-based ranks (low, high) of the distribution-free confidence interval of the q-quantile: the order
    statistics ceil(n q -+ z sqrt(n q (1 - q))) (1-based), from the normal approximation to the binomial count of
    values below the quantile, clipped to [0, n - 1]. The coverage is approximate: it is the normal approximation's
    (poor for n q or n (1 - q) below about 5), and clipping at either end lowers it."""
    if n < 1 or not 0.0 <= q <= 1.0 or z < 0:
        raise ValueError("n must be at least 1, q within [0, 1] and z non-negative")
    mid, half = n * q, z * math.sqrt(n * q * (1.0 - q))
    clip = (lambda k: min(n - 1, max(0, k - 1)))
    return clip(math.ceil(mid - half)), clip(math.ceil(mid + half))


def order_stats_from_words(words, n_points: int, columns: int, n_ranks: int) -> List[List[List[List[OrderStat]]]]:
    """[n_points * columns * 4 * n_ranks * 3] uint64 words (or int64 holding the same bits) of msim_order_stat ->
    order[point][column][quantity][j] as OrderStat triples of Python ints."""
    a = np.asarray(words).reshape(-1).view(np.uint64) if isinstance(words, np.ndarray) else np.asarray(
        [int(x) & 0xFFFFFFFFFFFFFFFF for x in words], dtype=np.uint64)
    if a.size != n_points * columns * 4 * n_ranks * 3:
        raise ValueError("the words do not match n_points x columns x 4 x n_ranks order statistics")
    flat = a.reshape(n_points, columns, 4, n_ranks, 3).tolist()
    return [[[[OrderStat(*t) for t in row] for row in col] for col in pt] for pt in flat]


def ranks_array(ranks: Sequence[int], n_runs: Optional[int] = None):
    """The ranks as a uint64 array: 1..MAX_RANKS of them, each below n_runs when that is given (msim_ranks_check)."""
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= MAX_RANKS or any(not 0 <= r < 1 << 64 for r in ranks):
        raise ValueError(f"1..{MAX_RANKS} ranks, each a uint64")
    arr = (ctypes.c_uint64 * len(ranks))(*ranks)
    if n_runs is not None and lib.msim_ranks_check(int(n_runs), arr, len(ranks)) != MSIM_OK:
        raise ValueError(f"every rank must be below the run count ({n_runs})")
    return arr


def ranks_of(n_runs: int, qs: Optional[Sequence[float]], ranks: Optional[Sequence[int]]) -> List[int]:
    """The ranks a run_quantiles call selects: `ranks` as given, else quantile_rank of every q."""
    if ranks is not None:
        return [int(r) for r in ranks]
    return [quantile_rank(n_runs, float(q)) for q in qs]


@dataclass
class QuantileResult:
    """What run_quantiles returns: the per-point results (stats_total and sums per miner, as run()'s) plus
    order[point][column][quantity][j] for the j-th of `ranks` (`qs`: the quantiles they came from, or None).
    Columns are miners, or classes when a class map was given."""

    points: list
    ranks: List[int]
    qs: Optional[List[float]]
    order: List[List[List[List[OrderStat]]]]
    n_runs: int = 0

    def value(self, column: int, quantity: str, j: int, point: int = 0) -> float:
        """The j-th selected value of a column as a number: blocks for found and stale, a fraction for share and
        rate (the term scaled by 2^-32)."""
        q = QUANTITIES.index(quantity)
        return self.order[point][column][q][j].value * _SCALE[q]

    @property
    def values(self) -> List[List[List[List[float]]]]:
        """values[point][column][quantity][j]: every selected value scaled as value() scales it."""
        return [[[[o.value * _SCALE[q] for o in row] for q, row in enumerate(col)] for col in pt] for pt in self.order]


# ---------------------------------------------------------------- launches (device tensors from torch)
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else None


def _bytes(t) -> int:
    return t.numel() * t.element_size()


def rank_workspace_bytes(m: int, n_points: int, n_ranks: int) -> int:
    n = int(lib.msim_rank_workspace_bytes(m, n_points, n_ranks))
    if n == 0:
        raise ValueError(f"no workspace for {m} columns, {n_points} points and {n_ranks} ranks")
    return n


def rank_counts_view(m: int, n_points: int, n_ranks: int) -> Tuple[int, int]:
    """(byte offset, uint64 words) of the digit counts inside the workspace: what ranks of a process group
    all-reduce between the count launches and the step launch of a pass."""
    off, words = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.msim_rank_counts_view(m, n_points, n_ranks, ctypes.byref(off), ctypes.byref(words)), "msim_rank_counts_view")
    return int(off.value), int(words.value)


def _launch_rank_begin(m: int, n_points: int, ranks: Sequence[int], d_ws, stream) -> None:
    arr = ranks_array(ranks)
    if _bytes(d_ws) < rank_workspace_bytes(m, n_points, len(arr)):
        raise ValueError("the workspace is smaller than msim_rank_workspace_bytes")
    check(lib.msim_rank_begin_launch(m, n_points, arr, len(arr), _ptr(d_ws), _bytes(d_ws), _stream(stream)),
          "msim_rank_begin_launch")


def _launch_rank_count(m: int, n_points: int, runs_per_point: int, d_per_run, d_best_height, pass_: int, d_ws,
                       stream) -> None:
    need = n_points * runs_per_point
    if _bytes(d_per_run) < need * m * 8 or _bytes(d_best_height) < need * 4:
        raise ValueError("a buffer is smaller than the launch reads")
    check(lib.msim_rank_count_launch(m, n_points, runs_per_point, _ptr(d_per_run), _ptr(d_best_height), pass_,
                                     _ptr(d_ws), _bytes(d_ws), _stream(stream)), "msim_rank_count_launch")


def _launch_rank_step(m: int, n_points: int, pass_: int, d_ws, d_out, d_status, stream) -> None:
    if d_status is None or _bytes(d_status) < 4:
        raise ValueError("d_status is one 32-bit word")
    check(lib.msim_rank_step_launch(m, n_points, pass_, _ptr(d_ws), _bytes(d_ws), _ptr(d_out), _ptr(d_status),
                                    _stream(stream)), "msim_rank_step_launch")


def _run_quantiles(fn, what: str, handle, n_points: int, m: int, n_runs: int, qs, ranks, class_of, n_classes,
                   run_begin: int, seed_base: int, device: int) -> QuantileResult:
    """msim_run_order_stats / msim_sweep_run_order_stats into a QuantileResult."""
    from ._lib import MsimStats, MsimSums
    from .classes import class_count, class_map_struct
    from .simulation import MinerStats, SimulationResult

    sel = ranks_of(n_runs, qs, ranks)
    arr = ranks_array(sel, n_runs)
    if class_of is not None:
        nc = class_count(class_of) if n_classes is None else int(n_classes)
        cmap = class_map_struct(class_of, m, nc)
    else:
        nc, cmap = 0, None
    cols = nc if class_of is not None else m
    stats = (MsimStats * (n_points * m))()
    sums = (MsimSums * (n_points * m))()
    order = (MsimOrderStat * (n_points * cols * 4 * len(sel)))()
    check(fn(handle, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, cmap, nc, arr, len(sel), stats, sums, order), what)
    words = np.ctypeslib.as_array(ctypes.cast(order, ctypes.POINTER(ctypes.c_uint64)), shape=(len(order) * 3,))
    points = [SimulationResult(
        stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
        sums=list(sums[p * m:(p + 1) * m]),
        n_runs=n_runs,
    ) for p in range(n_points)]
    return QuantileResult(points=points, ranks=sel, qs=None if ranks is not None else [float(q) for q in qs],
                          order=order_stats_from_words(words, n_points, cols, len(sel)), n_runs=n_runs)


# ---------------------------------------------------------------- report
def rank_labels(result: QuantileResult) -> List[str]:
    """How report_quantiles names each selected rank: "q0.05" for a quantile, "rank 12" for a rank given directly."""
    if result.qs is not None:
        return [f"q{q:g}" for q in result.qs]
    return [f"rank {r}" for r in result.ranks]


def quantile_columns(col: Sequence[Sequence[OrderStat]], labels: Sequence[str]) -> str:
    """The text report_quantiles (and host/msim_main --quantiles) puts behind a line's head, from one column's
    order[quantity][j]: blocks found, share of blocks and stale rate at every selected rank."""
    found = ", ".join(f"{lb} = {o.value}" for lb, o in zip(labels, col[0]))
    share = ", ".join(f"{lb} = {o.value * _SCALE[2] * 100:g}%" for lb, o in zip(labels, col[2]))
    rate = ", ".join(f"{lb} = {o.value * _SCALE[3] * 100:g}%" for lb, o in zip(labels, col[3]))
    return f" blocks found: {found}; share of blocks: {share}; stale rate: {rate}."


def report_quantiles(miners, result: QuantileResult, point: int = 0, members=None) -> str:
    """One line per miner of a run_quantiles result (per class with the `members` lists of a class map): the
    selected ranks' blocks found, share of blocks and stale rate."""
    cols = result.order[point]
    labels = rank_labels(result)
    if members is None:
        if len(cols) != len(miners):
            raise ValueError(f"{len(cols)} columns in the result, {len(miners)} miners")
        return "\n".join(f"  - Miner {mn.id} ({mn.perc}% of network hashrate)" + quantile_columns(c, labels)
                         for mn, c in zip(miners, cols))
    if len(cols) != len(members):
        raise ValueError(f"{len(cols)} classes in the result, {len(members)} member lists")
    total = sum(mn.perc for mn in miners)
    return "\n".join(f"  - Class {c} ({len(g)} miners, {sum(miners[k].perc for k in g) * 100.0 / total:g}% of network "
                     f"hashrate)" + quantile_columns(col, labels) for c, (g, col) in enumerate(zip(members, cols)))

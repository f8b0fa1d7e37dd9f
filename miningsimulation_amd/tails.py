"""Tail statistics: the moments of a column over the runs below, or at, a quantile of a column (include/msim.h:
msim_tail_item, msim_tail, msim_tail_launch, msim_run_tails; kernel in csrc/msim_tail.hip).

run_quantiles says what a bad year looks like for a 1 % miner as one number. What lies behind that number needs
sums over exactly those runs: how bad they are on average (the expected shortfall), whether the miner's stale rate was
up in them, whose shares rose, and what the same seeds gave at another point of a sweep. The device compares one
column's key with a threshold per run and adds the target column's moments terms for the runs below it and for the
ties, as exact integers; the per-run records never leave device memory, and the sums are identical for any split of
the runs into workgroups, chunks, launches or ranks.

Quantities are indexed as in quantiles.QUANTITIES. A spec names a condition (point, column, quantity), the index of
the selected rank whose order statistic is the threshold, and a target (point, column); an item is a spec with the
threshold filled in. Ties at the threshold are weighted (k - n_below) / n_equal each, the expectation over a uniform
choice among them."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from fractions import Fraction
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import (MSIM_MAX_TAIL_ITEMS, MSIM_OK, MsimMoments, MsimOrderStat, MsimTail, MsimTailItem, MsimTailSpec, check,
                   lib)
from .moments import MOMENT_WORDS, errors_from_moments, join_limbs
from .quantiles import QUANTITIES, QuantileResult, order_stats_from_words, quantile_rank, ranks_array

TAIL_WORDS = 2 + 2 * MOMENT_WORDS
MAX_TAIL_ITEMS = MSIM_MAX_TAIL_ITEMS
SIDES = ("below", "at_most", "above", "at_least")


class TailSpec(NamedTuple):
    cond_point: int
    cond_column: int
    quantity: int
    rank_index: int
    target_point: int
    target_column: int


class TailItem(NamedTuple):
    cond_point: int
    cond_column: int
    quantity: int
    target_point: int
    target_column: int
    value: int


def _quantity(q) -> int:
    return QUANTITIES.index(q) if isinstance(q, str) else int(q)


def own_tails(n_points: int, m: int, quantity="share", rank_index: int = 0) -> List[TailSpec]:
    """Every column conditioned on itself, point-major and column-minor."""
    q = _quantity(quantity)
    return [TailSpec(p, k, q, rank_index, p, k) for p in range(n_points) for k in range(m)]


def tails_given(point: int, column: int, quantity, m: int, rank_index: int = 0,
                target_point: Optional[int] = None) -> List[TailSpec]:
    """All m columns (of target_point, default the condition's) given one condition, column-minor."""
    tp = point if target_point is None else target_point
    return [TailSpec(point, column, _quantity(quantity), rank_index, tp, k) for k in range(m)]


def specs_struct(specs: Sequence[TailSpec], n_points: int, columns: int, n_ranks: int):
    """The specs as an msim_tail_spec array, checked against the points, columns and ranks of a run."""
    specs = [TailSpec(*(int(x) for x in s)) for s in specs]
    if not 1 <= len(specs) <= MAX_TAIL_ITEMS:
        raise ValueError(f"1..{MAX_TAIL_ITEMS} tail specs")
    for s in specs:
        if not (0 <= s.cond_point < n_points and 0 <= s.target_point < n_points and 0 <= s.cond_column < columns
                and 0 <= s.target_column < columns and 0 <= s.quantity < 4 and 0 <= s.rank_index < n_ranks):
            raise ValueError(f"{s} lies outside {n_points} points x {columns} columns x {n_ranks} ranks")
    return specs, (MsimTailSpec * len(specs))(*[MsimTailSpec(*s) for s in specs])


def items_words(items: Sequence[TailItem]) -> np.ndarray:
    """[n, 8] uint32 words of msim_tail_item (reserved = 0), e.g. for torch.from_numpy(...view(np.int32))."""
    out = np.zeros((len(items), 8), dtype=np.uint32)
    for i, it in enumerate(items):
        v = int(it.value)
        if not 0 <= v < 1 << 64 or any(not 0 <= int(x) <= 0xFFFFFFFF for x in it[:5]):
            raise ValueError(f"{it} does not fit msim_tail_item")
        out[i] = (it.cond_point, it.cond_column, it.quantity, it.target_point, it.target_column, 0,
                  v & 0xFFFFFFFF, v >> 32)
    return out


def items_check(items: Sequence[TailItem], n_points: int, m: int) -> bool:
    """msim_tail_items_check: whether there are 1..MAX_TAIL_ITEMS items and all lie within n_points x m."""
    w = np.ascontiguousarray(items_words(items))
    ptr = ctypes.cast(ctypes.c_void_p(w.ctypes.data), ctypes.POINTER(MsimTailItem)) if len(items) else None
    return lib.msim_tail_items_check(m, n_points, ptr, len(items)) == MSIM_OK


def items_from_specs(specs: Sequence[TailSpec], order) -> List[TailItem]:
    """The items of `specs` at the order statistics order[point][column][quantity][j]."""
    return [TailItem(s.cond_point, s.cond_column, s.quantity, s.target_point, s.target_column,
                     order[s.cond_point][s.cond_column][s.quantity][s.rank_index].value) for s in specs]


def tail_from_words(row) -> dict:
    """One item's 42 msim_tail words -> {n_below, n_equal, below, equal} with the moments as join_limbs dicts."""
    w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in row]
    assert len(w) == TAIL_WORDS
    return {"n_below": w[0], "n_equal": w[1], "below": join_limbs(w[2:2 + MOMENT_WORDS]),
            "equal": join_limbs(w[2 + MOMENT_WORDS:])}


def tails_from_words(words) -> List[dict]:
    return [tail_from_words(r) for r in np.asarray(words).reshape(-1, TAIL_WORDS).tolist()]


def _launch_tails(m: int, n_points: int, runs_per_point: int, d_per_run, d_best_height, d_items, n_items: int, d_tails,
                  stream) -> None:
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr()))
    sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    need = n_points * runs_per_point
    if (d_per_run.numel() * d_per_run.element_size() < need * m * 8 or
            d_best_height.numel() * d_best_height.element_size() < need * 4 or
            d_items.numel() * d_items.element_size() < n_items * 32 or
            d_tails.numel() * d_tails.element_size() < n_items * TAIL_WORDS * 8):
        raise ValueError("a buffer is smaller than the launch reads or writes")
    check(lib.msim_tail_launch(m, n_points, runs_per_point, ptr(d_per_run), ptr(d_best_height), ptr(d_items), n_items,
                               ptr(d_tails), sh), "msim_tail_launch")


def _u64_words(words, shape) -> np.ndarray:
    a = np.asarray(words)
    a = a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)
    return np.ascontiguousarray(a.reshape(shape))


@dataclass
class TailResult(QuantileResult):
    """What run_tails returns: QuantileResult's fields, the columns' total moments (moments[point][column], Python
    ints) and per spec the tail (tails[i]: n_below, n_equal and the target's moments below and at the threshold).
    The raw words are kept for msim_tail_side / msim_tail_means, whose complements are limb-wise differences."""

    specs: List[TailSpec] = field(default_factory=list)
    items: List[TailItem] = field(default_factory=list)
    moments: List[List[dict]] = field(default_factory=list)
    tails: List[dict] = field(default_factory=list)
    moment_words: Optional[np.ndarray] = field(default=None, compare=False)  # [points, columns, 20] uint64
    tail_words: Optional[np.ndarray] = field(default=None, compare=False)    # [n_specs, 42] uint64

    def _c_tail(self, i: int):
        t = MsimTail()
        ctypes.memmove(ctypes.byref(t), self.tail_words[i].ctypes.data, TAIL_WORDS * 8)
        s = self.specs[i]
        tot = MsimMoments()
        ctypes.memmove(ctypes.byref(tot), self.moment_words[s.target_point, s.target_column].ctypes.data, MOMENT_WORDS * 8)
        return t, tot

    def side(self, i: int, which: str) -> Tuple[dict, int]:
        """msim_tail_side: (the target's moments over the runs of one side of spec i's threshold, their count)."""
        t, tot = self._c_tail(i)
        out, n = MsimMoments(), ctypes.c_uint64()
        check(lib.msim_tail_side(ctypes.byref(t), ctypes.byref(tot), self.n_runs, SIDES.index(which), ctypes.byref(out),
                                 ctypes.byref(n)), "msim_tail_side")
        words = np.ctypeslib.as_array(ctypes.cast(ctypes.byref(out), ctypes.POINTER(ctypes.c_uint64)), shape=(MOMENT_WORDS,))
        return join_limbs(words.tolist()), int(n.value)

    def k(self, i: int, upper: bool = False) -> int:
        """How many runs spec i's tail holds: rank + 1 smallest, or n_runs - rank largest."""
        r = self.ranks[self.specs[i].rank_index]
        return self.n_runs - r if upper else r + 1

    def means(self, i: int, upper: bool = False) -> dict:
        """msim_tail_means: the target's mean found, stale, share and rate over the k smallest (largest) runs of
        the condition, k from the rank, ties weighted (k - n_strict) / n_equal."""
        t, tot = self._c_tail(i)
        out = (ctypes.c_double * 4)()
        check(lib.msim_tail_means(ctypes.byref(t), ctypes.byref(tot), self.n_runs, self.k(i, upper), int(bool(upper)), out),
              "msim_tail_means")
        return dict(zip(QUANTITIES, out))

    def own_item(self, column: int, point: int = 0) -> int:
        """The index of the first spec that conditions (point, column) on itself."""
        for i, s in enumerate(self.specs):
            if (s.cond_point, s.cond_column) == (point, column) == (s.target_point, s.target_column):
                return i
        raise ValueError(f"no spec conditions column {column} of point {point} on itself")

    def target_item(self, column: int, point: int = 0) -> int:
        """The index of the first spec whose target is (point, column)."""
        for i, s in enumerate(self.specs):
            if (s.target_point, s.target_column) == (point, column):
                return i
        raise ValueError(f"no spec has column {column} of point {point} as its target")

    def expected_shortfall(self, column: int, point: int = 0) -> Fraction:
        """(S_below + (k - n_below) value) / k of the column's own conditioned quantity, exact, in the quantity's
        units (terms of 2^-32 for share and rate)."""
        i = self.own_item(column, point)
        t, k = self.tails[i], self.k(i)
        s_below = t["below"][QUANTITIES[self.specs[i].quantity]]
        return Fraction(s_below + (k - t["n_below"]) * self.items[i].value, k)

    def errors(self, i: int, which: str = "below") -> dict:
        """error_bars' arithmetic on one side: the conditional means and the standard errors of a sample of that
        many runs GIVEN the threshold (the threshold's own sampling error is not in them)."""
        mo, n = self.side(i, which)
        if n == 0:
            raise ValueError("the side holds no run")
        return errors_from_moments([mo], n)[0]


def _q_list(q) -> List[float]:
    return [float(x) for x in q] if isinstance(q, (list, tuple)) else [float(q)]


def make_result(points, sel, qs, order, n_runs, specs, moment_words, tail_words) -> TailResult:
    n_points, cols = len(order), len(order[0])
    mw = _u64_words(moment_words, (n_points, cols, MOMENT_WORDS))
    tw = _u64_words(tail_words, (len(specs), TAIL_WORDS))
    return TailResult(points=points, ranks=sel, qs=qs, order=order, n_runs=n_runs, specs=list(specs),
                      items=items_from_specs(specs, order),
                      moments=[[join_limbs(r) for r in pt] for pt in mw.tolist()], tails=tails_from_words(tw),
                      moment_words=mw, tail_words=tw)


def _run_tails(fn, what: str, handle, n_points: int, m: int, n_runs: int, q, ranks, specs, class_of, n_classes,
               run_begin: int, seed_base: int, device: int) -> TailResult:
    """msim_run_tails / msim_sweep_run_tails into a TailResult."""
    from ._lib import MsimStats, MsimSums
    from .classes import class_count, class_map_struct
    from .simulation import MinerStats, SimulationResult

    qs = None if ranks is not None else _q_list(q)
    sel = [int(r) for r in ranks] if ranks is not None else [quantile_rank(n_runs, x) for x in qs]
    arr = ranks_array(sel, n_runs)
    if class_of is not None:
        nc = class_count(class_of) if n_classes is None else int(n_classes)
        cmap = class_map_struct(class_of, m, nc)
    else:
        nc, cmap = 0, None
    cols = nc if class_of is not None else m
    specs, sarr = specs_struct(own_tails(n_points, cols) if specs is None else specs, n_points, cols, len(sel))
    stats = (MsimStats * (n_points * m))()
    sums = (MsimSums * (n_points * m))()
    order = (MsimOrderStat * (n_points * cols * 4 * len(sel)))()
    mom = (MsimMoments * (n_points * cols))()
    tails = (MsimTail * len(specs))()
    check(fn(handle, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, cmap, nc, arr, len(sel), sarr, len(specs), stats,
             sums, order, mom, tails), what)
    as_words = (lambda a, n: np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy())
    points = [SimulationResult(
        stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
        sums=list(sums[p * m:(p + 1) * m]),
        n_runs=n_runs,
    ) for p in range(n_points)]
    return make_result(points, sel, qs, order_stats_from_words(as_words(order, len(order) * 3), n_points, cols, len(sel)),
                       n_runs, specs, as_words(mom, len(mom) * MOMENT_WORDS), as_words(tails, len(tails) * TAIL_WORDS))


# ---------------------------------------------------------------- report
def tail_columns(k: int, n_runs: int, means: dict, all_runs: dict, given: str = "") -> str:
    """The text report_tails (and host/msim_main --tails) puts behind a line's head: the k of N runs (the column's
    own worst ones, or those `given` names), then blocks found, share of blocks and stale rate averaged over them,
    each next to its all-runs mean."""
    which = f"in the {k} of {n_runs} runs with {given}" if given else f"in its worst {k} of {n_runs} runs"
    return (f" {which} found {means['found']:g} blocks (all runs: {all_runs['found_mean']:g})"
            f" i.e. {means['share'] * 100:g}% of blocks ({all_runs['share_mean'] * 100:g}%)."
            f" Stale rate: {means['rate'] * 100:g}% ({all_runs['rate_mean'] * 100:g}%).")


def report_tails(miners, result: TailResult, point: int = 0, members=None) -> str:
    """One line per miner of a run_tails result (per class with the `members` lists of a class map), from the first
    spec whose target is the column: the k of N runs, then blocks found, share and stale rate averaged over them (the
    column's own worst runs, or those of the spec's condition), next to the all-runs means."""
    cols = result.moments[point]
    all_runs = errors_from_moments(cols, result.n_runs)
    tail = []
    for c in range(len(cols)):
        i = result.target_item(c, point)
        s = result.specs[i]
        own = (s.cond_point, s.cond_column) == (point, c)
        given = "" if own else (f"the lowest {QUANTITIES[s.quantity]} of column {s.cond_column}" +
                                (f" at point {s.cond_point}" if s.cond_point != point else ""))
        tail.append(tail_columns(result.k(i), result.n_runs, result.means(i), all_runs[c], given))
    if members is None:
        if len(cols) != len(miners):
            raise ValueError(f"{len(cols)} columns in the result, {len(miners)} miners")
        return "\n".join(f"  - Miner {mn.id} ({mn.perc}% of network hashrate)" + t for mn, t in zip(miners, tail))
    if len(cols) != len(members):
        raise ValueError(f"{len(cols)} classes in the result, {len(members)} member lists")
    total = sum(mn.perc for mn in miners)
    return "\n".join(f"  - Class {c} ({len(g)} miners, {sum(miners[k].perc for k in g) * 100.0 / total:g}% of network "
                     f"hashrate)" + t for c, (g, t) in enumerate(zip(members, tail)))

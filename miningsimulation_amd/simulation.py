"""Host-side mirror of the reference's configuration and driver surface, over libmsim's C ABI.

Reference surface (/root/reference/main.cpp):
  SIM_DURATION  main.cpp:7    months{12} = 31 556 952 000 ms
  SIM_RUNS      main.cpp:10   16 * 2048
  SetupMiners   main.cpp:44-65
  MinerStats    main.cpp:13-41 (blocks_found, blocks_share, stale_rate; operator+=)
  main          main.cpp:195-235 (batch driver + report)
and Miner(id, perc, propagation, selfish=false) from simulation.h:57-59.

Simulation.run() is the GPU replacement for main()'s std::async loop; report() prints main.cpp:224-234's
lines so outputs can be diffed against the reference's stdout.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (MSIM_SWEEP_SHARED_DRAWS, MsimCross, MsimMiner, MsimMoments, MsimRunRecord, MsimStats, MsimSums,
                   MsimSweepPlan, MsimTiming, check, lib)
from .classes import class_count, class_map_struct
from .contrasts import CROSS_WORDS, Pair, cross_from_words, pairs_struct
from .moments import MOMENT_WORDS, HistSpec, moments_from_words
from .quantiles import (QuantileResult, _launch_rank_begin, _launch_rank_count, _launch_rank_step, _run_quantiles,
                        rank_counts_view, rank_workspace_bytes)
from .tails import TailResult, TailSpec, _launch_tails, _run_tails
from .bootstrap import (DEFAULT_BOOT_SEED, BootItem, BootstrapResult, _launch_boot_begin, _launch_boot_below,
                        _launch_boot_count, _launch_boot_step, _run_bootstrap)

SIM_DURATION_MS = 31_556_952_000  # main.cpp:7 std::chrono::months{12}
SIM_RUNS = 16 * 2048              # main.cpp:10
BLOCK_INTERVAL_MS = 600_000       # simulation.h:16
DEFAULT_SEED_BASE = 1000          # SURVEY §8d seed convention


@dataclass(frozen=True)
class Miner:
    """Miner(unsigned id, uint64_t perc, milliseconds prop, bool selfish) — simulation.h:57-59."""

    id: int
    perc: int
    propagation_ms: int
    is_selfish: bool = False


def setup_miners(propagation_ms: int = 1000, selfish_perc: Optional[int] = None) -> List[Miner]:
    """SetupMiners() (main.cpp:44-65): the 2025 hashrate approximation, homogeneous propagation.

    With ``selfish_perc`` = h, miner 0 is selfish with h% and miner 1 gets 59-h% (README.md:85-107 uses
    h = 40; SURVEY §8d C4 sweeps h over 10..49)."""
    percs = [30, 29, 12, 11, 8, 5, 3, 1, 1]
    selfish = False
    if selfish_perc is not None:
        percs[0], percs[1] = selfish_perc, 59 - selfish_perc
        selfish = True
    return [Miner(k, p, propagation_ms, selfish and k == 0) for k, p in enumerate(percs)]


# BASELINE.json configs: C1 plumbing, C2 single-GPU bench, C3 selfish 40%.
PRESETS = {
    "c1": lambda: setup_miners(10_000),
    "c2": lambda: setup_miners(100),
    "c3": lambda: setup_miners(1_000, selfish_perc=40),
    "default": lambda: setup_miners(1_000),
}
C5_TOTAL_WEIGHT = 102_400


def c5_network(propagation_ms: int = 1000) -> List[Miner]:
    """BASELINE.json configs[4]: 2 pools + 1024 small miners, integer weights summing to
    W = 102400 (pool 0 30%, pool 1 29%, 1024 x 41 = 41%), all honest. Not expressible in the reference
    (integer percentages summing to 100, main.cpp:43); run with Simulation(..., total_weight=C5_TOTAL_WEIGHT)."""
    w = [30720, 29696] + [41] * 1024
    return [Miner(k, x, propagation_ms) for k, x in enumerate(w)]


PRESET_WEIGHTS = {"c5": C5_TOTAL_WEIGHT}
PRESETS["c5"] = c5_network
C4_SELFISH_PERCS = list(range(10, 50))
C4_PROPAGATIONS_MS = [100, 250, 500, 1000, 2000, 5000, 10000, 20000, 30000]


def c4_grid() -> List[List[Miner]]:
    """The 360-point sweep of BASELINE.json configs[3]: h in 10..49 x propagation 0.1..30 s."""
    return [setup_miners(p, selfish_perc=h) for h in C4_SELFISH_PERCS for p in C4_PROPAGATIONS_MS]


@dataclass
class MinerStats:
    """MinerStats (main.cpp:13-41)."""

    blocks_found: int = 0
    blocks_share: float = 0.0
    stale_rate: float = 0.0

    def __iadd__(self, other: "MinerStats") -> "MinerStats":  # main.cpp:34-40
        self.blocks_found += other.blocks_found
        self.blocks_share += other.blocks_share
        self.stale_rate += other.stale_rate
        return self


@dataclass
class SimulationResult:
    stats_total: List[MinerStats]              # like main.cpp:199 stats_total (sums over runs)
    sums: List[MsimSums]                        # fixed-point device sums
    found: Optional[np.ndarray] = None          # [n_runs, M] uint32, per-run blocks_found
    stale: Optional[np.ndarray] = None          # [n_runs, M] uint32, per-run stale_blocks
    best_height: Optional[np.ndarray] = None    # [n_runs] uint32, |best chain| - 1
    n_runs: int = 0
    extra: dict = field(default_factory=dict)
    moments: Optional[list] = None              # per-miner dicts of Python ints (moments.join_limbs): run_moments
    hist: Optional[np.ndarray] = None           # [M, 2, bins + 2] uint64 counts (0 = share, 1 = rate), or None


@dataclass
class ContrastResult:
    """What run_contrasts returns: the per-point results (moments filled) plus the pairs and their cross sums.
    contrasts(result) turns them into differences, ratios and correlations with standard errors."""

    points: List[SimulationResult]   # one per sweep point (one for a Simulation)
    pairs: List[Pair]
    cross: List[dict]                # per pair Python ints (contrasts.join_cross)
    n_runs: int = 0


def _launch_moments(m: int, n_points: int, runs_per_point: int, d_per_run, d_best_height, d_moments,
                    hist_spec: Optional[HistSpec], d_hist, stream) -> None:
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None)
    sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    if (hist_spec is None) != (d_hist is None):
        raise ValueError("hist_spec and d_hist go together")
    need = n_points * runs_per_point
    if (d_per_run.numel() * d_per_run.element_size() < need * m * 8 or
            d_best_height.numel() * d_best_height.element_size() < need * 4 or
            d_moments.numel() * d_moments.element_size() < n_points * m * MOMENT_WORDS * 8 or
            (d_hist is not None and
             d_hist.numel() * d_hist.element_size() < n_points * m * 2 * (hist_spec.bins + 2) * 8)):
        raise ValueError("a buffer is smaller than the launch reads or writes")
    spec = ctypes.byref(hist_spec.struct()) if hist_spec is not None else None
    check(lib.msim_moments_launch(m, n_points, runs_per_point, ptr(d_per_run), ptr(d_best_height), spec,
                                  ptr(d_moments), ptr(d_hist), sh), "msim_moments_launch")


def _launch_cross(m: int, n_points: int, runs_per_point: int, d_per_run, d_best_height, d_pairs, n_pairs: int,
                  d_cross, stream) -> None:
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr()))
    sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    need = n_points * runs_per_point
    if (d_per_run.numel() * d_per_run.element_size() < need * m * 8 or
            d_best_height.numel() * d_best_height.element_size() < need * 4 or
            d_pairs.numel() * d_pairs.element_size() < n_pairs * 16 or
            d_cross.numel() * d_cross.element_size() < n_pairs * CROSS_WORDS * 8):
        raise ValueError("a buffer is smaller than the launch reads or writes")
    check(lib.msim_cross_launch(m, n_points, runs_per_point, ptr(d_per_run), ptr(d_best_height), ptr(d_pairs),
                                n_pairs, ptr(d_cross), sh), "msim_cross_launch")


def _run_contrasts(fn, what: str, handle, n_points: int, m: int, n_runs: int, pairs: Sequence[Pair], run_begin: int,
                   seed_base: int, device: int) -> ContrastResult:
    pairs = [Pair(*q) for q in pairs]
    arr = pairs_struct(pairs, n_points, m)
    cross = (MsimCross * len(pairs))()
    points = _run_moments(
        lambda h, b, n, sb, dev, stats, sums, mom, spec, counts: fn(h, b, n, sb, dev, arr, len(pairs), stats, sums,
                                                                     mom, cross),
        what, handle, n_points, m, n_runs, run_begin, seed_base, device, None)
    words = np.ctypeslib.as_array(ctypes.cast(cross, ctypes.POINTER(ctypes.c_uint64)), shape=(len(pairs), CROSS_WORDS))
    return ContrastResult(points=points, pairs=pairs, cross=cross_from_words(words), n_runs=n_runs)


def _run_moments(fn, what: str, handle, n_points: int, m: int, n_runs: int, run_begin: int, seed_base: int,
                 device: int, hist: Optional[HistSpec]) -> List[SimulationResult]:
    nm = n_points * m
    stats = (MsimStats * nm)()
    sums = (MsimSums * nm)()
    mom = (MsimMoments * nm)()
    row = hist.bins + 2 if hist is not None else 0
    counts = (ctypes.c_uint64 * (nm * 2 * row))() if hist is not None else None
    spec = ctypes.byref(hist.struct()) if hist is not None else None
    check(fn(handle, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, stats, sums, mom, spec, counts), what)
    words = np.ctypeslib.as_array(ctypes.cast(mom, ctypes.POINTER(ctypes.c_uint64)), shape=(nm, MOMENT_WORDS))
    h = np.ctypeslib.as_array(counts).reshape(n_points, m, 2, row).copy() if hist is not None else None
    return [SimulationResult(
        stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
        sums=list(sums[p * m:(p + 1) * m]),
        n_runs=n_runs,
        moments=moments_from_words(words[p * m:(p + 1) * m]),
        hist=h[p] if h is not None else None,
    ) for p in range(n_points)]


def _launch_fold(m: int, n_points: int, runs_per_point: int, d_per_run, d_class_of, n_classes: int, d_class_run,
                 stream) -> None:
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr()))
    sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    need = n_points * runs_per_point
    if (d_per_run.numel() * d_per_run.element_size() < need * m * 8 or
            d_class_of.numel() * d_class_of.element_size() < m * 4 or
            d_class_run.numel() * d_class_run.element_size() < need * n_classes * 8):
        raise ValueError("a buffer is smaller than the launch reads or writes")
    check(lib.msim_fold_launch(m, n_points, runs_per_point, ptr(d_per_run), ptr(d_class_of), n_classes,
                               ptr(d_class_run), sh), "msim_fold_launch")


def _run_classes(fn, what: str, handle, n_points: int, m: int, n_runs: int, class_of: Sequence[int],
                 n_classes: Optional[int], pairs: Optional[Sequence[Pair]], hist: Optional[HistSpec], run_begin: int,
                 seed_base: int, device: int):
    """The per-point SimulationResults of msim_run_classes / msim_sweep_run_classes (stats_total and sums per miner,
    moments and hist per class), inside a ContrastResult when pairs of (point, class) columns were given."""
    nc = class_count(class_of) if n_classes is None else int(n_classes)
    cmap = class_map_struct(class_of, m, nc)
    stats = (MsimStats * (n_points * m))()
    sums = (MsimSums * (n_points * m))()
    mom = (MsimMoments * (n_points * nc))()
    row = hist.bins + 2 if hist is not None else 0
    counts = (ctypes.c_uint64 * (n_points * nc * 2 * row))() if hist is not None else None
    spec = ctypes.byref(hist.struct()) if hist is not None else None
    if pairs is not None:
        pairs = [Pair(*q) for q in pairs]
        arr = pairs_struct(pairs, n_points, nc)
        cross = (MsimCross * len(pairs))()
    else:
        arr, cross = None, None
    check(fn(handle, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, cmap, nc, arr, len(pairs) if pairs else 0,
             stats, sums, mom, spec, counts, cross), what)
    words = np.ctypeslib.as_array(ctypes.cast(mom, ctypes.POINTER(ctypes.c_uint64)), shape=(n_points * nc, MOMENT_WORDS))
    h = np.ctypeslib.as_array(counts).reshape(n_points, nc, 2, row).copy() if hist is not None else None
    points = [SimulationResult(
        stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
        sums=list(sums[p * m:(p + 1) * m]),
        n_runs=n_runs,
        moments=moments_from_words(words[p * nc:(p + 1) * nc]),
        hist=h[p] if h is not None else None,
    ) for p in range(n_points)]
    if pairs is None:
        return points
    cw = np.ctypeslib.as_array(ctypes.cast(cross, ctypes.POINTER(ctypes.c_uint64)), shape=(len(pairs), CROSS_WORDS))
    return ContrastResult(points=points, pairs=pairs, cross=cross_from_words(cw), n_runs=n_runs)


def _miners_struct(miners: Sequence[Miner]):
    arr = (MsimMiner * len(miners))()
    for i, m in enumerate(miners):
        arr[i] = MsimMiner(m.id, m.perc, m.propagation_ms, 1 if m.is_selfish else 0)
    return arr


class Simulation:
    """A network description bound to the device library (msim_config)."""

    def __init__(self, miners: Sequence[Miner], duration_ms: int = SIM_DURATION_MS, total_weight: int = 100):
        """total_weight = 100: Miner.perc are the reference's integer percentages (SetupMiners, main.cpp:43).
        Otherwise Miner.perc are integer weights summing to total_weight."""
        self.miners = list(miners)
        self.duration_ms = int(duration_ms)
        self.total_weight = int(total_weight)
        handle = ctypes.c_void_p()
        if self.total_weight == 100:
            check(lib.msim_config_create(_miners_struct(self.miners), len(self.miners), self.duration_ms,
                                         ctypes.byref(handle)), "msim_config_create")
        else:
            check(lib.msim_config_create_weighted(_miners_struct(self.miners), len(self.miners), self.duration_ms,
                                                  self.total_weight, ctypes.byref(handle)), "msim_config_create_weighted")
        self._h = handle

    @property
    def wide(self) -> bool:
        """True when the network runs on the large-network pipeline (msim_wide.h)."""
        return bool(lib.msim_config_is_wide(self._h))

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def set_concurrent_launches(self, n: int) -> None:
        """msim_config_set_concurrent_launches: how many launches of this config the caller keeps in flight
        (e.g. steps alternating over n HIP streams). A grid-planning hint, no effect on results; it changes
        workspace_bytes, so call it before sizing the workspace."""
        check(lib.msim_config_set_concurrent_launches(self._h, int(n)), "msim_config_set_concurrent_launches")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.msim_config_destroy(h)
            self._h = None

    def run(self, n_runs: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE, device: int = 0,
            per_run: bool = False) -> SimulationResult:
        m = len(self.miners)
        stats = (MsimStats * m)()
        sums = (MsimSums * m)()
        rec = (MsimRunRecord * (n_runs * m))() if per_run else None
        bh = (ctypes.c_uint32 * n_runs)() if per_run else None
        check(lib.msim_run(self._h, run_begin, n_runs, seed_base & 0xFFFFFFFF, device, stats, sums, rec, bh), "msim_run")
        res = SimulationResult(
            stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats],
            sums=list(sums),
            n_runs=n_runs,
        )
        if per_run:
            a = np.ctypeslib.as_array(ctypes.cast(rec, ctypes.POINTER(ctypes.c_uint32)), shape=(n_runs, m, 2)).copy()
            res.found = a[:, :, 0]
            res.stale = a[:, :, 1]
            res.best_height = np.ctypeslib.as_array(bh).copy()
        return res

    def run_moments(self, n_runs: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE, device: int = 0,
                    hist: Optional[HistSpec] = None) -> SimulationResult:
        """msim_run_moments: run() plus the exact second moments of the per-run terms (`moments`) and, with a
        HistSpec, their histograms (`hist`); the per-run records never leave device memory. error_bars(result)
        turns the moments into standard errors."""
        return _run_moments(lib.msim_run_moments, "msim_run_moments", self._h, 1, len(self.miners), n_runs, run_begin,
                            seed_base, device, hist)[0]

    def launch_moments(self, n_runs: int, d_per_run, d_best_height, d_moments, hist_spec: Optional[HistSpec] = None,
                       d_hist=None, stream=None) -> None:
        """msim_moments_launch on the current device over a launch's records: d_per_run int32 [n_runs, M, 2],
        d_best_height int32 [n_runs], d_moments int64 [M, 20] and d_hist int64 [M, 2, bins + 2] (overwritten)."""
        _launch_moments(len(self.miners), 1, n_runs, d_per_run, d_best_height, d_moments, hist_spec, d_hist, stream)

    def run_contrasts(self, n_runs: int, pairs: Sequence[Pair], run_begin: int = 0,
                      seed_base: int = DEFAULT_SEED_BASE, device: int = 0) -> ContrastResult:
        """msim_run_contrasts: run_moments() plus the exact cross sums of `pairs` (every pair within point 0, e.g.
        pairs_between_miners(M)); contrasts(result) gives the differences between miners with standard errors."""
        return _run_contrasts(lib.msim_run_contrasts, "msim_run_contrasts", self._h, 1, len(self.miners), n_runs,
                              pairs, run_begin, seed_base, device)

    def launch_cross(self, n_runs: int, d_per_run, d_best_height, d_pairs, n_pairs: int, d_cross, stream=None) -> None:
        """msim_cross_launch on the current device over a launch's records: d_pairs int32 [n_pairs, 4] and d_cross
        int64 [n_pairs, 12] (overwritten); the other buffers as launch_moments."""
        _launch_cross(len(self.miners), 1, n_runs, d_per_run, d_best_height, d_pairs, n_pairs, d_cross, stream)

    def run_classes(self, n_runs: int, class_of: Sequence[int], pairs: Optional[Sequence[Pair]] = None,
                    hist: Optional[HistSpec] = None, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                    device: int = 0, n_classes: Optional[int] = None):
        """msim_run_classes: run_moments() per class of a class map (classes_of, classes_from_groups): `moments` and
        `hist` have one entry per class (the class as one miner), stats_total and sums stay per miner. n_classes
        defaults to one past the map's largest class. With `pairs` of (point, class) columns (every pair within
        point 0, e.g. pairs_between_miners(n_classes)) the result is a ContrastResult whose `cross` is per class
        too. error_bars, hist_quantile, contrasts and report_contrasts work on the results unchanged."""
        res = _run_classes(lib.msim_run_classes, "msim_run_classes", self._h, 1, len(self.miners), n_runs, class_of,
                           n_classes, pairs, hist, run_begin, seed_base, device)
        return res if pairs is not None else res[0]

    def launch_fold(self, n_runs: int, d_per_run, d_class_of, n_classes: int, d_class_run, stream=None) -> None:
        """msim_fold_launch on the current device over a launch's records: d_per_run int32 [n_runs, M, 2], d_class_of
        int32 [M] (NONE = -1) and d_class_run int32 [n_runs, n_classes, 2] (every record overwritten); launch_moments
        and launch_cross of a Simulation of n_classes miners read d_class_run as they read d_per_run."""
        _launch_fold(len(self.miners), 1, n_runs, d_per_run, d_class_of, n_classes, d_class_run, stream)

    def run_quantiles(self, n_runs: int, qs: Sequence[float] = (0.05, 0.5, 0.95), ranks: Optional[Sequence[int]] = None,
                      class_of: Optional[Sequence[int]] = None, n_classes: Optional[int] = None, run_begin: int = 0,
                      seed_base: int = DEFAULT_SEED_BASE, device: int = 0) -> QuantileResult:
        """msim_run_order_stats: run() plus the exact order statistics of the per-run found, stale, share and rate
        terms of every miner (of every class with a class map) at the quantiles `qs` (quantile_rank), or at the
        0-based `ranks` when given; the per-run records never leave device memory. result.order[0][column]
        [quantity][j] is an OrderStat (value, below, equal) of Python ints; result.values scales them."""
        return _run_quantiles(lib.msim_run_order_stats, "msim_run_order_stats", self._h, 1, len(self.miners), n_runs,
                              qs, ranks, class_of, n_classes, run_begin, seed_base, device)

    def rank_workspace_bytes(self, n_ranks: int, columns: Optional[int] = None) -> int:
        """msim_rank_workspace_bytes for this network's columns (`columns`: the class count of folded records)."""
        return rank_workspace_bytes(columns or len(self.miners), 1, n_ranks)

    def rank_counts_view(self, n_ranks: int, columns: Optional[int] = None):
        """msim_rank_counts_view: (byte offset, uint64 words) of the counts inside the workspace."""
        return rank_counts_view(columns or len(self.miners), 1, n_ranks)

    def launch_rank_begin(self, ranks: Sequence[int], d_ws, stream=None, columns: Optional[int] = None) -> None:
        """msim_rank_begin_launch on the current device: d_ws uint8 [rank_workspace_bytes(len(ranks))] or larger."""
        _launch_rank_begin(columns or len(self.miners), 1, ranks, d_ws, stream)

    def launch_rank_count(self, n_runs: int, d_per_run, d_best_height, pass_: int, d_ws, stream=None,
                          columns: Optional[int] = None) -> None:
        """msim_rank_count_launch of pass `pass_` over a launch's records (as launch_moments reads them); it adds to
        the workspace's counts, so several record buffers feed one pass."""
        _launch_rank_count(columns or len(self.miners), 1, n_runs, d_per_run, d_best_height, pass_, d_ws, stream)

    def launch_rank_step(self, pass_: int, d_ws, d_out, d_status, stream=None, columns: Optional[int] = None) -> None:
        """msim_rank_step_launch of pass `pass_`: d_out int64 [M, 4, n_ranks, 3] (required at the last pass, else it
        may be None), d_status int32 [1] (added to)."""
        _launch_rank_step(columns or len(self.miners), 1, pass_, d_ws, d_out, d_status, stream)

    def run_tails(self, n_runs: int, q=0.05, *, ranks: Optional[Sequence[int]] = None,
                  specs: Optional[Sequence[TailSpec]] = None, class_of: Optional[Sequence[int]] = None,
                  n_classes: Optional[int] = None, seed_base: int = DEFAULT_SEED_BASE, run_begin: int = 0,
                  device: int = 0) -> TailResult:
        """msim_run_tails: run_quantiles() at the quantile(s) `q` (or the 0-based `ranks`) plus the columns' total
        moments and, per spec (tails.own_tails by default: every column's own share at rank index 0), the target
        column's moments over the runs below and at the selected order statistic. result.means(i),
        result.expected_shortfall(column), result.side(i, ...) and report_tails(miners, result) work on it."""
        return _run_tails(lib.msim_run_tails, "msim_run_tails", self._h, 1, len(self.miners), n_runs, q, ranks, specs,
                          class_of, n_classes, run_begin, seed_base, device)

    def launch_tails(self, n_runs: int, d_per_run, d_best_height, d_items, n_items: int, d_tails, stream=None,
                     columns: Optional[int] = None) -> None:
        """msim_tail_launch on the current device over a launch's records: d_items int32 [n_items, 8]
        (tails.items_words) and d_tails int64 [n_items, 42] (overwritten); the other buffers as launch_moments."""
        _launch_tails(columns or len(self.miners), 1, n_runs, d_per_run, d_best_height, d_items, n_items, d_tails, stream)

    def run_bootstrap(self, n_runs: int, items: Optional[Sequence[BootItem]] = None, qs: Sequence[float] = (0.05,),
                      replicates: int = 200, boot_seed: int = DEFAULT_BOOT_SEED,
                      class_of: Optional[Sequence[int]] = None, n_classes: Optional[int] = None,
                      seed_base: int = DEFAULT_SEED_BASE, run_begin: int = 0, device: int = 0) -> BootstrapResult:
        """msim_run_bootstrap: run_quantiles() at `qs` plus the Poisson bootstrap of `items` (bootstrap.own_bootstrap
        by default: every column's share at qs[0]) with `replicates` replicates, replicate 0 being the data.
        result.se(i), result.shortfall_se(i), result.interval(i), result.difference(i, j) and
        report_bootstrap(miners, result) work on it."""
        return _run_bootstrap(lib.msim_run_bootstrap, "msim_run_bootstrap", self._h, 1, len(self.miners), n_runs, items,
                              qs, replicates, boot_seed, class_of, n_classes, run_begin, seed_base, device)

    def launch_boot_begin(self, items: Sequence[BootItem], replicates: int, ranks: Sequence[int], n_q: int, d_ws,
                          stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_begin_launch on the current device: ranks is [n_q][replicates] flat (bootstrap.boot_ranks of the
        complete W), d_ws a buffer of bootstrap.boot_workspace_bytes(len(items), replicates) bytes."""
        _launch_boot_begin(columns or len(self.miners), 1, items, replicates, ranks, n_q, d_ws, stream)

    def launch_boot_count(self, n_runs: int, d_per_run, d_best_height, boot_seed: int, run_begin: int, n_items: int,
                          replicates: int, pass_: int, d_ws, stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_count_launch: pass `pass_` over a launch's records, whose first run is the absolute run
        `run_begin`; adds to the workspace's counts."""
        _launch_boot_count(columns or len(self.miners), 1, boot_seed, run_begin, n_runs, d_per_run, d_best_height,
                           n_items, replicates, pass_, d_ws, stream)

    def launch_boot_step(self, n_items: int, replicates: int, pass_: int, d_ws, d_rows, d_status, stream=None) -> None:
        """msim_boot_step_launch; d_rows int64 [n_items, replicates, 5] (required at the last pass), d_status int32
        [1] (added to)."""
        _launch_boot_step(n_items, replicates, pass_, d_ws, d_rows, d_status, stream)

    def launch_boot_below(self, n_runs: int, d_per_run, d_best_height, boot_seed: int, run_begin: int, n_items: int,
                          replicates: int, d_ws, d_rows, stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_below_launch: adds the weighted halves of the keys below each row's value to d_rows."""
        _launch_boot_below(columns or len(self.miners), 1, boot_seed, run_begin, n_runs, d_per_run, d_best_height,
                           n_items, replicates, d_ws, d_rows, stream)

    def run_multi(self, n_runs: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                  devices: Sequence[int] = (0,)) -> SimulationResult:
        """msim_run_multi: the runs sharded over `devices` (one host thread each) and combined with one RCCL
        all-reduce of the integer sums; bit-identical to run() for any device list."""
        m = len(self.miners)
        stats = (MsimStats * m)()
        sums = (MsimSums * m)()
        devs = (ctypes.c_int * len(devices))(*devices)
        shard_ms = (ctypes.c_double * (2 * len(devices)))()
        check(lib.msim_run_multi_timed(self._h, run_begin, n_runs, seed_base & 0xFFFFFFFF, devs, len(devices), stats,
                                       sums, shard_ms), "msim_run_multi_timed")
        return SimulationResult(
            stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats],
            sums=list(sums),
            n_runs=n_runs,
            # per device: [launches ms, all-reduce ms] (msim_run_multi_timed)
            extra={"shard_ms": [(shard_ms[2 * g], shard_ms[2 * g + 1]) for g in range(len(devices))]},
        )

    def pipeline_info(self, n_runs: int) -> dict:
        """How msim_launch executes n_runs on the current device (msim_pipeline_info)."""
        pl = _lib.MsimPipelineLayout()
        check(lib.msim_pipeline_info(self._h, n_runs, ctypes.byref(pl)), "msim_pipeline_info")
        return {f: getattr(pl, f) for f, _ in pl._fields_}

    # ---- device-resident form (torch tensors as HBM buffers; used by bench.py and the RCCL path)
    def workspace_bytes(self, n_runs: int) -> int:
        return int(lib.msim_workspace_bytes(self._h, n_runs))

    def launch(self, n_runs: int, run_begin: int, seed_base: int, d_sums, d_workspace, d_status,
               d_per_run=None, d_best_height=None, stream=None) -> None:
        """Asynchronous launch on the current device: all buffers are torch CUDA (HIP) tensors.

        d_sums: int64 [M, 6] (msim_sums); d_status: int32 [2]; d_workspace: uint8 [workspace_bytes]."""
        ptr = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None)
        sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        check(lib.msim_launch(self._h, run_begin, n_runs, seed_base & 0xFFFFFFFF, ptr(d_sums), ptr(d_per_run),
                              ptr(d_best_height), ptr(d_status), ptr(d_workspace), d_workspace.numel(), sh),
              "msim_launch")


def sample_picks(sim: "Simulation", seed: int, n: int, device: int = 0) -> np.ndarray:
    """test.cpp:15-63 MinerPickerSample on the GPU: per-miner counts of n PickFinder draws of RNG{seed}
    (the last entry counts draws where the reference would assert), identical to the sequential loop."""
    m = len(sim.miners)
    out = (ctypes.c_uint64 * (m + 1))()
    check(lib.msim_sample_picks(sim.handle, seed, n, out, device), "msim_sample_picks")
    return np.array(out[:], dtype=np.uint64)


def sample_intervals(seed: int, n: int, device: int = 0) -> dict:
    """test.cpp:191-208 BlockIntervalSample on the GPU: exact integer moments of n NextBlockInterval draws
    of RNG{seed}, plus the mean and standard deviation the reference prints."""
    mo = _lib.MsimIntervalMoments()
    check(lib.msim_sample_intervals(seed, n, ctypes.byref(mo), device), "msim_sample_intervals")
    sumsq = (int(mo.sumsq_hi) << 64) | int(mo.sumsq_lo)
    mean = mo.sum / n if n else 0.0
    var = sumsq / n - mean * mean if n else 0.0
    return {"n": int(mo.n), "sum": int(mo.sum), "sumsq": sumsq, "max": int(mo.max), "mean": mean,
            "std": var ** 0.5 if var > 0 else 0.0}


class Sweep:
    """A grid of networks run in ONE device launch (BASELINE configs[3]; msim_sweep_* in include/msim.h).

    The reference covers a grid by editing SetupMiners (main.cpp:44-65) and rebuilding per point
    (README.md:21-27). Point p, run r of a sweep is bit-identical to Simulation(points[p]).run for run
    run_begin + r: every point sees the same seeds.

    shared_draws=True asks for the shared-draw form (msim_sweep_create_ex, MSIM_SWEEP_SHARED_DRAWS): honest points
    with the same weights share ONE draw pass per slice; only the short per-point tails run per point. Same
    results, bit for bit; a sweep the form does not serve (a selfish point, a delay the pipeline does not take)
    runs as without it. plan() tells which engine serves the sweep.

    total_weight != 100 (Miner.perc are integer weights summing to it) or more than 15 honest miners: every point
    runs on the large-network pipeline (engine 2). Without shared_draws each point is a plain launch of that
    pipeline; with it, points with equal weights share one draw pass on the group's envelope network (every miner
    at its largest delay over the group). The shared form can fail a run (MSIM_E_CAPACITY) that the point's own
    launch would not, but only when the ENVELOPE's candidate list overflows (an 8-sigma event)."""

    def __init__(self, points: Sequence[Sequence[Miner]], duration_ms: int = SIM_DURATION_MS,
                 shared_draws: bool = False, total_weight: int = 100):
        self.sims = [Simulation(p, duration_ms, total_weight) for p in points]
        self.m = len(self.sims[0].miners)
        handles = (ctypes.c_void_p * len(self.sims))(*[s.handle.value for s in self.sims])
        h = ctypes.c_void_p()
        check(lib.msim_sweep_create_ex(handles, len(self.sims), MSIM_SWEEP_SHARED_DRAWS if shared_draws else 0,
                                       ctypes.byref(h)), "msim_sweep_create_ex")
        self._h = h

    def plan(self, runs_per_point: int) -> dict:
        """msim_sweep_info: engine (0 per-lane kernel, 1 shared-draw pipeline, 2 large-network pipeline, 3 entity
        engine, 4 general engine), draw_groups, largest_group, slice_runs, workspace_bytes. For engine 2 draw_groups
        counts every group (without shared_draws: one per point) and slice_runs is the smallest group's slice.
        Host only."""
        pl = MsimSweepPlan()
        check(lib.msim_sweep_info(self._h, runs_per_point, ctypes.byref(pl)), "msim_sweep_info")
        return {f: int(getattr(pl, f)) for f, _ in MsimSweepPlan._fields_}

    def group_of(self, p: int) -> int:
        """The draw group of point p, or -1 when the sweep does not run in the shared-draw form. Host only."""
        return int(lib.msim_sweep_group_of(self._h, p))

    def __len__(self) -> int:
        return len(self.sims)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.msim_sweep_destroy(h)
            self._h = None

    def run_multi(self, runs_per_point: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                  devices: Sequence[int] = (0,)) -> List[SimulationResult]:
        """msim_sweep_run_multi: every device runs every point on its shard of the runs, one RCCL all-reduce;
        bit-identical to run()'s sums for any device list."""
        n, m = len(self.sims), self.m
        stats = (MsimStats * (n * m))()
        sums = (MsimSums * (n * m))()
        devs = (ctypes.c_int * len(devices))(*devices)
        check(lib.msim_sweep_run_multi(self._h, run_begin, runs_per_point, seed_base & 0xFFFFFFFF, devs, len(devices),
                                       stats, sums), "msim_sweep_run_multi")
        return [SimulationResult(
            stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
            sums=list(sums[p * m:(p + 1) * m]),
            n_runs=runs_per_point,
        ) for p in range(n)]

    def run(self, runs_per_point: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE, device: int = 0,
            per_run: bool = False) -> List[SimulationResult]:
        n, m = len(self.sims), self.m
        stats = (MsimStats * (n * m))()
        sums = (MsimSums * (n * m))()
        rec = (MsimRunRecord * (n * runs_per_point * m))() if per_run else None
        bh = (ctypes.c_uint32 * (n * runs_per_point))() if per_run else None
        check(lib.msim_sweep_run(self._h, run_begin, runs_per_point, seed_base & 0xFFFFFFFF, device, stats, sums, rec, bh),
              "msim_sweep_run")
        out = []
        for p in range(n):
            res = SimulationResult(
                stats_total=[MinerStats(s.blocks_found, s.blocks_share, s.stale_rate) for s in stats[p * m:(p + 1) * m]],
                sums=list(sums[p * m:(p + 1) * m]),
                n_runs=runs_per_point,
            )
            if per_run:
                a = np.ctypeslib.as_array(ctypes.cast(rec, ctypes.POINTER(ctypes.c_uint32)),
                                          shape=(n, runs_per_point, m, 2))
                res.found = a[p, :, :, 0].copy()
                res.stale = a[p, :, :, 1].copy()
                res.best_height = np.ctypeslib.as_array(bh).reshape(n, runs_per_point)[p].copy()
            out.append(res)
        return out

    def run_moments(self, runs_per_point: int, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                    device: int = 0, hist: Optional[HistSpec] = None) -> List[SimulationResult]:
        """msim_sweep_run_moments: run() plus per-point `moments` and (with a HistSpec) `hist`."""
        return _run_moments(lib.msim_sweep_run_moments, "msim_sweep_run_moments", self._h, len(self.sims), self.m,
                            runs_per_point, run_begin, seed_base, device, hist)

    def launch_moments(self, runs_per_point: int, d_per_run, d_best_height, d_moments,
                       hist_spec: Optional[HistSpec] = None, d_hist=None, stream=None) -> None:
        """msim_moments_launch over a sweep launch's records; d_moments int64 [n_points, M, 20]."""
        _launch_moments(self.m, len(self.sims), runs_per_point, d_per_run, d_best_height, d_moments, hist_spec,
                        d_hist, stream)

    def run_contrasts(self, runs_per_point: int, pairs: Sequence[Pair], run_begin: int = 0,
                      seed_base: int = DEFAULT_SEED_BASE, device: int = 0) -> ContrastResult:
        """msim_sweep_run_contrasts: run_moments() plus the exact cross sums of `pairs` (e.g.
        pairs_vs_baseline(len(sweep), M)). Every point runs on the same seeds, so contrasts(result) gives the
        differences between points with the standard error of the per-run difference."""
        return _run_contrasts(lib.msim_sweep_run_contrasts, "msim_sweep_run_contrasts", self._h, len(self.sims),
                              self.m, runs_per_point, pairs, run_begin, seed_base, device)

    def launch_cross(self, runs_per_point: int, d_per_run, d_best_height, d_pairs, n_pairs: int, d_cross,
                     stream=None) -> None:
        """msim_cross_launch over a sweep launch's records; d_pairs int32 [n_pairs, 4], d_cross int64 [n_pairs, 12]."""
        _launch_cross(self.m, len(self.sims), runs_per_point, d_per_run, d_best_height, d_pairs, n_pairs, d_cross,
                      stream)

    def run_classes(self, runs_per_point: int, class_of: Sequence[int], pairs: Optional[Sequence[Pair]] = None,
                    hist: Optional[HistSpec] = None, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                    device: int = 0, n_classes: Optional[int] = None):
        """msim_sweep_run_classes: Simulation.run_classes over a sweep, one class map for all points. Per point a
        SimulationResult with per-class `moments` and `hist`; with `pairs` of (point, class) columns (e.g.
        pairs_vs_baseline(len(sweep), n_classes)) a ContrastResult over them."""
        return _run_classes(lib.msim_sweep_run_classes, "msim_sweep_run_classes", self._h, len(self.sims), self.m,
                            runs_per_point, class_of, n_classes, pairs, hist, run_begin, seed_base, device)

    def launch_fold(self, runs_per_point: int, d_per_run, d_class_of, n_classes: int, d_class_run,
                    stream=None) -> None:
        """msim_fold_launch over a sweep launch's records; d_class_run int32 [n_points, runs_per_point, n_classes, 2]."""
        _launch_fold(self.m, len(self.sims), runs_per_point, d_per_run, d_class_of, n_classes, d_class_run, stream)

    def run_quantiles(self, runs_per_point: int, qs: Sequence[float] = (0.05, 0.5, 0.95),
                      ranks: Optional[Sequence[int]] = None, class_of: Optional[Sequence[int]] = None,
                      n_classes: Optional[int] = None, run_begin: int = 0, seed_base: int = DEFAULT_SEED_BASE,
                      device: int = 0) -> QuantileResult:
        """msim_sweep_run_order_stats: Simulation.run_quantiles over a sweep; result.order[point][column][quantity][j]."""
        return _run_quantiles(lib.msim_sweep_run_order_stats, "msim_sweep_run_order_stats", self._h, len(self.sims),
                              self.m, runs_per_point, qs, ranks, class_of, n_classes, run_begin, seed_base, device)

    def rank_workspace_bytes(self, n_ranks: int, columns: Optional[int] = None) -> int:
        return rank_workspace_bytes(columns or self.m, len(self.sims), n_ranks)

    def rank_counts_view(self, n_ranks: int, columns: Optional[int] = None):
        return rank_counts_view(columns or self.m, len(self.sims), n_ranks)

    def launch_rank_begin(self, ranks: Sequence[int], d_ws, stream=None, columns: Optional[int] = None) -> None:
        """msim_rank_begin_launch for a sweep launch's records (every point selects the same ranks)."""
        _launch_rank_begin(columns or self.m, len(self.sims), ranks, d_ws, stream)

    def launch_rank_count(self, runs_per_point: int, d_per_run, d_best_height, pass_: int, d_ws, stream=None,
                          columns: Optional[int] = None) -> None:
        """msim_rank_count_launch over a sweep launch's records."""
        _launch_rank_count(columns or self.m, len(self.sims), runs_per_point, d_per_run, d_best_height, pass_, d_ws,
                           stream)

    def launch_rank_step(self, pass_: int, d_ws, d_out, d_status, stream=None, columns: Optional[int] = None) -> None:
        """msim_rank_step_launch; d_out int64 [n_points, M, 4, n_ranks, 3]."""
        _launch_rank_step(columns or self.m, len(self.sims), pass_, d_ws, d_out, d_status, stream)

    def run_tails(self, runs_per_point: int, q=0.05, *, ranks: Optional[Sequence[int]] = None,
                  specs: Optional[Sequence[TailSpec]] = None, class_of: Optional[Sequence[int]] = None,
                  n_classes: Optional[int] = None, seed_base: int = DEFAULT_SEED_BASE, run_begin: int = 0,
                  device: int = 0) -> TailResult:
        """msim_sweep_run_tails: Simulation.run_tails over a sweep; a spec's condition and target may lie at
        different points (the same seeds on both sides)."""
        return _run_tails(lib.msim_sweep_run_tails, "msim_sweep_run_tails", self._h, len(self.sims), self.m,
                          runs_per_point, q, ranks, specs, class_of, n_classes, run_begin, seed_base, device)

    def launch_tails(self, runs_per_point: int, d_per_run, d_best_height, d_items, n_items: int, d_tails, stream=None,
                     columns: Optional[int] = None) -> None:
        """msim_tail_launch over a sweep launch's records."""
        _launch_tails(columns or self.m, len(self.sims), runs_per_point, d_per_run, d_best_height, d_items, n_items,
                      d_tails, stream)

    def run_bootstrap(self, runs_per_point: int, items: Optional[Sequence[BootItem]] = None, qs: Sequence[float] = (0.05,),
                      replicates: int = 200, boot_seed: int = DEFAULT_BOOT_SEED,
                      class_of: Optional[Sequence[int]] = None, n_classes: Optional[int] = None,
                      seed_base: int = DEFAULT_SEED_BASE, run_begin: int = 0, device: int = 0) -> BootstrapResult:
        """msim_sweep_run_bootstrap: run_quantiles() at `qs` plus the Poisson bootstrap of `items` (bootstrap.own_bootstrap
        by default: every column's share at qs[0]) with `replicates` replicates, replicate 0 being the data.
        result.se(i), result.shortfall_se(i), result.interval(i), result.difference(i, j) and
        report_bootstrap(miners, result) work on it."""
        return _run_bootstrap(lib.msim_sweep_run_bootstrap, "msim_sweep_run_bootstrap", self._h, len(self.sims), self.m, runs_per_point, items,
                              qs, replicates, boot_seed, class_of, n_classes, run_begin, seed_base, device)

    def launch_boot_begin(self, items: Sequence[BootItem], replicates: int, ranks: Sequence[int], n_q: int, d_ws,
                          stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_begin_launch on the current device: ranks is [n_q][replicates] flat (bootstrap.boot_ranks of the
        complete W), d_ws a buffer of bootstrap.boot_workspace_bytes(len(items), replicates) bytes."""
        _launch_boot_begin(columns or self.m, len(self.sims), items, replicates, ranks, n_q, d_ws, stream)

    def launch_boot_count(self, runs_per_point: int, d_per_run, d_best_height, boot_seed: int, run_begin: int, n_items: int,
                          replicates: int, pass_: int, d_ws, stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_count_launch: pass `pass_` over a launch's records, whose first run is the absolute run
        `run_begin`; adds to the workspace's counts."""
        _launch_boot_count(columns or self.m, len(self.sims), boot_seed, run_begin, runs_per_point, d_per_run, d_best_height,
                           n_items, replicates, pass_, d_ws, stream)

    def launch_boot_step(self, n_items: int, replicates: int, pass_: int, d_ws, d_rows, d_status, stream=None) -> None:
        """msim_boot_step_launch; d_rows int64 [n_items, replicates, 5] (required at the last pass), d_status int32
        [1] (added to)."""
        _launch_boot_step(n_items, replicates, pass_, d_ws, d_rows, d_status, stream)

    def launch_boot_below(self, runs_per_point: int, d_per_run, d_best_height, boot_seed: int, run_begin: int, n_items: int,
                          replicates: int, d_ws, d_rows, stream=None, columns: Optional[int] = None) -> None:
        """msim_boot_below_launch: adds the weighted halves of the keys below each row's value to d_rows."""
        _launch_boot_below(columns or self.m, len(self.sims), boot_seed, run_begin, runs_per_point, d_per_run, d_best_height,
                           n_items, replicates, d_ws, d_rows, stream)

    def workspace_bytes(self, runs_per_point: int) -> int:
        return int(lib.msim_sweep_workspace_bytes(self._h, runs_per_point))

    def launch(self, runs_per_point: int, run_begin: int, seed_base: int, d_sums, d_workspace, d_status,
               d_per_run=None, d_best_height=None, stream=None) -> None:
        """Asynchronous launch on the current device; d_sums: int64 [n_points, M, 6]."""
        ptr = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None)
        sh = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        check(lib.msim_sweep_launch(self._h, run_begin, runs_per_point, seed_base & 0xFFFFFFFF, ptr(d_sums),
                                    ptr(d_per_run), ptr(d_best_height), ptr(d_status), ptr(d_workspace),
                                    d_workspace.numel(), sh), "msim_sweep_launch")


def propagation_sweep(miners: Sequence[Miner], delays_ms: Sequence[int], duration_ms: int = SIM_DURATION_MS,
                      total_weight: int = 100) -> Sweep:
    """One network at several uniform propagation delays (the reference's first example, README.md:21-27: the
    same hashrates at 10 s and at 100 ms, one rebuild each) as a shared-draw sweep: point i is `miners` with every
    propagation_ms = delays_ms[i]. All points share their draws, so run_contrasts(..., pairs_vs_baseline(...))
    gives the differences between delays with the per-run difference's error. Large networks (c5_network() with
    total_weight=C5_TOTAL_WEIGHT) take the large-network pipeline's shared form."""
    points = [[Miner(mn.id, mn.perc, int(d), mn.is_selfish) for mn in miners] for d in delays_ms]
    return Sweep(points, duration_ms, shared_draws=True, total_weight=total_weight)


def timing_enable(on: bool = True) -> None:
    """Start (or stop) stage timing: HIP events on the launch stream around every msim_launch and every
    draw kernel (K1) it issues (msim_timing_enable)."""
    check(lib.msim_timing_enable(1 if on else 0), "msim_timing_enable")


def timing_read() -> dict:
    """Summed draw-kernel / entity-engine / whole-launch milliseconds and the launch count since the last
    enable/read (synchronises). draws_ms: K1 / W1 (honest pipelines; 0 for selfish networks); engine_ms: E1.
    *_busy_ms: the union of those intervals over every stream (msim_timing_read_all): the stage's share of the
    wall clock when launches overlap on several streams."""
    t = MsimTiming()
    check(lib.msim_timing_read_all(ctypes.byref(t)), "msim_timing_read_all")
    return {k: getattr(t, k) for k, _ in MsimTiming._fields_}


def sums_to_stats(sums_rows: Iterable[Sequence[int]]) -> List[MinerStats]:
    """Fixed-point msim_sums rows ([found, stale, share_hi, share_lo, rate_hi, rate_lo]) -> MinerStats.

    Each Q32.32 sum is converted with one rounding of its exact value (hi << 32) + lo (as
    msim_sums_to_stats), so the result is the same for every split of the runs into launches or ranks."""
    out = []
    for r in sums_rows:
        found, _stale, sh, sl, rh, rl = (int(x) for x in r)
        out.append(MinerStats(found, float((sh << 32) + sl) * 2.0 ** -32, float((rh << 32) + rl) * 2.0 ** -32))
    return out


def exact_stats_total(found: np.ndarray, stale: np.ndarray, best_height: np.ndarray) -> List[MinerStats]:
    """MinerStats per run (main.cpp:22-30) summed in run order (main.cpp:211-217), bit-exact."""
    n, m = found.shape
    tot = [MinerStats() for _ in range(m)]
    for r in range(n):
        L = float(best_height[r])
        for k in range(m):
            f = int(found[r, k])
            share = 0.0 if f == 0 else f / L
            rate = 0.0 if f == 0 else int(stale[r, k]) / f
            tot[k] += MinerStats(f, share, rate)
    return tot


def report(miners: Sequence[Miner], stats_total: Sequence[MinerStats], sim_runs: int,
           duration_ms: int = SIM_DURATION_MS) -> str:
    """The report lines of main.cpp:224-234 (iostream default float format = %g, 6 digits)."""
    days = duration_ms // 86_400_000
    lines = [f"After running {sim_runs} simulations for {days}d each, on average:"]
    for m, s in zip(miners, stats_total):
        line = (f"  - Miner {m.id} ({m.perc}% of network hashrate) found {int(s.blocks_found) // sim_runs} blocks i.e. "
                f"{s.blocks_share * 100 / sim_runs:.6g}% of blocks. Stale rate: {s.stale_rate * 100 / sim_runs:.6g}%.")
        if m.is_selfish:
            line += " ('selfish mining' strategy)"
        lines.append(line)
    return "\n".join(lines)

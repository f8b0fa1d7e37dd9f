"""ctypes binding of libmsim.so (include/msim.h).

The library is GPU-only: there is no CPU fallback anywhere in the product path. Importing this module
without a built ``libmsim.so`` raises immediately; calling into it without a HIP device returns
MSIM_E_HIP, which the wrappers turn into :class:`MsimError`.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSIM_LIB", os.path.join(_HERE, "libmsim.so"))

MSIM_OK = 0
MSIM_E_INVALID = -1
MSIM_E_WEIGHTS = -2
MSIM_E_SELFISH = -3
MSIM_E_MINERS = -4
MSIM_E_HIP = -5
MSIM_E_CAPACITY = -6
MSIM_E_PICK = -7
MSIM_MAX_MINERS = 15
MSIM_MAX_SELFISH = 4

# Every symbol include/msim.h declares (checked by tests/test_abi.py).
EXPORTED = (
    "msim_config_create",
    "msim_config_create_weighted",
    "msim_config_is_wide",
    "msim_config_set_concurrent_launches",
    "msim_config_destroy",
    "msim_config_miner_count",
    "msim_run",
    "msim_run_multi",
    "msim_run_multi_timed",
    "msim_multi_release",
    "msim_sweep_run_multi",
    "msim_sweep_point_count",
    "msim_sweep_miner_count",
    "msim_workspace_bytes",
    "msim_launch",
    "msim_device_log1p",
    "msim_device_intervals",
    "msim_device_picks",
    "msim_device_k1_quads",  # test surface: bound where it is used (tests/test_gpu_k1_quads.py)
    "msim_sums_to_stats",
    "msim_timing_enable",
    "msim_timing_read",
    "msim_timing_read_stages",
    "msim_timing_read_all",
    "msim_pipeline_info",
    "msim_sweep_create",
    "msim_sweep_create_ex",
    "msim_sweep_group_of",
    "msim_sweep_info",
    "msim_sweep_destroy",
    "msim_sweep_workspace_bytes",
    "msim_sweep_launch",
    "msim_sweep_run",
    "msim_strerror",
    "msim_version",
    "msim_sample_picks",
    "msim_sample_intervals",
    "msim_moments_launch",
    "msim_run_moments",
    "msim_sweep_run_moments",
    "msim_moments_to_errors",
    "msim_cross_launch",
    "msim_pairs_check",
    "msim_run_contrasts",
    "msim_sweep_run_contrasts",
    "msim_cross_to_contrasts",
    "msim_fold_launch",
    "msim_classes_check",
    "msim_run_classes",
    "msim_sweep_run_classes",
    "msim_rank_workspace_bytes",
    "msim_rank_counts_view",
    "msim_rank_begin_launch",
    "msim_rank_count_launch",
    "msim_rank_step_launch",
    "msim_rank_launch",
    "msim_ranks_check",
    "msim_run_order_stats",
    "msim_sweep_run_order_stats",
    "msim_tail_launch",
    "msim_tail_items_check",
    "msim_tail_side",
    "msim_tail_means",
    "msim_run_tails",
    "msim_sweep_run_tails",
    "msim_boot_workspace_bytes",
    "msim_boot_counts_view",
    "msim_boot_items_check",
    "msim_boot_rank",
    "msim_boot_weights_launch",
    "msim_boot_begin_launch",
    "msim_boot_count_launch",
    "msim_boot_step_launch",
    "msim_boot_below_launch",
    "msim_run_bootstrap",
    "msim_sweep_run_bootstrap",
)
MSIM_CLASS_NONE = 0xFFFFFFFF
MSIM_MAX_RANKS = 32
MSIM_RANK_PASSES = 8
MSIM_MAX_TAIL_ITEMS = 65535 * 128
MSIM_MAX_BOOT_REPLICATES = 4096
MSIM_MAX_BOOT_ITEMS = 65535
MSIM_BOOT_MAX_RUNS = 1 << 28
MSIM_BOOT_EMPTY = 0xFFFFFFFFFFFFFFFF
MSIM_TAIL_BELOW, MSIM_TAIL_AT_MOST, MSIM_TAIL_ABOVE, MSIM_TAIL_AT_LEAST = range(4)


class MsimTiming(ctypes.Structure):
    _fields_ = [("draws_ms", ctypes.c_double), ("engine_ms", ctypes.c_double), ("launch_ms", ctypes.c_double),
                ("draws_busy_ms", ctypes.c_double), ("engine_busy_ms", ctypes.c_double),
                ("launch_busy_ms", ctypes.c_double), ("launches", ctypes.c_uint32)]


class MsimMiner(ctypes.Structure):
    _fields_ = [
        ("id", ctypes.c_uint32),
        ("perc", ctypes.c_uint64),
        ("propagation_ms", ctypes.c_int64),
        ("is_selfish", ctypes.c_uint8),
    ]


class MsimStats(ctypes.Structure):
    _fields_ = [("blocks_found", ctypes.c_int64), ("blocks_share", ctypes.c_double), ("stale_rate", ctypes.c_double)]


class MsimSums(ctypes.Structure):
    _fields_ = [
        ("blocks_found", ctypes.c_int64),
        ("stale_blocks", ctypes.c_int64),
        ("share_hi", ctypes.c_uint64),
        ("share_lo", ctypes.c_uint64),
        ("rate_hi", ctypes.c_uint64),
        ("rate_lo", ctypes.c_uint64),
    ]


class MsimRunRecord(ctypes.Structure):
    _fields_ = [("found", ctypes.c_uint32), ("stale", ctypes.c_uint32)]


class MsimPipelineLayout(ctypes.Structure):
    _fields_ = [
        ("uses_pipeline", ctypes.c_uint32),
        ("slice_runs", ctypes.c_uint32),
        ("segment_blocks", ctypes.c_uint32),
        ("segments", ctypes.c_uint32),
        ("blocks_per_run", ctypes.c_uint64),
        ("workspace_bytes", ctypes.c_uint64),
        ("rho", ctypes.c_double),
    ]


class MsimSweepPlan(ctypes.Structure):
    _fields_ = [
        ("engine", ctypes.c_uint32),
        ("draw_groups", ctypes.c_uint32),
        ("largest_group", ctypes.c_uint32),
        ("slice_runs", ctypes.c_uint32),
        ("workspace_bytes", ctypes.c_uint64),
    ]


MSIM_SWEEP_SHARED_DRAWS = 1


class MsimError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {strerror(code)} ({code})" if what else f"{strerror(code)} ({code})")


class MsimIntervalMoments(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("sum", ctypes.c_uint64), ("sumsq_lo", ctypes.c_uint64),
                ("sumsq_hi", ctypes.c_uint64), ("max", ctypes.c_uint64)]


class MsimMoments(ctypes.Structure):
    """msim_moments: 20 uint64 per miner, every field a plain sum over runs (limbs not normalised)."""
    _fields_ = [("first", MsimSums), ("found_sq", ctypes.c_uint64 * 2), ("stale_sq", ctypes.c_uint64 * 2),
                ("found_stale", ctypes.c_uint64 * 2), ("share_sq", ctypes.c_uint64 * 4),
                ("rate_sq", ctypes.c_uint64 * 4)]


class MsimHistSpec(ctypes.Structure):
    _fields_ = [("bins", ctypes.c_uint32), ("share_shift", ctypes.c_uint32), ("rate_shift", ctypes.c_uint32),
                ("share_lo", ctypes.c_uint64), ("rate_lo", ctypes.c_uint64)]


class MsimErrors(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("found_mean", "found_se", "share_mean", "share_se", "rate_mean",
                                               "rate_se", "pooled_rate", "pooled_rate_se")]


class MsimPair(ctypes.Structure):
    """msim_pair: side a and side b of a contrast, each a (point, miner) column of one launch's records."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("point_a", "miner_a", "point_b", "miner_b")]


class MsimCross(ctypes.Structure):
    """msim_cross: 12 uint64 per pair, the sums over runs of the sides' products (limbs not normalised)."""
    _fields_ = [("found_found", ctypes.c_uint64 * 2), ("stale_stale", ctypes.c_uint64 * 2),
                ("share_share", ctypes.c_uint64 * 4), ("rate_rate", ctypes.c_uint64 * 4)]


class MsimContrast(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "found_diff", "found_diff_se", "found_corr", "found_ratio", "found_ratio_se",
        "stale_diff", "stale_diff_se", "stale_corr",
        "share_diff", "share_diff_se", "share_corr", "share_ratio", "share_ratio_se",
        "rate_diff", "rate_diff_se", "rate_corr")]


class MsimOrderStat(ctypes.Structure):
    """msim_order_stat: the r-th smallest key of a column, and how many keys lie below it and equal it."""
    _fields_ = [("value", ctypes.c_uint64), ("below", ctypes.c_uint64), ("equal", ctypes.c_uint64)]


class MsimTailItem(ctypes.Structure):
    """msim_tail_item: the condition (point, column, quantity), the target (point, column) and the threshold."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("cond_point", "cond_column", "quantity", "target_point",
                                               "target_column", "reserved")] + [("value", ctypes.c_uint64)]


class MsimTail(ctypes.Structure):
    """msim_tail: 42 uint64 per item, the run counts below and at the threshold and the target's moments over them."""
    _fields_ = [("n_below", ctypes.c_uint64), ("n_equal", ctypes.c_uint64), ("below", MsimMoments),
                ("equal", MsimMoments)]


class MsimTailSpec(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("cond_point", "cond_column", "quantity", "rank_index", "target_point",
                                               "target_column")]


class MsimBootItem(ctypes.Structure):
    """msim_boot_item: the (point, column, quantity) whose key is resampled and the index of its quantile."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("point", "column", "quantity", "q_index")]


class MsimBootRow(ctypes.Structure):
    """msim_boot_row: one replicate's order statistic and the weighted sum of the keys below it, in two halves."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("value", "below", "equal", "s_hi", "s_lo")]


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libmsim.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the simulation path is HIP-only; there is no CPU fallback)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_size_t
    lib.msim_config_create.argtypes = [ctypes.POINTER(MsimMiner), u32, i64, ctypes.POINTER(vp)]
    lib.msim_config_create.restype = ctypes.c_int
    lib.msim_config_create_weighted.argtypes = [ctypes.POINTER(MsimMiner), u32, i64, u64, ctypes.POINTER(vp)]
    lib.msim_config_create_weighted.restype = ctypes.c_int
    lib.msim_config_is_wide.argtypes = [vp]
    lib.msim_config_is_wide.restype = ctypes.c_int
    lib.msim_config_set_concurrent_launches.argtypes = [vp, u32]
    lib.msim_config_set_concurrent_launches.restype = ctypes.c_int
    lib.msim_config_destroy.argtypes = [vp]
    lib.msim_config_destroy.restype = None
    lib.msim_config_miner_count.argtypes = [vp]
    lib.msim_config_miner_count.restype = u32
    lib.msim_run.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(MsimStats), ctypes.POINTER(MsimSums),
                             ctypes.POINTER(MsimRunRecord), ctypes.POINTER(u32)]
    lib.msim_run.restype = ctypes.c_int
    lib.msim_run_multi.argtypes = [vp, u64, u64, u32, ctypes.POINTER(ctypes.c_int), u32, ctypes.POINTER(MsimStats),
                                   ctypes.POINTER(MsimSums)]
    lib.msim_run_multi.restype = ctypes.c_int
    lib.msim_run_multi_timed.argtypes = [vp, u64, u64, u32, ctypes.POINTER(ctypes.c_int), u32,
                                         ctypes.POINTER(MsimStats), ctypes.POINTER(MsimSums),
                                         ctypes.POINTER(ctypes.c_double)]
    lib.msim_run_multi_timed.restype = ctypes.c_int
    lib.msim_multi_release.argtypes = []
    lib.msim_multi_release.restype = ctypes.c_int
    lib.msim_sweep_run_multi.argtypes = [vp, u64, u64, u32, ctypes.POINTER(ctypes.c_int), u32,
                                         ctypes.POINTER(MsimStats), ctypes.POINTER(MsimSums)]
    lib.msim_sweep_run_multi.restype = ctypes.c_int
    lib.msim_sweep_point_count.argtypes = [vp]
    lib.msim_sweep_point_count.restype = u32
    lib.msim_sweep_miner_count.argtypes = [vp]
    lib.msim_sweep_miner_count.restype = u32
    lib.msim_workspace_bytes.argtypes = [vp, u64]
    lib.msim_workspace_bytes.restype = sz
    lib.msim_launch.argtypes = [vp, u64, u64, u32, vp, vp, vp, vp, vp, sz, vp]
    lib.msim_launch.restype = ctypes.c_int
    lib.msim_device_log1p.argtypes = [vp, vp, u64, vp]
    lib.msim_device_log1p.restype = ctypes.c_int
    lib.msim_device_intervals.argtypes = [vp, vp, u64, vp]
    lib.msim_device_intervals.restype = ctypes.c_int
    lib.msim_device_picks.argtypes = [vp, vp, vp, u64, vp]
    lib.msim_device_picks.restype = ctypes.c_int
    lib.msim_sums_to_stats.argtypes = [ctypes.POINTER(MsimSums), u32, ctypes.POINTER(MsimStats)]
    lib.msim_sums_to_stats.restype = None
    lib.msim_timing_enable.argtypes = [ctypes.c_int]
    lib.msim_timing_enable.restype = ctypes.c_int
    lib.msim_timing_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(u32)]
    lib.msim_timing_read.restype = ctypes.c_int
    lib.msim_timing_read_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]
    lib.msim_timing_read_stages.restype = ctypes.c_int
    lib.msim_timing_read_all.argtypes = [ctypes.POINTER(MsimTiming)]
    lib.msim_timing_read_all.restype = ctypes.c_int
    lib.msim_pipeline_info.argtypes = [vp, u64, ctypes.POINTER(MsimPipelineLayout)]
    lib.msim_pipeline_info.restype = ctypes.c_int
    lib.msim_sweep_create.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(vp)]
    lib.msim_sweep_create.restype = ctypes.c_int
    lib.msim_sweep_create_ex.argtypes = [ctypes.POINTER(vp), u32, u32, ctypes.POINTER(vp)]
    lib.msim_sweep_create_ex.restype = ctypes.c_int
    lib.msim_sweep_group_of.argtypes = [vp, u32]
    lib.msim_sweep_group_of.restype = ctypes.c_int
    lib.msim_sweep_info.argtypes = [vp, u64, ctypes.POINTER(MsimSweepPlan)]
    lib.msim_sweep_info.restype = ctypes.c_int
    lib.msim_sweep_destroy.argtypes = [vp]
    lib.msim_sweep_destroy.restype = None
    lib.msim_sweep_workspace_bytes.argtypes = [vp, u64]
    lib.msim_sweep_workspace_bytes.restype = sz
    lib.msim_sweep_launch.argtypes = [vp, u64, u64, u32, vp, vp, vp, vp, vp, sz, vp]
    lib.msim_sweep_launch.restype = ctypes.c_int
    lib.msim_sweep_run.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(MsimStats),
                                   ctypes.POINTER(MsimSums), ctypes.POINTER(MsimRunRecord), ctypes.POINTER(u32)]
    lib.msim_sweep_run.restype = ctypes.c_int
    lib.msim_strerror.argtypes = [ctypes.c_int]
    lib.msim_strerror.restype = ctypes.c_char_p
    lib.msim_sample_picks.argtypes = [vp, u64, u64, ctypes.POINTER(u64), ctypes.c_int]
    lib.msim_sample_picks.restype = ctypes.c_int
    lib.msim_sample_intervals.argtypes = [u64, u64, ctypes.POINTER(MsimIntervalMoments), ctypes.c_int]
    lib.msim_sample_intervals.restype = ctypes.c_int
    lib.msim_moments_launch.argtypes = [u32, u32, u64, vp, vp, ctypes.POINTER(MsimHistSpec), vp, vp, vp]
    lib.msim_moments_launch.restype = ctypes.c_int
    lib.msim_run_moments.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(MsimStats),
                                     ctypes.POINTER(MsimSums), ctypes.POINTER(MsimMoments),
                                     ctypes.POINTER(MsimHistSpec), ctypes.POINTER(u64)]
    lib.msim_run_moments.restype = ctypes.c_int
    lib.msim_sweep_run_moments.argtypes = lib.msim_run_moments.argtypes
    lib.msim_sweep_run_moments.restype = ctypes.c_int
    lib.msim_moments_to_errors.argtypes = [ctypes.POINTER(MsimMoments), u32, u64, ctypes.POINTER(MsimErrors)]
    lib.msim_moments_to_errors.restype = None
    lib.msim_cross_launch.argtypes = [u32, u32, u64, vp, vp, vp, u32, vp, vp]
    lib.msim_cross_launch.restype = ctypes.c_int
    lib.msim_pairs_check.argtypes = [u32, u32, ctypes.POINTER(MsimPair), u32]
    lib.msim_pairs_check.restype = ctypes.c_int
    lib.msim_run_contrasts.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(MsimPair), u32,
                                       ctypes.POINTER(MsimStats), ctypes.POINTER(MsimSums),
                                       ctypes.POINTER(MsimMoments), ctypes.POINTER(MsimCross)]
    lib.msim_run_contrasts.restype = ctypes.c_int
    lib.msim_sweep_run_contrasts.argtypes = lib.msim_run_contrasts.argtypes
    lib.msim_sweep_run_contrasts.restype = ctypes.c_int
    lib.msim_cross_to_contrasts.argtypes = [ctypes.POINTER(MsimMoments), u32, ctypes.POINTER(MsimPair),
                                            ctypes.POINTER(MsimCross), u32, u64, ctypes.POINTER(MsimContrast)]
    lib.msim_cross_to_contrasts.restype = None
    lib.msim_fold_launch.argtypes = [u32, u32, u64, vp, vp, u32, vp, vp]
    lib.msim_fold_launch.restype = ctypes.c_int
    lib.msim_classes_check.argtypes = [u32, ctypes.POINTER(u32), u32]
    lib.msim_classes_check.restype = ctypes.c_int
    lib.msim_run_classes.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(u32), u32,
                                     ctypes.POINTER(MsimPair), u32, ctypes.POINTER(MsimStats),
                                     ctypes.POINTER(MsimSums), ctypes.POINTER(MsimMoments),
                                     ctypes.POINTER(MsimHistSpec), ctypes.POINTER(u64), ctypes.POINTER(MsimCross)]
    lib.msim_run_classes.restype = ctypes.c_int
    lib.msim_sweep_run_classes.argtypes = lib.msim_run_classes.argtypes
    lib.msim_sweep_run_classes.restype = ctypes.c_int
    lib.msim_rank_workspace_bytes.argtypes = [u32, u32, u32]
    lib.msim_rank_workspace_bytes.restype = sz
    lib.msim_rank_counts_view.argtypes = [u32, u32, u32, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.msim_rank_counts_view.restype = ctypes.c_int
    lib.msim_rank_begin_launch.argtypes = [u32, u32, ctypes.POINTER(u64), u32, vp, sz, vp]
    lib.msim_rank_begin_launch.restype = ctypes.c_int
    lib.msim_rank_count_launch.argtypes = [u32, u32, u64, vp, vp, u32, vp, sz, vp]
    lib.msim_rank_count_launch.restype = ctypes.c_int
    lib.msim_rank_step_launch.argtypes = [u32, u32, u32, vp, sz, vp, vp, vp]
    lib.msim_rank_step_launch.restype = ctypes.c_int
    lib.msim_rank_launch.argtypes = [u32, u32, u64, vp, vp, ctypes.POINTER(u64), u32, vp, vp, vp, sz, vp]
    lib.msim_rank_launch.restype = ctypes.c_int
    lib.msim_ranks_check.argtypes = [u64, ctypes.POINTER(u64), u32]
    lib.msim_ranks_check.restype = ctypes.c_int
    lib.msim_run_order_stats.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(u32), u32,
                                         ctypes.POINTER(u64), u32, ctypes.POINTER(MsimStats),
                                         ctypes.POINTER(MsimSums), ctypes.POINTER(MsimOrderStat)]
    lib.msim_run_order_stats.restype = ctypes.c_int
    lib.msim_sweep_run_order_stats.argtypes = lib.msim_run_order_stats.argtypes
    lib.msim_sweep_run_order_stats.restype = ctypes.c_int
    lib.msim_tail_launch.argtypes = [u32, u32, u64, vp, vp, vp, u32, vp, vp]
    lib.msim_tail_launch.restype = ctypes.c_int
    lib.msim_tail_items_check.argtypes = [u32, u32, ctypes.POINTER(MsimTailItem), u32]
    lib.msim_tail_items_check.restype = ctypes.c_int
    lib.msim_tail_side.argtypes = [ctypes.POINTER(MsimTail), ctypes.POINTER(MsimMoments), u64, ctypes.c_int,
                                   ctypes.POINTER(MsimMoments), ctypes.POINTER(u64)]
    lib.msim_tail_side.restype = ctypes.c_int
    lib.msim_tail_means.argtypes = [ctypes.POINTER(MsimTail), ctypes.POINTER(MsimMoments), u64, u64, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_double)]
    lib.msim_tail_means.restype = ctypes.c_int
    lib.msim_run_tails.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(u32), u32, ctypes.POINTER(u64), u32,
                                   ctypes.POINTER(MsimTailSpec), u32, ctypes.POINTER(MsimStats),
                                   ctypes.POINTER(MsimSums), ctypes.POINTER(MsimOrderStat),
                                   ctypes.POINTER(MsimMoments), ctypes.POINTER(MsimTail)]
    lib.msim_run_tails.restype = ctypes.c_int
    lib.msim_sweep_run_tails.argtypes = lib.msim_run_tails.argtypes
    lib.msim_sweep_run_tails.restype = ctypes.c_int
    lib.msim_boot_workspace_bytes.argtypes = [u32, u32]
    lib.msim_boot_workspace_bytes.restype = sz
    lib.msim_boot_counts_view.argtypes = [u32, u32, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.msim_boot_counts_view.restype = ctypes.c_int
    lib.msim_boot_items_check.argtypes = [u32, u32, u32, ctypes.POINTER(MsimBootItem), u32]
    lib.msim_boot_items_check.restype = ctypes.c_int
    lib.msim_boot_rank.argtypes = [u64, ctypes.c_double]
    lib.msim_boot_rank.restype = u64
    lib.msim_boot_weights_launch.argtypes = [u64, u64, u64, u32, vp, vp]
    lib.msim_boot_weights_launch.restype = ctypes.c_int
    lib.msim_boot_begin_launch.argtypes = [u32, u32, ctypes.POINTER(MsimBootItem), u32, u32, ctypes.POINTER(u64), u32,
                                           vp, sz, vp]
    lib.msim_boot_begin_launch.restype = ctypes.c_int
    lib.msim_boot_count_launch.argtypes = [u32, u32, u64, u64, u64, vp, vp, u32, u32, u32, vp, sz, vp]
    lib.msim_boot_count_launch.restype = ctypes.c_int
    lib.msim_boot_step_launch.argtypes = [u32, u32, u32, vp, sz, vp, vp, vp]
    lib.msim_boot_step_launch.restype = ctypes.c_int
    lib.msim_boot_below_launch.argtypes = [u32, u32, u64, u64, u64, vp, vp, u32, u32, vp, sz, vp, vp]
    lib.msim_boot_below_launch.restype = ctypes.c_int
    lib.msim_run_bootstrap.argtypes = [vp, u64, u64, u32, ctypes.c_int, ctypes.POINTER(u32), u32, ctypes.POINTER(u64),
                                       u32, ctypes.POINTER(MsimBootItem), u32, ctypes.POINTER(ctypes.c_double), u32,
                                       u32, u64, ctypes.POINTER(MsimStats), ctypes.POINTER(MsimSums),
                                       ctypes.POINTER(MsimOrderStat), ctypes.POINTER(u64), ctypes.POINTER(MsimBootRow)]
    lib.msim_run_bootstrap.restype = ctypes.c_int
    lib.msim_sweep_run_bootstrap.argtypes = lib.msim_run_bootstrap.argtypes
    lib.msim_sweep_run_bootstrap.restype = ctypes.c_int
    lib.msim_version.argtypes = []
    lib.msim_version.restype = ctypes.c_char_p
    return lib


lib = _load()


def strerror(code: int) -> str:
    return lib.msim_strerror(code).decode()


def check(code: int, what: str = "") -> None:
    if code != MSIM_OK:
        raise MsimError(code, what)

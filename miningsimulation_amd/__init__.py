"""miningsimulation_amd — MI355X-native engine for darosior/miningsimulation's per-run simulation loop.

One simulation run per GPU lane (hand-written gfx950 HIP, libmsim.so behind the C ABI in
include/msim.h); runs shard across GPUs with one RCCL all-reduce of integer sums (bench.py,
miningsimulation_amd.distributed). See DESIGN.md.
"""
from ._lib import MsimError, LIB_PATH  # noqa: F401  (raises ImportError when libmsim.so is missing)
from .simulation import (  # noqa: F401
    C4_PROPAGATIONS_MS,
    C4_SELFISH_PERCS,
    C5_TOTAL_WEIGHT,
    ContrastResult,
    PRESET_WEIGHTS,
    DEFAULT_SEED_BASE,
    PRESETS,
    SIM_DURATION_MS,
    SIM_RUNS,
    Miner,
    MinerStats,
    Simulation,
    SimulationResult,
    Sweep,
    c4_grid,
    c5_network,
    exact_stats_total,
    propagation_sweep,
    report,
    sample_intervals,
    sample_picks,
    setup_miners,
    sums_to_stats,
    timing_enable,
    timing_read,
)

from .moments import (  # noqa: F401,E402
    HistSpec,
    error_bars,
    errors_from_moments,
    hist_quantile,
    report_with_errors,
)

from .contrasts import (  # noqa: F401,E402
    Pair,
    contrasts,
    contrasts_from_sums,
    join_cross,
    pairs_between_miners,
    pairs_vs_baseline,
    report_contrasts,
    split_cross,
)

from .classes import (  # noqa: F401,E402
    classes_from_groups,
    classes_of,
    report_classes,
)

from .quantiles import (  # noqa: F401,E402
    OrderStat,
    QuantileResult,
    order_stats_from_words,
    quantile_ci_ranks,
    quantile_rank,
    report_quantiles,
)

from .tails import (  # noqa: F401,E402
    TailItem,
    TailResult,
    TailSpec,
    items_words,
    own_tails,
    report_tails,
    tails_from_words,
    tails_given,
)

from .bootstrap import (  # noqa: F401,E402
    BootItem,
    BootstrapResult,
    across_points,
    boot_ranks,
    launch_boot_weights,
    own_bootstrap,
    report_bootstrap,
)

from . import model  # noqa: F401,E402  (first-order analytical stale-rate model, plot.py restated)

__version__ = "0.1.0"

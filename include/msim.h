/*
 * msim.h — C ABI of libmsim, the MI355X (gfx950) engine for darosior/miningsimulation's per-run
 * simulation loop. Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   msim_miner            <- Miner(unsigned id, uint64_t perc, milliseconds prop, bool selfish)
 *                            simulation.h:57-59, as built by SetupMiners() main.cpp:44-65
 *   msim_config_create    <- SetupMiners() + SIM_DURATION (main.cpp:7, 44-65); validates what the
 *                            reference only asserts (simulation.h:220: percentages must sum to 100)
 *   msim_run              <- the std::async batch loop of main() (main.cpp:195-220): SIM_RUNS calls of
 *                            RunSimulation(SIM_DURATION, miners) (main.cpp:128-192, :209) and the
 *                            stats_total[j] += stats[j] aggregation (main.cpp:211-217)
 *   msim_stats            <- MinerStats {long blocks_found; double blocks_share; double stale_rate;}
 *                            (main.cpp:13-20), same field order and types
 *   msim_run_multi        <- the same loop over several GPUs: shards + one RCCL all-reduce of msim_sums
 *   msim_launch           <- device-resident form of msim_run for hosts that own streams and an
 *                            RCCL communicator (multi-GPU: shard runs, all-reduce msim_sums)
 * Seeds: RunSimulation draws two 32-bit std::random_device values (main.cpp:131-134); run r of a
 * launch uses (seed_base + 2r, seed_base + 2r + 1) mod 2^32 for (block_interval, miner_picker).
 */
#ifndef MSIM_H
#define MSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSIM_OK 0
#define MSIM_E_INVALID (-1)  /* bad argument (null pointer, n == 0, negative duration/propagation) */
#define MSIM_E_WEIGHTS (-2)  /* weights do not add up to 100 (or total_weight): the reference asserts */
#define MSIM_E_SELFISH (-3)  /* reserved (round 2 rejected selfish networks the entity engine cannot serve;
                                every network with selfish miners now runs, those on the general engine) */
#define MSIM_E_MINERS (-4)   /* network too large for the general engine: one run's explicit chains (miners x
                                blocks a run can have x 12 B) would exceed 96 GiB (msim_config_create), or the
                                launch's workspace exceeds the device's free memory (msim_run, msim_sweep_run) */
#define MSIM_E_HIP (-5)      /* HIP runtime error (no device, launch failure, out of memory) */
#define MSIM_E_CAPACITY (-6) /* a run outgrew every window of the general engine (its last window holds every
                                block a run of the config's duration can have: practically never) */
#define MSIM_E_PICK (-7)     /* PickFinder fell through (simulation.h:220 assert): percentages < 100 */
/* Durations. Any duration_ms >= 0 is accepted and exact; what changes with it is the engine. The event-skipping
 * pipeline cuts a run into at most 256 draw segments of at most 65 504 blocks (its draw kernel packs a segment's
 * per-miner counts into 16 bits, and one miner can own every block of a segment), so it serves honest networks up to
 * about 318 years (256 x 65 504 blocks at one per 600 s, less the 8-sigma margin of the pre-generated blocks). A
 * longer run is not refused: msim_config_create keeps it on the per-lane kernel (msim_pipeline_info: uses_pipeline 0,
 * as under MSIM_NO_PIPELINE), slower and exact; a shared-draw sweep of such points runs as the plain sweep. No plan
 * ever has a segment of more than 65 535 blocks, whatever the run count, the wave slots or the launches in flight.
 * The general engine refuses (MSIM_E_MINERS) a selfish network whose last window, every block a run can have, would
 * pass 96 GiB of chains for one lane or 2^32 blocks (about 81 000 years). */

#define MSIM_MAX_MINERS 15        /* networks on the compact per-lane / entity-engine state */
#define MSIM_MAX_SELFISH 4        /* selfish miners per network on the entity engine (msim_sel.h); more run on
                                     the general engine (msim_general.h) */
#define MSIM_MAX_WIDE_MINERS 4096 /* honest networks on the large-network pipeline (BASELINE configs[4]); larger
                                     honest networks run on the general engine */

typedef struct msim_miner {
    uint32_t id;            /* Miner::id (simulation.h:43) */
    uint64_t perc;          /* Miner::perc, integer percent of network hashrate (simulation.h:45) */
    int64_t propagation_ms; /* Miner::propagation (simulation.h:47) */
    uint8_t is_selfish;     /* Miner::is_selfish (simulation.h:55) */
} msim_miner;

typedef struct msim_config msim_config;

/* Per-miner aggregate over runs, bit layout of MinerStats (main.cpp:13-20). */
typedef struct msim_stats {
    int64_t blocks_found;
    double blocks_share;
    double stale_rate;
} msim_stats;

/* Order-independent device sums per miner (integers, so 1/2/4/8-GPU all-reduces are bit-identical).
 * share and stale_rate are summed as Q32.32 fixed point split into 32-bit limbs:
 *   sum(share) = share_hi + share_lo * 2^-32 (exact integer sums of per-run round(share * 2^32)). */
typedef struct msim_sums {
    int64_t blocks_found;
    int64_t stale_blocks;
    uint64_t share_hi, share_lo;
    uint64_t rate_hi, rate_lo;
} msim_sums;

/* Per-run, per-miner integer counters (the bit-exact parity surface). */
typedef struct msim_run_record {
    uint32_t found; /* blocks of this miner in the final best chain (main.cpp:24-26) */
    uint32_t stale; /* Miner::stale_blocks at the end of the run (simulation.h:133) */
} msim_run_record;

int msim_config_create(const msim_miner *miners, uint32_t n, int64_t duration_ms, msim_config **out);
/* Weight generalisation (not expressible in the reference, whose perc are integer
 * percentages, simulation.h:45, main.cpp:43): `perc` holds integer weights that must add up to
 * total_weight W < 2^31, and PickFinder uses UINT64_MAX / W in place of PERC_MULTIPLIER
 * (simulation.h:18, 217). W = 100 is exactly msim_config_create. Honest networks of more than
 * MSIM_MAX_MINERS miners (up to MSIM_MAX_WIDE_MINERS), or with W != 100, run on the large-network
 * pipeline; networks with up to MSIM_MAX_SELFISH selfish miners and n <= MSIM_MAX_MINERS (any W) run
 * on the entity engine; every other network with selfish miners (more selfish miners, or more miners) runs
 * on the general engine (msim_general.h: the reference's explicit chains in bounded windows of device
 * memory, slower per block, exact), which also finishes the runs the entity engine cannot (a selfish
 * majority whose withheld chain outgrows its window). The general engine also serves honest networks of
 * more than MSIM_MAX_WIDE_MINERS miners and every network whose ids are not distinct or include UINT_MAX
 * (Genesis's id, simulation.h:31-33): the reference identifies blocks, stale blocks and found blocks by
 * Miner::id (simulation.h:35-38, 133; main.cpp:24-26), and so does that engine. */
int msim_config_create_weighted(const msim_miner *miners, uint32_t n, int64_t duration_ms, uint64_t total_weight,
                                msim_config **out);
/* 1 when the config runs on the large-network pipeline (set MSIM_FORCE_WIDE=1 in the environment before
 * msim_config_create to route small honest networks there too, e.g. for cross-path parity checks).
 * A second test switch, MSIM_MAX_SLICE_RUNS=<n> (n > 0), read at every sizing and launch call: a slice of the
 * honest pipeline, the large-network pipeline and the entity engine (single networks, the opt-in
 * segment-parallel form and sweeps) holds at most n runs, rounded up to a multiple of 256, so a few hundred
 * runs exercise the slice loops that otherwise begin past 16 GiB of workspace or 2^22 runs per point.
 * msim_workspace_bytes, msim_launch, msim_run, msim_pipeline_info (slice_runs) and the sweep and multi-GPU
 * entry points all follow it; the general engine has no slices. Unset, nothing changes.
 * A third, MSIM_PIPE_FORCE_RETRY (set to anything), read at every launch of the honest pipeline: its combine
 * kernel flags every run, so the retry kernel computes them all (what MSIM_SEL_FORCE_RETRY does on the entity
 * engine); at most 65 536 runs per launch then, the retry list's size.
 * A fourth, MSIM_MOMENTS_CHUNK_RUNS=<n> (n > 0), read only by msim_run_moments, msim_sweep_run_moments,
 * msim_run_contrasts, msim_sweep_run_contrasts, msim_run_classes and msim_sweep_run_classes at every call: a chunk
 * of runs whose records stay in device memory holds at most n runs (per point), so a few hundred runs exercise the
 * chunk loop and its limb-by-limb addition. msim_run_order_stats and msim_sweep_run_order_stats follow it too.
 * MSIM_RANK_TEST_WG_RUNS=<n> (n > 0), read at every msim_rank_count_launch: a workgroup of the count kernel takes at
 * most n runs, so a few hundred runs give several workgroups along the run axis (see msim_rank_count_launch).
 * MSIM_TAIL_TEST_WG_RUNS=<n> (n > 0) does the same for msim_tail_launch, and msim_run_tails and msim_sweep_run_tails
 * follow MSIM_MOMENTS_CHUNK_RUNS.
 * Five more, MSIM_PIPE_TEST_*, read at every sizing and launch call of the honest pipeline (single networks and
 * shared-draw sweeps). Each only ever lowers a capacity below its 8-sigma size (the smaller of the natural value and
 * n, n > 0), and does so in the layout computation, so the buffers are exactly as large as the kernels are told:
 *   MSIM_PIPE_TEST_CAP=<n>         slow-block slots per (run, segment) of the pipeline's layout and of a shared-draw
 *                                  group's envelope layout
 *   MSIM_PIPE_TEST_LCAP=<n>        episode-list length of the same two
 *   MSIM_PIPE_TEST_POINT_CAP=<n>   the slots per (run, segment) of every point of a shared-draw group
 *   MSIM_PIPE_TEST_POINT_LCAP=<n>  the index-list length of every point of a shared-draw group
 *   MSIM_PIPE_TEST_K2_KIND=<0|1>   the episode kernel's state machine (0 lean, 1 mid) for every one of those layouts,
 *                                  whatever the network's rho; any other value is ignored
 * A run that outgrows a lowered capacity is flagged and recomputed by the retry kernel like any other, so results
 * stay the same and status[0] counts the retried runs. Unset, nothing changes.
 * Two more, for the large-network pipeline (single networks and sweeps), read at every sizing and launch call; they
 * too only ever lower (the smaller of the natural value and n, n > 0) and act in the layout computation:
 *   MSIM_WIDE_TEST_RCAP=<n>        candidate slots per run of a plain wide launch and of a shared-draw group's envelope
 *   MSIM_WIDE_TEST_POINT_RCAP=<n>  candidate slots per run of every point of a shared-draw group of more than one point
 * The large-network pipeline has no retry kernel: a run that outgrows a capacity fails (status[1] counts it, its
 * records stay unwritten, msim_run / msim_sweep_run return MSIM_E_CAPACITY). Unset, nothing changes.
 * Five more, MSIM_GEN_TEST_*, for the general engine (a network it serves alone, and the runs it finishes for the
 * entity engine), read at every sizing and launch call. They too only ever lower (the smaller of the natural value
 * and n) and act in the layout computation, before any offset; a value outside the stated range is ignored:
 *   MSIM_GEN_TEST_LANES=<n> (n >= 1)     lanes of every tier, not rounded to waves: a lane then serves its runs in turn
 *   MSIM_GEN_TEST_CAP1=<n> (n >= 8)      the window (blocks per chain) of tier 1,
 *   MSIM_GEN_TEST_CAP2=<n> (n >= 8)      of tier 2,
 *   MSIM_GEN_TEST_CAP3=<n> (n >= 8)      of tier 3. A lowered window removes no tier and adds none but the third below
 *                                        a lowered second (short runs, whose last window is the second's 4 096
 *                                        blocks), so a lowered last window can be too small: such a run fails
 *                                        (status[1] counts it, its records stay unwritten, msim_run / msim_sweep_run
 *                                        return MSIM_E_CAPACITY)
 *   MSIM_GEN_TEST_LIST_CAP=<n> (n >= 1)  the length of the tier lists that the kernels are told; the lists keep their
 *                                        natural allocation. A run that finds no room in a list fails in the same way
 * msim_pipeline_info reports the lowered geometry (slice_runs: tier-1 lanes, segment_blocks: tier-1 window,
 * blocks_per_run: last window). Unset, nothing changes.
 * MSIM_K1_SLOTS=<n>, read at every sizing and launch call of the honest pipeline (single networks and shared-draw
 * sweeps): the draw kernel's wave slots, in place of the device's (compute units x resident waves), for which the
 * run is cut into segments. One launch in flight plans for 3 n slots, j launches for 2 n / j. A measurement switch
 * and a test switch: 1 with two launches in flight gives the fewest, longest segments the planner lays out
 * (tests/test_gpu_long_runs.py), and a pinned value makes msim_pipeline_info independent of the device
 * (tests/host_plans.py). It changes the geometry and the workspace size, never a result. */
int msim_config_is_wide(const msim_config *cfg);
/* How many launches of this config the caller keeps in flight at once (default 1; e.g. 2 when steps
 * alternate over two HIP streams). The event-skipping pipeline plans its draw kernel's grid for it: three
 * rounds of resident waves for one launch, one round each for two. A tuning hint with no effect on results;
 * it changes msim_workspace_bytes, so set it before sizing the workspace. MSIM_E_INVALID outside 1..64.
 * (No reference counterpart: the reference runs one std::async batch at a time, main.cpp:205-220.) */
int msim_config_set_concurrent_launches(msim_config *cfg, uint32_t n);
void msim_config_destroy(msim_config *cfg);
uint32_t msim_config_miner_count(const msim_config *cfg);

/* Run runs [run_begin, run_begin + n_runs) on HIP device `device`.
 * out_sums: M entries (like stats_total, main.cpp:199); with opt_per_run given, the share/stale_rate
 *           doubles are summed on the host in run order exactly as main.cpp:211-217 does; otherwise
 *           they come from the fixed-point device sums (relative error < 1e-9: that bounds the fixed-point
 *           aggregate against the run-order f64 sum, i.e. the per-run rounding to 2^-32 and the summation
 *           order; the device sums themselves equal their definition, the integer sum of the per-run terms
 *           round(x * 2^32), exactly, on every engine).
 * opt_per_run: n_runs * M records or NULL; opt_best_height: n_runs entries (|best chain| - 1) or NULL.
 * opt_sums: M fixed-point msim_sums or NULL. */
int msim_run(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
             msim_stats *out_sums, msim_sums *opt_sums, msim_run_record *opt_per_run, uint32_t *opt_best_height);

/* Several GPUs of one node (the std::async loop of main.cpp:205-220 across devices): runs
 * [run_begin, run_begin + n_runs) cut into contiguous shards, one per device in `devices` (NULL = devices
 * 0 .. n_devices - 1), each through msim_launch on its own stream (all devices run concurrently), then ONE
 * ncclAllReduce (RCCL over xGMI, single-process communicator from ncclCommInitAll, created once per device
 * list and kept for the process, issued for every device inside one group; none for one device) of the
 * integer msim_sums. Every device's buffers are allocated before anything runs, so
 * an allocation failure returns MSIM_E_HIP without entering a collective. The result is bit-identical to
 * msim_run for every n_devices (out_sums from the fixed-point sums; opt_sums or NULL). */
int msim_run_multi(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base,
                   const int *devices, uint32_t n_devices, msim_stats *out_sums, msim_sums *opt_sums);
/* msim_run_multi plus per-device timing: opt_shard_ms (2 * n_devices doubles or NULL) receives, for device g,
 * [2g] the milliseconds of its shard's launches and [2g + 1] those of the all-reduce that follows them
 * (HIP events on the device's stream), so a host can see how evenly the shards ran. */
int msim_run_multi_timed(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base,
                         const int *devices, uint32_t n_devices, msim_stats *out_sums, msim_sums *opt_sums,
                         double *opt_shard_ms);
/* Lifetime of the cached communicators of msim_run_multi / msim_sweep_run_multi: one set per device list,
 * created on first use and kept for the process. msim_multi_release destroys every set no call is using and
 * returns how many it released (a host that cycles through many device lists, or that resets its devices,
 * calls it first). A set whose collectives fail is destroyed at once and re-created by the next call. */
int msim_multi_release(void);

/* Device-resident launch on the current HIP device and the given hipStream_t (NULL = default).
 * d_sums: M msim_sums in device memory (overwritten). d_per_run / d_best_height: device buffers or NULL.
 * d_status: 2 uint32_t in device memory (required): [0] = runs that needed the retry kernel, [1] = runs
 * that failed even there (each failed run contributes nothing to d_sums: check it before using d_sums).
 * d_workspace / workspace_bytes: scratch from msim_workspace_bytes(); the call does no allocation
 * and no synchronisation, so it can be captured into a hipGraph. */
size_t msim_workspace_bytes(const msim_config *cfg, uint64_t n_runs);
int msim_launch(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, void *d_sums,
                void *d_per_run, void *d_best_height, void *d_status, void *d_workspace, size_t workspace_bytes,
                void *stream);

/* Device draw primitives (bit-exact with the reference's host libm; test and sampler surface):
 *   msim_device_log1p     glibc log1p on the reference's domain (xoroshiro128++.h:19)
 *   msim_device_intervals NextBlockInterval of given uniform u64 draws, in ms (simulation.h:205-210),
 *                         through the draw kernel's production path (msim_fastdraw.h + exact fallback)
 *   msim_device_picks     PickFinder index of given uniform u64 draws (simulation.h:213-221), through
 *                         the draw kernel's table lookup; -1 where the reference would assert
 *   msim_device_k1_quads  the draw kernel's quad of four blocks (its fast draws, then their exact redraw when the
 *                         quad is flagged) from n pairs of xoroshiro128++ states: d_states holds s0, s1 of the
 *                         interval stream and s0, s1 of the picker stream per quad; d_out receives per quad
 *                         the four intervals in ms, then the four finders (15 where PickFinder falls through).
 *                         Honest networks of the pipeline only; the kernel's uniform-delay or per-finder
 *                         instantiation is chosen as for a run of cfg
 * All pointers are device memory; launches go to `stream` (hipStream_t, NULL = default). */
int msim_device_k1_quads(const msim_config *cfg, const uint64_t *d_states, uint32_t *d_out, uint64_t n, void *stream);
int msim_device_log1p(const double *d_x, double *d_out, uint64_t n, void *stream);
int msim_device_intervals(const uint64_t *d_uniform, int64_t *d_out_ms, uint64_t n, void *stream);
int msim_device_picks(const msim_config *cfg, const uint64_t *d_uniform, int32_t *d_out_index, uint64_t n,
                      void *stream);

/* Parameter sweeps (BASELINE configs[3]: selfish share x propagation grid). The reference runs one
 * network per build (SetupMiners, main.cpp:44-65, edited by hand per README.md:21-27); a sweep runs
 * every point of a grid in ONE device launch, one lane per (point, run). Point p, run r gives exactly
 * the result of msim_run(cfgs[p], run_begin, ...) for run run_begin + r (same seeds for every point).
 * All points must have the same miner count. Sums / records are point-major:
 *   sums[p * M + k], per_run[(p * runs_per_point + r) * M + k], best_height[p * runs_per_point + r].
 * The points are either all narrow (at most MSIM_MAX_MINERS miners with percentages) or all on the large-network
 * pipeline (msim_config_is_wide: more than MSIM_MAX_MINERS honest miners, or integer weights with W != 100; engine 2
 * below); a sweep mixing the two is MSIM_E_INVALID, unless some point runs on the general engine, which then serves
 * every point. A sweep of large-network points is one plain launch of that pipeline per point (into the sweep's
 * outputs, one workspace), or the shared-draw form below. */
typedef struct msim_sweep msim_sweep;
int msim_sweep_create(const msim_config *const *cfgs, uint32_t n_points, msim_sweep **out);
/* msim_sweep_create with flags (0: exactly msim_sweep_create; unknown bits: MSIM_E_INVALID).
 * MSIM_SWEEP_SHARED_DRAWS: the shared-draw form of honest sweeps. The reference compares propagation delays by
 * editing SetupMiners and rebuilding once per point (README.md:21-27: the same hashrates at 10 s and at 100 ms).
 * Points of a sweep with the same weights and duration see the same seeds and so the same draws; only which blocks
 * start a fork episode depends on the delays. Such points form a draw group: the draw kernel runs ONCE per group
 * (on the group's envelope network: every miner at its largest delay over the group), a split kernel derives each
 * point's own episode list from the envelope's, and the episode and combine kernels run per point. Results are those
 * of msim_sweep_create, bit for bit. The flag takes effect only when the event-skipping pipeline takes every point
 * (honest, at most MSIM_MAX_MINERS miners with percentages, delays below 262 s, rare forks; MSIM_NO_PIPELINE unset at
 * config creation); any other sweep runs exactly as without it. A group whose envelope the pipeline does not take is
 * split (its point with the largest delay leaves it) until it does.
 * A test switch, MSIM_SWEEP_SHARED_MAX_GROUP=<n> (0 < n < 8), read at every launch: a split pass serves at most n
 * points of a group, so a group of five takes the further split passes (never further draw passes) that otherwise
 * begin past 8 points.
 * Sweeps of large-network points (engine 2) take the flag too: points with equal weights, equal W and equal duration
 * form a draw group; per group and slice the draw kernel W1 runs once on the envelope network, a split kernel derives
 * each point's candidate list from the envelope's, and the episode and combine kernels run per point. A group whose
 * envelope the large-network pipeline does not take (its fork rate is past what the combine kernel's LDS holds) loses
 * its point with the largest delay to a group of its own until it is taken; a group of one is the plain launch.
 * Results are those of the flags-0 sweep bit for bit, with ONE exception: that pipeline has no retry kernel, and a run
 * whose ENVELOPE candidate list overflows its (8-sigma) capacity fails at every point of the group, so the shared form
 * can fail a run (status[1], MSIM_E_CAPACITY) that the point's own launch would not. A point's own list overflows
 * exactly when its own launch's would, and fails the run at that point only. */
#define MSIM_SWEEP_SHARED_DRAWS 1u
int msim_sweep_create_ex(const msim_config *const *cfgs, uint32_t n_points, uint32_t flags, msim_sweep **out);
/* Host only, no device: the draw group of a point (0 .. draw_groups - 1), or -1 when the sweep does not run in the
 * shared-draw form (flags 0, or a sweep the flag has no effect on) or the point does not exist. (The reference has
 * one network per build, README.md:21-27; no counterpart.) */
int msim_sweep_group_of(const msim_sweep *sweep, uint32_t point);
/* How msim_sweep_launch will execute runs_per_point runs of every point, as msim_pipeline_info for a config (the
 * reference: one rebuild per point, README.md:21-27). */
typedef struct msim_sweep_plan {
    uint32_t engine;          /* 0: per-lane kernel, one lane per (point, run); 1: shared-draw pipeline; 2: large-network
                                 pipeline (msim_pipeline_info's value for it), with or without shared draws; 3: entity
                                 engine (a point with selfish miners); 4: general engine */
    uint32_t draw_groups;     /* engines 1, 2: draw passes per slice (engine 2 with flags 0: n_points); else 0 */
    uint32_t largest_group;   /* engines 1, 2: points of the largest draw group (engine 2 with flags 0: 1); else 0 */
    uint32_t slice_runs;      /* runs per point and slice (engines 1, 2: of the group with the smallest slices) */
    uint64_t workspace_bytes; /* msim_sweep_workspace_bytes */
} msim_sweep_plan;
int msim_sweep_info(const msim_sweep *sweep, uint64_t runs_per_point, msim_sweep_plan *out);
void msim_sweep_destroy(msim_sweep *sweep);
size_t msim_sweep_workspace_bytes(const msim_sweep *sweep, uint64_t runs_per_point);
/* Device-resident, asynchronous on `stream`; d_sums: n_points * M msim_sums; d_status as msim_launch. */
int msim_sweep_launch(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                      void *d_sums, void *d_per_run, void *d_best_height, void *d_status, void *d_workspace,
                      size_t workspace_bytes, void *stream);
uint32_t msim_sweep_point_count(const msim_sweep *sweep);
uint32_t msim_sweep_miner_count(const msim_sweep *sweep);
/* Host convenience: out_stats n_points * M (fixed-point sums converted), optional sums / records. */
int msim_sweep_run(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                   int device, msim_stats *out_stats, msim_sums *opt_sums, msim_run_record *opt_per_run,
                   uint32_t *opt_best_height);
/* A sweep over several GPUs as msim_run_multi: every device runs every point on its shard of the runs,
 * one RCCL all-reduce of the n_points * M sums; bit-identical to msim_sweep_run. */
int msim_sweep_run_multi(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                         const int *devices, uint32_t n_devices, msim_stats *out_stats, msim_sums *opt_sums);

/* Stage timing for measurement (bench.py): while enabled, every msim_launch records HIP events on its
 * stream around the whole launch and around each draw kernel (K1, the dominant kernel of the
 * event-skipping pipeline). msim_timing_read synchronises on those events, returns the summed
 * elapsed milliseconds and the number of launches since the last enable/read, and clears them. */
int msim_timing_enable(int on);
int msim_timing_read(double *draws_ms, double *launch_ms, uint32_t *launches);
/* Same, plus the entity engine's stage (networks with selfish miners: the E1 kernels of every slice;
 * draws_ms is then the word-draw kernel D1). */
int msim_timing_read_stages(double *draws_ms, double *engine_ms, double *launch_ms, uint32_t *launches);
/* Same, plus BUSY time: the union of the stage's (begin, end) intervals over every stream, i.e. how long at
 * least one such kernel was running (two launches in flight on two streams count their overlap once). With
 * launches alternating over streams this is the stage's share of the wall clock, never more than it. */
typedef struct msim_timing {
    double draws_ms, engine_ms, launch_ms;                 /* summed per-launch intervals */
    double draws_busy_ms, engine_busy_ms, launch_busy_ms;  /* union of the intervals */
    uint32_t launches;
} msim_timing;
int msim_timing_read_all(msim_timing *out);

/* How msim_launch will execute n_runs of this config on the current device. */
typedef struct msim_pipeline_layout {
    uint32_t uses_pipeline;   /* 1: event-skipping pipeline (honest network); 2: large-network pipeline;
                                 3: entity engine (selfish miners); 4: general engine (slice_runs = its
                                 lanes, segment_blocks = its first window, segments = window tiers,
                                 blocks_per_run = its last window); 6: segment-parallel selfish runs
                                 (opt-in, environment MSIM_SELSEG=1; one selfish miner: settled-form workers
                                 per segment + per-run stitch, rho = the expected cuts per find); 0: per-lane
                                 kernel (5 was the removed selfish pipeline) */
    uint32_t slice_runs;      /* runs per pipeline slice */
    uint32_t segment_blocks;  /* blocks per draw-kernel worker */
    uint32_t segments;        /* workers per run */
    uint64_t blocks_per_run;  /* pre-generated blocks per run (segments * segment_blocks) */
    uint64_t workspace_bytes; /* pipeline part of msim_workspace_bytes */
    double rho;               /* probability that a block starts a fork episode */
} msim_pipeline_layout;
int msim_pipeline_info(const msim_config *cfg, uint64_t n_runs, msim_pipeline_layout *out);

/* GPU-scale forms of test.cpp's samplers. One RNG stream RNG{seed} (xoroshiro128++.h:23)
 * of n draws, exactly as the reference's single loops draw it (integer results identical for any n):
 *   msim_sample_picks      out_counts[k] = #{i < n : PickFinder(draw i) == k}, k < M; out_counts[M] = draws
 *                          where PickFinder would assert (simulation.h:220). test.cpp:15-63
 *                          MinerPickerSample (10^8 picks over 100 miners of 1 %) and the stream of
 *                          test.cpp:68-118 MinerPickerSmallBig. out_counts: M + 1 host entries.
 *   msim_sample_intervals  exact integer moments of n NextBlockInterval draws (simulation.h:205-210):
 *                          test.cpp:191-208 BlockIntervalSample (mean and std dev follow from them).
 * Synchronous, on HIP device `device`. */
typedef struct msim_interval_moments {
    uint64_t n;
    uint64_t sum;                /* sum of intervals (ms) */
    uint64_t sumsq_lo, sumsq_hi; /* sum of squared intervals, 128-bit */
    uint64_t max;                /* largest interval (ms) */
} msim_interval_moments;
int msim_sample_picks(const msim_config *cfg, uint64_t seed, uint64_t n, uint64_t *out_counts, int device);
int msim_sample_intervals(uint64_t seed, uint64_t n, msim_interval_moments *out, int device);

/* Per-miner error bars: exact second moments and histograms of the per-run terms, reduced on the device from the
 * records a launch writes on request (d_per_run, d_best_height). For one run and one miner, with f = record.found,
 * s = record.stale and L = best_height[run], the terms are the ones every engine adds to its msim_sums:
 *   share_t = (f == 0 || L == 0) ? 0 : (uint64)((double)f / (double)L * 2^32 + 0.5)
 *   rate_t  = (f == 0)           ? 0 : (uint64)((double)s / (double)f * 2^32 + 0.5)
 * (L == 0 with f > 0 only happens to a miner holding Genesis's id, simulation.h:31-33, in a run without blocks;
 * the engines' own share term f / 0 has no value there, and `first` counts 0 for it.)
 * Every field is a plain integer sum over runs, so it is identical for any split into workgroups, launches or
 * ranks and can be all-reduced. `first` follows msim_sums' limb convention. A square sum holds, in limb i, the sum
 * of the i-th 32-bit pieces of the runs' full 128-bit (64-bit for found/stale) products: its value is
 * sum(limb[i] << 32 i), limbs are not normalised (join them with carries), exact up to 2^32 runs. */
typedef struct msim_moments {
    msim_sums first;         /* recomputed from the records */
    uint64_t found_sq[2];    /* sum f^2 */
    uint64_t stale_sq[2];    /* sum s^2 */
    uint64_t found_stale[2]; /* sum f s */
    uint64_t share_sq[4];    /* sum share_t^2 */
    uint64_t rate_sq[4];     /* sum rate_t^2 */
} msim_moments;

/* Histograms of the terms, bin widths powers of two in term units (2^-32):
 *   bin(t) = 0 if t < lo;  bins + 1 if ((t - lo) >> shift) >= bins;  1 + ((t - lo) >> shift) otherwise.
 * Counts are uint64 [points][M][2][bins + 2], index 0 = share, 1 = rate; every row adds up to the run count. */
typedef struct msim_hist_spec {
    uint32_t bins; /* 1..1024 */
    uint32_t share_shift, rate_shift; /* 0..63 */
    uint64_t share_lo, rate_lo;
} msim_hist_spec;

/* Device-resident and asynchronous on `stream` (hipStream_t, NULL = default): no allocation, no synchronisation,
 * independent of any config. d_per_run: n_points * runs_per_point * m msim_run_record and d_best_height:
 * n_points * runs_per_point uint32_t, in msim_launch's / msim_sweep_launch's layouts (device memory). d_moments:
 * n_points * m msim_moments, and d_hist_or_NULL (with opt_hist_spec): the counts above; both are overwritten
 * (zeroed inside the launch, as d_sums is). Results are meaningless for a launch whose d_status[1] != 0: a failed
 * run writes no record. MSIM_E_INVALID for m == 0, no runs, more than 2^32 - 1 runs per point, bins outside
 * 1..1024, a shift above 63, or exactly one of opt_hist_spec / d_hist_or_NULL. */
int msim_moments_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                        const void *d_best_height, const msim_hist_spec *opt_hist_spec, void *d_moments,
                        void *d_hist_or_NULL, void *stream);
/* Host conveniences shaped like msim_run / msim_sweep_run: the records and best heights stay in device memory,
 * only sums, status, moments and histograms come back; chunks of runs are added limb by limb on the host.
 * out_stats: from the fixed-point sums. out_moments: M (n_points * M) entries; opt_hist with opt_hist_spec:
 * M * 2 * (bins + 2) (times n_points) counts, or both NULL. MSIM_E_CAPACITY on a failed run, as msim_run.
 * A test switch, MSIM_MOMENTS_CHUNK_RUNS=<n> (n > 0), read only by these two functions and their contrast forms
 * below: a chunk holds at most n runs (per point), so a few hundred runs exercise the chunk loop. */
int msim_run_moments(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                     msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                     const msim_hist_spec *opt_hist_spec, uint64_t *opt_hist);
int msim_sweep_run_moments(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                           int device, msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                           const msim_hist_spec *opt_hist_spec, uint64_t *opt_hist);

/* Means and standard errors per miner from the moments of N = n_runs runs: mean = S1 / N and
 * se = sqrt((N S2 - S1^2) / (N^2 (N - 1))), share and rate scaled by 2^-32. pooled_rate = sum s / sum f (0 when
 * sum f = 0) with its delta-method error sqrt(N / (N - 1) (F^2 sum s^2 - 2 S F sum fs + S^2 sum f^2)) / F^2
 * (0 when F = 0). The integer numerators are formed exactly, then a handful of correctly rounded f64 operations
 * follow, so differently normalised limbs of one value give the same bits. Every *_se is NaN for N == 1. */
typedef struct msim_errors {
    double found_mean, found_se;
    double share_mean, share_se;
    double rate_mean, rate_se;
    double pooled_rate, pooled_rate_se;
} msim_errors;
/* Host only. */
void msim_moments_to_errors(const msim_moments *moments, uint32_t m, uint64_t n_runs, msim_errors *out);

/* Paired contrasts: the difference, ratio and correlation of two (point, miner) columns of ONE launch's records,
 * with standard errors. (No reference counterpart: the reference prints three means per miner of one network,
 * main.cpp:224-234, and compares networks by rebuilding, README.md:21-27.) A sweep runs every point on the same
 * seeds (above), so the two sides of a contrast between points share their draws and the per-run difference is far
 * less noisy than either side; two miners of one network are negatively correlated, so there the independent
 * formula understates the error. What msim_moments lacks for either is the cross term, summed here exactly.
 * A pair names side a and side b; with f, s, share_t, rate_t of each side's record (and its own point's best
 * height) as defined for msim_moments, msim_cross holds the sums over runs of f_a f_b, s_a s_b (64-bit products,
 * two limbs), share_t,a share_t,b and rate_t,a rate_t,b (128-bit products, four limbs) in msim_moments' limb
 * convention: limb i is the sum of the products' i-th 32-bit pieces, limbs are not normalised, exact up to
 * 2^32 - 1 runs. Plain integer sums: identical for any split into workgroups, chunks, launches or ranks. A pair of
 * a column with itself gives that column's four square sums of msim_moments. */
typedef struct msim_pair {
    uint32_t point_a, miner_a, point_b, miner_b;
} msim_pair;
typedef struct msim_cross {
    uint64_t found_found[2]; /* sum f_a f_b */
    uint64_t stale_stale[2]; /* sum s_a s_b */
    uint64_t share_share[4]; /* sum share_t,a share_t,b */
    uint64_t rate_rate[4];   /* sum rate_t,a rate_t,b */
} msim_cross;
#define MSIM_MAX_PAIRS 16776960u /* 65 535 tiles of 256 pairs: the grid of one msim_cross_launch */

/* Device-resident and asynchronous on `stream`, as msim_moments_launch: no allocation, no synchronisation,
 * independent of any config. d_per_run / d_best_height: as msim_moments_launch. d_pairs: n_pairs msim_pair in device
 * memory. d_cross: n_pairs msim_cross, overwritten (zeroed inside the launch). A pair with a point >= n_points or a
 * miner >= m reads nothing and leaves its twelve words zero (the launch cannot see device memory; validate on the
 * host with msim_pairs_check). MSIM_E_INVALID, with nothing written, for m == 0, no points, no runs, more than
 * 2^32 - 1 runs per point, n_pairs == 0 or above MSIM_MAX_PAIRS, or a null pointer. */
int msim_cross_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                      const void *d_best_height, const void *d_pairs, uint32_t n_pairs, void *d_cross, void *stream);
/* Host only: MSIM_OK when there are 1..MSIM_MAX_PAIRS pairs and every one lies within n_points x m, else
 * MSIM_E_INVALID. */
int msim_pairs_check(uint32_t m, uint32_t n_points, const msim_pair *pairs, uint32_t n_pairs);
/* msim_run_moments / msim_sweep_run_moments plus the cross sums of `pairs` (checked with msim_pairs_check, uploaded
 * once; for a single config every pair has point_a == point_b == 0): every chunk adds msim_cross_launch on the same
 * stream, and the chunks' cross words are added limb by limb on the host. out_cross: n_pairs entries. They follow
 * MSIM_MOMENTS_CHUNK_RUNS as the two moments functions do. */
int msim_run_contrasts(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                       const msim_pair *pairs, uint32_t n_pairs, msim_stats *out_stats, msim_sums *opt_sums,
                       msim_moments *out_moments, msim_cross *out_cross);
int msim_sweep_run_contrasts(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point,
                             uint32_t seed_base, int device, const msim_pair *pairs, uint32_t n_pairs,
                             msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                             msim_cross *out_cross);

/* One pair's contrasts from N = n_runs runs. For each quantity, A and B are the sides' first sums, S_aa and S_bb
 * their square sums (both from msim_moments), S_ab the cross sum:
 *   diff     = (A - B) / N
 *   diff_se  = sqrt((N (S_aa - 2 S_ab + S_bb) - (A - B)^2) / (N^2 (N - 1)))     the per-run difference's error
 *   corr     = (N S_ab - A B) / sqrt((N S_aa - A^2) (N S_bb - B^2))             NaN when a variance is zero
 *   ratio    = A / B (NaN for B == 0),  ratio_se = sqrt(N / (N - 1) (B^2 S_aa - 2 A B S_ab + A^2 S_bb)) / B^2
 *              (found and share only; the delta method, as msim_errors' pooled_rate_se)
 * share and rate differences are scaled by 2^-32. Every *_se and *_corr is NaN for N == 1. The integer numerators
 * are formed exactly, signs handled explicitly, then a handful of correctly rounded f64 operations follow, so
 * differently normalised limbs of one value give the same bits. */
typedef struct msim_contrast {
    double found_diff, found_diff_se, found_corr, found_ratio, found_ratio_se;
    double stale_diff, stale_diff_se, stale_corr;
    double share_diff, share_diff_se, share_corr, share_ratio, share_ratio_se;
    double rate_diff, rate_diff_se, rate_corr;
} msim_contrast;
/* Host only. moments: n_points * m entries (of n_runs runs each), indexed point * m + miner by the pairs; pairs
 * must pass msim_pairs_check for those counts. */
void msim_cross_to_contrasts(const msim_moments *moments, uint32_t m, const msim_pair *pairs, const msim_cross *cross,
                             uint32_t n_pairs, uint64_t n_runs, msim_contrast *out);

/* Miner classes: statistics of groups of miners ("the 1 024 small miners as one column", "everyone but the selfish
 * miner", "what if miners 7 and 8 pooled"). (No reference counterpart: the reference prints three means per miner,
 * main.cpp:224-234.) A class map is class_of[k] for k < m: a class index < n_classes, or MSIM_CLASS_NONE for a miner
 * that belongs to no class. 1 <= n_classes <= m; empty classes are allowed, and so is a map that is all NONE. A
 * sweep uses one map for all its points.
 * The fold adds, per run, the records of a class's miners into one msim_run_record per class:
 *   found = sum over class_of[k] == c of found_k,  stale = sum over class_of[k] == c of stale_k
 * as uint32 sums, i.e. modulo 2^32. No record a launch writes can wrap them: a class's found blocks are at most the
 * run's best height, and its stale blocks are fewer than the blocks drawn in the run. The folded records are laid
 * out as a launch's with m = n_classes ([point][run][class]), and the best height stays the run's own, so
 * msim_moments_launch and msim_cross_launch work on them unchanged. A class's terms are therefore share_t and rate_t
 * of msim_moments applied to the CLASS record: the class as one miner, one rounded division of the class's counts.
 * That is not the sum of its members' rounded terms (which differs from it by up to half a unit of 2^-32 per member
 * for the share, and is a different quantity altogether for the stale rate: a sum of ratios, not the ratio of sums). */
#define MSIM_CLASS_NONE 0xFFFFFFFFu
/* Device-resident and asynchronous on `stream`, as msim_moments_launch: no allocation, no synchronisation,
 * independent of any config, capturable. d_per_run: n_points * runs_per_point * m msim_run_record in msim_launch's /
 * msim_sweep_launch's layout; d_class_of: m uint32_t in device memory; d_class_run: n_points * runs_per_point *
 * n_classes msim_run_record, every one of them overwritten (nothing of the buffer is read or accumulated into, so it
 * needs no clearing). An entry of the device map that is neither < n_classes nor MSIM_CLASS_NONE reads as NONE (the
 * launch cannot see device memory; validate on the host with msim_classes_check). MSIM_E_INVALID, with nothing
 * written, for m == 0, no points, more than 65 535 points, no runs, more than 2^32 - 1 runs per point,
 * n_classes == 0, n_classes > m, or a null pointer. */
int msim_fold_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_class_of, uint32_t n_classes, void *d_class_run, void *stream);
/* Host only: MSIM_OK when class_of is not null, 1 <= n_classes <= m and every entry is < n_classes or
 * MSIM_CLASS_NONE, else MSIM_E_INVALID. */
int msim_classes_check(uint32_t m, const uint32_t *class_of, uint32_t n_classes);
/* msim_run_moments / msim_run_contrasts (and the sweep forms) per class: every chunk runs the launch, then
 * msim_fold_launch into a chunk * n_points * n_classes record buffer, then msim_moments_launch (and msim_cross_launch
 * when pairs are given) on the folded records with m = n_classes; chunks are added limb by limb and follow
 * MSIM_MOMENTS_CHUNK_RUNS as those functions do. class_of: m entries, checked with msim_classes_check. out_stats (M,
 * or n_points * M) and opt_sums stay per MINER, as msim_run's. out_class_moments: n_classes (n_points * n_classes)
 * entries; opt_class_hist with opt_hist_spec: n_classes * 2 * (bins + 2) (times n_points) counts, or both NULL.
 * pairs_or_NULL: n_pairs pairs of (point, CLASS) columns, checked with msim_pairs_check(n_classes, ...), with
 * opt_cross: n_pairs entries; or NULL, 0 and NULL. */
int msim_run_classes(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                     const uint32_t *class_of, uint32_t n_classes, const msim_pair *pairs_or_NULL, uint32_t n_pairs,
                     msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_class_moments,
                     const msim_hist_spec *opt_hist_spec, uint64_t *opt_class_hist, msim_cross *opt_cross);
int msim_sweep_run_classes(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                           int device, const uint32_t *class_of, uint32_t n_classes, const msim_pair *pairs_or_NULL,
                           uint32_t n_pairs, msim_stats *out_stats, msim_sums *opt_sums,
                           msim_moments *out_class_moments, const msim_hist_spec *opt_hist_spec,
                           uint64_t *opt_class_hist, msim_cross *opt_cross);

/* Exact quantiles: order statistics of the per-run terms, selected on the device from the records a launch writes
 * on request. (No reference counterpart: the reference prints three means per miner, main.cpp:224-234.) For one run
 * and one column (a miner, or a class after msim_fold_launch) the four quantities are found, stale, share_t and
 * rate_t exactly as defined for msim_moments, each a uint64 key (found and stale zero-extended); quantity index
 * 0 = found, 1 = stale, 2 = share_t, 3 = rate_t. For a 0-based rank r < N over the N runs of a column:
 *   value = the r-th smallest key,  below = #{key < value},  equal = #{key == value}  (below <= r < below + equal).
 * The k-th smallest of a multiset of integers does not depend on how the runs are split into workgroups, chunks,
 * launches or ranks, and the selection works from digit counts that are plain integer sums, so they can be
 * all-reduced. The q-quantile in msim_moments' histogram convention is the k-th smallest with k = max(1, ceil(q N)),
 * i.e. rank k - 1.
 * The method is MSD radix selection: MSIM_RANK_PASSES passes of 8 bits from the top of the key. A pass is one count
 * launch per record buffer, which ADDS to the 256 digit counts of every (point, column, quantity, rank) row the keys
 * that carry the row's prefix, then one step launch, which picks per row the digit whose running total first
 * exceeds what remains of the rank, narrows the row's {prefix, remaining} state and clears the counts. Count and
 * step are separate launches on one stream; the kernel boundary is their only synchronisation. */
#define MSIM_MAX_RANKS 32u
#define MSIM_RANK_PASSES 8u
typedef struct msim_order_stat {
    uint64_t value, below, equal;
} msim_order_stat; /* per [point][column][4][rank] */

/* Host only: the bytes of workspace the launches below need for m columns, n_points points and n_ranks ranks
 * (state of every row plus n_points * m * 4 * n_ranks * 256 uint64 counts); 0 for m == 0, no points, more than
 * 65 535 points or n_ranks outside 1..MSIM_MAX_RANKS. */
size_t msim_rank_workspace_bytes(uint32_t m, uint32_t n_points, uint32_t n_ranks);
/* Host only: where the counts lie inside the workspace, as a byte offset and a number of uint64 words, for an
 * all-reduce (sum) between the count launches and the step launch of a pass when the runs are spread over ranks of
 * a process group. Every rank must have begun with the same m, n_points and ranks. MSIM_E_INVALID as above or for a
 * null pointer. */
int msim_rank_counts_view(uint32_t m, uint32_t n_points, uint32_t n_ranks, size_t *offset, size_t *words);
/* The launches: device-resident and asynchronous on `stream`, as msim_moments_launch: no allocation, no
 * synchronisation, independent of any config. d_ws: ws_bytes >= msim_rank_workspace_bytes(...) of device memory,
 * 256-byte aligned, the same for every launch of one selection. All return MSIM_E_INVALID, with nothing written, for
 * m == 0, no points, more than 65 535 points, no runs, more than 2^32 - 1 runs per point, n_ranks outside
 * 1..MSIM_MAX_RANKS, pass >= MSIM_RANK_PASSES, a workspace that is too small, or a null pointer.
 * begin: clears everything the later launches read (the workspace may hold anything before) and sets every row to
 * {prefix 0, remaining = its rank}. `ranks` is host memory, n_ranks 0-based ranks in any order, duplicates allowed;
 * they are copied into the call's arguments. A rank is not checked against the run count here (the launch does not
 * know it): see msim_ranks_check and the step's status word. */
int msim_rank_begin_launch(uint32_t m, uint32_t n_points, const uint64_t *ranks, uint32_t n_ranks, void *d_ws,
                           size_t ws_bytes, void *stream);
/* count, pass p: d_per_run / d_best_height as msim_moments_launch (n_points * runs_per_point records of m columns).
 * Adds to the counts and never clears them, so several record buffers (chunks of runs, or other ranks through an
 * all-reduce of msim_rank_counts_view) feed one pass. The workspace must be the one begin was given for the same m
 * and n_points; a launch on any other does nothing. Ranks of a row group that still share a prefix have identical
 * counts: only the lowest of them is counted (at pass 0, rank 0 alone) and the step reads its row for all of them.
 * A test switch, MSIM_RANK_TEST_WG_RUNS=<n> (n > 0), read at every count launch: it only lowers the number of runs a
 * workgroup takes (the smaller of the natural value and n), so a few hundred runs give several workgroups along
 * the run axis. */
int msim_rank_count_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                           const void *d_best_height, uint32_t pass, void *d_ws, size_t ws_bytes, void *stream);
/* step, pass p: narrows every row and clears the counts for the next pass. At the last pass (MSIM_RANK_PASSES - 1)
 * d_out_or_NULL is required: n_points * m * 4 * n_ranks msim_order_stat in device memory, [point][column][quantity]
 * [rank in the order given to begin]. d_status: one uint32_t in device memory that the launch ADDS to (clear it
 * before the first pass): a row whose counts do not exceed what remains of its rank (a rank >= N) adds one per
 * pass, keeps its state and writes no msim_order_stat; every other row is unaffected. */
int msim_rank_step_launch(uint32_t m, uint32_t n_points, uint32_t pass, void *d_ws, size_t ws_bytes,
                          void *d_out_or_NULL, void *d_status, void *stream);
/* begin, then MSIM_RANK_PASSES x (count + step) over one record buffer. d_status is added to, as by the step. */
int msim_rank_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_best_height, const uint64_t *ranks, uint32_t n_ranks, void *d_out, void *d_status,
                     void *d_ws, size_t ws_bytes, void *stream);
/* Host only: MSIM_OK when ranks is not null, n_ranks lies in 1..MSIM_MAX_RANKS and every rank is below n_runs, else
 * MSIM_E_INVALID. */
int msim_ranks_check(uint64_t n_runs, const uint64_t *ranks, uint32_t n_ranks);
/* Host conveniences shaped like msim_run_moments / msim_run_classes: out_stats and opt_sums per miner as msim_run's;
 * out_order: [n_points][columns][4][n_ranks] msim_order_stat over all n_runs (runs_per_point) runs, columns = M, or
 * n_classes with a class map (class_of_or_NULL: m entries checked with msim_classes_check; NULL with n_classes 0
 * for per-miner columns). ranks are checked with msim_ranks_check against the total run count. The runs are
 * simulated once, in chunks as msim_run_moments' (they follow MSIM_MOMENTS_CHUNK_RUNS); every chunk's records stay
 * resident in a device buffer of their own until the eight passes are done (with a class map the folded records
 * only; the per-miner chunk buffer is reused), and each pass counts every buffer, then steps once. That costs
 * n_points * n_runs * (8 * columns + 4) bytes of device memory beside one chunk's launch buffers and the
 * selection's workspace; an allocation that fails is MSIM_E_HIP. MSIM_E_CAPACITY on a failed run, as
 * msim_run_moments. */
int msim_run_order_stats(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                         const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                         msim_stats *out_stats, msim_sums *opt_sums, msim_order_stat *out_order);
int msim_sweep_run_order_stats(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point,
                               uint32_t seed_base, int device, const uint32_t *class_of_or_NULL, uint32_t n_classes,
                               const uint64_t *ranks, uint32_t n_ranks, msim_stats *out_stats, msim_sums *opt_sums,
                               msim_order_stat *out_order);

/* Tail statistics: the moments of a column over the runs that lie below, or at, a quantile of a column. (No
 * reference counterpart: the reference prints three means per miner, main.cpp:224-234.) An order statistic says
 * what a bad year looks like as one number; these sums say how bad those years are on average (the expected
 * shortfall), what else happened in them (the same miner's stale rate, every other miner's share), and what the same
 * seeds gave at another point of a sweep. Quantities are indexed as for msim_order_stat: 0 = found, 1 = stale,
 * 2 = share_t, 3 = rate_t; and keys are the uint64 terms of msim_moments.
 * For run r of an item, `key` is the quantity's term of record (cond_point, r, cond_column) with that point's best
 * height. The run belongs to `below` if key < value, to `equal` if key == value, and to neither otherwise. For each
 * set the target column's record (target_point, r, target_column) contributes exactly what it contributes to its
 * msim_moments, with the target point's own best height. The condition and the target may lie at different points
 * of a sweep: a sweep runs every point on the same seeds, so run r is the same draws on both sides.
 * Everything is a plain integer sum in msim_moments' limb convention: identical for any split into workgroups,
 * chunks, launches or ranks, and it can be all-reduced. Unnormalised limbs of a subset never exceed the same limbs
 * over all runs, so the complement sets follow by limb-wise subtraction from the target column's total
 * msim_moments, with nothing recomputed: above = total - below - equal, at least = total - below.
 * `value` is usually the value of an msim_order_stat; then n_below and n_equal reproduce its `below` and `equal`
 * (two independent kernels). Any other threshold is allowed: quantity 0 with value 1 makes `below` the runs without
 * a single block.
 * Ties. The k smallest runs of a column (k = r + 1 for a 0-based rank r, so n_below < k <= n_below + n_equal) are all
 * of `below` plus k - n_below of the ties; which ties is not a property of the data. Every tie is weighted by
 * (k - n_below) / n_equal, the expectation over a uniformly random choice among the ties: deterministic, and
 * independent of any split of the runs. For a first sum S of the target column:
 *   mean_k = (S_below * n_equal + (k - n_below) * S_equal) / (k * n_equal)
 * numerator and denominator formed exactly, then one correctly rounded f64 division. Where the target is the
 * condition's own column and quantity, S_equal = n_equal * value and mean_k is exactly the expected shortfall
 * (S_below + (k - n_below) value) / k. The upper form, the k largest, mirrors it on `above` and `equal`. */
typedef struct msim_tail_item {      /* 32 bytes */
    uint32_t cond_point, cond_column, quantity; /* the column and quantity whose key is compared */
    uint32_t target_point, target_column;       /* the column whose moments are summed */
    uint32_t reserved;                          /* 0 */
    uint64_t value;                             /* the threshold */
} msim_tail_item;
typedef struct msim_tail {           /* 42 uint64 */
    uint64_t n_below, n_equal;       /* #{runs: key < value}, #{runs: key == value} */
    msim_moments below, equal;       /* msim_moments of the TARGET column over those two sets of runs */
} msim_tail;
#define MSIM_MAX_TAIL_ITEMS 8388480u /* 65 535 tiles of 128 items: the grid of one msim_tail_launch */

/* Device-resident and asynchronous on `stream`, as msim_cross_launch: no allocation, no synchronisation,
 * independent of any config, capturable. d_per_run / d_best_height: as msim_moments_launch. d_items: n_items
 * msim_tail_item in device memory, 16-byte aligned. d_tails: n_items msim_tail, overwritten (zeroed inside the
 * launch). An item with a point >= n_points, a column >= m, a quantity >= 4 or reserved != 0 reads nothing and leaves
 * its 42 words zero (the launch cannot see device memory; validate on the host with msim_tail_items_check).
 * MSIM_E_INVALID, with nothing written, for m == 0, no points, no runs, more than 2^32 - 1 runs per point,
 * n_items == 0 or above MSIM_MAX_TAIL_ITEMS, or a null pointer. Item lists are best column-minor (consecutive items
 * on consecutive columns), so that consecutive lanes read consecutive records.
 * A test switch, MSIM_TAIL_TEST_WG_RUNS=<n> (n > 0), read at every launch: it only lowers the number of runs a
 * workgroup takes (the smaller of the natural value and n), so a few hundred runs give several workgroups along
 * the run axis. */
int msim_tail_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_best_height, const void *d_items, uint32_t n_items, void *d_tails, void *stream);
/* Host only: MSIM_OK when there are 1..MSIM_MAX_TAIL_ITEMS items and every one lies within n_points x m with a
 * quantity below 4 and reserved == 0, else MSIM_E_INVALID. */
int msim_tail_items_check(uint32_t m, uint32_t n_points, const msim_tail_item *items, uint32_t n_items);

/* Host only: the chosen set's msim_moments and run count. ABOVE and AT_LEAST need the target column's total moments
 * over the n_runs runs (total_or_NULL); the other two ignore it. MSIM_E_INVALID for a null pointer, an unknown side,
 * counts that exceed n_runs, or a total that some limb of the tail exceeds. `out` is a plain msim_moments, so
 * msim_moments_to_errors(out, 1, *out_n, ...) gives the conditional means with standard errors unchanged. That error
 * is the one of a sample of *out_n runs GIVEN the threshold: it does not include the sampling error of the threshold
 * itself (of the quantile that chose the runs). */
enum { MSIM_TAIL_BELOW, MSIM_TAIL_AT_MOST, MSIM_TAIL_ABOVE, MSIM_TAIL_AT_LEAST };
int msim_tail_side(const msim_tail *t, const msim_moments *total_or_NULL, uint64_t n_runs, int side,
                   msim_moments *out, uint64_t *out_n);
/* Host only: mean_k of found, stale, share (x 2^-32) and rate (x 2^-32) of the target over the k smallest (upper = 0)
 * or k largest (upper = 1, needs the total) runs of the condition, ties weighted as above. MSIM_E_INVALID unless k
 * lies in the tie range (n_strict < k <= n_strict + n_equal, n_strict = n_below or the count above). */
int msim_tail_means(const msim_tail *t, const msim_moments *total_or_NULL, uint64_t n_runs, uint64_t k, int upper,
                    double out[4]);

/* msim_run_order_stats / msim_sweep_run_order_stats plus the tails at the selected order statistics. A spec names a
 * condition (point, column, quantity), which of the `ranks` supplies the threshold (rank_index < n_ranks) and a
 * target (point, column); columns are classes with a class map, as for out_order. The runs are simulated once in
 * chunks whose (folded) records stay resident; every chunk also runs msim_moments_launch, and the chunks' totals are
 * added limb by limb on the host (out_moments: n_points * columns entries). After the eight selection passes the
 * order statistics come to the host, every spec becomes an item whose value is its order statistic's, the items are
 * uploaded once and msim_tail_launch runs on every resident buffer; the chunks' words are added on the host
 * (out_tails: n_specs entries, whose n_below / n_equal equal the order statistic's below / equal). Everything
 * msim_run_order_stats validates is validated, and the specs against (n_points, columns, n_ranks), 1..
 * MSIM_MAX_TAIL_ITEMS of them; MSIM_E_CAPACITY on a failed run. They follow MSIM_MOMENTS_CHUNK_RUNS. */
typedef struct msim_tail_spec {
    uint32_t cond_point, cond_column, quantity, rank_index, target_point, target_column;
} msim_tail_spec;
int msim_run_tails(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                   const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                   const msim_tail_spec *specs, uint32_t n_specs, msim_stats *out_stats, msim_sums *opt_sums,
                   msim_order_stat *out_order, msim_moments *out_moments, msim_tail *out_tails);
int msim_sweep_run_tails(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                         int device, const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks,
                         uint32_t n_ranks, const msim_tail_spec *specs, uint32_t n_specs, msim_stats *out_stats,
                         msim_sums *opt_sums, msim_order_stat *out_order, msim_moments *out_moments,
                         msim_tail *out_tails);

/* Bootstrap: resampled quantiles and expected shortfalls with integer weights, exact on the device. (No reference
 * counterpart.) A Poisson bootstrap gives run r the weight boot_weight(seed, b, r) in replicate b: 1 for b == 0 (the
 * data itself), else with G = 0x9E3779B97F4A7C15 and mix = SplitMix64's output function
 *   c = mix(seed ^ ((uint64)(b >> 1) * G)),  z = mix(c + G * (r + 1)),  u = b odd ? z >> 32 : z & 0xFFFFFFFF,
 *   weight = #{k in 0..12 : u >= T[k]},  T[k] = floor(2^32 * sum_{i<=k} e^-1 / i!)   (csrc/msim_boot.h),
 * Poisson(1) to within 2^-32 per cell and at most 13. r is the ABSOLUTE run index; nothing else enters the weight
 * (not the point, column, chunk, shard or workgroup), so replicates are paired across the points of a sweep and
 * identical for any split of the runs. W_b = sum_r weight is the replicate's size (W_0 = N) and its rank is
 * max(1, ceil(q W_b)) - 1 with q W_b the rounded double product. An item names (point, column, quantity, q_index);
 * per (item, replicate) the row is the order statistic at that rank of the weighted multiset of keys and the
 * weighted sum of the keys below it, in two halves:
 *   below = sum w [key < value],  equal = sum w [key == value],
 *   s_hi = sum w (key >> 32) [key < value],  s_lo = sum w (key & 0xFFFFFFFF) [key < value].
 * The replicate's expected shortfall is (S_below + (k - below) value) / k with k = rank + 1 and
 * S_below = s_hi 2^32 + s_lo (msim_tail's tie convention). A replicate with W_b == 0 has no quantile: its rows are
 * all zero, and equal == 0 marks them. s_hi is exact while 13 * 2^32 * N < 2^64: the drivers refuse
 * N >= MSIM_BOOT_MAX_RUNS runs per point. The selection is msim_rank's, eight passes of weighted digit counts, all
 * plain integer sums: identical for any split and world size, and they can be all-reduced. */
#define MSIM_MAX_BOOT_REPLICATES 4096u /* rows of one item; the ranks of one quantile */
#define MSIM_MAX_BOOT_ITEMS 65535u     /* the grid's z extent of a count launch */
#define MSIM_BOOT_MAX_RUNS (1ull << 28)
#define MSIM_BOOT_EMPTY 0xFFFFFFFFFFFFFFFFull /* the rank that marks an empty replicate in `ranks` */
typedef struct msim_boot_item {
    uint32_t point, column, quantity, q_index;
} msim_boot_item;
typedef struct msim_boot_row {
    uint64_t value, below, equal, s_hi, s_lo;
} msim_boot_row; /* per [item][replicate] */

/* Host only: bytes of workspace for n_items items of B replicates (header, items, three state words per row and
 * n_items * B * 256 uint64 counts); 0 for n_items outside 1..MSIM_MAX_BOOT_ITEMS or B outside
 * 1..MSIM_MAX_BOOT_REPLICATES. msim_boot_counts_view: where the counts lie, as msim_rank_counts_view. */
size_t msim_boot_workspace_bytes(uint32_t n_items, uint32_t replicates);
int msim_boot_counts_view(uint32_t n_items, uint32_t replicates, size_t *offset, size_t *words);
/* Host only: MSIM_OK for 1..MSIM_MAX_BOOT_ITEMS items that all lie within n_points x m, with a quantity below 4 and
 * q_index < n_q (n_q in 1..MSIM_MAX_RANKS), else MSIM_E_INVALID. */
int msim_boot_items_check(uint32_t m, uint32_t n_points, uint32_t n_q, const msim_boot_item *items, uint32_t n_items);
/* Host only: the rank of the q-quantile of a replicate of total weight W: max(1, ceil(q W)) - 1, or MSIM_BOOT_EMPTY
 * for W == 0. q outside [0, 1] (or NaN) also gives MSIM_BOOT_EMPTY. */
uint64_t msim_boot_rank(uint64_t total_weight, double q);
/* The launches are device-resident and asynchronous on `stream` unless said otherwise; all return MSIM_E_INVALID,
 * with nothing written, for a zero count, a count past its cap, more than 2^32 - 1 runs per point, more than
 * 65 535 points, pass >= MSIM_RANK_PASSES, a workspace that is too small, or a null pointer.
 * weights: ADDS the weights of the absolute runs [run_begin, run_begin + runs) to d_W[replicates] (uint64; clear it
 * before the first chunk). It serves chunks and shards: W is a plain sum. */
int msim_boot_weights_launch(uint64_t seed, uint64_t run_begin, uint64_t runs, uint32_t replicates, void *d_W,
                             void *stream);
/* begin: `items` (checked with msim_boot_items_check) and ranks[n_q][replicates] are HOST memory, the ranks computed
 * with msim_boot_rank from the complete W. Copies them into the workspace (which may hold anything before), sets every
 * row to {prefix 0, remaining = its rank}, clears the counts and writes the header; the copy from host memory
 * synchronises the stream once. A rank of MSIM_BOOT_EMPTY makes an empty row. */
int msim_boot_begin_launch(uint32_t m, uint32_t n_points, const msim_boot_item *items, uint32_t n_items,
                           uint32_t replicates, const uint64_t *ranks, uint32_t n_q, void *d_ws, size_t ws_bytes,
                           void *stream);
/* count, pass p: adds to every non-empty row's 256 counts the weights of the keys of [run_begin, run_begin + runs)
 * that carry the row's prefix; never clears them, so several buffers (and an all-reduce) feed one pass. seed and
 * run_begin (the absolute index of the buffer's first run) must be the ones of the weights launches. A workspace
 * that begin did not prepare for the same m, n_points, n_items and replicates makes the launch do nothing.
 * A test switch, MSIM_BOOT_TEST_WG_RUNS=<n> (n > 0), read at every count and below launch, only lowers the number of
 * runs a workgroup takes (at most 2^24, so 13 * 2^24 cannot wrap a 32-bit counter). */
int msim_boot_count_launch(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs_per_point,
                           const void *d_per_run, const void *d_best_height, uint32_t n_items, uint32_t replicates,
                           uint32_t pass, void *d_ws, size_t ws_bytes, void *stream);
/* step, pass p: narrows every row and zeroes its counts. At the last pass d_out_or_NULL is required:
 * n_items * replicates msim_boot_row, whose five words are all written ({value, below, equal, 0, 0}; zeros for an
 * empty row). d_status: one uint32_t the launch adds to for a row whose counts do not reach its rank (a rank that
 * was not computed from W). Does nothing on an unprepared workspace. */
int msim_boot_step_launch(uint32_t n_items, uint32_t replicates, uint32_t pass, void *d_ws, size_t ws_bytes,
                          void *d_out_or_NULL, void *d_status, void *stream);
/* below, after the last step: ADDS to s_hi and s_lo of every non-empty row of d_rows (the step's output) the
 * weighted halves of the buffer's keys below the row's value. Items are read from the workspace. */
int msim_boot_below_launch(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs_per_point,
                           const void *d_per_run, const void *d_best_height, uint32_t n_items, uint32_t replicates,
                           void *d_ws, size_t ws_bytes, void *d_rows, void *stream);
/* msim_run_order_stats / msim_sweep_run_order_stats plus the bootstrap of `items` at the quantiles qs[n_q] (each in
 * [0, 1]) with `replicates` replicates: the same resident chunks and class-map folding; W per chunk from the weights
 * launch; then begin, eight rounds of count-per-buffer and step, and the below pass. `ranks` are the order
 * statistics' as before (for replicate 0 to be compared with, pass the ranks of qs over n_runs). out_W:
 * [replicates]; out_rows: [n_items][replicates]. MSIM_E_INVALID also for n_runs >= MSIM_BOOT_MAX_RUNS. */
int msim_run_bootstrap(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                       const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                       const msim_boot_item *items, uint32_t n_items, const double *qs, uint32_t n_q,
                       uint32_t replicates, uint64_t boot_seed, msim_stats *out_stats, msim_sums *opt_sums,
                       msim_order_stat *out_order, uint64_t *out_W, msim_boot_row *out_rows);
int msim_sweep_run_bootstrap(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                             int device, const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks,
                             uint32_t n_ranks, const msim_boot_item *items, uint32_t n_items, const double *qs,
                             uint32_t n_q, uint32_t replicates, uint64_t boot_seed, msim_stats *out_stats,
                             msim_sums *opt_sums, msim_order_stat *out_order, uint64_t *out_W,
                             msim_boot_row *out_rows);

/* Convert fixed-point sums to MinerStats-style doubles. */
void msim_sums_to_stats(const msim_sums *sums, uint32_t n, msim_stats *out);

const char *msim_strerror(int code);
const char *msim_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSIM_H */

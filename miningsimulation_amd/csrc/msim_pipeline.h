// msim_pipeline.h — the event-skipping pipeline for honest networks.
//
// RunSimulation (/root/reference/main.cpp:128-192) spends almost every event in one state: all
// chains identical and published ("quiet"). From a quiet state, a block i found at T_i by an honest
// miner k whose successor comes later than its arrival (I_{i+1} > prop_k) is adopted by everyone at
// T_i + prop_k and leaves the network quiet again — a "fast" block. Everything else is an EPISODE,
// a pure function of the draws from its first block on (translation-invariant in time apart from the
// end of the run). So one run is computed as
//
//   K1 msim_draws_kernel    (run, segment) workers, jump-ahead to draw j*SEG, draw every block
//                           (interval, finder, fast bit), keep per-segment time and per-owner counts,
//                           and append every non-fast block to a dense episode list together with both
//                           RNG states there; nothing is stored per block (the band where a run can end
//                           keeps per-group sums, counts and the RNG states at each group start);
//   K2 msim_episode_kernel  one lane per listed block: the full state machine (msim_model.h) from a
//                           quiet state at that block, until quiet again or the end of the run;
//   K3 msim_combine_kernel  one lane per run: locate the end of the run (first T_i >= D), chain the
//                           episodes that start from a quiet state, and combine
//                              found_k = #{i < n_end : finder_i = k} + sum(episode deltas)
//                           stale_k = sum(episode stale counts).
// Runs that hit any capacity (draw budget, slots, list) are flagged and recomputed by the per-lane
// retry kernel, so results never depend on these capacities.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "msim_fastdraw.h"
#include "msim_model.h"

namespace msim {

// K2's state machine comes in three sizes (KIND). Lean (0: networks with rho <= K2_LEAN_RHO): 2 extra in-flight
// blocks and no deep-branch counters; at rho <= 0.002 an episode that needs more is < 1e-3 of the runs of a
// 12-month simulation; configs[1] (rho = 1.7e-4): K2 125 -> 77 us per launch (no spills instead of 134 VGPR
// spills; profiles/r04/k2v). Mid (1: every other pipeline network, rho <= PIPE_MAX_RHO): 4 extra blocks, no
// deep branches — a fork deeper than the 16-height window needs 16 finds inside one propagation delay, which
// no network the pipeline takes (delays up to ~50 s) makes in practice, and an episode that would is flagged
// and its run recomputed by the retry kernel. Full (2): deep branches too (kept for A/B builds).
// An episode that outgrows its capacities flags its run for the retry kernel: results never depend on them.
constexpr double K2_LEAN_RHO = 0.002;
#ifndef MSIM_K2_KIND_HI
#define MSIM_K2_KIND_HI 1  // K2 above K2_LEAN_RHO: 1 mid, 2 full (A/B builds)
#endif
constexpr uint32_t K2_KIND_HI = MSIM_K2_KIND_HI;
constexpr uint32_t GROUP = 32;          // blocks per group (end-of-run search metadata)
constexpr uint32_t SGROUP = 8;          // groups per super-group (K3 searches super-group ends, then groups)
constexpr uint32_t MIN_SEG = 512;       // shortest K1 worker (keeps the jump-ahead cost < 5 %)
constexpr uint32_t CNT_WORDS = 8;       // per-owner counters packed as u16 pairs (<= 16 owners)
#ifndef MSIM_K1_QB
#define MSIM_K1_QB 4  // blocks drawn together by K1 (one exactness branch per batch)
#endif
constexpr int K1_QB = MSIM_K1_QB;

constexpr uint32_t EP_HOLE = 0xFFFFFFFFu;  // EpEntry::run of a list slot K1 reserved but did not use

struct EpEntry {
    uint32_t run;     // slice-local run (EP_HOLE: an unused slot of a wave's reserved chunk)
    uint32_t block;   // block index within the run
    uint64_t offset;  // T_block - (start time of its segment), ms
    uint32_t w0, w1;  // (interval << 5 | finder) of the block and of the next one
    uint32_t skip;    // draws from ri / rp's position to the block after w1 (1-4)
    uint32_t pad;
    Rng ri, rp;       // both streams at the start of K1's quad of w1's block: `skip` draws before the block after w1
};

// A group of the band (where a run can end): the first block's word and both streams after it.
struct GroupRec {
    Rng ri, rp;
    uint32_t w0;
    uint32_t pad;
};

struct PipeLayout {
    uint32_t nr;       // runs in a slice (multiple of 256)
    uint32_t seg;      // blocks per K1 worker (multiple of GROUP)
    uint32_t gps;      // groups per segment (seg / GROUP)
    uint32_t nsg;      // super-groups per segment (ceil(gps / SGROUP))
    uint32_t nseg;     // segments (K1 workers) per run
    uint32_t nb;       // nseg * seg pre-generated blocks per run
    uint32_t cap;      // slow-block slots per (run, segment)
    uint32_t band_lo;  // first segment with group metadata (where the run can end)
    uint32_t nband;
    uint32_t lcap;     // episode list capacity
    uint32_t lchunk;   // list slots a K1 wave reserves at a time (one atomic per chunk, not per append)
    uint32_t rec_words;
    uint32_t k2_kind;  // K2's state machine: 0 lean (rho <= K2_LEAN_RHO), 1 mid, 2 full (msim_kernels.hip)
    size_t segsum_off, segcnt_off, nslow_off, slots_off, gsum_off, gend_off, gcum_off, grec_off, list_off, recs_off,
        count_off, total;
};

// Device tables (per config, per device): pick table, log table, jump matrices.
struct PipeTables {
    const PickTab *pick;
    const LogTab *logt;
    const uint32_t *jump;  // nseg * 128 columns of 4 words
    // K1's own tables (msim_fastdraw.h, "K1's form"; built by k1_tables_build in K1's translation unit)
    const PickTab *k1pick;
    const K1Log *k1log;
    uint32_t k1_uni;   // 1: every miner honest with the fast threshold k1_fthr (K1's uniform-delay instantiation)
    uint32_t k1_fthr;
};

struct DrawArgs {
    PipeTables tab;
    uint64_t run_begin;   // absolute index of the slice's first run
    uint32_t n;           // valid runs in the slice
    uint32_t seed_base;
    uint32_t nr, seg, gps, nseg, cap, band_lo, lcap, lchunk;
    uint64_t *segsum;     // [nseg][nr]
    uint32_t *segcnt;     // [nseg][8][nr]
    uint32_t *nslow;      // [nseg][nr]
    uint32_t *slots;      // [nseg][cap][nr]
    uint32_t *gsum;       // [nband][gps][nr]
    uint64_t *gend;       // [nband][nsg][nr]: time from the segment's start to the end of each super-group
    uint32_t *gcum;       // [nband][gps][8][nr]
    GroupRec *grec;       // [nband][gps][nr]
    EpEntry *list;        // [lcap]
    uint32_t *list_count;
};

struct PipeArgs {  // K2 / K3
    uint32_t nr, seg, gps, nseg, nb, cap, band_lo, lcap, rec_words;
    PipeTables tab;       // K2 / K3 redraw blocks from stored RNG states
    const uint64_t *segsum;
    const uint32_t *segcnt;
    const uint32_t *nslow;
    const uint32_t *slots;
    const uint32_t *gsum;
    const uint64_t *gend;
    const uint32_t *gcum;
    const GroupRec *grec;
    const EpEntry *list;
    const uint32_t *list_count;
    uint32_t *recs;       // [lcap][rec_words]: end, flags, F[M], S[M], first block
};

enum : uint32_t { REC_ENDED = 1u, REC_ERR = 2u, REC_SKIP = 4u };

// ---------------------------------------------------------------- sizing (host)
// Every capacity has a >= 8-sigma margin; a run that exceeds one anyway is recomputed by the retry
// kernel, so the sizes only affect speed, never results. rho = P(block is not fast).
// `slots` = wave slots of K1 on the device (CUs x resident waves per CU). The run is cut into `nseg`
// workers of `seg` blocks so that the K1 grid fills the device in whole rounds: every wave does the
// same work, so a partial last round would leave SIMDs idle.

// Test limits (msim.h MSIM_PIPE_TEST_*): capacities a test lowers below their 8-sigma sizes so that a few hundred
// runs reach the overflow branches of K1, S1, K2 and K3. A limit only ever lowers (min with the natural value), and it
// enters here, before the offsets are laid out, so the buffers and every kernel argument agree on it.
struct PipeLimits {
    uint32_t cap = 0, lcap = 0;  // 0: the natural capacity
    int32_t k2_kind = -1;        // 0 lean or 1 mid: K2's state machine whatever rho says; anything else: by rho
};

// Blocks to pre-generate per run (P(more) < 1e-15 per run).
inline double pipe_need(int64_t duration_ms)
{
    const double mu = (double)duration_ms / 599999.5, sd = sqrt(mu > 1.0 ? mu : 1.0);
    return mu + 8.0 * sd + 64.0;
}

// The longest segment a plan may have. K1 packs a segment's per-owner counts as u16 pairs (CNT_WORDS; DevCtx::packed in
// msim_drawgen.hip, `c & 0xFFFFu` / `c >> 16` in combine_run), and one miner can own every block of a segment, so a
// segment holds at most 65 535 blocks: the largest multiple of GROUP below that.
constexpr uint32_t PIPE_MAX_SEG = 0xFFFFu / GROUP * GROUP;
constexpr uint32_t PIPE_MAX_WORKERS = 256;

// Whether PIPE_MAX_WORKERS workers of at most PIPE_MAX_SEG blocks cover a run of this duration (up to ~318 years).
// The pipeline takes no longer run: msim_config_create sends it to the per-lane kernel.
inline bool pipe_fits(int64_t duration_ms)
{
    return ceil(pipe_need(duration_ms) / PIPE_MAX_WORKERS / GROUP) * GROUP <= (double)PIPE_MAX_SEG;
}

// Workers per run for a slice of nr runs on `slots` wave slots: minimise rounds(w) * (seg(w) + jump cost), jump ~ 25
// blocks of work. When that choice makes segments longer than PIPE_MAX_SEG (few wave slots, many runs, long runs: the
// grid is full with few workers), the same minimum over the worker counts whose segments fit; a plan whose segments
// fit is what it always was.
inline uint32_t pipe_workers(int64_t duration_ms, uint32_t nr, uint32_t slots)
{
    const double need = pipe_need(duration_ms);
    const double rows = nr / 64.0;
    if (slots < 1) slots = 1;
    auto seg_of = [&](uint32_t w) { return (uint32_t)ceil(need / w / GROUP) * GROUP; };
    auto best_from = [&](uint32_t w0) {
        uint32_t best_w = w0;
        double best_f = 1e300;
        for (uint32_t w = w0; w <= PIPE_MAX_WORKERS; ++w) {
            const uint32_t sg = seg_of(w);
            if (sg < MIN_SEG && w > w0) break;
            const double rounds = ceil(rows * w / slots);
            const double f = rounds * (sg + 25.0);
            if (f < best_f * 0.999) {
                best_f = f;
                best_w = w;
            }
        }
        return best_w;
    };
    const uint32_t w = best_from(1);
    if (seg_of(w) <= PIPE_MAX_SEG) return w;
    uint32_t w0 = (uint32_t)ceil(need / PIPE_MAX_SEG);  // the fewest workers whose segments fit
    while (w0 < PIPE_MAX_WORKERS && seg_of(w0) > PIPE_MAX_SEG) ++w0;
    return best_from(w0 < PIPE_MAX_WORKERS ? w0 : PIPE_MAX_WORKERS);
}

// The layout of a slice of exactly nr runs (a multiple of 256) cut into nseg workers per run: K2's episode records,
// band records per group.
inline PipeLayout pipe_layout_w(double rho, uint32_t m, int64_t duration_ms, uint32_t nr, uint32_t nseg,
                                const PipeLimits &lim = PipeLimits())
{
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    PipeLayout L;
    const double D = (double)duration_ms;
    const double mu = D / 599999.5, sd = sqrt(mu > 1.0 ? mu : 1.0);
    const double need = pipe_need(duration_ms);
    L.rec_words = 3 + 2 * m;
    L.k2_kind = rho <= K2_LEAN_RHO ? 0u : K2_KIND_HI;
    if (lim.k2_kind == 0 || lim.k2_kind == 1) L.k2_kind = (uint32_t)lim.k2_kind;
    L.nr = nr;
    L.nseg = nseg;
    L.seg = (uint32_t)ceil(need / nseg / GROUP) * GROUP;
    if (L.seg < GROUP) L.seg = GROUP;
    L.gps = L.seg / GROUP;
    L.nsg = (L.gps + SGROUP - 1) / SGROUP;
    L.nb = L.nseg * L.seg;
    const double lo = mu - 8.0 * sd - 64.0;
    L.band_lo = lo > 0 ? (uint32_t)floor(lo / L.seg) : 0u;
    if (L.band_lo >= L.nseg) L.band_lo = L.nseg - 1;
    L.nband = L.nseg - L.band_lo;
    const double lam = rho * L.seg;
    L.cap = (uint32_t)ceil(lam + 8.0 * sqrt(lam) + 8.0);
    if (lim.cap && lim.cap < L.cap) L.cap = lim.cap;
    const double ent = (double)L.nr * rho * L.nb;
    // A K1 wave reserves list slots a chunk at a time: one same-address atomic per chunk instead of one per
    // append (at rho = 1.7 % — configs[0] — the per-append atomics serialised K1 to 30x its draw time). The
    // chunk follows a wave's expected appends; its unused tail (< lchunk slots per wave) is marked EP_HOLE.
    const double per_wave = 64.0 * rho * L.seg;
    L.lchunk = 16;
    while (L.lchunk < 256 && L.lchunk < per_wave / 4.0) L.lchunk *= 2;
    const double holes = (double)(L.nr / 64) * L.nseg * L.lchunk;
    L.lcap = (uint32_t)ceil(ent + 8.0 * sqrt(ent) + 1024.0 + holes);
    if (lim.lcap && lim.lcap < L.lcap) L.lcap = lim.lcap;
    size_t o = 0;
    L.segsum_off = o;
    o = al(o + (size_t)L.nseg * L.nr * 8);
    L.segcnt_off = o;
    o = al(o + (size_t)L.nseg * CNT_WORDS * L.nr * 4);
    L.nslow_off = o;
    o = al(o + (size_t)L.nseg * L.nr * 4);
    L.slots_off = o;
    o = al(o + (size_t)L.nseg * L.cap * L.nr * 4);
    const size_t grp = L.gps;  // band records per segment
    L.gsum_off = o;
    o = al(o + (size_t)L.nband * L.gps * L.nr * 4);
    L.gend_off = o;
    o = al(o + (size_t)L.nband * L.nsg * L.nr * 8);
    L.gcum_off = o;
    o = al(o + (size_t)L.nband * grp * CNT_WORDS * L.nr * 4);
    L.grec_off = o;
    o = al(o + (size_t)L.nband * grp * L.nr * sizeof(GroupRec));
    L.list_off = o;
    o = al(o + (size_t)L.lcap * sizeof(EpEntry));
    L.recs_off = o;
    o = al(o + (size_t)L.lcap * L.rec_words * 4);
    L.count_off = o;
    o = al(o + 4);
    L.total = o;
    return L;
}

// The same with the workers per run chosen for `slots` wave slots (pipe_workers).
inline PipeLayout pipe_layout_nr(double rho, uint32_t m, int64_t duration_ms, uint32_t nr, uint32_t slots,
                                 const PipeLimits &lim = PipeLimits())
{
    return pipe_layout_w(rho, m, duration_ms, nr, pipe_workers(duration_ms, nr, slots), lim);
}

// The layout of the largest slice, `nr` runs (a multiple of 256) or fewer, whose `total` bytes fit the budget. A layout's
// geometry depends on its slice size, so it shrinks in steps: by the excess and 2 % more, to whole 256s, at least 256
// at a time, not below 256. layout_at(nr) is computed once per step and the last one is returned.
template <class LayoutAt>
inline auto fit_slice(uint64_t nr, double budget, LayoutAt layout_at) -> decltype(layout_at(0u))
{
    for (;;) {
        const auto L = layout_at((uint32_t)nr);
        if ((double)L.total <= budget || nr <= 256) return L;
        uint64_t next = (uint64_t)((double)nr * budget / (double)L.total * 0.98) / 256 * 256;
        if (next >= nr) next = nr - 256;
        nr = next < 256 ? 256 : next;
    }
}

// The largest slice (all n_runs, or fewer) whose layout fits the budget.
inline PipeLayout pipe_layout_for(double rho, uint32_t m, int64_t duration_ms, uint64_t n_runs, double budget,
                                  uint32_t slots, const PipeLimits &lim = PipeLimits())
{
    return fit_slice((n_runs + 255) / 256 * 256, budget,
                     [&](uint32_t nr) { return pipe_layout_nr(rho, m, duration_ms, nr, slots, lim); });
}

// The launch arguments a layout determines, for a slice region at `ws`: every field but run_begin, n and seed_base,
// which the caller sets per slice and launch.
inline DrawArgs draw_args(const PipeLayout &L, char *ws, const PipeTables &tab)
{
    DrawArgs a = {};
    a.tab = tab;
    a.nr = L.nr;
    a.seg = L.seg;
    a.gps = L.gps;
    a.nseg = L.nseg;
    a.cap = L.cap;
    a.band_lo = L.band_lo;
    a.lcap = L.lcap;
    a.lchunk = L.lchunk;
    a.segsum = (uint64_t *)(ws + L.segsum_off);
    a.segcnt = (uint32_t *)(ws + L.segcnt_off);
    a.nslow = (uint32_t *)(ws + L.nslow_off);
    a.slots = (uint32_t *)(ws + L.slots_off);
    a.gsum = (uint32_t *)(ws + L.gsum_off);
    a.gend = (uint64_t *)(ws + L.gend_off);
    a.gcum = (uint32_t *)(ws + L.gcum_off);
    a.grec = (GroupRec *)(ws + L.grec_off);
    a.list = (EpEntry *)(ws + L.list_off);
    a.list_count = (uint32_t *)(ws + L.count_off);
    return a;
}

inline PipeArgs pipe_args(const PipeLayout &L, char *ws, const PipeTables &tab)
{
    const DrawArgs d = draw_args(L, ws, tab);  // K2 and K3 read what K1 wrote
    PipeArgs a = {};
    a.nr = L.nr;
    a.seg = L.seg;
    a.gps = L.gps;
    a.nseg = L.nseg;
    a.nb = L.nb;
    a.cap = L.cap;
    a.band_lo = L.band_lo;
    a.lcap = L.lcap;
    a.rec_words = L.rec_words;
    a.tab = tab;
    a.segsum = d.segsum;
    a.segcnt = d.segcnt;
    a.nslow = d.nslow;
    a.slots = d.slots;
    a.gsum = d.gsum;
    a.gend = d.gend;
    a.gcum = d.gcum;
    a.grec = d.grec;
    a.list = d.list;
    a.list_count = d.list_count;
    a.recs = (uint32_t *)(ws + L.recs_off);
    return a;
}

// ---------------------------------------------------------------- K1 lane body (shared host/device)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __noinline__ int32_t interval_ms_exact_dev(uint64_t u);
#endif

MSIM_HD uint32_t draw_interval(Rng &ri, const LogTab *__restrict__ lt, FdConsts kc = MSIM_FD_DEFAULT)
{
    const uint64_t u = rng_next(ri);
    bool ok;
    const int32_t q = interval_ms_fast(u, lt, ok, kc);
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(ok ? q : interval_ms_exact_dev(u));
#else
    return (uint32_t)(ok ? q : (int32_t)interval_ms_of(u));
#endif
}

// Both draws of one block as a word: interval << 5 | finder (pick_info's low nibble).
MSIM_HD uint32_t draw_word(Rng &ri, Rng &rp, const LogTab *__restrict__ lt, const PickTab *__restrict__ pt)
{
    const uint32_t I = draw_interval(ri, lt);
    return (I << 5) | info_finder(pick_info(rng_next(rp), pt));
}

// Episode draw source (K2): the stored words of its first two blocks, then the streams redrawn.
struct EpSrc {
    const LogTab *lt;
    const PickTab *pt;
    Rng ri, rp;
    uint32_t nb, index, cur, nxt;
    bool have_nxt;
    MSIM_HD uint32_t word() const { return cur; }
    MSIM_HD bool advance()
    {
        if (index + 1 >= nb) return false;  // past the pre-generated budget: the run is retried
        ++index;
        if (have_nxt) {
            cur = nxt;
            have_nxt = false;
        } else {
            cur = draw_word(ri, rp, lt, pt);
        }
        return true;
    }
};

// The draws of four consecutive blocks, each by its fast path, with their exactness checks folded into
// one flag; the rare quad that needs an exact path (an interval within 1 ns of a millisecond boundary,
// or a PickFinder index the high word cannot settle: ~8e-6 of quads) is redrawn by draw_quad_exact from
// the streams at its start. Batching four draws lets their table reads be in flight together.
MSIM_HD bool draw_quad_fast(Rng &ri, Rng &rp, const LogTab *__restrict__ lt, const PickTab *__restrict__ pt,
                            FdConsts kc, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB])
{
    uint32_t ki = 0, kp = 0;  // largest acceptance keys of the quad
#pragma unroll
    for (int q = 0; q < K1_QB; ++q) {
        const uint64_t ui = rng_next(ri), up = rng_next(rp);
        uint32_t a, b;
        I[q] = (uint32_t)interval_ms_fast_key(ui, lt, a, kc);
        info[q] = pt->info[pick_q_fast_key(up, b)];
        ki = a > ki ? a : ki;
        kp = b > kp ? b : kp;
    }
    return ki >= FD_OK_RANGE || kp >= PICK_RARE_LO;
}
MSIM_HD void draw_quad_exact(Rng ri, Rng rp, const LogTab *__restrict__ lt, const PickTab *__restrict__ pt,
                             uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB])
{
#pragma unroll
    for (int q = 0; q < K1_QB; ++q) {
        I[q] = draw_interval(ri, lt);  // the exact glibc sequence stays out of line (interval_ms_exact_dev)
        info[q] = pt->info[pick_q_exact(rng_next(rp))];
    }
}

// K1's own forms of the same draws (msim_fastdraw.h, "K1's form" and "the packed form"): any 64-bit draw still gets
// the reference's interval and finder. Of K1Log the lane body reads the packed table P (the quad) and, for the
// redraw by the general form, invc and row e = 0 of A2 (A0): K1 keeps only those in LDS.
MSIM_HD uint32_t k1_draw_interval(Rng &ri, const double *__restrict__ invc, const double *__restrict__ A0, FdConsts kc)
{
    const uint64_t u = rng_next(ri);
    bool ok;
    const int32_t q = k1_interval_general_on(u, invc, A0, ok, kc);
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(ok ? q : interval_ms_exact_dev(u));
#else
    return (uint32_t)(ok ? q : (int32_t)interval_ms_of(u));
#endif
}
// As draw_quad_fast, on the packed form and the high-word picker by one multiply with 400 (msim_fastdraw.h
// pick_off400_key), both streams stepped with the one-instruction s1 << 21 (msim_draws.h rng_next<true>). The
// exponent limit of the folded table is checked once per quad: the smallest high word of the four v's against
// K1P_VH_MIN.
MSIM_HD bool k1p_quad_fast(Rng &ri, Rng &rp, const K1Pair *__restrict__ P, const PickTab *__restrict__ kp, FdConsts kc,
                           uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB])
{
    uint32_t ki = 0, kk = 0, vmin = 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q < K1_QB; ++q) {
        const uint64_t ui = rng_next<true>(ri);
        const uint32_t hp = rng_next_hi<true>(rp);
        uint32_t a, b, vh;
        I[q] = (uint32_t)k1p_interval_key(ui, P, a, vh, kc);
        info[q] = *(const uint32_t *)((const char *)kp->info + pick_off400_key(hp, b));
        ki = a > ki ? a : ki;
        kk = b > kk ? b : kk;
        vmin = vh < vmin ? vh : vmin;
    }
    return ki >= K1P_OK_HI || kk >= PICK400_RARE_LO || vmin < K1P_VH_MIN;
}
// The redraw of a flagged quad: every interval by the general form first (3e-5 of draws only left the folded
// table's exponent range), glibc's sequence for the one within the margin of a millisecond boundary; every pick
// exactly, on the full draw.
MSIM_HD void k1_quad_exact(Rng ri, Rng rp, const double *__restrict__ invc, const double *__restrict__ A0,
                           const PickTab *__restrict__ kp, FdConsts kc, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB])
{
#pragma unroll
    for (int q = 0; q < K1_QB; ++q) {
        I[q] = k1_draw_interval(ri, invc, A0, kc);
        info[q] = kp->info[pick_q_exact(rng_next(rp))];
    }
}

// The draw forms behind draw_segment_with: the first block's draws, a quad of fast draws with its exactness
// flag, the quad's exact redraw, a block's fast bit and the counter row count() is called with.
// GeneralDraws: the general tables (what K2 and K3 redraw with; the host checks run the lane body on it).
struct GeneralDraws {
    const LogTab *lt;
    const PickTab *pt;
    FdConsts kc;
    MSIM_HD void begin() { kc = fd_consts(); }
    MSIM_HD uint32_t interval(Rng &ri) const { return draw_interval(ri, lt, kc); }
    MSIM_HD uint32_t pick(Rng &rp) const { return pick_info(rng_next(rp), pt); }
    MSIM_HD bool quad_fast(Rng &ri, Rng &rp, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB]) const
    {
        return draw_quad_fast(ri, rp, lt, pt, kc, I, info);
    }
    MSIM_HD void quad_exact(const Rng &ri, const Rng &rp, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB]) const
    {
        draw_quad_exact(ri, rp, lt, pt, I, info);
    }
    MSIM_HD bool slow(uint32_t next, uint32_t info) const { return next <= info_fthr(info); }
    MSIM_HD uint32_t row(uint32_t info) const { return info; }
};
// K1Draws: K1's tables. UNI (k1_uniform_fthr): one scalar fast threshold, and the pick entry IS the row offset.
template <bool UNI>
struct K1Draws {
    const K1Pair *P;                // K1Log's packed table
    const double *invc, *A0;        // K1Log's invc and row e = 0 of A2 (the general-form redraw)
    const PickTab *kp;  // build_k1_pick(uni = UNI)
    uint32_t fthr;      // UNI: every finder's fast threshold
    FdConsts kc;
    MSIM_HD void begin()
    {
        kc = MSIM_K1_CONSTS;
#if defined(__HIP_DEVICE_COMPILE__)
        // every addend in an SGPR; the leading coefficient, a multiplicand beside the SGPR addend (one VOP3 reads
        // at most one SGPR), in a VGPR pair held across the loop: at 4 waves per SIMD the budget has room for it
        asm("" : "+s"(kc.c1));
        asm("" : "+s"(kc.c2));
        asm("" : "+s"(kc.c3));
#if !MSIM_FD_DEG4
        asm("" : "+s"(kc.c4));
#endif
        asm volatile("" : "+v"(kc.MSIM_K1_LEAD));
#endif
    }
    MSIM_HD uint32_t interval(Rng &ri) const { return k1_draw_interval(ri, invc, A0, kc); }
    MSIM_HD uint32_t pick(Rng &rp) const { return kp->info[pick_q_exact(rng_next(rp))]; }
    MSIM_HD bool quad_fast(Rng &ri, Rng &rp, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB]) const
    {
        return k1p_quad_fast(ri, rp, P, kp, kc, I, info);
    }
    MSIM_HD void quad_exact(const Rng &ri, const Rng &rp, uint32_t (&I)[K1_QB], uint32_t (&info)[K1_QB]) const
    {
        k1_quad_exact(ri, rp, invc, A0, kp, kc, I, info);
    }
    MSIM_HD bool slow(uint32_t next, uint32_t info) const { return next <= (UNI ? fthr : info_fthr(info)); }
    MSIM_HD uint32_t row(uint32_t info) const { return UNI ? info : info & (15u << INFO_K_SHIFT); }
};

// One (run, segment) worker: SEG blocks from the jumped RNG states. `d` is the draw form (above). Ctx supplies
// the side effects:
//   count(row)                        per-owner counter of this lane (+1 for owner info_finder(row); row = d.row(info))
//   vote(s)                           nonzero when s holds for some active lane of the wave (host: s)
//   slow(s, block, offset, w0, w1, ri, rp, skip)
//                                     called after a nonzero vote: records a non-fast block when s
//                                     (offset = its find time minus the segment's start; its word, the
//                                     next one; both streams at the quad's start, `skip` draws before the
//                                     block after the next one: the consumer steps them, not the wave)
//   group(g, sum, end)                band only: sum of the group's intervals, and the time from the segment's
//                                     start to the group's end
//   group_start(g, w0, ri, rp)        band only: before group g's first block (its word and the streams
//                                     after it; snapshot the counters)
// Blocks are drawn four at a time (draw_quad_fast); the streams after a block inside a quad, needed only
// by the rare non-fast block, are re-stepped from the quad's start. Time is summed per group in 32 bits
// (32 intervals < 2^25 ms each) and folded into 64 bits per group.
template <class Ctx, class Draws>
MSIM_HD uint64_t draw_segment_with(Ctx &cx, Draws &d, Rng &ri, Rng &rp, uint32_t b0, uint32_t seg, bool band)
{
    d.begin();
    uint32_t Icur = d.interval(ri);
    uint32_t infocur = d.pick(rp);
    uint64_t tsum = 0;
    for (uint32_t g = 0; g < seg / GROUP; ++g) {
        if (band) cx.group_start(g, (Icur << 5) | info_finder(infocur), ri, rp);
        uint32_t gacc = 0;
        for (uint32_t q4 = 0; q4 < GROUP / K1_QB; ++q4) {
            uint32_t I[K1_QB], info[K1_QB];
            // The quad's start states are read only on the two rare paths below; at a register budget of 96 VGPRs
            // or fewer (5 or more waves per SIMD, msim_drawgen.hip) the compiler keeps them in scratch, written
            // once per quad; at the shipped 4 waves they stay in registers. Measured on MI355X: recovering them by
            // inverse stepping instead (no scratch, 84 VGPRs) made K1 11 % slower at the same occupancy
            // (profiles/r03/INDEX.md, k1 A/B).
            const Rng ri0 = ri, rp0 = rp;
            if (d.quad_fast(ri, rp, I, info)) d.quad_exact(ri0, rp0, I, info);
#pragma unroll
            for (int q = 0; q < K1_QB; ++q) {
                gacc += Icur;
                const bool slow = d.slow(I[q], infocur);  // I_{i+1} vs the finder's delay
                cx.count(d.row(infocur));
                if (cx.vote(slow))  // the streams after block i+1 are the quad's start + q + 1 draws (K2 steps them)
                    cx.slow(slow, b0 + g * GROUP + q4 * K1_QB + (uint32_t)q, tsum + gacc, (Icur << 5) | info_finder(infocur),
                            (I[q] << 5) | info_finder(info[q]), ri0, rp0, (uint32_t)q + 1u);
                Icur = I[q];
                infocur = info[q];
            }
        }
        if (band) cx.group(g, gacc, tsum + gacc);
        tsum += gacc;
    }
    return tsum;
}
// The lane body on the general tables.
template <class Ctx>
MSIM_HD uint64_t draw_segment(Ctx &cx, Rng &ri, Rng &rp, const LogTab *__restrict__ lt,
                              const PickTab *__restrict__ pt, uint32_t b0, uint32_t seg, bool band)
{
    GeneralDraws d{lt, pt, MSIM_FD_DEFAULT};
    return draw_segment_with(cx, d, ri, rp, b0, seg, band);
}
// The lane body as K1 runs it (msim_drawgen.hip): K1's tables, uniform-delay form when uni.
template <bool UNI, class Ctx>
MSIM_HD uint64_t draw_segment_k1(Ctx &cx, Rng &ri, Rng &rp, const K1Log *__restrict__ kl,
                                 const PickTab *__restrict__ kp, uint32_t fthr, uint32_t b0, uint32_t seg, bool band)
{
    K1Draws<UNI> d{kl->P, kl->invc, kl->A2 + (K1_EROWS - 1) * LOG_TAB, kp, fthr, MSIM_K1_CONSTS};
    return draw_segment_with(cx, d, ri, rp, b0, seg, band);
}
// The same on the three arrays of K1Log the lane body reads (K1 holds only these in LDS).
template <bool UNI, class Ctx>
MSIM_HD uint64_t draw_segment_k1_on(Ctx &cx, Rng &ri, Rng &rp, const K1Pair *__restrict__ P, const double *__restrict__ invc,
                                    const double *__restrict__ A0, const PickTab *__restrict__ kp, uint32_t fthr, uint32_t b0,
                                    uint32_t seg, bool band)
{
    K1Draws<UNI> d{P, invc, A0, kp, fthr, MSIM_K1_CONSTS};
    return draw_segment_with(cx, d, ri, rp, b0, seg, band);
}

// ---------------------------------------------------------------- K3 lane body (shared host/device)
// Adds the M owner counters of a packed row; returns PickFinder's fall-through count (owner 15).
template <int M>
MSIM_HD uint32_t add_packed(uint32_t (&F)[M], const uint32_t *__restrict__ src, size_t stride)
{
#pragma unroll
    for (int w = 0; w < (M + 1) / 2; ++w) {
        const uint32_t c = src[(size_t)w * stride];
        F[2 * w] += c & 0xFFFFu;
        if (2 * w + 1 < M) F[2 * w + 1] += c >> 16;
    }
    return src[(size_t)(CNT_WORDS - 1) * stride] >> 16;
}

// K3 phase timing (diagnostic builds only, -DK3_PROF=1: scripts/build_variant.sh): clock at each phase of
// combine_run for the first lane of a few workgroups.
#if defined(__HIP_DEVICE_COMPILE__) && defined(K3_PROF) && K3_PROF
#define K3T(i) k3t[i] = clock64()
#define K3T_DECL uint64_t k3t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; K3T(0)
#define K3T_PRINT                                                                                               \
    if (threadIdx.x == 0 && blockIdx.x % 16 == 0)                                                               \
        printf("K3PROF blk %u seg %llu cnt %llu idxhdr %llu groups %llu chain %llu redraw %llu prevgrp %llu eps %llu\n", \
               blockIdx.x, (unsigned long long)(k3t[1] - k3t[0]), (unsigned long long)(k3t[2] - k3t[1]),       \
               (unsigned long long)(k3t[3] - k3t[2]), (unsigned long long)(k3t[4] - k3t[3]),                    \
               (unsigned long long)(k3t[5] - k3t[4]), (unsigned long long)(k3t[6] - k3t[5]),                    \
               (unsigned long long)(k3t[7] - k3t[6]), (unsigned long long)(k3t[8] - k3t[7]))
#else
#define K3T(i)
#define K3T_DECL
#define K3T_PRINT
#endif

// Combine one run r of a slice. Returns false when the run must be recomputed by the retry path.
// nsw: K3_SCRATCH words of per-run scratch at stride nss (device: the lane's LDS column): the list counts of
// the run's segments (later the first blocks of the candidate episodes), the candidates' record indices, and
// their (end << 2 | ended << 1 | unusable) words.
//
// K3 is latency-bound (one lane per run, a fraction of a wave per SIMD): its time is set by its dependent
// memory rounds and by single-wave instruction latency. The reads are ordered so that independent ones share a
// round and the episode reads stay in flight behind the end-of-run search: (1) segment sums; (2) list counts +
// per-owner counts; (3) slot indices; (4) episode headers + super-group ends; (5) group sums; (6) the end
// group's records + the first candidates' deltas, which land while the end group is redrawn. The episode
// chain is built from the headers without the end block (the episodes are in block order, so the end only
// truncates it) and cut once the redraw found it.
#ifndef MSIM_K3_EP_MAX
#define MSIM_K3_EP_MAX 32  // 24: 76.8 us, 16: 99.1 us vs 67.7 us per c2 launch (more runs on the one-read-at-a-time path)
#endif
constexpr uint32_t K3_SEG_MAX = 32, K3_EP_MAX = MSIM_K3_EP_MAX, K3_SCRATCH = K3_SEG_MAX + 2 * K3_EP_MAX;
// combine_run keeps its candidate starts in the segment-count rows (nsw[na * nss], na < K3_EP_MAX): a larger
// K3_EP_MAX would overwrite the record indices at rows K3_SEG_MAX + t before they are read
static_assert(K3_EP_MAX <= K3_SEG_MAX, "MSIM_K3_EP_MAX must not exceed K3_SEG_MAX");
template <int M>
MSIM_HD bool combine_run(const SimParams &p, const PipeArgs &a, uint32_t r, uint32_t (&F)[M], uint32_t (&S)[M],
                         uint32_t *nsw, size_t nss)
{
    const int64_t D = p.duration_ms;
    K3T_DECL;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        F[k] = 0;
        S[k] = 0;
    }
    // 1. Segment containing the end of the run: the first whose last block is found at >= D. The sums are
    // loaded KB at a time (independent loads in flight together), then scanned.
    constexpr uint32_t KB = 16;
    int64_t T = 0;
    int e = -1;
    for (uint32_t j0 = 0; j0 < a.nseg && e < 0; j0 += KB) {
        uint64_t ss[KB];
#pragma unroll
        for (uint32_t j = 0; j < KB; ++j) {  // unconditional (clamped) loads: all KB in flight together
            const uint32_t jj = j0 + j < a.nseg ? j0 + j : a.nseg - 1;
            ss[j] = a.segsum[(size_t)jj * a.nr + r];
        }
#pragma unroll
        for (uint32_t j = 0; j < KB; ++j) {
            if (e < 0 && j0 + j < a.nseg) {
                if (T + (int64_t)ss[j] >= D) e = (int)(j0 + j);
                else T += (int64_t)ss[j];
            }
        }
    }
    K3T(1);
    if (e < (int)a.band_lo) return false;  // past the pre-generated draws or outside the band
    constexpr uint32_t EP_MAX = K3_EP_MAX, SEG_MAX = K3_SEG_MAX;
    const bool fits = (uint32_t)e < SEG_MAX;
    // 2. List counts of segments 0..e (issued first) and per-owner counts of the segments before e, in one
    // round (no early exit between them: a fall-through in any segment is checked once at the end).
    uint32_t nsv[SEG_MAX];
    if (fits) {
#pragma unroll
        for (uint32_t j = 0; j < SEG_MAX; ++j) nsv[j] = a.nslow[(size_t)(j <= (uint32_t)e ? j : (uint32_t)e) * a.nr + r];
    }
    {
        uint32_t ft = 0;
        for (int j0 = 0; j0 < e; j0 += (int)KB) {
            uint32_t c[KB][CNT_WORDS];
#pragma unroll
            for (uint32_t j = 0; j < KB; ++j) {
                const int jj = j0 + (int)j < e ? j0 + (int)j : e - 1;  // clamped: unconditional loads, masked below
#pragma unroll
                for (uint32_t w = 0; w < CNT_WORDS; ++w) {
                    const uint32_t v = (w < (uint32_t)(M + 1) / 2 || w == CNT_WORDS - 1)
                                           ? a.segcnt[((size_t)jj * CNT_WORDS + w) * a.nr + r]
                                           : 0u;
                    c[j][w] = j0 + (int)j < e ? v : 0u;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < KB; ++j) {
#pragma unroll
                for (int w = 0; w < (M + 1) / 2; ++w) {
                    F[2 * w] += c[j][w] & 0xFFFFu;
                    if (2 * w + 1 < M) F[2 * w + 1] += c[j][w] >> 16;
                }
                ft |= c[j][CNT_WORDS - 1] >> 16;
            }
        }
        if (ft) return false;  // PickFinder fell through (owner 15): the retry kernel reports it
    }
    uint32_t tot = 0;
    if (fits) {
#pragma unroll
        for (uint32_t j = 0; j < SEG_MAX; ++j) {
            const uint32_t v = j <= (uint32_t)e ? nsv[j] : 0u;
            if (v > a.cap) return false;
            tot += v;
            nsw[j * nss] = v;  // read back below at data-dependent positions
        }
    }
    K3T(2);
    // 3. The run's episodes in block order (segments 0..e): record indices, then headers. The header loads
    // are not waited for here: they stay in flight through the group search.
    const bool batched = fits && tot <= EP_MAX;
    uint32_t st[EP_MAX], en[EP_MAX], fl[EP_MAX];
    bool bad_idx = false;
    if (batched) {
        // entry t -> (segment, slot): a walk over the counts in LDS, no memory reads; then every slot index and
        // every header is loaded without a branch (entries past tot read slot 0 / record 0 and are masked), so
        // no load waits behind a divergent block for the ones issued before it
        uint32_t pos[EP_MAX];
        {
            uint32_t j = 0, c = 0, nj = nsw[0];  // (segment, slot) of entry t; nj = count of segment j
#pragma unroll
            for (uint32_t t = 0; t < EP_MAX; ++t) {
                uint32_t v = 0;
                if (t < tot) {
                    while (c >= nj) {
                        ++j;
                        c = 0;
                        nj = nsw[j * nss];
                    }
                    v = j * a.cap + c;
                    ++c;
                }
                pos[t] = v;
            }
        }
        uint32_t idx[EP_MAX];
#pragma unroll
        for (uint32_t t = 0; t < EP_MAX; ++t) idx[t] = a.slots[(size_t)pos[t] * a.nr + r];
#pragma unroll
        for (uint32_t t = 0; t < EP_MAX; ++t) {
            const bool in = t < tot;
            bad_idx |= in && idx[t] >= a.lcap;
            const uint32_t i = in && idx[t] < a.lcap ? idx[t] : 0u;
            const uint32_t *rec = a.recs + (size_t)i * a.rec_words;
            st[t] = rec[2 + 2 * M];  // the episode's first block (K2 copies it from the list entry)
            en[t] = rec[0];
            fl[t] = rec[1];
            nsw[(SEG_MAX + t) * nss] = i;
        }
    }
    K3T(3);
    // 4. Group, then block, where T first reaches D: n_end = #{i : T_i < D} (main.cpp:150,153). Two rounds: the
    // ends of the segment's super-groups (time from the segment's start, KS at a time), then the SGROUP group
    // sums of the super-group that reaches D.
    const size_t gb = (size_t)(e - (int)a.band_lo) * a.gps;
    const uint32_t nsg = (a.gps + SGROUP - 1) / SGROUP;
    const size_t sb = (size_t)(e - (int)a.band_lo) * nsg;
    constexpr uint32_t KS = 24;
    uint32_t sg = nsg;
    uint64_t base = 0;  // time from the segment's start to the start of super-group sg
    for (uint32_t s0 = 0; s0 < nsg && sg == nsg; s0 += KS) {
        uint64_t ps[KS];
#pragma unroll
        for (uint32_t j = 0; j < KS; ++j) ps[j] = a.gend[(sb + (s0 + j < nsg ? s0 + j : nsg - 1)) * a.nr + r];
#pragma unroll
        for (uint32_t j = 0; j < KS; ++j) {
            if (sg == nsg && s0 + j < nsg) {
                if (T + (int64_t)ps[j] >= D) sg = s0 + j;
                else base = ps[j];
            }
        }
    }
    if (sg == nsg) return false;
    T += (int64_t)base;
    uint32_t G = a.gps;
    {
        const uint32_t g0 = sg * SGROUP;
        uint32_t gs[SGROUP];
#pragma unroll
        for (uint32_t g = 0; g < SGROUP; ++g) gs[g] = a.gsum[(gb + (g0 + g < a.gps ? g0 + g : a.gps - 1)) * a.nr + r];
#pragma unroll
        for (uint32_t g = 0; g < SGROUP; ++g) {
            if (G == a.gps && g0 + g < a.gps) {
                if (T + (int64_t)gs[g] >= D) G = g0 + g;
                else T += (int64_t)gs[g];
            }
        }
    }
    if (G == a.gps || bad_idx) return false;
    K3T(4);
    // 5. The end group's stream record and counters are issued, then the candidate chain is built from the
    // headers (an episode is a candidate when its first block is reached quiet, ignoring the end of the run),
    // then the first APPLY_B candidates' deltas are issued; the group redraw waits for the stream record only.
    const GroupRec gr = a.grec[(gb + G) * a.nr + r];
    uint32_t gc[CNT_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < CNT_WORDS; ++w)
        gc[w] = (w < (uint32_t)(M + 1) / 2 || w == CNT_WORDS - 1) ? a.gcum[((gb + G) * CNT_WORDS + w) * a.nr + r] : 0u;
    constexpr uint32_t APPLY_B = 8;
    uint32_t na = 0;
    uint32_t d[APPLY_B][2 * M];
    if (batched) {
        uint32_t cursor = 0;
        bool stop = false;
#pragma unroll
        for (uint32_t t = 0; t < EP_MAX; ++t) {
            if (stop || t >= tot || st[t] < cursor) continue;  // consumed by the previous candidate
            const bool ended = (fl[t] & REC_ENDED) != 0u;
            nsw[na * nss] = st[t];
            nsw[(SEG_MAX + na) * nss] = nsw[(SEG_MAX + t) * nss];  // na <= t: compacts in place
            nsw[(SEG_MAX + EP_MAX + na) * nss] =
                (en[t] << 2) | (ended ? 2u : 0u) | ((fl[t] & (REC_ERR | REC_SKIP)) ? 1u : 0u);
            ++na;
            cursor = en[t];
            stop = ended;  // the run ended inside this episode
        }
        if (na) {
#pragma unroll
            for (uint32_t b = 0; b < APPLY_B; ++b) {
                const uint32_t t = b < na ? b : na - 1;  // clamped: unconditional loads, masked below
                const uint32_t *rec = a.recs + (size_t)nsw[(SEG_MAX + t) * nss] * a.rec_words;
#pragma unroll
                for (int k = 0; k < 2 * M; ++k) d[b][k] = rec[2 + k];
            }
        }
    }
    K3T(5);
#pragma unroll
    for (int w = 0; w < (M + 1) / 2; ++w) {
        F[2 * w] += gc[w] & 0xFFFFu;
        if (2 * w + 1 < M) F[2 * w + 1] += gc[w] >> 16;
    }
    if (gc[CNT_WORDS - 1] >> 16) return false;
    const uint32_t bg = (uint32_t)e * a.seg + G * GROUP;
    uint32_t n_end = 0, klast = 15u;
    int64_t t_last = 0;
    bool done = false;
    {  // redraw the group from its first block's stored streams, four blocks at a time as K1 drew them
       // (draw_quad_fast, the exact form for a flagged quad): the four draws' table reads and interval
       // polynomials are independent, so they overlap instead of forming one chain of 31 draws
        Rng ri = gr.ri, rp = gr.rp;
        uint32_t Ic = gr.w0 >> 5, kc = gr.w0 & 15u;  // the current block (q) and its finder
        for (uint32_t q0 = 0; q0 < GROUP && !done; q0 += K1_QB) {
            uint32_t I[K1_QB], info[K1_QB];
            const Rng ri0 = ri, rp0 = rp;
            if (draw_quad_fast(ri, rp, a.tab.logt, a.tab.pick, MSIM_FD_DEFAULT, I, info))
                draw_quad_exact(ri0, rp0, a.tab.logt, a.tab.pick, I, info);
#pragma unroll
            for (uint32_t b = 0; b < K1_QB; ++b) {
                if (done) continue;
                const int64_t Tn = T + (int64_t)Ic;
                if (Tn >= D) {
                    done = true;
                    n_end = bg + q0 + b;
                    t_last = T;
                    continue;
                }
                T = Tn;
                klast = kc;
                if (klast == 15u) return false;  // PickFinder fell through (simulation.h:220): the retry reports it
#pragma unroll
                for (int kk = 0; kk < M; ++kk) F[kk] += (klast == (uint32_t)kk) ? 1u : 0u;
                Ic = I[b];
                kc = info_finder(info[b]);
            }
        }
    }
    if (!done) return false;
    K3T(6);
    if (n_end == bg && n_end > 0) {  // the block before the end is the previous group's last one
        size_t pg;
        if (G > 0) pg = gb + G - 1;
        else if (e > (int)a.band_lo) pg = gb - 1;
        else return false;
        const GroupRec gp = a.grec[pg * a.nr + r];
        // only the finder of its last block is needed: the picker stream alone, stepped to block GROUP - 1
        Rng rp = gp.rp;
        for (uint32_t q = 1; q + 1 < GROUP; ++q) rng_next(rp);
        klast = info_finder(pick_info(rng_next(rp), a.tab.pick));
    }
    K3T(7);
    // 6. Episodes: the candidates that start before the end apply (a prefix of the chain).
    uint32_t cursor = 0;  // first block not consumed yet; ~0 once the run ended inside an episode
    if (batched) {
        uint32_t naf = 0;
        for (uint32_t t = 0; t < na && nsw[t * nss] < n_end; ++t) {
            const uint32_t x = nsw[(SEG_MAX + EP_MAX + t) * nss];
            if (x & 1u) return false;  // an applied episode K2 could not finish, or one it skipped
            cursor = (x & 2u) ? 0xFFFFFFFFu : (x >> 2);
            ++naf;
        }
#pragma unroll
        for (uint32_t b = 0; b < APPLY_B; ++b)
#pragma unroll
            for (int k = 0; k < M; ++k) {
                F[k] += b < naf ? d[b][k] : 0u;
                S[k] += b < naf ? d[b][M + k] : 0u;
            }
        for (uint32_t t0 = APPLY_B; t0 < naf; t0 += APPLY_B) {  // more than APPLY_B applied episodes (rare)
            uint32_t dd[APPLY_B][2 * M];
#pragma unroll
            for (uint32_t b = 0; b < APPLY_B; ++b) {
                const uint32_t t = t0 + b < naf ? t0 + b : naf - 1;
                const uint32_t *rec = a.recs + (size_t)nsw[(SEG_MAX + t) * nss] * a.rec_words;
#pragma unroll
                for (int k = 0; k < 2 * M; ++k) dd[b][k] = rec[2 + k];
            }
#pragma unroll
            for (uint32_t b = 0; b < APPLY_B; ++b)
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    F[k] += t0 + b < naf ? dd[b][k] : 0u;
                    S[k] += t0 + b < naf ? dd[b][M + k] : 0u;
                }
        }
    } else {  // more than EP_MAX episodes up to the end segment (never at BASELINE sizes): one read at a time
        bool stop = false;
        for (int j = 0; j <= e && !stop; ++j) {
            const uint32_t ns = a.nslow[(size_t)j * a.nr + r];
            if (ns > a.cap) return false;
            for (uint32_t c = 0; c < ns; ++c) {
                const uint32_t idx = a.slots[((size_t)j * a.cap + c) * a.nr + r];
                if (idx >= a.lcap) return false;
                const uint32_t *rec = a.recs + (size_t)idx * a.rec_words;
                const uint32_t s0 = rec[2 + 2 * M];
                if (s0 >= n_end) {
                    stop = true;
                    break;
                }
                if (s0 < cursor) continue;
                const uint32_t f0 = rec[1];
                if (f0 & (REC_ERR | REC_SKIP)) return false;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    F[k] += rec[2 + k];
                    S[k] += rec[2 + M + k];
                }
                cursor = rec[0];
                if (f0 & REC_ENDED) {
                    cursor = 0xFFFFFFFFu;
                    stop = true;
                    break;
                }
            }
        }
    }
    K3T(8);
    K3T_PRINT;
    // 7. The run ended quiet and its last block was a fast one: it counts only if it arrived by D.
    if (cursor != 0xFFFFFFFFu && n_end > 0 && cursor < n_end) {
        const uint32_t k = klast;
        int64_t pk = 0;
#pragma unroll
        for (int kk = 0; kk < M; ++kk)
            if ((uint32_t)kk == k) pk = p.prop[kk];
        if (t_last + pk > D) {
#pragma unroll
            for (int kk = 0; kk < M; ++kk) F[kk] -= ((uint32_t)kk == k) ? 1u : 0u;
        }
    }
    return true;
}

// ---------------------------------------------------------------- K2 lane body (shared host/device)
// SEL (shared-draw sweeps, msim_sweepsplit.h): K2 is handed the point's index list sel_p in a.slots (K2 reads no
// slots otherwise, and PipeArgs stays what the plain pipeline passes): entry idx of it names the listed block of the
// envelope's list; the record, list_count and lcap are the point's own.
template <int M, int KIND, bool SEL = false>
MSIM_HD void episode_entry(const SimParams &p, const PipeArgs &a, uint32_t idx)
{
    const EpEntry e = a.list[SEL ? a.slots[idx] : idx];
    if (e.run == EP_HOLE) return;  // never referenced by a run's slots
    uint32_t *rec = a.recs + (size_t)idx * a.rec_words;
    rec[2 + 2 * M] = e.block;
    const uint32_t seg = e.block / a.seg;
    int64_t T = (int64_t)e.offset;
    // the segment sums before the episode's segment, 8 independent loads at a time
    for (uint32_t j0 = 0; j0 < seg; j0 += 8) {
        uint64_t ss[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) ss[j] = a.segsum[(size_t)(j0 + j < seg ? j0 + j : seg - 1) * a.nr + e.run];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) T += j0 + j < seg ? (int64_t)ss[j] : 0;  // clamped loads, masked
    }
    if (T >= p.duration_ms) {  // beyond the end of the run: never applied
        rec[1] = REC_SKIP;
        return;
    }
    EpSrc src;
    src.lt = a.tab.logt;
    src.pt = a.tab.pick;
    src.ri = e.ri;
    src.rp = e.rp;
    for (uint32_t t = 0; t < e.skip; ++t) {  // K1 stored its quad's start states (EpEntry::skip)
        rng_next(src.ri);
        rng_next(src.rp);
    }
    src.nb = a.nb;
    src.index = e.block;
    src.cur = e.w0;
    src.nxt = e.w1;
    src.have_nxt = true;
    // K2's capacities (K2_LEAN_RHO above); the retry kernel recomputes a flagged run with NX_WIDE and deep branches
    Sim<M, false, KIND == 2, KIND == 0 ? 2 : NX_FAST, NG_FAST> s;
    EpisodeOut<M> o;
    s.episode(p, src, T, o);
    rec[0] = o.end;
    rec[1] = (o.ended ? REC_ENDED : 0u) | (o.err ? REC_ERR : 0u);
#pragma unroll
    for (int k = 0; k < M; ++k) {
        rec[2 + k] = o.F[k];
        rec[2 + M + k] = o.S[k];
    }
}

}  // namespace msim

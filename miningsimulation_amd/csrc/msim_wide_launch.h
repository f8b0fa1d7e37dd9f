// msim_wide_launch.h — host-side interface of the large-network pipeline (msim_wide.h / msim_wide.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "msim_wide.h"

namespace msim {

struct WideArgs {
    // per-config device tables
    const uint64_t *cf;       // [m + 1] cumulative weight | fast threshold << 32 (msim_wide.h wide_pick)
    const uint16_t *bucket;   // [WB_N]
    const int64_t *prop;                   // [m] propagation (ms)
    const LogTab *logt;
    const uint32_t *jmain;  // [64][128] uint4: T^(lane * S0)
    const uint32_t *jtail;  // [64][128] uint4: T^(B0 + lane * ST)
    const uint32_t *jstep;  // [128] uint4: T^(63 * ST - 1) (next tail chunk)
    uint32_t m, W;
    uint64_t mult;
    int64_t D;
    uint64_t run_begin;  // absolute index of the slice's first run
    uint32_t n;          // runs in the slice
    uint32_t seed_base;
    uint32_t S0, ST, nch, rcap;
    uint64_t B0;
    // per-slice workspace
    uint32_t *hist;   // [nr][m]
    uint32_t *info;   // [nr][4]: n_end, finder of block n_end - 1, candidates, error bits
    int64_t *tlast;   // [nr] T_{n_end - 1}
    WideLane *lanes;  // [nr][1 + nch][64]
    WideCand *cand;   // [nr][rcap]
    uint32_t *recs;   // [nr][rcap][WREC_WORDS]
    uint32_t *work;   // [nr * rcap] dense list of candidate slots (r * rcap + c) for W2
    uint32_t *retry;  // [nr * rcap] slots the first W2 pass flagged WREC_RETRY
    uint32_t *counts; // [2]: work entries, retry entries (zeroed per slice)
};

struct WideOut {
    uint64_t *sums;     // [m][6] msim_sums layout, zeroed before the launch
    uint32_t *records;  // [n_total][m][2] or null
    uint32_t *best_h;   // [n_total] or null
    uint32_t *fail;     // failed-run counter (zeroed before the launch)
    uint64_t run_begin;
    uint64_t n_total;
    uint32_t rel_begin;  // set per slice
};

struct WideLayout {
    uint32_t nr, rcap;
    WideGeom g;
    size_t hist_off, info_off, tlast_off, lanes_off, cand_off, recs_off, work_off, retry_off, counts_off, total;
};

// rho = P(a block is not fast) = sum_k w_k/W * P(I <= prop_k). max_nr (a multiple of 256; 0: none) caps the runs
// per slice below what the budget allows (test switch MSIM_MAX_SLICE_RUNS, msim_api.hip).
// Candidate capacity of a run: mean + 8 sigma of its non-fast blocks. rcap_limit (0: none) only ever lowers it
// (test switches MSIM_WIDE_TEST_RCAP / MSIM_WIDE_TEST_POINT_RCAP, msim_api.hip).
inline uint32_t wide_rcap(double rho, const WideGeom &g, uint32_t rcap_limit = 0)
{
    const double blocks = (double)g.B0 + 64.0 * g.ST * g.nch + 64.0;
    const double lam = rho * blocks;
    double rc = ceil(lam + 8.0 * sqrt(lam) + 16.0);
    if (rc > 32000.0) rc = 32000.0;  // slot index fits 15 bits in the combine
    const uint32_t r = (uint32_t)rc;
    return rcap_limit && rcap_limit < r ? rcap_limit : r;
}

inline WideLayout wide_layout_for(double rho, uint32_t m, int64_t duration_ms, uint64_t n_runs, double budget,
                                  uint32_t max_nr = 0, uint32_t rcap_limit = 0)
{
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    WideLayout L;
    L.g = wide_geom(duration_ms);
    L.rcap = wide_rcap(rho, L.g, rcap_limit);
    const double per_run = m * 4.0 + 16 + 8 + (1.0 + L.g.nch) * 64 * sizeof(WideLane) +
                           L.rcap * (sizeof(WideCand) + 4.0 * WREC_WORDS + 8.0) + 64;
    uint64_t cap = (uint64_t)(budget / per_run) / 256 * 256;
    if (cap < 256) cap = 256;
    if (max_nr && max_nr < cap) cap = max_nr;
    const uint64_t want = (n_runs + 3) / 4 * 4;
    L.nr = (uint32_t)(want < cap ? want : cap);
    size_t o = 0;
    L.hist_off = o;
    o = al(o + (size_t)L.nr * m * 4);
    L.info_off = o;
    o = al(o + (size_t)L.nr * 16);
    L.tlast_off = o;
    o = al(o + (size_t)L.nr * 8);
    L.lanes_off = o;
    o = al(o + (size_t)L.nr * (1 + L.g.nch) * 64 * sizeof(WideLane));
    L.cand_off = o;
    o = al(o + (size_t)L.nr * L.rcap * sizeof(WideCand));
    L.recs_off = o;
    o = al(o + (size_t)L.nr * L.rcap * WREC_WORDS * 4);
    L.work_off = o;
    o = al(o + (size_t)L.nr * L.rcap * 4);
    L.retry_off = o;
    o = al(o + (size_t)L.nr * L.rcap * 4);
    L.counts_off = o;
    o = al(o + 16);
    L.total = o;
    return L;
}

// ---------------------------------------------------------------- shared-draw groups (msim_widesplit.h)
// Per-point arguments of the W2 / W3 variants that read a point's selection of the envelope's candidates.
struct WideSel {
    const uint32_t *sel;    // [nr][rcap_p] envelope slots of the point's candidates, in block order
    const uint32_t *pinfo;  // [nr] the point's candidate count, or WIDE_NONE (failed run)
    uint32_t rcap_env;      // stride of the envelope's candidate list
};
// One point of a WS pass.
struct WideSplitPoint {
    const uint32_t *fthr;  // [m] the point's listing thresholds (wsplit_fthr)
    uint32_t *sel, *pinfo;
    uint32_t *work;        // the point's dense W2 work list
    uint32_t *count;       // its length
    uint32_t rcap;
    uint32_t pad;
};
constexpr uint32_t WSPLIT_MAX_POINTS = 16;  // per WS pass (kernel arguments); larger groups take several passes
struct WideSplitArgs {
    const uint32_t *info;
    const WideLane *lanes;
    const WideCand *cand;
    uint32_t n, nch, rcap_env, np;
    WideSplitPoint pt[WSPLIT_MAX_POINTS];
};

// Region of a draw group of more than one point, for slices of nr runs: the envelope's draw-side arrays and the
// group's counters, then per point pinfo, sel, recs, work and retry at the point's own rcap.
struct WideGroupLayout {
    uint32_t nr, rcap_env;
    WideGeom g;
    size_t hist_off, info_off, tlast_off, lanes_off, cand_off, counts_off, total;  // counts: [1 + np][2]
    std::vector<uint32_t> rcap;  // per point
    std::vector<size_t> pinfo_off, sel_off, recs_off, work_off, retry_off;
};
inline WideGroupLayout wide_group_layout_for(double rho_env, const std::vector<double> &rhos, uint32_t m,
                                             int64_t duration_ms, uint64_t n_runs, double budget, uint32_t max_nr,
                                             uint32_t rcap_limit_env, uint32_t rcap_limit_point)
{
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    WideGroupLayout L;
    L.g = wide_geom(duration_ms);
    L.rcap_env = wide_rcap(rho_env, L.g, rcap_limit_env);
    double per_run = m * 4.0 + 16 + 8 + (1.0 + L.g.nch) * 64 * sizeof(WideLane) + L.rcap_env * (double)sizeof(WideCand) + 64;
    for (double rho : rhos) {
        L.rcap.push_back(wide_rcap(rho, L.g, rcap_limit_point));
        per_run += 4.0 + L.rcap.back() * (4.0 + 4.0 * WREC_WORDS + 8.0) + 64;
    }
    uint64_t cap = (uint64_t)(budget / per_run) / 256 * 256;
    if (cap < 256) cap = 256;
    if (max_nr && max_nr < cap) cap = max_nr;
    const uint64_t want = (n_runs + 3) / 4 * 4;
    L.nr = (uint32_t)(want < cap ? want : cap);
    size_t o = 0;
    L.hist_off = o;
    o = al(o + (size_t)L.nr * m * 4);
    L.info_off = o;
    o = al(o + (size_t)L.nr * 16);
    L.tlast_off = o;
    o = al(o + (size_t)L.nr * 8);
    L.lanes_off = o;
    o = al(o + (size_t)L.nr * (1 + L.g.nch) * 64 * sizeof(WideLane));
    L.cand_off = o;
    o = al(o + (size_t)L.nr * L.rcap_env * sizeof(WideCand));
    L.counts_off = o;
    o = al(o + (1 + rhos.size()) * 8);
    for (uint32_t rc : L.rcap) {
        L.pinfo_off.push_back(o);
        o = al(o + (size_t)L.nr * 4);
        L.sel_off.push_back(o);
        o = al(o + (size_t)L.nr * rc * 4);
        L.recs_off.push_back(o);
        o = al(o + (size_t)L.nr * rc * WREC_WORDS * 4);
        L.work_off.push_back(o);
        o = al(o + (size_t)L.nr * rc * 4);
        L.retry_off.push_back(o);
        o = al(o + (size_t)L.nr * rc * 4);
    }
    L.total = o;
    return L;
}
// One point of a group launch: its delays, thresholds and outputs (out.fail may be shared by the points).
struct WideGroupPoint {
    const int64_t *prop;
    const uint32_t *fthr;
    WideOut out;
};

constexpr uint32_t W1_MAX_RUNS = 8;  // runs (waves) per W1 workgroup: 1, 2, 4 or 8, chosen per network
size_t wide_w1_lds(uint32_t m, uint32_t runs);
uint32_t wide_w1_runs(uint32_t m);
size_t wide_w3_lds(uint32_t m, uint32_t rcap, uint32_t nch);
// Runs out.n_total runs slice by slice (L.nr) on stream s; proto carries the tables and geometry.
hipError_t launch_wide(const WideArgs &proto, const WideLayout &L, char *ws, const WideOut &out, hipStream_t s,
                       std::vector<hipEvent_t> *w1_events);
// A draw group of more than one point: per slice W1 once on the envelope (proto: its tables and geometry), WS, then
// W2 (both passes) and W3 per point. n_total runs from run_begin; every point's out.run_begin / n_total are ignored.
hipError_t launch_wide_group(const WideArgs &proto, const WideGroupLayout &L, const std::vector<WideGroupPoint> &pts,
                             char *ws, uint64_t run_begin, uint64_t n_total, hipStream_t s);
size_t wide_split_lds(uint32_t rcap_env, uint32_t nch);
hipError_t launch_sample(int mode, const uint32_t *pow2_jumps, uint64_t seed, uint64_t n, uint32_t S, const uint64_t *cf,
                         const uint16_t *bucket, uint32_t m, uint32_t W, uint64_t mult, const LogTab *logt,
                         unsigned long long *out, hipStream_t s);
hipError_t launch_wide_picks(const WideArgs &a, const uint64_t *u, int32_t *out, uint64_t n, hipStream_t s);

}  // namespace msim

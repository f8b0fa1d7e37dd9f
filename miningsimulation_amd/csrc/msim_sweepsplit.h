// msim_sweepsplit.h — shared-draw sweeps of the event-skipping pipeline: S1's lane body.
//
// The reference compares propagation delays by editing SetupMiners and rebuilding once per point
// (the reference's README.md:21-27). Points of a sweep that share weights and duration share every draw (same
// seeds, same intervals, same finders); among everything K1 writes (msim_pipeline.h) only the LISTING of non-fast
// blocks depends on the delays: block i of finder k is non-fast at point p iff I_{i+1} <= prop_p[k]. So K1 runs once
// per group of such points on the ENVELOPE network (prop_env[k] = max_p prop_p[k]); its list is a superset of every
// point's, and S1 derives each point's own listing from it:
//
//   S1 msim_sweep_split_kernel   one lane per (run, segment): walks the envelope's slots in block order, reads w0 and
//                                w1 of each listed entry, and writes for every point p of the group
//                                   sel_p[j]                 dense list of indices into the envelope's list
//                                   nslow_p[seg][run]        the point's own count
//                                   slots_p[seg][c][run] = j in block order
//                                exactly the blocks {i : (w1 >> 5) <= prop_p[w0 & 15]} K1 would have listed on the
//                                point's own tables, in the same order.
// K2 then runs lane j on list[sel_p[j]] with the point's SimParams (episode_entry<M, KIND, true>, which is handed sel_p
// where the plain K2 has the slots it never reads), K3 combines with the
// shared segment / group arrays and the point's nslow_p / slots_p / recs_p.
//
// Positions in sel_p are reserved per wave (one atomic per wave and point); their order varies from launch to
// launch, results do not (K3 reaches every record through slots_p).
//
// Overflow rules (every flagged run is recomputed by the retry kernel with that point's SimParams, so results never
// depend on a capacity):
//   - a (run, segment) whose envelope count exceeds the envelope's cap, or that holds an index >= the envelope's
//     lcap, stores nslow_p = cap_p + 1 at EVERY point of the group: K3 flags the run at every point;
//   - a point's own overflow flags the run at that point only: more than cap_p blocks store the true count
//     (> cap_p: K3 flags it) and list nothing; a position j >= lcap_p is stored in slots_p (K3 flags the index) and
//     not in sel_p.
#pragma once
#include "msim_pipeline.h"

namespace msim {

// Points per split pass: the lane holds a count and a base per point in registers, the workgroup the points' delays in
// LDS. A larger group takes further split passes over the same envelope list, never further draw passes.
constexpr uint32_t SPLIT_MAX_POINTS = 8;
constexpr uint32_t SPLIT_SKIP = 0xFFFFFFFFu;
constexpr uint32_t SPLIT_B = 4;  // listed blocks read together by split_segment

struct SplitPoint {
    uint32_t *nslow;  // [nseg][nr]
    uint32_t *slots;  // [nseg][cap][nr]
    uint32_t *sel;    // [lcap]
    uint32_t *count;  // positions of sel reserved so far (zeroed before the pass)
    uint32_t cap, lcap;
};

struct SplitArgs {
    uint32_t nr, nseg, cap, lcap;  // the envelope's layout
    uint32_t np;                   // points in this pass (<= SPLIT_MAX_POINTS)
    const uint32_t *nslow;         // the envelope's [nseg][nr]
    const uint32_t *slots;         // the envelope's [nseg][cap][nr]
    const EpEntry *list;           // the envelope's [lcap]
    const uint32_t *fthr;          // [np][16]: prop_p[k] of miner k (split_thresholds)
    SplitPoint pt[SPLIT_MAX_POINTS];
};

// One (run, segment). fthr: the points' thresholds, [np][16] (device: LDS). res.reserve(count, n) returns the first
// of n positions reserved on *count; every lane of a wave calls it once per point (n = 0 when it lists nothing).
template <class Res>
MSIM_HD void split_segment(const SplitArgs &a, const uint32_t *__restrict__ fthr, uint32_t r, uint32_t seg, Res &res)
{
    const uint32_t ns = a.nslow[(size_t)seg * a.nr + r];
    bool bad = ns > a.cap;  // the envelope's own overflow: every point flags the run
    const uint32_t nw = bad ? 0u : ns;
    uint32_t cnt[SPLIT_MAX_POINTS], base[SPLIT_MAX_POINTS];
#pragma unroll
    for (uint32_t p = 0; p < SPLIT_MAX_POINTS; ++p) cnt[p] = 0;
    // Both walks take SPLIT_B entries at a time: their slot reads, then their entry reads, are in flight together
    // (clamped indices, masked below), so a lane waits for two memory rounds per SPLIT_B blocks, not per block.
    for (uint32_t c0 = 0; c0 < nw; c0 += SPLIT_B) {
        uint32_t idx[SPLIT_B], w0[SPLIT_B], nxt[SPLIT_B];
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b)
            idx[b] = a.slots[((size_t)seg * a.cap + (c0 + b < nw ? c0 + b : nw - 1u)) * a.nr + r];
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b) {
            bad = bad || idx[b] >= a.lcap;  // a clamped read repeats a checked index
            const EpEntry &e = a.list[idx[b] < a.lcap ? idx[b] : 0u];
            w0[b] = e.w0;
            nxt[b] = e.w1 >> 5;
        }
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b)
#pragma unroll
            for (uint32_t p = 0; p < SPLIT_MAX_POINTS; ++p)
                if (p < a.np && c0 + b < nw) cnt[p] += nxt[b] <= fthr[p * 16u + (w0[b] & 15u)] ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t p = 0; p < SPLIT_MAX_POINTS; ++p) {
        if (p >= a.np) continue;  // wave-uniform
        const SplitPoint &q = a.pt[p];
        const bool lists = !bad && cnt[p] <= q.cap;
        base[p] = res.reserve(q.count, lists ? cnt[p] : 0u);
        q.nslow[(size_t)seg * a.nr + r] = bad ? q.cap + 1u : cnt[p];
        cnt[p] = lists ? 0u : SPLIT_SKIP;  // from here on: the point's next slot
    }
    if (bad) return;
    for (uint32_t c0 = 0; c0 < nw; c0 += SPLIT_B) {
        uint32_t idx[SPLIT_B], w0[SPLIT_B], nxt[SPLIT_B];
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b)
            idx[b] = a.slots[((size_t)seg * a.cap + (c0 + b < nw ? c0 + b : nw - 1u)) * a.nr + r];
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b) {
            const EpEntry &e = a.list[idx[b]];  // every index was checked by the first walk
            w0[b] = e.w0;
            nxt[b] = e.w1 >> 5;
        }
#pragma unroll
        for (uint32_t b = 0; b < SPLIT_B; ++b) {  // in block order
            if (c0 + b >= nw) continue;
#pragma unroll
            for (uint32_t p = 0; p < SPLIT_MAX_POINTS; ++p) {
                if (p >= a.np || cnt[p] == SPLIT_SKIP || nxt[b] > fthr[p * 16u + (w0[b] & 15u)]) continue;
                const SplitPoint &q = a.pt[p];
                const uint32_t j = base[p] + cnt[p];
                if (j < q.lcap) q.sel[j] = idx[b];
                q.slots[((size_t)seg * q.cap + cnt[p]) * a.nr + r] = j;
                ++cnt[p];
            }
        }
    }
}

// The thresholds of a point as split_segment reads them: prop[k] of miner k (honest, below FTHR_CAP), FTHR_CAP for
// the rest, as build_pick_table.
inline void split_thresholds(const int64_t *prop, uint32_t m, uint32_t (&fthr)[16])
{
    for (uint32_t k = 0; k < 16; ++k)
        fthr[k] = k < m && prop[k] < (int64_t)FTHR_CAP ? (uint32_t)prop[k] : FTHR_CAP;
}

}  // namespace msim

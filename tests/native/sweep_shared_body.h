// sweep_shared_body.h — TEST INFRASTRUCTURE: a host (CPU) execution of the shared-draw sweep
// (miningsimulation_amd/csrc/msim_sweepsplit.h) built from the SAME lane bodies the gfx950 kernels run: the
// envelope's draw_segment, split_segment, episode_entry<M, KIND, true> and combine_run per point, then the per-lane
// model with the retry kernel's capacities for every flagged run. Shared by libsweep_shared_host.so (against the
// oracle, tests/test_sweep_shared_host.py) and the stand-alone sweep_shared_check (sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_dispatch.h"
#include "../../miningsimulation_amd/csrc/msim_jump.h"
#include "../../miningsimulation_amd/csrc/msim_pipeline.h"
#include "../../miningsimulation_amd/csrc/msim_sweepsplit.h"

namespace sshost {
using namespace msim;

struct HostCtx {  // K1's side effects on the host (as tests/native/pipeline_host.cpp)
    PipeLayout L;
    uint32_t r, seg, jb, nsl = 0;
    uint32_t cnt[CNT_WORDS] = {0};
    std::vector<uint32_t> *slots, *gsum, *gcum;
    std::vector<uint64_t> *gend;
    std::vector<GroupRec> *grec;
    std::vector<EpEntry> *list;
    void count(uint32_t info)
    {
        const uint32_t k = info_finder(info);
        cnt[k >> 1] += 1u << (16u * (k & 1u));
    }
    bool vote(bool s) const { return s; }
    void slow(bool s, uint32_t block, uint64_t offset, uint32_t w0, uint32_t w1, const Rng &ri, const Rng &rp, uint32_t skip)
    {
        if (!s) return;
        const uint32_t idx = (uint32_t)list->size();
        list->push_back(EpEntry{r, block, offset, w0, w1, skip, 0, ri, rp});
        if (nsl < L.cap) (*slots)[((size_t)seg * L.cap + nsl) * L.nr + r] = idx;
        ++nsl;
    }
    void group_start(uint32_t g, uint32_t w0, const Rng &ri, const Rng &rp)
    {
        (*grec)[((size_t)jb * L.gps + g) * L.nr + r] = GroupRec{ri, rp, w0, 0};
        for (uint32_t w = 0; w < CNT_WORDS; ++w) (*gcum)[(((size_t)jb * L.gps + g) * CNT_WORDS + w) * L.nr + r] = cnt[w];
    }
    void group(uint32_t g, uint32_t sum, uint64_t end)
    {
        (*gsum)[((size_t)jb * L.gps + g) * L.nr + r] = sum;
        if (g % SGROUP == SGROUP - 1 || g + 1 == L.gps) (*gend)[((size_t)jb * L.nsg + g / SGROUP) * L.nr + r] = end;
    }
};

// K1's output for n runs on one network's general tables.
struct Drawn {
    PipeLayout L;
    PickTab pick;
    LogTab logt;
    std::vector<uint32_t> jump, segcnt, nslow, slots, gsum, gcum;
    std::vector<uint64_t> segsum, gend;
    std::vector<GroupRec> grec;
    std::vector<EpEntry> list;
};

inline double rho_of(const uint64_t *perc, const int64_t *prop, int m)
{
    double rho = 0;
    for (int k = 0; k < m; ++k) rho += (double)perc[k] / 100.0 * (1.0 - exp(-((double)prop[k] + 1.0) / 599999.5));
    return rho;
}

// cap: the slots per (run, segment) to lay out (the caller's override or the layout's); the list is unbounded here,
// an `lcap` below its size makes the entries past it unreachable, as on the device.
inline void draw_all(const uint64_t *perc, const int64_t *prop, int m, int64_t duration_ms, uint32_t seed_base,
                     uint64_t run_begin, uint32_t n, uint32_t wave_slots, uint32_t cap, Drawn &d)
{
    std::vector<uint8_t> self((size_t)m, 0);
    PipeLayout L = pipe_layout_for(rho_of(perc, prop, m), (uint32_t)m, duration_ms, n, 1e18, wave_slots);
    L.nr = n;  // no padding on the host
    if (cap) L.cap = cap;
    d.L = L;
    build_pick_table(perc, prop, self.data(), m, &d.pick);
    build_log_table(&d.logt);
    d.jump.assign((size_t)L.nseg * 128 * 4, 0);
    build_jump_table(L.nseg, L.seg, d.jump.data());
    d.grec.assign((size_t)L.nband * L.gps * n, GroupRec{});
    d.segcnt.assign((size_t)L.nseg * CNT_WORDS * n, 0);
    d.nslow.assign((size_t)L.nseg * n, 0);
    d.slots.assign((size_t)L.nseg * L.cap * n, 0xFFFFFFFFu);
    d.gsum.assign((size_t)L.nband * L.gps * n, 0);
    d.gcum.assign((size_t)L.nband * L.gps * CNT_WORDS * n, 0);
    d.segsum.assign((size_t)L.nseg * n, 0);
    d.gend.assign((size_t)L.nband * L.nsg * n, 0);
    d.list.clear();
    for (uint32_t r = 0; r < n; ++r) {
        const uint64_t run = run_begin + r;
        const Rng si = rng_seed(seed_interval(seed_base, run)), sp = rng_seed(seed_picker(seed_base, run));
        for (uint32_t j = 0; j < L.nseg; ++j) {
            Rng ri, rp;
            Mat128 mt;
            for (int c = 0; c < 128; ++c) {
                const uint32_t *w = &d.jump[((size_t)j * 128 + c) * 4];
                mt.lo[c] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                mt.hi[c] = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            }
            mat_apply(mt, si.s0, si.s1, ri.s0, ri.s1);
            mat_apply(mt, sp.s0, sp.s1, rp.s0, rp.s1);
            HostCtx cx;
            cx.L = L;
            cx.r = r;
            cx.seg = j;
            cx.jb = j - L.band_lo;
            cx.grec = &d.grec;
            cx.slots = &d.slots;
            cx.gsum = &d.gsum;
            cx.gend = &d.gend;
            cx.gcum = &d.gcum;
            cx.list = &d.list;
            d.segsum[(size_t)j * n + r] = draw_segment(cx, ri, rp, &d.logt, &d.pick, j * L.seg, L.seg, j >= L.band_lo);
            for (uint32_t w = 0; w < CNT_WORDS; ++w) d.segcnt[((size_t)j * CNT_WORDS + w) * n + r] = cx.cnt[w];
            d.nslow[(size_t)j * n + r] = cx.nsl;
        }
    }
}

struct HostReserve {
    uint32_t reserve(uint32_t *count, uint32_t n) const
    {
        const uint32_t b = *count;
        *count += n;
        return b;
    }
};

// np points (props[p * m + k]) of one draw group over n runs. Capacity overrides (0: the layout's): env_cap, env_lcap
// for the envelope; pt_cap[p], pt_lcap[p] per point. max_group: points per split pass. Outputs per point and run:
// found / stale [np][n][m], ok [np][n] (1: the pipeline combined the run, 0: it was flagged and the retry machine
// computed it, 2: the retry machine failed too); listing_ok[p]: 1 when the split's listing of every (run, segment)
// the envelope did not overflow equals, block by block and in order, the one draw_segment produces on the point's own
// tables. Returns 0, or a negative code.
template <int M>
int shared_run(const uint64_t *perc, const int64_t *props, uint32_t np, int64_t duration_ms, uint32_t seed_base,
               uint64_t run_begin, uint32_t n, uint32_t wave_slots, uint32_t env_cap, uint32_t env_lcap,
               const uint32_t *pt_cap, const uint32_t *pt_lcap, uint32_t max_group, uint32_t *found, uint32_t *stale,
               uint8_t *ok, uint8_t *listing_ok, uint32_t *n_env_entries, int k2_kind = -1)
{
    if (max_group == 0 || max_group > SPLIT_MAX_POINTS) max_group = SPLIT_MAX_POINTS;
    std::vector<uint8_t> self((size_t)M, 0);
    int64_t penv[M];
    for (int k = 0; k < M; ++k) {
        penv[k] = 0;
        for (uint32_t p = 0; p < np; ++p) penv[k] = props[(size_t)p * M + k] > penv[k] ? props[(size_t)p * M + k] : penv[k];
    }
    Drawn E;
    draw_all(perc, penv, M, duration_ms, seed_base, run_begin, n, wave_slots, env_cap, E);
    const PipeLayout &L = E.L;
    const uint32_t elcap = env_lcap ? env_lcap : 0xFFFFFFF0u;
    *n_env_entries = (uint32_t)E.list.size();
    if (E.list.size() > elcap) {  // exactly elcap entries, as the device's buffer: an unguarded index fails under ASan
        std::vector<EpEntry> cut(E.list.begin(), E.list.begin() + elcap);
        E.list.swap(cut);
    }
    if (E.list.empty()) E.list.push_back(EpEntry{});  // a valid pointer for record 0's masked reads

    // per point state
    struct Pt {
        SimParams sp;
        uint32_t cap, lcap, k2_kind, count;
        std::vector<uint32_t> nslow, slots, sel, recs;
    };
    std::vector<Pt> P(np);
    std::vector<uint32_t> fthr((size_t)np * 16);
    for (uint32_t p = 0; p < np; ++p) {
        const int64_t *pp = props + (size_t)p * M;
        if (make_params(perc, pp, self.data(), M, duration_ms, &P[p].sp)) return -2;
        const PipeLayout Lp = pipe_layout_nr(rho_of(perc, pp, M), M, duration_ms, (n + 255) / 256 * 256, wave_slots);
        P[p].cap = pt_cap && pt_cap[p] ? pt_cap[p] : Lp.cap;
        P[p].lcap = pt_lcap && pt_lcap[p] ? pt_lcap[p] : (uint32_t)E.list.size() + 1u;
        P[p].k2_kind = k2_kind >= 0 && k2_kind <= 2 ? (uint32_t)k2_kind : Lp.k2_kind;
        P[p].count = 0;
        P[p].nslow.assign((size_t)L.nseg * n, 0xDEADBEEFu);
        P[p].slots.assign((size_t)L.nseg * P[p].cap * n, 0xFFFFFFFFu);
        P[p].sel.assign(P[p].lcap, 0xFFFFFFFFu);
        P[p].recs.assign((size_t)P[p].lcap * L.rec_words + 1, 0xFFFFFFFFu);
        uint32_t f[16];
        split_thresholds(pp, M, f);
        memcpy(&fthr[(size_t)p * 16], f, sizeof(f));
    }
    // S1 in passes of max_group points
    for (uint32_t p0 = 0; p0 < np; p0 += max_group) {
        SplitArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.nr = n;
        sa.nseg = L.nseg;
        sa.cap = L.cap;
        sa.lcap = elcap;
        sa.np = np - p0 < max_group ? np - p0 : max_group;
        sa.nslow = E.nslow.data();
        sa.slots = E.slots.data();
        sa.list = E.list.data();
        sa.fthr = &fthr[(size_t)p0 * 16];
        for (uint32_t i = 0; i < sa.np; ++i) {
            Pt &q = P[p0 + i];
            sa.pt[i] = SplitPoint{q.nslow.data(), q.slots.data(), q.sel.data(), &q.count, q.cap, q.lcap};
        }
        HostReserve res;
        for (uint32_t j = 0; j < L.nseg; ++j)
            for (uint32_t r = 0; r < n; ++r) split_segment(sa, sa.fthr, r, j, res);
    }
    for (uint32_t p = 0; p < np; ++p) {
        Pt &q = P[p];
        // the listing against draw_segment on the point's own tables
        {
            Drawn O;
            draw_all(perc, props + (size_t)p * M, M, duration_ms, seed_base, run_begin, n, wave_slots, 1u, O);  // only its counts and its list

            bool same = O.L.seg == L.seg && O.L.nseg == L.nseg;
            size_t at = 0;  // O.list is in (run, segment, block) order
            for (uint32_t r = 0; r < n && same; ++r)
                for (uint32_t j = 0; j < L.nseg && same; ++j) {
                    const uint32_t own = O.nslow[(size_t)j * n + r];
                    const uint32_t got = q.nslow[(size_t)j * n + r];
                    const bool env_over = E.nslow[(size_t)j * n + r] > L.cap;
                    bool walk = !env_over && got <= q.cap;
                    for (uint32_t c = 0; c < E.nslow[(size_t)j * n + r] && c < L.cap && walk; ++c)
                        walk = E.slots[((size_t)j * L.cap + c) * n + r] < elcap;
                    if (walk) {
                        same = same && got == own;
                        for (uint32_t c = 0; c < got && same; ++c) {
                            const uint32_t pos = q.slots[((size_t)j * q.cap + c) * n + r];
                            if (pos >= q.lcap) continue;  // the point's own list overflow: flagged, not listed
                            same = q.sel[pos] < E.list.size() && E.list[q.sel[pos]].block == O.list[at + c].block &&
                                   E.list[q.sel[pos]].run == r;
                        }
                    }
                    at += own;
                }
            listing_ok[p] = same ? 1 : 0;
        }
        PipeArgs a;
        a.nr = n;
        a.seg = L.seg;
        a.gps = L.gps;
        a.nseg = L.nseg;
        a.nb = L.nb;
        a.cap = q.cap;
        a.band_lo = L.band_lo;
        a.lcap = q.lcap;
        a.rec_words = L.rec_words;
        a.tab = PipeTables{&E.pick, &E.logt, E.jump.data()};  // the envelope's tables serve every point
        a.grec = E.grec.data();
        a.segsum = E.segsum.data();
        a.segcnt = E.segcnt.data();
        a.nslow = q.nslow.data();
        a.slots = q.slots.data();
        a.gsum = E.gsum.data();
        a.gend = E.gend.data();
        a.gcum = E.gcum.data();
        a.list = E.list.data();
        a.list_count = &q.count;
        a.recs = q.recs.data();
        PipeArgs a2 = a;  // K2 is handed the index list in `slots` (msim_pipeline.h episode_entry)
        a2.slots = q.sel.data();
        const uint32_t lim = q.count < q.lcap ? q.count : q.lcap;
        for (uint32_t i = 0; i < lim; ++i) {
            if (q.k2_kind == 0) episode_entry<M, 0, true>(q.sp, a2, i);
            else if (q.k2_kind == 1) episode_entry<M, 1, true>(q.sp, a2, i);
            else episode_entry<M, 2, true>(q.sp, a2, i);
        }
        for (uint32_t r = 0; r < n; ++r) {
            uint32_t F[M], S[M];
            uint32_t nsw[K3_SCRATCH];
            uint8_t st = combine_run<M>(q.sp, a, r, F, S, nsw, 1) ? 1 : 0;
            if (!st) {  // the retry kernel's machine (msim_kernels.hip launch_retry)
                RunResult rr;
                Sim<M, false, true, NX_WIDE, NG_WIDE> s;
                const uint64_t run = run_begin + r;
                s.run(q.sp, rng_seed(seed_interval(seed_base, run)), rng_seed(seed_picker(seed_base, run)), rr);
                for (int k = 0; k < M; ++k) {
                    F[k] = rr.found[k];
                    S[k] = rr.stale[k];
                }
                if (rr.err) st = 2;
            }
            ok[(size_t)p * n + r] = st;
            for (int k = 0; k < M; ++k) {
                found[((size_t)p * n + r) * M + k] = F[k];
                stale[((size_t)p * n + r) * M + k] = S[k];
            }
        }
    }
    return 0;
}

inline int shared_run_m(int m, const uint64_t *perc, const int64_t *props, uint32_t np, int64_t duration_ms,
                        uint32_t seed_base, uint64_t run_begin, uint32_t n, uint32_t wave_slots, uint32_t env_cap,
                        uint32_t env_lcap, const uint32_t *pt_cap, const uint32_t *pt_lcap, uint32_t max_group,
                        uint32_t *found, uint32_t *stale, uint8_t *ok, uint8_t *listing_ok, uint32_t *n_env_entries,
                        int k2_kind = -1)
{
#define CASE(MM) \
    case MM:     \
        return shared_run<MM>(perc, props, np, duration_ms, seed_base, run_begin, n, wave_slots, env_cap, env_lcap, pt_cap, \
                              pt_lcap, max_group, found, stale, ok, listing_ok, n_env_entries, k2_kind);
    switch (m) {
        MSIM_FOR_EACH_M(CASE)
    default:
        return -1;
    }
#undef CASE
}

}  // namespace sshost

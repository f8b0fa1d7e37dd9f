// wide_sweep_body.h — TEST INFRASTRUCTURE: a sequential host (CPU) execution of one draw group of the shared-draw
// form of large-network sweeps (miningsimulation_amd/csrc/msim_widesplit.h), built from the SAME lane bodies the
// gfx950 kernels run (wide_pick, draw_interval, wsplit_keep / wsplit_select, wide_episode), composed the way W1, WS,
// W2 and W3 compose them: list on the envelope (every block W1 draws in its phases, blocks past the end of the run
// included), select per point, run the episodes of sel_p with the point's delays, combine.
// Included by wide_sweep_host.cpp (a shared library for the tests) and wide_sweep_check.cpp (a stand-alone program
// under ASan + UBSan). Never part of the product path.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_widesplit.h"

namespace wsweep {
using namespace msim;

// Runs [run_begin, run_begin + n) of np points sharing weights w (summing to W) and duration D; props [np][m].
// rcap_env / rcap_pt[p]: capacities (0: none). found / stale [np][n][m]; ok [np][n] (1: combined, 0: failed);
// counts [1 + np][n]: candidates of the envelope (row 0) and of every point, as W1 would list them.
// Returns 0, or 1 + p when point p's selection differs from the listing on its own thresholds.
inline int run_group(const uint64_t *w, const int64_t *props, uint32_t m, uint32_t np, uint64_t W, int64_t D,
                     uint32_t seed_base, uint64_t run_begin, uint32_t n, uint32_t rcap_env, const uint32_t *rcap_pt,
                     uint32_t *found, uint32_t *stale, uint8_t *ok, uint32_t *counts)
{
    std::vector<int64_t> penv(m, 0);
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t k = 0; k < m; ++k) penv[k] = props[(size_t)p * m + k] > penv[k] ? props[(size_t)p * m + k] : penv[k];
    std::vector<uint32_t> fenv(m);
    std::vector<std::vector<uint32_t>> fpt(np, std::vector<uint32_t>(m));
    for (uint32_t k = 0; k < m; ++k) {
        fenv[k] = wsplit_fthr(penv[k]);
        for (uint32_t p = 0; p < np; ++p) fpt[p][k] = wsplit_fthr(props[(size_t)p * m + k]);
    }
    std::vector<uint64_t> cf(m + 1);
    std::vector<uint16_t> bucket(WB_N);
    build_wide_pick(w, fenv.data(), m, (uint32_t)W, cf.data(), bucket.data());
    LogTab lt;
    build_log_table(&lt);
    const uint64_t mult = 0xFFFFFFFFFFFFFFFFull / W;
    const WideGeom g = wide_geom(D);
    for (uint32_t r = 0; r < n; ++r) {
        const uint64_t run = run_begin + r;
        Rng ri = rng_seed(seed_interval(seed_base, run)), rp = rng_seed(seed_picker(seed_base, run));
        std::vector<uint32_t> I, F;
        std::vector<int64_t> T;
        std::vector<Rng> SI, SP;  // states after drawing block i
        int64_t t = 0;
        auto draw = [&](uint64_t upto) {
            while (I.size() < upto) {
                const uint32_t x = draw_interval(ri, &lt);
                uint32_t th;
                const uint32_t f = wide_pick(rng_next(rp), cf.data(), bucket.data(), (uint32_t)W, mult, th);
                t += x;
                I.push_back(x);
                F.push_back(f);
                T.push_back(t);
                SI.push_back(ri);
                SP.push_back(rp);
            }
        };
        // W1's phases: the main segments (B0 blocks), then tail chunks of 64 x ST blocks, through the phase whose
        // last block is found at >= D; one more draw decides fast / slow of the last block listed
        uint64_t nlist = g.B0;
        bool done = false;
        if (g.B0) {
            draw(g.B0);
            done = T[g.B0 - 1] >= D;
        }
        for (uint32_t c = 0; c < g.nch && !done; ++c) {
            nlist = g.B0 + (uint64_t)(c + 1) * 64 * g.ST;
            draw(nlist);
            done = T[nlist - 1] >= D;
        }
        draw(nlist + 1);
        uint32_t n_end = 0;
        while (n_end < nlist && T[n_end] < D) ++n_end;
        uint32_t err = done ? 0u : (uint32_t)WERR_DRAWS;
        for (uint32_t i = 0; i < n_end; ++i)
            if (F[i] >= m) err |= WERR_PICK;
        // the envelope's list in block order (slot = position)
        std::vector<uint32_t> eblk, epk, ein;
        for (uint32_t i = 0; i < nlist; ++i)
            if (F[i] < m && I[i + 1] <= fenv[F[i]]) {
                epk.push_back(wsplit_pack((uint32_t)eblk.size() & 0xFFFFu, F[i]));
                ein.push_back(I[i + 1]);
                eblk.push_back(i);
            }
        counts[r] = (uint32_t)eblk.size();
        const bool env_fail = err != 0 || (rcap_env && eblk.size() > rcap_env) || eblk.size() > 0xFFFFu;
        for (uint32_t p = 0; p < np; ++p) {
            const int64_t *prop = props + (size_t)p * m;
            uint32_t *Fo = found + ((size_t)p * n + r) * m, *So = stale + ((size_t)p * n + r) * m;
            memset(Fo, 0, 4 * m);
            memset(So, 0, 4 * m);
            // the listing W1 would produce on the point's own thresholds
            std::vector<uint32_t> own;
            for (uint32_t i = 0; i < nlist; ++i)
                if (F[i] < m && I[i + 1] <= fpt[p][F[i]]) own.push_back(i);
            counts[(size_t)(1 + p) * n + r] = (uint32_t)own.size();
            ok[(size_t)p * n + r] = 0;
            if (env_fail) continue;
            const uint32_t rc = rcap_pt && rcap_pt[p] ? rcap_pt[p] : (uint32_t)eblk.size();
            std::vector<uint32_t> sel(rc ? rc : 1);
            const uint32_t cnt = wsplit_select(epk.data(), ein.data(), (uint32_t)eblk.size(), fpt[p].data(), rc, sel.data());
            if (cnt == WIDE_NONE) {
                if (own.size() <= rc) return 1 + (int)p;
                continue;
            }
            if (cnt != own.size()) return 1 + (int)p;
            for (uint32_t j = 0; j < cnt; ++j)
                if (eblk[sel[j]] != own[j]) return 1 + (int)p;
            for (uint32_t i = 0; i < n_end; ++i) Fo[F[i]]++;
            uint32_t cursor = 0;
            bool ended = false, bad = false;
            for (uint32_t j = 0; j < cnt && !bad; ++j) {
                const uint32_t s = eblk[sel[j]];
                if (s >= n_end) break;
                if (s < cursor) continue;
                WideSrc src{SI[s + 1], SP[s + 1], &lt, cf.data(), bucket.data(), (uint32_t)W, mult};
                WideEpOut o;
                wide_episode<WE_FAST, WA_FAST>(prop, m, D, s, T[s], F[s], I[s + 1], F[s + 1], src, o);
                if (o.flags & WREC_RETRY) {
                    WideSrc src2{SI[s + 1], SP[s + 1], &lt, cf.data(), bucket.data(), (uint32_t)W, mult};
                    wide_episode<WE, WA>(prop, m, D, s, T[s], F[s], I[s + 1], F[s + 1], src2, o);
                    if (o.flags & WREC_RETRY) o.flags = WREC_ERR;
                }
                if (o.flags & WREC_ERR) {
                    bad = true;
                    break;
                }
                for (uint32_t e = 0; e < o.ne; ++e) {
                    Fo[o.gid[e]] += o.dF[e];
                    So[o.gid[e]] += o.dS[e];
                }
                cursor = o.end;
                if (o.flags & WREC_ENDED) {
                    ended = true;
                    break;
                }
            }
            if (bad) continue;
            if (!ended && n_end > 0 && cursor < n_end) {
                const uint32_t f = F[n_end - 1];
                if (T[n_end - 1] + prop[f] > D) Fo[f] -= 1;
            }
            ok[(size_t)p * n + r] = 1;
        }
    }
    return 0;
}

}  // namespace wsweep

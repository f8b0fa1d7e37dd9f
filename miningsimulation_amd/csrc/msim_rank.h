// msim_rank.h — exact order statistics of the per-run terms by MSD radix selection (include/msim.h:
// msim_order_stat, msim_rank_launch, msim_run_order_stats). For one run and one column the four quantities are
// found, stale, share_t and rate_t of msim_moments.h, each a uint64 key (found and stale zero-extended). The r-th
// smallest key of a column is found digit by digit, eight passes of eight bits from the top: a pass counts, per
// requested rank, the next digit of the keys that share the rank's prefix, and a step picks the digit whose
// running total first exceeds what remains of the rank.
//
// The key, match, digit and step functions are __host__ __device__: the gfx950 kernels (msim_rank.hip) and the
// sequential host selection below (tests/native/rank_host.cpp, tests/native/rank_check.cpp) run the same lines.
#ifndef MSIM_RANK_H
#define MSIM_RANK_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "msim_moments.h"

namespace msim {

constexpr uint32_t RANK_QUANTITIES = 4;  // found, stale, share_t, rate_t
constexpr uint32_t RANK_BINS = 256;      // one digit
constexpr uint32_t RANK_MAGIC = 0x6B6E6172u;

struct RankState {
    uint64_t prefix;     // the digits chosen so far, in place; the bits below them zero
    uint64_t remaining;  // the rank among the keys that carry the prefix
};

// The four keys of one record, in msim_order_stat's quantity order.
MSIM_MHD void rank_keys(uint32_t f, uint32_t s, uint32_t L, uint64_t key[RANK_QUANTITIES])
{
    key[0] = f;
    key[1] = s;
    key[2] = mom_share_term(f, L);
    key[3] = mom_rate_term(f, s);
}

// Whether the key's top 8 * pass bits are the prefix's: every key at pass 0 (no shift by 64).
MSIM_MHD bool rank_matches(uint64_t key, uint64_t prefix, uint32_t pass)
{
    return pass == 0 || ((key ^ prefix) >> (64 - 8 * pass)) == 0;
}

MSIM_MHD uint32_t rank_digit(uint64_t key, uint32_t pass) { return (uint32_t)(key >> (56 - 8 * pass)) & 255u; }

// The state after a pass whose chosen digit has `before` matching keys in the bins below it.
MSIM_MHD RankState rank_narrow(RankState st, uint32_t digit, uint64_t before, uint32_t pass)
{
    st.prefix |= (uint64_t)digit << (56 - 8 * pass);
    st.remaining -= before;
    return st;
}

// The order statistic a state stands for after the last pass: `equal` is the chosen bin's count there.
MSIM_MHD msim_order_stat rank_result(RankState st, uint64_t rank, uint64_t equal)
{
    msim_order_stat o;
    o.value = st.prefix;
    o.below = rank - st.remaining;
    o.equal = equal;
    return o;
}

// ---------------------------------------------------------------- workspace layout (uint64 words)
// header {magic | m << 32, n_points | n_ranks << 32}, the ranks (MSIM_MAX_RANKS slots), then per (point, column,
// quantity) row group: the mask of the ranks that count this pass (one word), the states of MSIM_MAX_RANKS ranks
// (two words each), and last the counts [group][n_ranks][256], the only part whose size follows n_ranks.
// Ranks that still share a prefix have identical counts, so only the lowest of them (its bit set in the mask)
// is counted, and the step reads its row for all of them; at pass 0 that is rank 0 alone.
struct RankLayout {
    uint64_t groups;  // n_points * m * 4
    size_t ranks_at, mask_at, state_at, counts_at, words;
};

MSIM_MHD RankLayout rank_layout(uint32_t m, uint32_t n_points, uint32_t n_ranks)
{
    RankLayout l;
    l.groups = (uint64_t)n_points * m * RANK_QUANTITIES;
    l.ranks_at = 2;
    l.mask_at = l.ranks_at + MSIM_MAX_RANKS;
    l.state_at = l.mask_at + l.groups;
    l.counts_at = (l.state_at + l.groups * MSIM_MAX_RANKS * 2 + 31) / 32 * 32;  // rows start on 256 bytes
    l.words = l.counts_at + l.groups * n_ranks * RANK_BINS;
    return l;
}

// ---------------------------------------------------------------- host: selection over a record array
// The first bin of a row of 256 counts whose running total exceeds `remaining`; false when the whole row does
// not (a rank at or past the number of keys).
inline bool rank_pick(const uint64_t *row, uint64_t remaining, uint32_t *digit, uint64_t *before)
{
    uint64_t run = 0;
    for (uint32_t b = 0; b < RANK_BINS; ++b) {
        if (run + row[b] > remaining) {
            *digit = b;
            *before = run;
            return true;
        }
        run += row[b];
    }
    return false;
}

// records [n_runs][m]{found, stale}, best_height [n_runs]; out: [m][4][n_ranks] msim_order_stat. Returns the
// number of (column, quantity, rank) rows whose rank is not below n_runs; their entries stay untouched. What the
// kernels compute, sequentially: eight count passes over the records, one step per row after each.
inline uint64_t rank_select_host(const msim_run_record *rec, const uint32_t *best_height, uint64_t n_runs, uint32_t m,
                                 const uint64_t *ranks, uint32_t n_ranks, msim_order_stat *out)
{
    const size_t rows = (size_t)m * RANK_QUANTITIES * n_ranks;
    std::vector<RankState> st(rows);
    std::vector<uint8_t> bad(rows, 0);
    std::vector<uint64_t> counts(rows * RANK_BINS);
    for (size_t i = 0; i < rows; ++i) st[i] = RankState{0, ranks[i % n_ranks]};
    for (uint32_t pass = 0; pass < MSIM_RANK_PASSES; ++pass) {
        std::fill(counts.begin(), counts.end(), 0);
        for (uint64_t r = 0; r < n_runs; ++r)
            for (uint32_t k = 0; k < m; ++k) {
                const msim_run_record &x = rec[r * m + k];
                uint64_t key[RANK_QUANTITIES];
                rank_keys(x.found, x.stale, best_height[r], key);
                for (uint32_t q = 0; q < RANK_QUANTITIES; ++q)
                    for (uint32_t j = 0; j < n_ranks; ++j) {
                        const size_t i = ((size_t)k * RANK_QUANTITIES + q) * n_ranks + j;
                        if (rank_matches(key[q], st[i].prefix, pass)) counts[i * RANK_BINS + rank_digit(key[q], pass)] += 1;
                    }
            }
        for (size_t i = 0; i < rows; ++i) {
            uint32_t digit;
            uint64_t before;
            if (bad[i] || !rank_pick(&counts[i * RANK_BINS], st[i].remaining, &digit, &before)) {
                bad[i] = 1;
                continue;
            }
            st[i] = rank_narrow(st[i], digit, before, pass);
            if (pass + 1 == MSIM_RANK_PASSES) out[i] = rank_result(st[i], ranks[i % n_ranks], counts[i * RANK_BINS + digit]);
        }
    }
    uint64_t n_bad = 0;
    for (size_t i = 0; i < rows; ++i) n_bad += bad[i];
    return n_bad;
}

}  // namespace msim

#endif  // MSIM_RANK_H

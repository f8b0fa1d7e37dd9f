// msim_boot.h — the Poisson bootstrap of order statistics and expected shortfalls (include/msim.h: msim_boot_item,
// msim_boot_row, msim_boot_*_launch, msim_run_bootstrap). Replicate b gives the absolute run r the integer weight
// boot_weight(seed, b, r); a replicate's quantile is the key at rank max(1, ceil(q W_b)) - 1 of the weighted
// multiset, found by msim_rank.h's radix selection over weighted digit counts, and its shortfall comes from the
// weighted sum of the keys below that value.
//
// The weight, key, layout and per-row step are __host__ __device__: the gfx950 kernels (msim_boot.hip) and the host
// mirrors below (tests/native/boot_host.cpp, tests/native/boot_check.cpp) run the same lines. The mirrors work on
// the kernels' workspace, one call per launch, so that two record buffers can feed one pass on the host too.
#ifndef MSIM_BOOT_H
#define MSIM_BOOT_H

#include <stddef.h>
#include <stdint.h>

#include <math.h>

#include <vector>

#include "msim_draws.h"
#include "msim_rank.h"

namespace msim {

constexpr uint32_t BOOT_MAGIC = 0x746F6F62u;
constexpr uint64_t BOOT_G = 0x9E3779B97F4A7C15ull;
constexpr uint32_t BOOT_MAX_WEIGHT = 13;
constexpr uint32_t BOOT_ROW_WORDS = 5;  // msim_boot_row

// floor(2^32 * sum_{i<=k} e^-1 / i!), k = 0..12 (tests/test_boot_host.py recomputes them with 80-digit decimals)
#define MSIM_BOOT_T0 1580030168u
#define MSIM_BOOT_T1 3160060337u
#define MSIM_BOOT_T2 3950075421u
#define MSIM_BOOT_T3 4213413783u
#define MSIM_BOOT_T4 4279248373u
#define MSIM_BOOT_T5 4292415291u
#define MSIM_BOOT_T6 4294609777u
#define MSIM_BOOT_T7 4294923276u
#define MSIM_BOOT_T8 4294962463u
#define MSIM_BOOT_T9 4294966817u
#define MSIM_BOOT_T10 4294967252u
#define MSIM_BOOT_T11 4294967292u
#define MSIM_BOOT_T12 4294967295u

// SplitMix64's output function: msim_draws.h's splitmix64 adds G to its state first, so start G below x.
MSIM_MHD uint64_t boot_mix(uint64_t x)
{
    uint64_t s = x - BOOT_G;
    return splitmix64(s);
}

// The constant of the replicate pair b >> 1, and the 64 bits the pair draws for one absolute run.
MSIM_MHD uint64_t boot_pair_const(uint64_t seed, uint32_t b) { return boot_mix(seed ^ ((uint64_t)(b >> 1) * BOOT_G)); }
MSIM_MHD uint64_t boot_pair_bits(uint64_t c, uint64_t run) { return boot_mix(c + BOOT_G * (run + 1)); }

// The number of thresholds at or below u: compares as plain constants, no table in memory. Past T3 lies 1.9 % of u.
MSIM_MHD uint32_t boot_weight_of(uint32_t u)
{
    uint32_t w = (uint32_t)(u >= MSIM_BOOT_T0) + (uint32_t)(u >= MSIM_BOOT_T1) + (uint32_t)(u >= MSIM_BOOT_T2) +
                 (uint32_t)(u >= MSIM_BOOT_T3);
    if (u >= MSIM_BOOT_T4)
        w += 1u + (uint32_t)(u >= MSIM_BOOT_T5) + (uint32_t)(u >= MSIM_BOOT_T6) + (uint32_t)(u >= MSIM_BOOT_T7) +
             (uint32_t)(u >= MSIM_BOOT_T8) + (uint32_t)(u >= MSIM_BOOT_T9) + (uint32_t)(u >= MSIM_BOOT_T10) +
             (uint32_t)(u >= MSIM_BOOT_T11) + (uint32_t)(u >= MSIM_BOOT_T12);
    return w;
}

// Replicate b's weight from its pair's bits: the high half for odd b, the low half for even b; replicate 0 is the data.
MSIM_MHD uint32_t boot_weight_from(uint64_t z, uint32_t b)
{
    if (b == 0) return 1;
    return boot_weight_of((b & 1u) ? (uint32_t)(z >> 32) : (uint32_t)z);
}

MSIM_MHD uint32_t boot_weight(uint64_t seed, uint32_t b, uint64_t run)
{
    if (b == 0) return 1;
    return boot_weight_from(boot_pair_bits(boot_pair_const(seed, b), run), b);
}

// The one key of an item's quantity: at most one division.
MSIM_MHD uint64_t boot_key(uint32_t quantity, uint32_t f, uint32_t s, uint32_t L)
{
    switch (quantity) {
        case 0: return f;
        case 1: return s;
        case 2: return mom_share_term(f, L);
        default: return mom_rate_term(f, s);
    }
}

MSIM_MHD bool boot_item_ok(const msim_boot_item &it, uint32_t m, uint32_t n_points, uint32_t n_q)
{
    return it.point < n_points && it.column < m && it.quantity < RANK_QUANTITIES && it.q_index < n_q;
}

inline bool boot_shape_ok(uint32_t n_items, uint32_t B)
{
    return n_items >= 1 && n_items <= MSIM_MAX_BOOT_ITEMS && B >= 1 && B <= MSIM_MAX_BOOT_REPLICATES;
}

// max(1, ceil(q W)) - 1 with the rounded double product, as quantiles.quantile_rank forms it.
inline uint64_t boot_rank(uint64_t W, double q)
{
    if (W == 0 || !(q >= 0.0 && q <= 1.0)) return MSIM_BOOT_EMPTY;
    const double k = ceil(q * (double)W);
    uint64_t ki = k < 1.0 ? 1 : (uint64_t)k;
    if (ki > W) ki = W;  // unreachable below 2^53: q <= 1
    return ki - 1;
}

// ---------------------------------------------------------------- workspace layout (uint64 words)
// header {magic | n_items << 32, B | m << 32, n_points, 0}; the items (two words each: point | column << 32,
// quantity | q_index << 32); per row (item-major, replicate-minor) three arrays: prefix, remaining, rank (rank ==
// MSIM_BOOT_EMPTY: an empty row); last the counts [row][256], rows starting on 256 bytes.
struct BootLayout {
    uint64_t rows;
    size_t items_at, prefix_at, remaining_at, rank_at, counts_at, words;
};

MSIM_MHD BootLayout boot_layout(uint32_t n_items, uint32_t B)
{
    BootLayout l;
    l.rows = (uint64_t)n_items * B;
    l.items_at = 4;
    l.prefix_at = l.items_at + 2 * (size_t)n_items;
    l.remaining_at = l.prefix_at + l.rows;
    l.rank_at = l.remaining_at + l.rows;
    l.counts_at = (l.rank_at + l.rows + 31) / 32 * 32;
    l.words = l.counts_at + l.rows * RANK_BINS;
    return l;
}

MSIM_MHD uint64_t boot_header0(uint32_t n_items) { return BOOT_MAGIC | (uint64_t)n_items << 32; }
MSIM_MHD uint64_t boot_header1(uint32_t B, uint32_t m) { return B | (uint64_t)m << 32; }

// Whether `ws` is what begin prepared for this shape (m == 0 and n_points == 0: the step, which knows neither).
template <class Word>
MSIM_MHD bool boot_prepared(const Word *ws, uint32_t m, uint32_t n_points, uint32_t n_items, uint32_t B)
{
    if ((uint64_t)ws[0] != boot_header0(n_items) || (uint32_t)ws[1] != B || (uint64_t)ws[3] != 0) return false;
    if (m == 0 && n_points == 0) return true;
    return (uint64_t)ws[1] == boot_header1(B, m) && (uint64_t)ws[2] == n_points;
}

template <class Word>
MSIM_MHD msim_boot_item boot_item_at(const Word *ws, const BootLayout &l, uint32_t i)
{
    const uint64_t a = ws[l.items_at + 2 * (size_t)i], b = ws[l.items_at + 2 * (size_t)i + 1];
    msim_boot_item it;
    it.point = (uint32_t)a;
    it.column = (uint32_t)(a >> 32);
    it.quantity = (uint32_t)b;
    it.q_index = (uint32_t)(b >> 32);
    return it;
}

// One row's step from its chosen bin: `before` is the total of the bins below `digit`, `equal` the bin's own count.
// Narrows the state; at the last pass fills the row's five words.
MSIM_MHD RankState boot_row_step(RankState st, uint64_t rank, uint32_t digit, uint64_t before, uint64_t equal,
                                 uint32_t pass, uint64_t *row_or_null)
{
    st = rank_narrow(st, digit, before, pass);
    if (pass + 1 == MSIM_RANK_PASSES && row_or_null) {
        const msim_order_stat o = rank_result(st, rank, equal);
        row_or_null[0] = o.value;
        row_or_null[1] = o.below;
        row_or_null[2] = o.equal;
        row_or_null[3] = 0;
        row_or_null[4] = 0;
    }
    return st;
}

// ---------------------------------------------------------------- host mirrors of the launches
inline void boot_weights_host(uint64_t seed, uint64_t run_begin, uint64_t runs, uint32_t B, uint64_t *W)
{
    for (uint32_t b = 0; b < B; ++b)
        for (uint64_t r = 0; r < runs; ++r) W[b] += boot_weight(seed, b, run_begin + r);
}

// ranks [n_q][B]; the caller has checked the items.
inline void boot_begin_host(uint32_t m, uint32_t n_points, const msim_boot_item *items, uint32_t n_items, uint32_t B,
                            const uint64_t *ranks, uint64_t *ws)
{
    const BootLayout l = boot_layout(n_items, B);
    ws[0] = boot_header0(n_items);
    ws[1] = boot_header1(B, m);
    ws[2] = n_points;
    ws[3] = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        ws[l.items_at + 2 * (size_t)i] = items[i].point | (uint64_t)items[i].column << 32;
        ws[l.items_at + 2 * (size_t)i + 1] = items[i].quantity | (uint64_t)items[i].q_index << 32;
        for (uint32_t b = 0; b < B; ++b) {
            const uint64_t row = (uint64_t)i * B + b, rk = ranks[(size_t)items[i].q_index * B + b];
            ws[l.prefix_at + row] = 0;
            ws[l.remaining_at + row] = rk;
            ws[l.rank_at + row] = rk;
        }
    }
    for (size_t i = l.rank_at + l.rows; i < l.words; ++i) ws[i] = 0;
}

// Where the mirrors take an item's key of run r from: a record buffer rec [n_points][runs][m] with best_height
// [n_points][runs], as the kernels do; the tests also feed raw keys, which reach values no record gives (2^64 - 1).
struct BootRecordKeys {
    const msim_run_record *rec;
    const uint32_t *best_height;
    uint64_t runs;
    uint32_t m;
    uint64_t operator()(const msim_boot_item &it, uint64_t r) const
    {
        const msim_run_record &x = rec[((size_t)it.point * runs + r) * m + it.column];
        return boot_key(it.quantity, x.found, x.stale, best_height[(size_t)it.point * runs + r]);
    }
};

// The buffer holds the absolute runs from run_begin on.
template <class KeyOf>
inline void boot_count_host(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs,
                            const KeyOf &key_of, uint32_t n_items, uint32_t B, uint32_t pass, uint64_t *ws)
{
    if (!boot_prepared(ws, m, n_points, n_items, B)) return;
    const BootLayout l = boot_layout(n_items, B);
    for (uint32_t i = 0; i < n_items; ++i) {
        const msim_boot_item it = boot_item_at(ws, l, i);
        for (uint64_t r = 0; r < runs; ++r) {
            const uint64_t key = key_of(it, r);
            for (uint32_t b = 0; b < B; ++b) {
                const uint64_t row = (uint64_t)i * B + b;
                if (ws[l.rank_at + row] == MSIM_BOOT_EMPTY || !rank_matches(key, ws[l.prefix_at + row], pass)) continue;
                ws[l.counts_at + row * RANK_BINS + rank_digit(key, pass)] += boot_weight(seed, b, run_begin + r);
            }
        }
    }
}

// Returns the number of rows whose counts do not reach their rank. rows_or_null: [n_items][B][5], written at the
// last pass.
inline uint64_t boot_step_host(uint32_t n_items, uint32_t B, uint32_t pass, uint64_t *ws, uint64_t *rows_or_null)
{
    if (!boot_prepared(ws, 0, 0, n_items, B)) return 0;
    const BootLayout l = boot_layout(n_items, B);
    uint64_t bad = 0;
    for (uint64_t row = 0; row < l.rows; ++row) {
        uint64_t *cnt = ws + l.counts_at + row * RANK_BINS;
        uint64_t *out = rows_or_null ? rows_or_null + row * BOOT_ROW_WORDS : nullptr;
        const uint64_t rank = ws[l.rank_at + row];
        uint32_t digit;
        uint64_t before;
        if (rank == MSIM_BOOT_EMPTY) {
            if (pass + 1 == MSIM_RANK_PASSES && out)
                for (uint32_t j = 0; j < BOOT_ROW_WORDS; ++j) out[j] = 0;
        } else if (!rank_pick(cnt, ws[l.remaining_at + row], &digit, &before)) {
            bad += 1;
        } else {
            const RankState st = boot_row_step(RankState{ws[l.prefix_at + row], ws[l.remaining_at + row]}, rank, digit,
                                               before, cnt[digit], pass, out);
            ws[l.prefix_at + row] = st.prefix;
            ws[l.remaining_at + row] = st.remaining;
        }
        for (uint32_t j = 0; j < RANK_BINS; ++j) cnt[j] = 0;
    }
    return bad;
}

template <class KeyOf>
inline void boot_below_host(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs,
                            const KeyOf &key_of, uint32_t n_items, uint32_t B, const uint64_t *ws, uint64_t *rows)
{
    if (!boot_prepared(ws, m, n_points, n_items, B)) return;
    const BootLayout l = boot_layout(n_items, B);
    for (uint32_t i = 0; i < n_items; ++i) {
        const msim_boot_item it = boot_item_at(ws, l, i);
        for (uint64_t r = 0; r < runs; ++r) {
            const uint64_t key = key_of(it, r);
            for (uint32_t b = 0; b < B; ++b) {
                uint64_t *row = rows + ((uint64_t)i * B + b) * BOOT_ROW_WORDS;
                if (row[2] == 0 || !(key < row[0])) continue;
                const uint64_t w = boot_weight(seed, b, run_begin + r);
                row[3] += w * (key >> 32);
                row[4] += w * (key & 0xFFFFFFFFull);
            }
        }
    }
}

// Sequential selection over one record array: W, the ranks from qs, begin, eight count + step rounds and the below
// pass, every row with counts of its own. out_W [B], out_rows [n_items][B][5]. Returns the rows whose counts did not
// reach their rank (0 for ranks computed from W), or -1 for arguments the drivers refuse.
template <class KeyOf>
inline long long boot_select_keys_host(const KeyOf &key_of, uint32_t n_points, uint64_t run_begin, uint64_t runs,
                                       uint32_t m, const msim_boot_item *items, uint32_t n_items, const double *qs,
                                       uint32_t n_q, uint32_t B, uint64_t seed, uint64_t *out_W, uint64_t *out_rows)
{
    if (!boot_shape_ok(n_items, B) || n_q == 0 || n_q > MSIM_MAX_RANKS || runs == 0 || runs >= MSIM_BOOT_MAX_RUNS)
        return -1;
    for (uint32_t i = 0; i < n_items; ++i)
        if (!boot_item_ok(items[i], m, n_points, n_q)) return -1;
    for (uint32_t b = 0; b < B; ++b) out_W[b] = 0;
    boot_weights_host(seed, run_begin, runs, B, out_W);
    std::vector<uint64_t> ranks((size_t)n_q * B);
    for (uint32_t j = 0; j < n_q; ++j)
        for (uint32_t b = 0; b < B; ++b) ranks[(size_t)j * B + b] = boot_rank(out_W[b], qs[j]);
    std::vector<uint64_t> ws(boot_layout(n_items, B).words);
    boot_begin_host(m, n_points, items, n_items, B, ranks.data(), ws.data());
    uint64_t bad = 0;
    for (uint32_t pass = 0; pass < MSIM_RANK_PASSES; ++pass) {
        boot_count_host(m, n_points, seed, run_begin, runs, key_of, n_items, B, pass, ws.data());
        bad += boot_step_host(n_items, B, pass, ws.data(), out_rows);
    }
    boot_below_host(m, n_points, seed, run_begin, runs, key_of, n_items, B, ws.data(), out_rows);
    return (long long)bad;
}

inline long long boot_select_host(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                  uint64_t run_begin, uint64_t runs, uint32_t m, const msim_boot_item *items,
                                  uint32_t n_items, const double *qs, uint32_t n_q, uint32_t B, uint64_t seed,
                                  uint64_t *out_W, uint64_t *out_rows)
{
    return boot_select_keys_host(BootRecordKeys{rec, best_height, runs, m}, n_points, run_begin, runs, m, items, n_items,
                                 qs, n_q, B, seed, out_W, out_rows);
}

}  // namespace msim

#endif  // MSIM_BOOT_H

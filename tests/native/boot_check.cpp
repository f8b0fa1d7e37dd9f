// boot_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_boot.h's host code (the weight function, the
// rank, the layout, the sequential selection and the launches' mirrors), built with -fsanitize=address,undefined and
// run by tests/test_boot_host.py as a child process. It feeds small record arrays with extreme values (all equal;
// found 0 and 2^32 - 1; a rate key of 2^64 - 2^32; 1 to 3 runs, where replicates are empty) and checks every row
// against a weighted multiset sorted independently here. Exit status 0 = all checks held.
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../miningsimulation_amd/csrc/msim_boot.h"

using namespace msim;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("boot_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                         \
        }                                                       \
    } while (0)

static void check_shape(uint64_t runs, uint32_t m, uint32_t B, uint64_t seed, uint64_t run_begin)
{
    std::vector<msim_run_record> rec(runs * m);
    std::vector<uint32_t> bh(runs);
    for (uint64_t r = 0; r < runs; ++r) {
        bh[r] = r % 5 == 4 ? 0 : 1000 + (uint32_t)(r * 37 % 900);
        for (uint32_t k = 0; k < m; ++k) {
            msim_run_record &x = rec[r * m + k];
            switch (k % 4) {
                case 0: x.found = 6, x.stale = 2; break;
                case 1: x.found = r % 2 ? 0xFFFFFFFFu : 0, x.stale = r % 2 ? 0 : 0xFFFFFFFFu; break;
                case 2: x.found = r % 3 ? 7 : 1, x.stale = r % 3 ? 3 : 0xFFFFFFFFu; break;
                default: x.found = (uint32_t)(r * 2654435761u) % 2000, x.stale = (uint32_t)r % 19; break;
            }
        }
    }
    const double qs[3] = {1e-9, 0.5, 1.0};
    std::vector<msim_boot_item> items;
    for (uint32_t k = 0; k < m; ++k)
        for (uint32_t q = 0; q < 4; ++q) items.push_back(msim_boot_item{0, k, q, (k + q) % 3});
    const uint32_t n = (uint32_t)items.size();
    std::vector<uint64_t> W(B), rows((size_t)n * B * BOOT_ROW_WORDS, ~0ull);
    CHECK(boot_select_host(rec.data(), bh.data(), 1, run_begin, runs, m, items.data(), n, qs, 3, B, seed, W.data(),
                           rows.data()) == 0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < B; ++b) {
            std::vector<std::pair<uint64_t, uint64_t>> kw;
            uint64_t total = 0;
            for (uint64_t r = 0; r < runs; ++r) {
                const msim_run_record &x = rec[r * m + items[i].column];
                kw.push_back({boot_key(items[i].quantity, x.found, x.stale, bh[r]), boot_weight(seed, b, run_begin + r)});
                total += kw.back().second;
            }
            CHECK(total == W[b]);
            const uint64_t *row = &rows[((size_t)i * B + b) * BOOT_ROW_WORDS];
            if (total == 0) {
                CHECK(row[0] == 0 && row[1] == 0 && row[2] == 0 && row[3] == 0 && row[4] == 0);
                continue;
            }
            std::sort(kw.begin(), kw.end());
            const uint64_t rank = boot_rank(total, qs[items[i].q_index]);
            CHECK(rank < total);
            uint64_t run = 0, value = 0;
            for (const auto &p : kw) {
                run += p.second;
                if (run > rank) {
                    value = p.first;
                    break;
                }
            }
            uint64_t below = 0, equal = 0, hi = 0, lo = 0;
            for (const auto &p : kw) {
                if (p.first < value) below += p.second, hi += p.second * (p.first >> 32), lo += p.second * (p.first & 0xFFFFFFFFull);
                if (p.first == value) equal += p.second;
            }
            CHECK(row[0] == value && row[1] == below && row[2] == equal && row[3] == hi && row[4] == lo);
            if (b == 0) CHECK(total == runs);
        }
}

int main()
{
    // the weight function's edges
    CHECK(boot_weight_of(0) == 0 && boot_weight_of(MSIM_BOOT_T0 - 1) == 0 && boot_weight_of(MSIM_BOOT_T0) == 1);
    CHECK(boot_weight_of(MSIM_BOOT_T3) == 4 && boot_weight_of(MSIM_BOOT_T4 - 1) == 4 && boot_weight_of(MSIM_BOOT_T4) == 5);
    CHECK(boot_weight_of(MSIM_BOOT_T12 - 1) == 12 && boot_weight_of(0xFFFFFFFFu) == BOOT_MAX_WEIGHT);
    CHECK(boot_weight(5, 0, 0) == 1 && boot_weight(5, 0, ~0ull) == 1);
    for (uint64_t run : {0ull, 0xFFFFFFFFull, 1ull << 63, ~0ull})
        for (uint32_t b = 1; b < 6; ++b) CHECK(boot_weight(~0ull, b, run) <= BOOT_MAX_WEIGHT);
    {  // an odd/even pair draws the two halves of one word
        const uint64_t z = boot_pair_bits(boot_pair_const(77, 6), 1234);
        CHECK(boot_pair_const(77, 6) == boot_pair_const(77, 7));
        CHECK(boot_weight(77, 6, 1234) == boot_weight_of((uint32_t)z) && boot_weight(77, 7, 1234) == boot_weight_of((uint32_t)(z >> 32)));
    }
    // the rank
    CHECK(boot_rank(0, 0.5) == MSIM_BOOT_EMPTY && boot_rank(10, 2.0) == MSIM_BOOT_EMPTY && boot_rank(10, -0.1) == MSIM_BOOT_EMPTY);
    CHECK(boot_rank(20, 0.05) == 0 && boot_rank(40, 0.05) == 1 && boot_rank(7, 1.0) == 6 && boot_rank(7, 0.0) == 0);
    CHECK(boot_rank(13ull << 28, 1.0) == (13ull << 28) - 1);
    // the layout: rows of counts on 256 bytes, nothing overlapping
    for (uint32_t n : {1u, 3u, 37u})
        for (uint32_t B : {1u, 2u, 33u, 257u}) {
            const BootLayout l = boot_layout(n, B);
            CHECK(l.counts_at % 32 == 0 && l.counts_at >= l.rank_at + l.rows && l.words == l.counts_at + l.rows * 256);
            CHECK(l.prefix_at == 4 + 2 * (size_t)n && l.remaining_at == l.prefix_at + l.rows);
        }
    CHECK(!boot_shape_ok(0, 1) && !boot_shape_ok(1, 0) && !boot_shape_ok(MSIM_MAX_BOOT_ITEMS + 1, 1) &&
          !boot_shape_ok(1, MSIM_MAX_BOOT_REPLICATES + 1) && boot_shape_ok(MSIM_MAX_BOOT_ITEMS, MSIM_MAX_BOOT_REPLICATES));
    // selections against an independent sort; 1 to 3 runs give empty replicates
    for (uint64_t runs : {1ull, 2ull, 3ull, 64ull, 257ull})
        for (uint32_t B : {1u, 2u, 33u, 65u}) check_shape(runs, runs < 64 ? 2 : 5, B, 0x1234567 + runs, runs == 64 ? (1ull << 40) : 0);
    {  // refusals
        msim_run_record x = {1, 1};
        uint32_t L = 1;
        msim_boot_item it = {0, 0, 0, 0}, bad = {0, 1, 0, 0};
        double q = 0.5;
        uint64_t W[2], rows[10];
        CHECK(boot_select_host(&x, &L, 1, 0, MSIM_BOOT_MAX_RUNS, 1, &it, 1, &q, 1, 1, 1, W, rows) == -1);
        CHECK(boot_select_host(&x, &L, 1, 0, 1, 1, &bad, 1, &q, 1, 1, 1, W, rows) == -1);
        CHECK(boot_select_host(&x, &L, 1, 0, 1, 1, &it, 1, &q, 1, MSIM_MAX_BOOT_REPLICATES + 1, 1, W, rows) == -1);
        CHECK(boot_select_host(&x, &L, 1, 0, 1, 1, &it, 1, &q, 1, 2, 1, W, rows) == 0 && rows[0] == 1 && rows[2] == 1);
    }
    if (failures) {
        printf("boot_check: %d checks failed\n", failures);
        return 1;
    }
    printf("boot_check: ok\n");
    return 0;
}

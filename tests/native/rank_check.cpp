// rank_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_rank.h's host code (the key, match, digit and
// narrowing functions and the sequential selection over a record array), built with -fsanitize=address,undefined
// and run by tests/test_rank_host.py as a child process. It feeds the extreme records (all zero; all equal; f = L;
// f = 1 with s = 2^32 - 1; L = 0; values that differ only in the lowest or only in the highest non-zero byte) and
// checks every order statistic against std::sort and counting written independently here. Exit status 0 = all
// checks held.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../miningsimulation_amd/csrc/msim_rank.h"

using namespace msim;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("rank_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                         \
        }                                                       \
    } while (0)

static void check_case(uint32_t n, uint32_t m, const std::vector<msim_run_record> &rec, const std::vector<uint32_t> &bh,
                       const std::vector<uint64_t> &ranks)
{
    const uint32_t nr = (uint32_t)ranks.size();
    std::vector<msim_order_stat> out((size_t)m * 4 * nr, msim_order_stat{~0ull, ~0ull, ~0ull});
    uint64_t want_bad = 0;
    for (uint64_t r : ranks) want_bad += r >= n ? (uint64_t)m * 4 : 0;
    CHECK(rank_select_host(rec.data(), bh.data(), n, m, ranks.data(), nr, out.data()) == want_bad);
    for (uint32_t k = 0; k < m; ++k)
        for (uint32_t q = 0; q < 4; ++q) {
            std::vector<uint64_t> keys(n);
            for (uint32_t r = 0; r < n; ++r) {
                const uint64_t f = rec[(size_t)r * m + k].found, s = rec[(size_t)r * m + k].stale, L = bh[r];
                const uint64_t st = (f == 0 || L == 0) ? 0 : (uint64_t)((double)f / (double)L * 4294967296.0 + 0.5);
                const uint64_t rt = f == 0 ? 0 : (uint64_t)((double)s / (double)f * 4294967296.0 + 0.5);
                keys[r] = q == 0 ? f : q == 1 ? s : q == 2 ? st : rt;
            }
            std::sort(keys.begin(), keys.end());
            for (uint32_t j = 0; j < nr; ++j) {
                const msim_order_stat &o = out[((size_t)k * 4 + q) * nr + j];
                if (ranks[j] >= n) {
                    CHECK(o.value == ~0ull && o.below == ~0ull && o.equal == ~0ull);  // untouched
                    continue;
                }
                const uint64_t v = keys[ranks[j]];
                const uint64_t below = (uint64_t)(std::lower_bound(keys.begin(), keys.end(), v) - keys.begin());
                const uint64_t upto = (uint64_t)(std::upper_bound(keys.begin(), keys.end(), v) - keys.begin());
                CHECK(o.value == v && o.below == below && o.equal == upto - below);
                CHECK(o.below <= ranks[j] && ranks[j] < o.below + o.equal);
            }
        }
}

int main()
{
    // the functions on their own
    CHECK(rank_matches(0xFFFFFFFFFFFFFFFFull, 0, 0) && rank_matches(0, 0xFF00000000000000ull, 0));
    CHECK(rank_matches(0xAB12345678ull, 0xAB00000000ull, 4) && !rank_matches(0xAB12345678ull, 0xAC00000000ull, 4));
    CHECK(rank_matches(0x1234567890ABCDEFull, 0x1234567890ABCD00ull, 7) &&
          !rank_matches(0x1234567890ABCDEFull, 0x1234567890ABCC00ull, 7));
    CHECK(rank_matches(0xFF00000000000000ull, 0xFF00000000000000ull, 1) && !rank_matches(0xFE00000000000000ull, 0xFF00000000000000ull, 1));
    CHECK(rank_digit(0xFF00000000000000ull, 0) == 0xFF && rank_digit(0x1234567890ABCDEFull, 7) == 0xEF &&
          rank_digit(0x1234567890ABCDEFull, 3) == 0x78);
    {
        uint64_t key[4];
        rank_keys(10, 3, 10, key);
        CHECK(key[0] == 10 && key[1] == 3 && key[2] == 1ull << 32);
        rank_keys(1, 0xFFFFFFFFu, 1, key);
        CHECK(key[1] == 0xFFFFFFFFull && key[3] == 0xFFFFFFFF00000000ull);
        rank_keys(5, 0, 0, key);
        CHECK(key[2] == 0 && key[3] == 0);
        const RankState s = rank_narrow(RankState{0xAB00000000000000ull, 9}, 0xCD, 4, 1);
        CHECK(s.prefix == 0xABCD000000000000ull && s.remaining == 5);
        const msim_order_stat o = rank_result(RankState{77, 2}, 10, 3);
        CHECK(o.value == 77 && o.below == 8 && o.equal == 3);
    }
    // the layout: counts start on 256 bytes and hold 256 words per (point, column, quantity, rank)
    for (uint32_t nr : {1u, 3u, 32u}) {
        const RankLayout l = rank_layout(1026, 3, nr);
        CHECK(l.counts_at % 32 == 0 && l.words - l.counts_at == (uint64_t)3 * 1026 * 4 * nr * 256);
        CHECK(l.state_at + l.groups * MSIM_MAX_RANKS * 2 <= l.counts_at && l.mask_at + l.groups == l.state_at);
    }

    const uint32_t U = 0xFFFFFFFFu;
    for (uint32_t n : {1u, 2u, 13u, 257u}) {
        // columns: all zero; all equal; f = L; f = 1, s = 2^32 - 1 on some rows; L = 0 on some rows; lowest byte
        // differs; highest non-zero byte differs; strictly increasing
        const uint32_t m = 8;
        std::vector<msim_run_record> rec((size_t)n * m);
        std::vector<uint32_t> bh(n);
        for (uint32_t r = 0; r < n; ++r) {
            bh[r] = r % 5 == 4 ? 0 : 1000 + r;
            rec[(size_t)r * m + 0] = {0, 0};
            rec[(size_t)r * m + 1] = {6, 2};
            rec[(size_t)r * m + 2] = {bh[r], r % 3};
            rec[(size_t)r * m + 3] = {r % 2 ? 1u : 7u, r % 2 ? U : 3u};
            rec[(size_t)r * m + 4] = {5, r % 7};
            rec[(size_t)r * m + 5] = {0x01020300u | (r % 2), 0xA0B0C000u | (r % 3)};
            rec[(size_t)r * m + 6] = {0x01000000u + ((r % 2) << 24), (r % 2 ? 0x80000000u : 0x40000000u)};
            rec[(size_t)r * m + 7] = {r + 1, 2 * r};
        }
        std::vector<uint64_t> ranks = {n / 2, 0, n - 1, 0, n / 2};
        check_case(n, m, rec, bh, ranks);
        ranks.push_back(n);         // a rank that is not below the run count
        ranks.push_back(~0ull);
        check_case(n, m, rec, bh, ranks);
        std::vector<uint64_t> all(MSIM_MAX_RANKS);
        for (uint32_t j = 0; j < MSIM_MAX_RANKS; ++j) all[j] = (uint64_t)(MSIM_MAX_RANKS - 1 - j) * (n - 1) / (MSIM_MAX_RANKS - 1);
        check_case(n, m, rec, bh, all);
    }
    if (failures) {
        printf("rank_check: %d checks failed\n", failures);
        return 1;
    }
    printf("rank_check: ok\n");
    return 0;
}

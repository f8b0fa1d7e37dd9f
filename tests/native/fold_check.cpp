// fold_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_fold.h's host-executed lane body, built
// with -fsanitize=address,undefined and run by tests/test_classes_host.py as a child process. It folds random and
// extreme records (class sums of exactly 2^32 - 1 and of 2^32 + 5, NONE entries, entries outside the map's classes,
// empty classes, an all-NONE map, the identity map) at the tile shapes the launch chooses and at forced small ones,
// and checks every output record against a plain loop written independently here. Exit status 0 = all checks held.
#include <stdio.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_fold.h"

using namespace msim;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("fold_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                         \
        }                                                       \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static void plain(const std::vector<msim_run_record> &rec, uint64_t n, uint32_t m, const std::vector<uint32_t> &map,
                  uint32_t C, std::vector<msim_run_record> &out)
{
    out.assign((size_t)n * C, msim_run_record{0, 0});
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t k = 0; k < m; ++k)
            if (map[k] < C) {
                out[r * C + map[k]].found += rec[r * m + k].found;
                out[r * C + map[k]].stale += rec[r * m + k].stale;
            }
}

static void one(uint64_t n, uint32_t m, const std::vector<uint32_t> &map, uint32_t C, bool big)
{
    std::vector<msim_run_record> rec((size_t)n * m), want, got;
    for (auto &x : rec) x = {big ? rnd() : rnd() % 2000, big ? rnd() : rnd() % 20};
    plain(rec, n, m, map, C, want);
    uint32_t tc, gw;
    fold_plan(m, C, n, &tc, &gw);
    CHECK(tc >= 1 && tc <= C && gw >= 1 && (uint64_t)FOLD_WAVES * gw * tc <= FOLD_POOL);
    CHECK(gw == 1 || (uint64_t)gw * m <= FOLD_SEGMENT_RECORDS);
    // the launch's shape, then forced ones: several class tiles with a partial last one, segments of 2 and 5 runs
    const uint32_t shapes[][2] = {{tc, gw}, {C <= 65 ? 1 : C / 2 + 1, 1}, {C < 3 ? C : 3, 2}, {C, 5}};
    for (const auto &s : shapes) {
        got.assign((size_t)n * C, msim_run_record{0xFFFFFFFFu, 0xFFFFFFFFu});  // the fold overwrites
        fold_host(rec.data(), n, m, map.data(), C, got.data(), s[0], s[1]);
        CHECK(memcmp(got.data(), want.data(), sizeof(msim_run_record) * got.size()) == 0);
    }
}

int main()
{
    for (uint32_t m : {1u, 2u, 9u, 63u, 64u, 65u, 257u, 1026u, 2049u}) {
        for (uint64_t n : {1ull, 5ull, 67ull}) {
            std::vector<uint32_t> ident(m), all(m, 0), none(m, MSIM_CLASS_NONE), mixed(m);
            for (uint32_t k = 0; k < m; ++k) ident[k] = k;
            const uint32_t C = m < 5 ? m : 5;
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t r = rnd() % (C + 2);
                mixed[k] = r < C ? r : (r == C ? MSIM_CLASS_NONE : C + 7);  // outside the map: read as NONE
                if (C > 1 && mixed[k] == 1) mixed[k] = 0;                     // class 1 stays empty
            }
            one(n, m, ident, m, true);
            one(n, m, all, 1, true);
            one(n, m, all, C, false);
            one(n, m, none, C, false);
            one(n, m, mixed, C, true);
        }
    }
    // identity: the output bytes are the input's
    {
        const uint32_t m = 1026;
        std::vector<uint32_t> ident(m);
        for (uint32_t k = 0; k < m; ++k) ident[k] = k;
        std::vector<msim_run_record> rec(3 * m), out(3 * m);
        for (auto &x : rec) x = {rnd(), rnd()};
        fold_host(rec.data(), 3, m, ident.data(), m, out.data(), m, 1);
        CHECK(memcmp(rec.data(), out.data(), sizeof(msim_run_record) * rec.size()) == 0);
    }
    // class sums of exactly 2^32 - 1 (found) and of 2^32 + 5 (stale): the second wraps to 5
    {
        const uint32_t m = 130;
        std::vector<uint32_t> map(m, 0);
        map[7] = MSIM_CLASS_NONE;
        std::vector<msim_run_record> rec(m, msim_run_record{0, 0}), out(2);
        rec[0] = {0xFFFFFF00u, 0xFFFFFFFFu};
        rec[64] = {0xFEu, 3};   // the same lane as record 0
        rec[65] = {1, 3};       // another lane
        rec[7] = {9, 9};        // in no class
        fold_host(rec.data(), 1, m, map.data(), 2, out.data(), 2, 1);
        CHECK(out[0].found == 0xFFFFFFFFu && out[0].stale == 5 && out[1].found == 0 && out[1].stale == 0);
    }
    // map validation
    {
        const uint32_t ok[3] = {0, MSIM_CLASS_NONE, 1}, bad[3] = {0, 2, 1};
        CHECK(fold_map_ok(3, ok, 2) && fold_map_ok(3, ok, 3) && !fold_map_ok(3, bad, 2) && !fold_map_ok(3, ok, 0));
        CHECK(!fold_map_ok(3, ok, 4) && !fold_map_ok(3, nullptr, 2) && !fold_map_ok(0, ok, 1));
        CHECK(fold_column(MSIM_CLASS_NONE, 5, 0, 5) == FOLD_SKIP && fold_column(5, 5, 0, 5) == FOLD_SKIP);
        CHECK(fold_column(4, 5, 3, 2) == 1 && fold_column(2, 5, 3, 2) == FOLD_SKIP && fold_column(3, 5, 0, 3) == FOLD_SKIP);
    }
    if (failures) {
        printf("fold_check: %d checks failed\n", failures);
        return 1;
    }
    printf("fold_check: ok\n");
    return 0;
}

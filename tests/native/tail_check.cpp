// tail_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_tail.h's host code (the item guard, the key,
// the per-run add, the sequential accumulation over a record array, the sides and the means), built with
// -fsanitize=address,undefined and run by tests/test_tail_host.py as a child process. It feeds the extreme records
// of rank_check.cpp (all zero; all equal; f = L; f = 1 with s = 2^32 - 1; L = 0; strictly increasing) with
// thresholds 0, a column's minimum, median and maximum and 2^64 - 1, and checks every word against sums written
// independently here in 128-bit arithmetic. Exit status 0 = all checks held.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../miningsimulation_amd/csrc/msim_tail.h"

using namespace msim;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("tail_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                         \
        }                                                       \
    } while (0)

static uint64_t share_term(uint64_t f, uint64_t L)
{
    return (f == 0 || L == 0) ? 0 : (uint64_t)((double)f / (double)L * 4294967296.0 + 0.5);
}
static uint64_t rate_term(uint64_t f, uint64_t s) { return f == 0 ? 0 : (uint64_t)((double)s / (double)f * 4294967296.0 + 0.5); }

static u128 join(const uint64_t *limb, int n)  // exact while the value stays below 2^128
{
    u128 v = 0;
    for (int i = n - 1; i >= 0; --i) v = (v << 32) + limb[i];
    return v;
}

struct Sums {
    u128 f = 0, s = 0, st = 0, rt = 0, ff = 0, ss = 0, fs = 0;
    uint64_t n = 0;
};

static void check_moments(const msim_moments &mo, const Sums &w)
{
    const uint64_t sh[2] = {mo.first.share_lo, mo.first.share_hi}, rt[2] = {mo.first.rate_lo, mo.first.rate_hi};
    CHECK((u128)(uint64_t)mo.first.blocks_found == w.f && (u128)(uint64_t)mo.first.stale_blocks == w.s);
    CHECK(join(sh, 2) == w.st && join(rt, 2) == w.rt);
    CHECK(join(mo.found_sq, 2) == w.ff && join(mo.stale_sq, 2) == w.ss && join(mo.found_stale, 2) == w.fs);
}

static void check_case(uint32_t np, uint32_t n, uint32_t m, const std::vector<msim_run_record> &rec,
                       const std::vector<uint32_t> &bh, const std::vector<msim_tail_item> &items)
{
    std::vector<msim_tail> out(items.size());
    memset(out.data(), 0xFF, sizeof(msim_tail) * out.size());
    tail_accumulate_host(rec.data(), bh.data(), np, n, m, items.data(), (uint32_t)items.size(), out.data());
    std::vector<msim_moments> total((size_t)np * m);
    for (uint32_t p = 0; p < np; ++p)
        mom_accumulate_host(rec.data() + (size_t)p * n * m, bh.data() + (size_t)p * n, n, m, nullptr, &total[(size_t)p * m],
                            nullptr);
    for (size_t i = 0; i < items.size(); ++i) {
        const msim_tail_item &it = items[i];
        const msim_tail &t = out[i];
        if (!tail_item_ok(it, np, m)) {
            for (uint32_t j = 0; j < TAIL_WORDS; ++j) CHECK(((const uint64_t *)&t)[j] == 0);
            continue;
        }
        Sums below, equal;
        for (uint32_t r = 0; r < n; ++r) {
            const size_t rc = (size_t)it.cond_point * n + r, rt = (size_t)it.target_point * n + r;
            const msim_run_record &c = rec[rc * m + it.cond_column], &x = rec[rt * m + it.target_column];
            const uint64_t key = it.quantity == 0 ? c.found : it.quantity == 1 ? c.stale
                               : it.quantity == 2 ? share_term(c.found, bh[rc]) : rate_term(c.found, c.stale);
            if (key > it.value) continue;
            Sums &w = key < it.value ? below : equal;
            w.n += 1;
            w.f += x.found;
            w.s += x.stale;
            w.st += share_term(x.found, bh[rt]);
            w.rt += rate_term(x.found, x.stale);
            w.ff += (u128)x.found * x.found;
            w.ss += (u128)x.stale * x.stale;
            w.fs += (u128)x.found * x.stale;
        }
        CHECK(t.n_below == below.n && t.n_equal == equal.n);
        check_moments(t.below, below);
        check_moments(t.equal, equal);
        // the four sides: below + equal + above is the total, limb by limb
        const msim_moments &tot = total[(size_t)it.target_point * m + it.target_column];
        msim_moments side[4];
        uint64_t cnt[4];
        for (int s = 0; s < 4; ++s) CHECK(tail_side(&t, &tot, n, s, &side[s], &cnt[s]) == MSIM_OK);
        CHECK(cnt[MSIM_TAIL_BELOW] + t.n_equal == cnt[MSIM_TAIL_AT_MOST] && cnt[MSIM_TAIL_AT_MOST] + cnt[MSIM_TAIL_ABOVE] == n &&
              cnt[MSIM_TAIL_BELOW] + cnt[MSIM_TAIL_AT_LEAST] == n);
        for (uint32_t j = 0; j < MOM_WORDS; ++j) {
            const uint64_t *b = (const uint64_t *)&side[MSIM_TAIL_BELOW], *a = (const uint64_t *)&side[MSIM_TAIL_ABOVE];
            CHECK(b[j] + ((const uint64_t *)&t.equal)[j] + a[j] == ((const uint64_t *)&tot)[j]);
            CHECK(b[j] + ((const uint64_t *)&side[MSIM_TAIL_AT_LEAST])[j] == ((const uint64_t *)&tot)[j]);
        }
        CHECK(tail_side(&t, nullptr, n, MSIM_TAIL_ABOVE, &side[0], &cnt[0]) == MSIM_E_INVALID);
        CHECK(tail_side(&t, &tot, n, 4, &side[0], &cnt[0]) == MSIM_E_INVALID);
        // the means: inside the tie range only; found and stale sums stay below 2^53 here unless s = 2^32 - 1 is
        // among them, so one double division of the exact numerator and denominator is the correctly rounded mean
        double mu[4];
        CHECK(tail_means(&t, &tot, n, t.n_below, 0, mu) == MSIM_E_INVALID);
        CHECK(tail_means(&t, &tot, n, t.n_below + t.n_equal + 1, 0, mu) == MSIM_E_INVALID);
        for (uint64_t k = t.n_below + 1; k <= t.n_below + t.n_equal; k += (t.n_equal > 3 ? t.n_equal / 3 : 1)) {
            CHECK(tail_means(&t, &tot, n, k, 0, mu) == MSIM_OK);
            const u128 num = below.f * equal.n + (u128)(k - below.n) * equal.f, den = (u128)k * equal.n;
            if (num < ((u128)1 << 53)) CHECK(mu[0] == (double)(uint64_t)num / (double)(uint64_t)den);
            const long double share = ((long double)below.st * equal.n + (long double)(k - below.n) * (long double)equal.st) /
                                      (long double)den / 4294967296.0L;
            CHECK(fabsl((long double)mu[2] - share) <= 1e-15L * share);
        }
    }
}

int main()
{
    // the key and the guard on their own
    CHECK(tail_key(0, 7, 3, 0) == 7 && tail_key(1, 7, 3, 0) == 3);
    CHECK(tail_key(2, 10, 3, 10) == 1ull << 32 && tail_key(2, 5, 0, 0) == 0);
    CHECK(tail_key(3, 1, 0xFFFFFFFFu, 1) == 0xFFFFFFFF00000000ull && tail_key(3, 0, 9, 1) == 0);
    {
        const msim_tail_item ok = {1, 2, 3, 0, 1, 0, 5};
        CHECK(tail_item_ok(ok, 2, 3));
        msim_tail_item bad = ok;
        bad.cond_point = 2;
        CHECK(!tail_item_ok(bad, 2, 3));
        bad = ok, bad.target_point = 2;
        CHECK(!tail_item_ok(bad, 2, 3));
        bad = ok, bad.cond_column = 3;
        CHECK(!tail_item_ok(bad, 2, 3));
        bad = ok, bad.target_column = 3;
        CHECK(!tail_item_ok(bad, 2, 3));
        bad = ok, bad.quantity = 4;
        CHECK(!tail_item_ok(bad, 2, 3));
        bad = ok, bad.reserved = 1;
        CHECK(!tail_item_ok(bad, 2, 3));
    }
    // the division: correctly rounded where a double division of exact operands is
    {
        const TailWide one = mw_from_u64<8>(1), three = mw_from_u64<8>(3), big = mw_from_u64<8>(0xFFFFFFFFFFFFFFFFull);
        CHECK(mw_div_to_double(one, three) == 1.0 / 3.0);
        CHECK(mw_div_to_double(mw_from_u64<8>(0), three) == 0.0);
        CHECK(mw_div_to_double(mw_mul(big, big), big) == 18446744073709551615.0);
        CHECK(mw_div_to_double(mw_from_u64<8>(1ull << 53 | 1), one) == 9007199254740992.0);       // tie to even
        CHECK(mw_div_to_double(mw_from_u64<8>((1ull << 54) | 2), mw_from_u64<8>(2)) == 9007199254740992.0);
        CHECK(mw_div_to_double(mw_from_u64<8>((1ull << 54) | 6), mw_from_u64<8>(2)) == 9007199254740996.0);
        CHECK(mw_div_to_double(mw_from_u64<8>((1ull << 55) | 5), mw_from_u64<8>(4)) == 9007199254740994.0);  // above a tie
        for (uint64_t a = 1; a < 200; a += 7)
            for (uint64_t b = 1; b < 200; b += 11) CHECK(mw_div_to_double(mw_from_u64<8>(a), mw_from_u64<8>(b)) == (double)a / (double)b);
    }

    const uint32_t U = 0xFFFFFFFFu;
    for (uint32_t np : {1u, 3u})
        for (uint32_t n : {1u, 2u, 13u, 257u}) {
            const uint32_t m = 7;
            std::vector<msim_run_record> rec((size_t)np * n * m);
            std::vector<uint32_t> bh((size_t)np * n);
            for (uint32_t p = 0; p < np; ++p)
                for (uint32_t r = 0; r < n; ++r) {
                    const size_t at = (size_t)p * n + r;
                    bh[at] = r % 5 == 4 ? 0 : 1000 + r + 17 * p;
                    rec[at * m + 0] = {0, 0};
                    rec[at * m + 1] = {6, 2};
                    rec[at * m + 2] = {bh[at], r % 3};
                    rec[at * m + 3] = {r % 2 ? 1u : 7u, r % 2 ? U : 3u};
                    rec[at * m + 4] = {5, r % 7};
                    rec[at * m + 5] = {r + 1 + p, 2 * r};
                    rec[at * m + 6] = {(r * 37 + p) % 11, (r * 13) % 4};
                }
            std::vector<msim_tail_item> items;
            for (uint32_t k = 0; k < m; ++k)
                for (uint32_t q = 0; q < 4; ++q) {
                    std::vector<uint64_t> keys(n);
                    for (uint32_t r = 0; r < n; ++r) keys[r] = tail_key(q, rec[(size_t)r * m + k].found, rec[(size_t)r * m + k].stale, bh[r]);
                    std::sort(keys.begin(), keys.end());
                    const uint64_t thresholds[5] = {0, keys[0], keys[n / 2], keys[n - 1], ~(uint64_t)0};
                    for (uint64_t v : thresholds) {
                        items.push_back({0, k, q, 0, k, 0, v});                        // own column
                        items.push_back({0, k, q, np - 1, (k + 3) % m, 0, v});         // another column, the last point
                    }
                }
            items.push_back({np, 0, 0, 0, 0, 0, 5});  // out of range, among valid neighbours
            items.push_back({0, 0, 4, 0, 0, 0, 5});
            items.push_back({0, 0, 0, 0, m, 0, 5});
            items.push_back({0, 0, 0, 0, 0, 1, 5});
            items.push_back({0, 5, 0, 0, 5, 0, n / 2});
            check_case(np, n, m, rec, bh, items);
        }
    if (failures) {
        printf("tail_check: %d checks failed\n", failures);
        return 1;
    }
    printf("tail_check: ok\n");
    return 0;
}

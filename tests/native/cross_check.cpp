// cross_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_cross.h's host code (the product, the
// accumulation over a record array with out-of-range pairs skipped, and the contrasts at the extremes), built with
// -fsanitize=address,undefined and run by tests/test_cross_host.py as a child process. Sums are checked against
// unsigned __int128 arithmetic written independently here. Exit status 0 = all checks held.
#include <stdio.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_cross.h"

using namespace msim;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("cross_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                          \
        }                                                        \
    } while (0)

static u128 join128(const uint64_t *l, int n)
{
    u128 v = 0;
    for (int i = 0; i < n && i < 4; ++i) v += (u128)l[i] << (32 * i);
    return v;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

static uint64_t share_t(uint64_t f, uint64_t L)
{
    return (f == 0 || L == 0) ? 0 : (uint64_t)((double)f / (double)L * 4294967296.0 + 0.5);
}
static uint64_t rate_t(uint64_t f, uint64_t s) { return f == 0 ? 0 : (uint64_t)((double)s / (double)f * 4294967296.0 + 0.5); }

int main()
{
    // the product against __int128, and the square as its special case
    const uint64_t vals[] = {0, 1, 0xFFFFFFFFull, 1ull << 32, 0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFFull,
                             0x123456789ABCDEFull, 0xFFFFFFFF00000001ull};
    for (uint64_t a : vals)
        for (uint64_t b : vals) {
            uint64_t p[4], q[4];
            cross_mul_pieces(a, b, p);
            CHECK(join128(p, 4) == (u128)a * b && (p[0] | p[1] | p[2] | p[3]) >> 32 == 0);
            cross_mul_pieces(b, a, q);
            CHECK(memcmp(p, q, sizeof(p)) == 0);
            if (a == b) {
                mom_square_pieces(a, q);
                CHECK(memcmp(p, q, sizeof(p)) == 0);
            }
        }

    // two points of three miners over the extreme records; point 1 holds point 0's rows in reverse order
    struct Row {
        uint32_t f, s, L;
    };
    const Row rows[] = {
        {0, 0, 10},          {0, 7, 10},          {5, 0, 0},  {10, 3, 10}, {11, 2, 10},
        {3, 9, 12},          {1, 0xFFFFFFFFu, 1}, {7, 7, 21}, {7, 7, 21},  {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
        {0xFFFFFFFFu, 1, 1}, {2, 0xFFFFFFFFu, 3}, {1, 1, 0xFFFFFFFFu},
    };
    const uint32_t n = sizeof(rows) / sizeof(rows[0]), m = 3, np = 2;
    std::vector<msim_run_record> rec((size_t)np * n * m);
    std::vector<uint32_t> bh((size_t)np * n);
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t r = 0; r < n; ++r) {
            const Row &x = rows[p ? n - 1 - r : r];
            rec[((size_t)p * n + r) * m + 0] = {x.f, x.s};
            rec[((size_t)p * n + r) * m + 1] = {6, 2};
            rec[((size_t)p * n + r) * m + 2] = {0, 0};
            bh[(size_t)p * n + r] = x.L;
        }
    const msim_pair pairs[] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 1, 0}, {2, 0, 0, 0}, {0, 1, 0, 0}, {0, 3, 0, 0},
                               {1, 1, 1, 0}, {0, 0, 0, 0xFFFFFFFFu}, {1, 0, 1, 0}, {0, 2, 1, 0}, {0, 0, 2, 0}};
    const uint32_t nq = sizeof(pairs) / sizeof(pairs[0]);
    std::vector<msim_cross> cr(nq);
    memset(cr.data(), 0xFF, sizeof(msim_cross) * nq);
    cross_accumulate_host(rec.data(), bh.data(), np, n, m, pairs, nq, cr.data());
    for (uint32_t i = 0; i < nq; ++i) {
        const msim_pair &q = pairs[i];
        const bool ok = q.point_a < np && q.point_b < np && q.miner_a < m && q.miner_b < m;
        CHECK(cross_pair_ok(q, np, m) == ok);
        u128 ff = 0, ss = 0, sh = 0, rt = 0;
        uint32_t sh_c = 0, rt_c = 0;  // carries out of 128 bits
        for (uint32_t r = 0; ok && r < n; ++r) {
            const size_t ra = (size_t)q.point_a * n + r, rb = (size_t)q.point_b * n + r;
            const msim_run_record a = rec[ra * m + q.miner_a], b = rec[rb * m + q.miner_b];
            ff += (u128)a.found * b.found, ss += (u128)a.stale * b.stale;
            const u128 x = (u128)share_t(a.found, bh[ra]) * share_t(b.found, bh[rb]);
            const u128 y = (u128)rate_t(a.found, a.stale) * rate_t(b.found, b.stale);
            sh += x, sh_c += sh < x, rt += y, rt_c += rt < y;
        }
        const msim_cross &x = cr[i];
        CHECK(join128(x.found_found, 2) == ff && join128(x.stale_stale, 2) == ss);
        const CrossWide js = cw_join(x.share_share, 4), jr = cw_join(x.rate_rate, 4);
        CHECK(join128(x.share_share, 4) == sh && js.w[4] == sh_c && js.w[5] == 0);
        CHECK(join128(x.rate_rate, 4) == rt && jr.w[4] == rt_c && jr.w[5] == 0);
        if (!ok)
            for (uint32_t j = 0; j < CROSS_WORDS; ++j) CHECK(((const uint64_t *)&x)[j] == 0);
    }
    CHECK(memcmp(&cr[1], &cr[2], sizeof(msim_cross)) == 0);  // (a, b) and (b, a)

    // a self pair is the column's four square sums of msim_moments
    std::vector<msim_moments> mo((size_t)np * m);
    for (uint32_t p = 0; p < np; ++p)
        mom_accumulate_host(rec.data() + (size_t)p * n * m, bh.data() + (size_t)p * n, n, m, nullptr, mo.data() + p * m,
                            nullptr);
    CHECK(memcmp(cr[0].found_found, mo[0].found_sq, 16) == 0 && memcmp(cr[0].stale_stale, mo[0].stale_sq, 16) == 0);
    CHECK(memcmp(cr[0].share_share, mo[0].share_sq, 32) == 0 && memcmp(cr[0].rate_rate, mo[0].rate_sq, 32) == 0);
    CHECK(memcmp(cr[8].share_share, mo[m].share_sq, 32) == 0 && memcmp(cr[8].rate_rate, mo[m].rate_sq, 32) == 0);

    // contrasts on the in-range pairs
    const msim_pair good[] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 1, 0}, {0, 1, 0, 0}, {1, 1, 0, 1}, {0, 0, 0, 2}, {0, 2, 0, 0}};
    const uint32_t ng = sizeof(good) / sizeof(good[0]);
    std::vector<msim_cross> gc(ng);
    cross_accumulate_host(rec.data(), bh.data(), np, n, m, good, ng, gc.data());
    std::vector<msim_contrast> c(ng), c2(ng);
    cross_to_contrasts(mo.data(), m, good, gc.data(), ng, n, c.data());
    // a column against itself: no difference, correlation one, ratio one
    CHECK(c[0].found_diff == 0.0 && c[0].found_diff_se == 0.0 && c[0].share_diff_se == 0.0 && c[0].rate_diff_se == 0.0);
    CHECK(c[0].found_corr == 1.0 && c[0].share_corr == 1.0 && c[0].found_ratio == 1.0 && c[0].found_ratio_se == 0.0);
    // (a, b) against (b, a): the difference changes sign, its error and the correlation stay
    CHECK(c[1].found_diff == -c[2].found_diff && c[1].share_diff == -c[2].share_diff);
    CHECK(same_bits(c[1].share_diff_se, c[2].share_diff_se) && same_bits(c[1].rate_corr, c[2].rate_corr));
    CHECK(c[1].found_diff == 0.0 && c[1].found_diff_se > 0.0);  // the same rows in another order
    // a constant side: no correlation; both constant: a constant difference
    CHECK(isnan(c[3].found_corr) && isnan(c[3].stale_corr) && c[3].found_diff_se > 0.0);
    CHECK(c[4].found_diff == 0.0 && c[4].found_diff_se == 0.0 && isnan(c[4].found_corr) && c[4].found_ratio == 1.0);
    // B == 0: no ratio; A == 0 over B: ratio zero
    CHECK(isnan(c[5].found_ratio) && isnan(c[5].found_ratio_se) && isnan(c[5].share_ratio) && isnan(c[5].share_ratio_se));
    CHECK(c[6].found_ratio == 0.0 && c[6].share_ratio == 0.0 && c[6].found_diff < 0.0);
    // the 2^64 - 2^32 terms: the ratio's numerator passes 2^256 here and stays finite and positive
    CHECK(c[1].share_ratio_se > 0.0 && c[1].share_ratio_se < 1e30 && c[2].share_ratio_se > 0.0);
    // widths at the ABI's limit: N = 2^32 - 1 runs of the largest term on both sides, one run short on side a
    {
        const uint64_t N = 0xFFFFFFFFull, T = 0xFFFFFFFF00000000ull;
        msim_moments w[2];
        memset(w, 0, sizeof(w));
        uint64_t p[4];
        cross_mul_pieces(T, T, p);
        for (int k = 0; k < 2; ++k) {
            const uint64_t cnt = k ? N : N - 1;
            w[k].first.share_hi = (T >> 32) * cnt;
            for (int i = 0; i < 4; ++i) w[k].share_sq[i] = p[i] * cnt;
        }
        msim_cross x;
        memset(&x, 0, sizeof(x));
        for (int i = 0; i < 4; ++i) x.share_share[i] = p[i] * (N - 1);
        const msim_pair q = {0, 0, 0, 1};
        msim_contrast o;
        cross_to_contrasts(w, 2, &q, &x, 1, N, &o);
        // a_i = T except one 0, b_i = T: the difference is -T / N; sum (B a_i - A b_i)^2 = T^4 N (N - 1)
        CHECK(o.share_diff == -((double)T / (double)N * 0x1.0p-32));
        const double want = sqrt((double)N * (double)N * (double)(N - 1) * pow((double)T, 4) / (double)(N - 1)) /
                            (pow((double)T, 2) * (double)N * (double)N);
        CHECK(fabs(o.share_ratio_se / want - 1.0) < 1e-12);
        CHECK(o.share_ratio == (double)(N - 1) / (double)N);
    }
    // renormalised limbs give the same bits
    std::vector<msim_cross> norm(gc);
    std::vector<msim_moments> mnorm(mo);
    auto carry = [](uint64_t *l, int cnt) {
        for (int i = 0; i + 1 < cnt; ++i) {
            l[i + 1] += l[i] >> 32;
            l[i] &= 0xFFFFFFFFull;
        }
    };
    for (auto &x : norm) carry(x.found_found, 2), carry(x.stale_stale, 2), carry(x.share_share, 4), carry(x.rate_rate, 4);
    for (auto &x : mnorm) {
        carry(x.found_sq, 2), carry(x.stale_sq, 2), carry(x.share_sq, 4), carry(x.rate_sq, 4);
        x.first.share_hi += x.first.share_lo >> 32, x.first.share_lo &= 0xFFFFFFFFull;
        x.first.rate_hi += x.first.rate_lo >> 32, x.first.rate_lo &= 0xFFFFFFFFull;
    }
    cross_to_contrasts(mnorm.data(), m, good, norm.data(), ng, n, c2.data());
    for (uint32_t i = 0; i < ng; ++i) {
        const double *a = &c[i].found_diff, *b = &c2[i].found_diff;
        for (int j = 0; j < 16; ++j) CHECK(same_bits(a[j], b[j]));
    }
    // one run: every error and correlation is NaN, differences and ratios are not
    for (uint32_t p = 0; p < np; ++p)
        mom_accumulate_host(rec.data() + (size_t)p * n * m + 3 * m, bh.data() + (size_t)p * n + 3, 1, m, nullptr,
                            mo.data() + p * m, nullptr);
    const msim_pair one = {0, 0, 0, 1};
    msim_cross oc;
    cross_accumulate_host(rec.data() + 3 * m, bh.data() + 3, 1, 1, m, &one, 1, &oc);
    msim_contrast o;
    cross_to_contrasts(mo.data(), m, &one, &oc, 1, 1, &o);
    CHECK(isnan(o.found_diff_se) && isnan(o.found_corr) && isnan(o.found_ratio_se) && isnan(o.share_diff_se) &&
          isnan(o.rate_diff_se) && isnan(o.rate_corr) && isnan(o.stale_corr) && isnan(o.share_ratio_se));
    CHECK(o.found_diff == 4.0 && o.found_ratio == 10.0 / 6.0);
    if (failures) {
        printf("cross_check: %d checks failed\n", failures);
        return 1;
    }
    printf("cross_check: ok\n");
    return 0;
}

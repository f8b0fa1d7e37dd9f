// moments_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over msim_moments.h's host code (the accumulation
// over a record array, the fixed-width unsigned helper and the error bars), built with
// -fsanitize=address,undefined and run by tests/test_moments_host.py as a child process. It feeds the extreme
// records (f = 0; L = 0 with f > 0; f = L; f = L + 1; s > f; f = 1 with s = 2^32 - 1; all-equal rows) and checks
// every sum against unsigned __int128 arithmetic written independently here. Exit status 0 = all checks held.
#include <stdio.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_moments.h"

using namespace msim;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("moments_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

// value of n unnormalised limbs modulo 2^128
static u128 join128(const uint64_t *l, int n)
{
    u128 v = 0;
    for (int i = 0; i < n && i < 4; ++i) v += (u128)l[i] << (32 * i);
    return v;
}

static u128 wide128(const MomWide &a)
{
    u128 v = 0;
    for (int i = 3; i >= 0; --i) v = (v << 32) | a.w[i];
    return v;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

int main()
{
    struct Row {
        uint32_t f, s, L;
    };
    const Row rows[] = {
        {0, 0, 10},           {0, 7, 10},          {5, 0, 0},          {10, 3, 10},         {11, 2, 10},
        {3, 9, 12},           {1, 0xFFFFFFFFu, 1}, {7, 7, 21},         {7, 7, 21},          {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
        {0xFFFFFFFFu, 1, 1},  {2, 0xFFFFFFFFu, 3}, {1, 1, 0xFFFFFFFFu},
    };
    const uint32_t n = sizeof(rows) / sizeof(rows[0]);
    const uint32_t m = 3;  // miner 0: the rows; miner 1: all-equal rows; miner 2: all zero
    std::vector<msim_run_record> rec((size_t)n * m);
    std::vector<uint32_t> bh(n);
    for (uint32_t r = 0; r < n; ++r) {
        rec[r * m + 0] = {rows[r].f, rows[r].s};
        rec[r * m + 1] = {6, 2};
        rec[r * m + 2] = {0, 0};
        bh[r] = rows[r].L;
    }
    msim_hist_spec spec = {8, 29, 30, 1u << 20, 0};
    std::vector<msim_moments> mo(m);
    std::vector<uint64_t> hist((size_t)m * 2 * (spec.bins + 2));
    mom_accumulate_host(rec.data(), bh.data(), n, m, &spec, mo.data(), hist.data());

    for (uint32_t k = 0; k < m; ++k) {
        u128 f1 = 0, s1 = 0, sh1 = 0, rt1 = 0, ff = 0, ss = 0, fs = 0, sh2 = 0, rt2 = 0;
        uint32_t sh2_c = 0, rt2_c = 0;  // carries out of 128 bits: sum t^2 can pass 2^128
        std::vector<uint64_t> hs(spec.bins + 2, 0), hr(spec.bins + 2, 0);
        for (uint32_t r = 0; r < n; ++r) {
            const uint64_t f = rec[r * m + k].found, s = rec[r * m + k].stale, L = bh[r];
            const uint64_t st = (f == 0 || L == 0) ? 0 : (uint64_t)((double)f / (double)L * 4294967296.0 + 0.5);
            const uint64_t rt = f == 0 ? 0 : (uint64_t)((double)s / (double)f * 4294967296.0 + 0.5);
            f1 += f, s1 += s, sh1 += st, rt1 += rt;
            ff += (u128)f * f, ss += (u128)s * s, fs += (u128)f * s;
            const u128 a = (u128)st * st, b = (u128)rt * rt;
            sh2 += a, sh2_c += sh2 < a, rt2 += b, rt2_c += rt2 < b;
            auto bin = [&](uint64_t t, uint64_t lo, uint32_t sh) -> uint32_t {
                if (t < lo) return 0;
                return ((t - lo) >> sh) >= spec.bins ? spec.bins + 1 : 1 + (uint32_t)((t - lo) >> sh);
            };
            hs[bin(st, spec.share_lo, spec.share_shift)]++;
            hr[bin(rt, spec.rate_lo, spec.rate_shift)]++;
        }
        const msim_moments &x = mo[k];
        CHECK((u128)x.first.blocks_found == f1 && (u128)x.first.stale_blocks == s1);
        CHECK((((u128)x.first.share_hi << 32) + x.first.share_lo) == sh1);
        CHECK((((u128)x.first.rate_hi << 32) + x.first.rate_lo) == rt1);
        CHECK(join128(x.found_sq, 2) == ff && join128(x.stale_sq, 2) == ss && join128(x.found_stale, 2) == fs);
        // the helper joins the same limbs to the same value, carries past 2^128 included
        const MomWide js = mw_join(x.share_sq, 4), jr = mw_join(x.rate_sq, 4);
        CHECK(join128(x.share_sq, 4) == sh2 && wide128(js) == sh2 && js.w[4] == sh2_c && js.w[5] == 0);
        CHECK(join128(x.rate_sq, 4) == rt2 && wide128(jr) == rt2 && jr.w[4] == rt2_c && jr.w[5] == 0);
        CHECK(wide128(mw_join(x.found_sq, 2)) == ff && wide128(mw_join(x.found_stale, 2)) == fs);
        uint64_t tot_s = 0, tot_r = 0;
        for (uint32_t b = 0; b < spec.bins + 2; ++b) {
            CHECK(hist[((size_t)k * 2 + 0) * (spec.bins + 2) + b] == hs[b]);
            CHECK(hist[((size_t)k * 2 + 1) * (spec.bins + 2) + b] == hr[b]);
            tot_s += hs[b], tot_r += hr[b];
        }
        CHECK(tot_s == n && tot_r == n);
    }
    // f = L gives 2^32 (square 2^64: piece 2 set), f = 1 with s = 2^32 - 1 gives 2^64 - 2^32
    CHECK(mom_share_term(10, 10) == 1ull << 32);
    CHECK(mom_rate_term(1, 0xFFFFFFFFu) == 0xFFFFFFFF00000000ull);
    uint64_t p[4];
    mom_square_pieces(1ull << 32, p);
    CHECK(p[0] == 0 && p[1] == 0 && p[2] == 1 && p[3] == 0);
    mom_square_pieces(0xFFFFFFFFFFFFFFFFull, p);
    CHECK(p[0] == 1 && p[1] == 0 && p[2] == 0xFFFFFFFEull && p[3] == 0xFFFFFFFFull);

    // the helper against __int128
    {
        const MomWide a = mw_from_u64(0xFFFFFFFFFFFFFFFFull), b = mw_from_u64(0xFFFFFFFF00000001ull);
        const u128 pa = (u128)0xFFFFFFFFFFFFFFFFull * 0xFFFFFFFF00000001ull;
        CHECK(wide128(mw_mul(a, b)) == pa);
        CHECK(wide128(mw_sub(mw_mul(a, a), mw_mul(a, b))) == (u128)0xFFFFFFFFFFFFFFFFull * 0xFFFFFFFFFFFFFFFFull - pa);
        CHECK(wide128(mw_add(a, b)) == (u128)0xFFFFFFFFFFFFFFFFull + 0xFFFFFFFF00000001ull);
        CHECK(mw_cmp(a, b) > 0 && mw_cmp(b, a) < 0 && mw_cmp(a, a) == 0);
        const MomWide big = mw_mul(mw_mul(a, a), mw_mul(a, a));  // (2^64 - 1)^4
        CHECK(mw_to_double(big) == 0x1.0p256);
        CHECK(mw_to_double(mw_from_u64((1ull << 53) + 1)) == 0x1.0p53);  // tie to even
        // 2^100 + 2^47 is a tie (half an ulp of 2^48): even is down; one more bit far below breaks it upwards
        MomWide t = mw_add(mw_mul(mw_from_u64(1ull << 50), mw_from_u64(1ull << 50)), mw_from_u64(1ull << 47));
        CHECK(mw_to_double(t) == 0x1.0p100);
        CHECK(mw_to_double(mw_add(t, mw_from_u64(1))) == 0x1.0000000000001p100);
    }

    // error bars: a constant series has se == 0 exactly, N == 1 gives NaN, renormalised limbs the same bits
    std::vector<msim_errors> e(m), e2(m);
    mom_to_errors(mo.data(), m, n, e.data());
    CHECK(e[1].found_se == 0.0 && e[1].rate_se == 0.0 && e[1].pooled_rate_se == 0.0);  // its share varies with L
    {
        std::vector<uint32_t> same(n, 18);
        std::vector<msim_moments> mc(m);
        mom_accumulate_host(rec.data(), same.data(), n, m, nullptr, mc.data(), nullptr);
        mom_to_errors(mc.data(), m, n, e2.data());
        CHECK(e2[1].share_se == 0.0 && e2[1].found_se == 0.0 && e2[1].share_mean == (double)mom_share_term(6, 18) * 0x1.0p-32);
    }
    CHECK(e[1].found_mean == 6.0 && e[1].pooled_rate == 2.0 / 6.0);
    CHECK(e[2].found_mean == 0.0 && e[2].pooled_rate == 0.0 && e[2].pooled_rate_se == 0.0 && e[2].share_se == 0.0);
    CHECK(e[0].found_se > 0.0 && e[0].share_se > 0.0 && e[0].rate_se > 0.0 && e[0].pooled_rate_se > 0.0);
    std::vector<msim_moments> norm(mo);
    for (uint32_t k = 0; k < m; ++k) {
        msim_moments &x = norm[k];
        auto carry = [](uint64_t *l, int cnt) {
            for (int i = 0; i + 1 < cnt; ++i) {
                l[i + 1] += l[i] >> 32;
                l[i] &= 0xFFFFFFFFull;
            }
        };
        carry(x.found_sq, 2), carry(x.stale_sq, 2), carry(x.found_stale, 2), carry(x.share_sq, 4), carry(x.rate_sq, 4);
        x.first.share_hi += x.first.share_lo >> 32, x.first.share_lo &= 0xFFFFFFFFull;
        x.first.rate_hi += x.first.rate_lo >> 32, x.first.rate_lo &= 0xFFFFFFFFull;
    }
    mom_to_errors(norm.data(), m, n, e2.data());
    for (uint32_t k = 0; k < m; ++k) {
        const double *a = &e[k].found_mean, *b = &e2[k].found_mean;
        for (int i = 0; i < 8; ++i) CHECK(same_bits(a[i], b[i]));
    }
    mom_accumulate_host(rec.data(), bh.data(), 1, m, nullptr, mo.data(), nullptr);
    mom_to_errors(mo.data(), m, 1, e.data());
    for (uint32_t k = 0; k < m; ++k)
        CHECK(isnan(e[k].found_se) && isnan(e[k].share_se) && isnan(e[k].rate_se) && isnan(e[k].pooled_rate_se));
    if (failures) {
        printf("moments_check: %d checks failed\n", failures);
        return 1;
    }
    printf("moments_check: ok\n");
    return 0;
}

// msim_moments.h — per-miner second moments and histograms of the per-run terms (include/msim.h: msim_moments,
// msim_hist_spec, msim_errors). Everything here is exact integer arithmetic on the terms every engine adds to
// its msim_sums (msim_wide.hip W3, msim_general.hip, msim_kernels.hip):
//   share_t = (f == 0 || L == 0) ? 0 : (uint64)((double)f / (double)L * 2^32 + 0.5)
//   rate_t  = (f == 0)           ? 0 : (uint64)((double)s / (double)f * 2^32 + 0.5)
// with f = record.found, s = record.stale, L = best_height[run]; one correctly rounded f64 division each
// (the library is built with -ffp-contract=off). The L == 0 guard only matters for a miner holding Genesis's
// id in a run without blocks, where the engines' own share term (f / 0) has no value.
//
// The term, square and bin functions are __host__ __device__: the gfx950 reduction kernel (msim_moments.hip),
// the host accumulation below (tests/native/moments_host.cpp, tests/native/moments_check.cpp) and
// msim_moments_to_errors all run the same lines.
#ifndef MSIM_MOMENTS_H
#define MSIM_MOMENTS_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/msim.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define MSIM_MHD __host__ __device__ inline
#else
#define MSIM_MHD inline
#endif

namespace msim {

constexpr uint32_t MOM_WORDS = 20;       // uint64 fields of msim_moments
constexpr uint32_t MOM_MAX_BINS = 1024;  // msim_hist_spec.bins

MSIM_MHD uint64_t mom_share_term(uint32_t f, uint32_t L)
{
    if (f == 0 || L == 0) return 0;
    return (uint64_t)((double)f / (double)L * 4294967296.0 + 0.5);
}

MSIM_MHD uint64_t mom_rate_term(uint32_t f, uint32_t s)
{
    if (f == 0) return 0;
    return (uint64_t)((double)s / (double)f * 4294967296.0 + 0.5);
}

// t * t as four 32-bit pieces (p[0] lowest), from the three 64-bit partial products of t's halves.
MSIM_MHD void mom_square_pieces(uint64_t t, uint64_t p[4])
{
    const uint64_t M = 0xFFFFFFFFull;
    const uint64_t a = t >> 32, b = t & M;
    const uint64_t lo = b * b, mid = a * b, hi = a * a;
    uint64_t c = (lo >> 32) + 2 * (mid & M);  // < 2^34
    p[0] = lo & M;
    p[1] = c & M;
    c = (c >> 32) + 2 * (mid >> 32) + (hi & M);  // < 2^35
    p[2] = c & M;
    p[3] = (c >> 32) + (hi >> 32);  // < 2^32: t * t < 2^128
}

// msim_hist_spec's bin of a term: 0 below lo, bins + 1 at or past lo + bins << shift.
MSIM_MHD uint32_t mom_bin(uint64_t t, uint64_t lo, uint32_t shift, uint32_t bins)
{
    if (t < lo) return 0;
    const uint64_t q = shift >= 64 ? 0 : (t - lo) >> shift;
    return q >= bins ? bins + 1 : 1 + (uint32_t)q;
}

// One run's contribution of one miner to the 20 words of its msim_moments, in field order.
MSIM_MHD void mom_add_run(uint64_t w[MOM_WORDS], uint32_t f, uint32_t s, uint64_t st, uint64_t rt)
{
    const uint64_t M = 0xFFFFFFFFull;
    uint64_t p[4];
    w[0] += f;
    w[1] += s;
    w[2] += st >> 32;
    w[3] += st & M;
    w[4] += rt >> 32;
    w[5] += rt & M;
    const uint64_t ff = (uint64_t)f * f, ss = (uint64_t)s * s, fs = (uint64_t)f * s;
    w[6] += ff & M;
    w[7] += ff >> 32;
    w[8] += ss & M;
    w[9] += ss >> 32;
    w[10] += fs & M;
    w[11] += fs >> 32;
    mom_square_pieces(st, p);
    w[12] += p[0];
    w[13] += p[1];
    w[14] += p[2];
    w[15] += p[3];
    mom_square_pieces(rt, p);
    w[16] += p[0];
    w[17] += p[1];
    w[18] += p[2];
    w[19] += p[3];
}

// ---------------------------------------------------------------- host: accumulation over a record array
// records [n_runs][m]{found, stale}, best_height [n_runs]; out: m msim_moments (overwritten); hist (or NULL):
// [m][2][bins + 2] counts (overwritten). What the kernel computes, sequentially.
inline void mom_accumulate_host(const msim_run_record *rec, const uint32_t *best_height, uint64_t n_runs, uint32_t m,
                                const msim_hist_spec *spec, msim_moments *out, uint64_t *hist)
{
    static_assert(sizeof(msim_moments) == MOM_WORDS * sizeof(uint64_t), "msim_moments is 20 uint64");
    memset(out, 0, sizeof(msim_moments) * m);
    const uint32_t row = spec ? spec->bins + 2 : 0;
    if (hist && spec) memset(hist, 0, sizeof(uint64_t) * 2 * row * (size_t)m);
    for (uint64_t r = 0; r < n_runs; ++r)
        for (uint32_t k = 0; k < m; ++k) {
            const msim_run_record &x = rec[r * m + k];
            const uint64_t st = mom_share_term(x.found, best_height[r]);
            const uint64_t rt = mom_rate_term(x.found, x.stale);
            mom_add_run((uint64_t *)&out[k], x.found, x.stale, st, rt);
            if (hist && spec) {
                hist[((size_t)k * 2 + 0) * row + mom_bin(st, spec->share_lo, spec->share_shift, spec->bins)] += 1;
                hist[((size_t)k * 2 + 1) * row + mom_bin(rt, spec->rate_lo, spec->rate_shift, spec->bins)] += 1;
            }
        }
}

// ---------------------------------------------------------------- host: fixed-width unsigned integers
// MomWide, 384 bits: the widest numerator below, F^2 * sum(s^2) + S^2 * sum(f^2) with F, S < 2^64 and the square
// sums < 2^97, stays under 2^226; N * (that) under 2^258. The helpers take any limb count (msim_cross.h needs
// more); results are exact integers, so they do not depend on it.
template <int LIMBS>
struct WideU {
    static constexpr int W = LIMBS;  // 32-bit limbs
    uint32_t w[W];
};
using MomWide = WideU<12>;

template <int W = MomWide::W>
inline WideU<W> mw_from_u64(uint64_t x)
{
    WideU<W> r;
    memset(&r, 0, sizeof(r));
    r.w[0] = (uint32_t)x;
    r.w[1] = (uint32_t)(x >> 32);
    return r;
}

template <int W>
inline WideU<W> mw_add(const WideU<W> &a, const WideU<W> &b)
{
    WideU<W> r;
    uint64_t c = 0;
    for (int i = 0; i < W; ++i) {
        c += (uint64_t)a.w[i] + b.w[i];
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}

// a - b for a >= b
template <int W>
inline WideU<W> mw_sub(const WideU<W> &a, const WideU<W> &b)
{
    WideU<W> r;
    uint64_t borrow = 0;
    for (int i = 0; i < W; ++i) {
        const uint64_t d = (uint64_t)a.w[i] - b.w[i] - borrow;
        r.w[i] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
    return r;
}

template <int W>
inline int mw_cmp(const WideU<W> &a, const WideU<W> &b)
{
    for (int i = W - 1; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

// a * b, truncated to the type's width (no product below comes near)
template <int W>
inline WideU<W> mw_mul(const WideU<W> &a, const WideU<W> &b)
{
    WideU<W> r;
    memset(&r, 0, sizeof(r));
    for (int i = 0; i < W; ++i) {
        if (a.w[i] == 0) continue;
        uint64_t c = 0;
        for (int j = 0; i + j < W; ++j) {
            c += (uint64_t)a.w[i] * b.w[j] + r.w[i + j];
            r.w[i + j] = (uint32_t)c;
            c >>= 32;
        }
    }
    return r;
}

// sum(limb[i] << 32 i) of n unnormalised 64-bit limbs
template <int W = MomWide::W>
inline WideU<W> mw_join(const uint64_t *limb, int n)
{
    WideU<W> r;
    memset(&r, 0, sizeof(r));
    for (int i = 0; i < n; ++i) {
        uint64_t c = (uint32_t)limb[i];
        uint64_t h = limb[i] >> 32;
        for (int j = i; j < W && (c || h); ++j) {
            c += r.w[j];
            r.w[j] = (uint32_t)c;
            c = (c >> 32) + h;
            h = 0;
        }
    }
    return r;
}

template <int W>
inline bool mw_is_zero(const WideU<W> &a)
{
    for (int i = 0; i < W; ++i)
        if (a.w[i]) return false;
    return true;
}

// the nearest double (ties to even): the top 64 bits, with the bits below them folded into a sticky bit,
// convert with one rounding; the scaling by a power of two is exact.
template <int W>
inline double mw_to_double(const WideU<W> &a)
{
    int top = W - 1;
    while (top >= 0 && a.w[top] == 0) --top;
    if (top < 0) return 0.0;
    if (top <= 1) return (double)(((uint64_t)(top == 1 ? a.w[1] : 0) << 32) | a.w[0]);
    int lz = 0;
    while (!((a.w[top] << lz) & 0x80000000u)) ++lz;
    // bits [hb - 63, hb] with hb = 32 top + 31 - lz
    const int lowbit = 32 * top + 31 - lz - 63;
    uint64_t v = 0;
    for (int b = 63; b >= 0; --b) {
        const int pos = lowbit + b;
        v = (v << 1) | ((a.w[pos >> 5] >> (pos & 31)) & 1u);
    }
    bool sticky = false;
    for (int pos = 0; pos < lowbit && !sticky; ++pos) sticky = (a.w[pos >> 5] >> (pos & 31)) & 1u;
    // v has its top bit set, so the double keeps bits 63..11; bit 0 is far below the rounding bit and can
    // carry the sticky information without changing a tie that the lower bits do not break
    if (sticky) v |= 1u;
    return ldexp((double)v, lowbit);
}

// sqrt((N * S2 - S1^2) / (N^2 (N - 1))) * scale; NaN for N == 1
inline double mom_se(const MomWide &s1, const MomWide &s2, uint64_t n, double scale)
{
    if (n < 2) return NAN;
    const MomWide N = mw_from_u64(n);
    const MomWide a = mw_mul(N, s2), b = mw_mul(s1, s1);
    if (mw_cmp(a, b) <= 0) return 0.0;  // equal for a constant series (Cauchy-Schwarz: never below)
    const double num = mw_to_double(mw_sub(a, b));
    const double den = mw_to_double(mw_mul(mw_mul(N, N), mw_from_u64(n - 1)));
    return sqrt(num / den) * scale;
}

inline void mom_to_errors(const msim_moments *mo, uint32_t m, uint64_t n_runs, msim_errors *out)
{
    const double q = 0x1.0p-32;
    const double nd = (double)n_runs;
    for (uint32_t k = 0; k < m; ++k) {
        const msim_moments &x = mo[k];
        msim_errors &e = out[k];
        const MomWide F = mw_from_u64((uint64_t)x.first.blocks_found), S = mw_from_u64((uint64_t)x.first.stale_blocks);
        const uint64_t sh[2] = {x.first.share_lo, x.first.share_hi}, rt[2] = {x.first.rate_lo, x.first.rate_hi};
        const MomWide SH = mw_join(sh, 2), RT = mw_join(rt, 2);
        const MomWide FF = mw_join(x.found_sq, 2), SS = mw_join(x.stale_sq, 2), FS = mw_join(x.found_stale, 2);
        const MomWide SH2 = mw_join(x.share_sq, 4), RT2 = mw_join(x.rate_sq, 4);
        e.found_mean = mw_to_double(F) / nd;
        e.found_se = mom_se(F, FF, n_runs, 1.0);
        e.share_mean = mw_to_double(SH) / nd * q;
        e.share_se = mom_se(SH, SH2, n_runs, q);
        e.rate_mean = mw_to_double(RT) / nd * q;
        e.rate_se = mom_se(RT, RT2, n_runs, q);
        if (mw_is_zero(F)) {
            e.pooled_rate = 0.0;
            e.pooled_rate_se = n_runs < 2 ? NAN : 0.0;
            continue;
        }
        const double fd = mw_to_double(F);
        e.pooled_rate = mw_to_double(S) / fd;
        if (n_runs < 2) {
            e.pooled_rate_se = NAN;
            continue;
        }
        // delta method: N / (N - 1) * sum (F s_i - S f_i)^2 = N / (N - 1) * (F^2 sum s^2 - 2 S F sum fs + S^2 sum f^2)
        const MomWide pos = mw_add(mw_mul(mw_mul(F, F), SS), mw_mul(mw_mul(S, S), FF));
        const MomWide sf = mw_mul(mw_mul(S, F), FS);
        const MomWide neg = mw_add(sf, sf);
        if (mw_cmp(pos, neg) <= 0) {
            e.pooled_rate_se = 0.0;
            continue;
        }
        const double num = mw_to_double(mw_mul(mw_from_u64(n_runs), mw_sub(pos, neg)));
        e.pooled_rate_se = sqrt(num / (double)(n_runs - 1)) / mw_to_double(mw_mul(F, F));
    }
}
}  // namespace msim

#endif  // MSIM_MOMENTS_H

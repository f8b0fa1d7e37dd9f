// msim_cross.h — paired contrasts between two (point, miner) columns of one launch's records (include/msim.h:
// msim_pair, msim_cross, msim_contrast). The terms are msim_moments.h's (mom_share_term, mom_rate_term), taken
// from each side's record and its own point's best height; a pair's twelve words are the exact integer sums over
// runs of the sides' products, in msim_moments' limb convention.
//
// The product, the per-run add and the pair guard are __host__ __device__: the gfx950 reduction kernel
// (msim_cross.hip), the host accumulation below (tests/native/cross_host.cpp, tests/native/cross_check.cpp) and
// msim_cross_to_contrasts all run the same lines.
#ifndef MSIM_CROSS_H
#define MSIM_CROSS_H

#include "msim_moments.h"

namespace msim {

constexpr uint32_t CROSS_WORDS = 12;  // uint64 fields of msim_cross

// a * b as four 32-bit pieces (p[0] lowest), from the four 64-bit partial products of the halves.
// mom_square_pieces(t) is the case a == b == t.
MSIM_MHD void cross_mul_pieces(uint64_t a, uint64_t b, uint64_t p[4])
{
    const uint64_t M = 0xFFFFFFFFull;
    const uint64_t a1 = a >> 32, a0 = a & M, b1 = b >> 32, b0 = b & M;
    const uint64_t ll = a0 * b0, lh = a0 * b1, hl = a1 * b0, hh = a1 * b1;
    uint64_t c = (ll >> 32) + (lh & M) + (hl & M);  // < 3 * 2^32
    p[0] = ll & M;
    p[1] = c & M;
    c = (c >> 32) + (lh >> 32) + (hl >> 32) + (hh & M);  // < 2^34
    p[2] = c & M;
    p[3] = (c >> 32) + (hh >> 32);  // < 2^32: a * b < 2^128
}

// A pair the records hold: every other pair contributes nothing and reads nothing.
MSIM_MHD bool cross_pair_ok(const msim_pair &q, uint32_t n_points, uint32_t m)
{
    return q.point_a < n_points && q.point_b < n_points && q.miner_a < m && q.miner_b < m;
}

// One run's contribution of one pair to the 12 words of its msim_cross, in field order; st / rt are the sides'
// share and rate terms.
MSIM_MHD void cross_add_run(uint64_t w[CROSS_WORDS], uint32_t fa, uint32_t sa, uint64_t sta, uint64_t rta, uint32_t fb,
                            uint32_t sb, uint64_t stb, uint64_t rtb)
{
    const uint64_t M = 0xFFFFFFFFull;
    uint64_t p[4];
    const uint64_t ff = (uint64_t)fa * fb, ss = (uint64_t)sa * sb;
    w[0] += ff & M;
    w[1] += ff >> 32;
    w[2] += ss & M;
    w[3] += ss >> 32;
    cross_mul_pieces(sta, stb, p);
    w[4] += p[0];
    w[5] += p[1];
    w[6] += p[2];
    w[7] += p[3];
    cross_mul_pieces(rta, rtb, p);
    w[8] += p[0];
    w[9] += p[1];
    w[10] += p[2];
    w[11] += p[3];
}

// ---------------------------------------------------------------- host: accumulation over a record array
// records [n_points][runs][m]{found, stale}, best_height [n_points][runs]; out: n_pairs msim_cross (overwritten).
// What the kernel computes, sequentially.
inline void cross_accumulate_host(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                  uint64_t runs, uint32_t m, const msim_pair *pairs, uint32_t n_pairs, msim_cross *out)
{
    static_assert(sizeof(msim_cross) == CROSS_WORDS * sizeof(uint64_t), "msim_cross is 12 uint64");
    static_assert(sizeof(msim_pair) == 16, "msim_pair is 4 uint32");
    memset(out, 0, sizeof(msim_cross) * (size_t)n_pairs);
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const msim_pair &q = pairs[i];
        if (!cross_pair_ok(q, n_points, m)) continue;
        for (uint64_t r = 0; r < runs; ++r) {
            const size_t ra = (size_t)q.point_a * runs + r, rb = (size_t)q.point_b * runs + r;
            const msim_run_record &a = rec[ra * m + q.miner_a], &b = rec[rb * m + q.miner_b];
            cross_add_run((uint64_t *)&out[i], a.found, a.stale, mom_share_term(a.found, best_height[ra]),
                          mom_rate_term(a.found, a.stale), b.found, b.stale, mom_share_term(b.found, best_height[rb]),
                          mom_rate_term(b.found, b.stale));
        }
    }
}

// ---------------------------------------------------------------- host: sums -> contrasts
// Widths, for what the ABI accepts: N < 2^32 runs, f, s < 2^32, terms t < 2^64. So, for found/stale and (in
// brackets) share/rate: first sums A, B < 2^64 [2^96]; S_aa, S_bb, S_ab < 2^96 [2^160].
//   diff_se:  N (S_aa + S_bb - 2 S_ab) - (A - B)^2          < 2^32 * 2^162 = 2^194
//   corr:     N S_ab, A B, N S_aa - A^2                     < 2^192 (each variance converts on its own; their
//             product, < 2^384, is formed in f64, far inside its exponent range)
//   ratio_se: B^2 S_aa + A^2 S_bb and 2 A B S_ab            < 2^353, times N < 2^385
// The last one passes MomWide's 384 bits, so everything here is formed in 448 bits.
using CrossWide = WideU<14>;

inline CrossWide cw_u64(uint64_t x) { return mw_from_u64<CrossWide::W>(x); }
inline CrossWide cw_join(const uint64_t *limb, int n) { return mw_join<CrossWide::W>(limb, n); }

// One quantity of one pair. `scale` turns term units into the quantity's (2^-32 for share and rate); out: diff,
// diff_se, corr and, with `ratio`, ratio and ratio_se, in msim_contrast's field order.
inline void cross_quantity(const CrossWide &A, const CrossWide &B, const CrossWide &Saa, const CrossWide &Sbb,
                           const CrossWide &Sab, uint64_t n, double scale, bool ratio, double *out)
{
    const CrossWide N = cw_u64(n);
    const double nd = (double)n;
    const bool neg = mw_cmp(A, B) < 0;
    const CrossWide D = neg ? mw_sub(B, A) : mw_sub(A, B);  // |A - B|
    const double d = mw_to_double(D) / nd * scale;
    out[0] = neg ? -d : d;
    double *r = out + 3;
    if (n < 2) {
        out[1] = out[2] = NAN;
    } else {
        // sum (a_i - b_i)^2 = S_aa + S_bb - 2 S_ab >= 0, and N times it >= (A - B)^2 (Cauchy-Schwarz)
        const CrossWide sq = mw_sub(mw_add(Saa, Sbb), mw_add(Sab, Sab));
        const CrossWide a = mw_mul(N, sq), b = mw_mul(D, D);
        if (mw_cmp(a, b) <= 0) {
            out[1] = 0.0;  // a constant difference
        } else {
            const double den = mw_to_double(mw_mul(mw_mul(N, N), cw_u64(n - 1)));
            out[1] = sqrt(mw_to_double(mw_sub(a, b)) / den) * scale;
        }
        const CrossWide naa = mw_mul(N, Saa), a2 = mw_mul(A, A), nbb = mw_mul(N, Sbb), b2 = mw_mul(B, B);
        if (mw_cmp(naa, a2) <= 0 || mw_cmp(nbb, b2) <= 0) {
            out[2] = NAN;  // a side that does not vary
        } else {
            const CrossWide nab = mw_mul(N, Sab), ab = mw_mul(A, B);
            const bool cneg = mw_cmp(nab, ab) < 0;
            const double num = mw_to_double(cneg ? mw_sub(ab, nab) : mw_sub(nab, ab));
            const double c = num / sqrt(mw_to_double(mw_sub(naa, a2)) * mw_to_double(mw_sub(nbb, b2)));
            out[2] = cneg ? -c : c;
        }
    }
    if (!ratio) return;
    if (mw_is_zero(B)) {
        r[0] = r[1] = NAN;
        return;
    }
    r[0] = mw_to_double(A) / mw_to_double(B);
    if (n < 2) {
        r[1] = NAN;
        return;
    }
    // delta method: N / (N - 1) * sum (B a_i - A b_i)^2 = N / (N - 1) * (B^2 S_aa - 2 A B S_ab + A^2 S_bb)
    const CrossWide B2 = mw_mul(B, B);
    const CrossWide pos = mw_add(mw_mul(B2, Saa), mw_mul(mw_mul(A, A), Sbb));
    const CrossWide abs_ = mw_mul(mw_mul(A, B), Sab);
    const CrossWide ng = mw_add(abs_, abs_);
    if (mw_cmp(pos, ng) <= 0) {
        r[1] = 0.0;
        return;
    }
    const double num = mw_to_double(mw_mul(N, mw_sub(pos, ng)));
    r[1] = sqrt(num / (double)(n - 1)) / mw_to_double(B2);
}

// moments: [n_points * m], indexed point * m + miner; every pair within them (msim_pairs_check).
inline void cross_to_contrasts(const msim_moments *mo, uint32_t m, const msim_pair *pairs, const msim_cross *cross,
                               uint32_t n_pairs, uint64_t n_runs, msim_contrast *out)
{
    static_assert(sizeof(msim_contrast) == 16 * sizeof(double), "msim_contrast is 16 doubles");
    const double q = 0x1.0p-32;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const msim_moments &a = mo[(size_t)pairs[i].point_a * m + pairs[i].miner_a];
        const msim_moments &b = mo[(size_t)pairs[i].point_b * m + pairs[i].miner_b];
        const msim_cross &x = cross[i];
        msim_contrast &c = out[i];
        const uint64_t sha[2] = {a.first.share_lo, a.first.share_hi}, shb[2] = {b.first.share_lo, b.first.share_hi};
        const uint64_t rta[2] = {a.first.rate_lo, a.first.rate_hi}, rtb[2] = {b.first.rate_lo, b.first.rate_hi};
        cross_quantity(cw_u64((uint64_t)a.first.blocks_found), cw_u64((uint64_t)b.first.blocks_found),
                       cw_join(a.found_sq, 2), cw_join(b.found_sq, 2), cw_join(x.found_found, 2), n_runs, 1.0, true,
                       &c.found_diff);
        cross_quantity(cw_u64((uint64_t)a.first.stale_blocks), cw_u64((uint64_t)b.first.stale_blocks),
                       cw_join(a.stale_sq, 2), cw_join(b.stale_sq, 2), cw_join(x.stale_stale, 2), n_runs, 1.0, false,
                       &c.stale_diff);
        cross_quantity(cw_join(sha, 2), cw_join(shb, 2), cw_join(a.share_sq, 4), cw_join(b.share_sq, 4),
                       cw_join(x.share_share, 4), n_runs, q, true, &c.share_diff);
        cross_quantity(cw_join(rta, 2), cw_join(rtb, 2), cw_join(a.rate_sq, 4), cw_join(b.rate_sq, 4),
                       cw_join(x.rate_rate, 4), n_runs, q, false, &c.rate_diff);
    }
}
}  // namespace msim

#endif  // MSIM_CROSS_H

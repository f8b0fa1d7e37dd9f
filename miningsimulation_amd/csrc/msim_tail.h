// msim_tail.h — tail statistics: the moments of a TARGET column over the runs whose CONDITION key lies below, or
// at, a threshold (include/msim.h: msim_tail_item, msim_tail, msim_tail_side, msim_tail_means). The keys are
// msim_rank.h's (found, stale and the two terms of msim_moments.h), the sums are mom_add_run's, so an item's 42
// words are exact integer sums over a subset of the runs, in msim_moments' limb convention.
//
// The item guard, the key and the per-run add are __host__ __device__: the gfx950 reduction kernel
// (msim_tail.hip), the host accumulation below (tests/native/tail_host.cpp, tests/native/tail_check.cpp) and the
// host arithmetic behind msim_tail_side / msim_tail_means all run the same lines.
#ifndef MSIM_TAIL_H
#define MSIM_TAIL_H

#include "msim_moments.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define MSIM_UNROLL _Pragma("unroll")
#define MSIM_MHD_FLAT __host__ __device__ __forceinline__  // its array arguments must stay in registers
#else
#define MSIM_UNROLL
#define MSIM_MHD_FLAT inline
#endif

namespace msim {

constexpr uint32_t TAIL_WORDS = 2 + 2 * MOM_WORDS;  // uint64 fields of msim_tail
constexpr uint32_t TAIL_QUANTITIES = 4;             // found, stale, share_t, rate_t, as msim_order_stat's

// An item the records hold: every other item contributes nothing and reads nothing.
MSIM_MHD bool tail_item_ok(const msim_tail_item &it, uint32_t n_points, uint32_t m)
{
    return it.cond_point < n_points && it.target_point < n_points && it.cond_column < m && it.target_column < m &&
           it.quantity < TAIL_QUANTITIES && it.reserved == 0;
}

// The key of one record for one quantity: only the term the quantity needs is evaluated (at most one division).
MSIM_MHD uint64_t tail_key(uint32_t quantity, uint32_t f, uint32_t s, uint32_t L)
{
    if (quantity == 0) return f;
    if (quantity == 1) return s;
    return quantity == 2 ? mom_share_term(f, L) : mom_rate_term(f, s);
}

// One run's contribution of the target record to the set it belongs to: `below` (key < value) or the ties
// (key == value). A run above the threshold is never passed here. The 20 addends are formed once and added to
// one of the two sets of words, each indexed statically.
MSIM_MHD_FLAT void tail_add_run(uint64_t w[TAIL_WORDS], bool below, uint32_t f, uint32_t s, uint64_t st, uint64_t rt)
{
    uint64_t a[MOM_WORDS];
    MSIM_UNROLL
    for (uint32_t i = 0; i < MOM_WORDS; ++i) a[i] = 0;
    mom_add_run(a, f, s, st, rt);
    // added under a mask, not in two branches: a compiler that merges the branches' common adds would index the
    // words by the predicate, and a runtime index sends the kernel's register array to scratch
    const uint64_t mb = below ? ~(uint64_t)0 : 0, me = ~mb;
    w[0] += 1 & mb;
    w[1] += 1 & me;
    MSIM_UNROLL
    for (uint32_t i = 0; i < MOM_WORDS; ++i) {
        w[2 + i] += a[i] & mb;
        w[2 + MOM_WORDS + i] += a[i] & me;
    }
}

// ---------------------------------------------------------------- host: accumulation over a record array
// records [n_points][runs][m]{found, stale}, best_height [n_points][runs]; out: n_items msim_tail (overwritten).
// What the kernel computes, sequentially.
inline void tail_accumulate_host(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                 uint64_t runs, uint32_t m, const msim_tail_item *items, uint32_t n_items,
                                 msim_tail *out)
{
    static_assert(sizeof(msim_tail) == TAIL_WORDS * sizeof(uint64_t), "msim_tail is 42 uint64");
    static_assert(sizeof(msim_tail_item) == 32, "msim_tail_item is 32 bytes");
    memset(out, 0, sizeof(msim_tail) * (size_t)n_items);
    for (uint32_t i = 0; i < n_items; ++i) {
        const msim_tail_item &it = items[i];
        if (!tail_item_ok(it, n_points, m)) continue;
        for (uint64_t r = 0; r < runs; ++r) {
            const size_t rc = (size_t)it.cond_point * runs + r, rt = (size_t)it.target_point * runs + r;
            const msim_run_record &c = rec[rc * m + it.cond_column];
            const uint64_t key = tail_key(it.quantity, c.found, c.stale, best_height[rc]);
            if (key > it.value) continue;
            const msim_run_record &x = rec[rt * m + it.target_column];
            tail_add_run((uint64_t *)&out[i], key < it.value, x.found, x.stale,
                         mom_share_term(x.found, best_height[rt]), mom_rate_term(x.found, x.stale));
        }
    }
}

// ---------------------------------------------------------------- host: sides and means
// The words of msim_moments as plain uint64 (first.blocks_found and first.stale_blocks are never negative).
inline const uint64_t *tail_words(const msim_moments *mo) { return (const uint64_t *)mo; }

// out = a - b limb by limb; false when a limb of b exceeds a's (b is no subset of a).
inline bool tail_sub_words(const uint64_t *a, const uint64_t *b, uint64_t *out)
{
    for (uint32_t i = 0; i < MOM_WORDS; ++i) {
        if (b[i] > a[i]) return false;
        out[i] = a[i] - b[i];
    }
    return true;
}

// One of the four sets of runs an msim_tail splits a column into. Unnormalised limbs of a subset never exceed
// the same limbs over all runs, so the complements are limb-wise differences from the total.
inline int tail_side(const msim_tail *t, const msim_moments *total, uint64_t n_runs, int side, msim_moments *out,
                     uint64_t *out_n)
{
    if (!t || !out || !out_n || n_runs == 0 || t->n_below > n_runs || t->n_equal > n_runs - t->n_below)
        return MSIM_E_INVALID;
    uint64_t w[MOM_WORDS], n;
    const uint64_t *b = tail_words(&t->below), *e = tail_words(&t->equal);
    if (side == MSIM_TAIL_BELOW) {
        memcpy(w, b, sizeof(w));
        n = t->n_below;
    } else if (side == MSIM_TAIL_AT_MOST) {
        for (uint32_t i = 0; i < MOM_WORDS; ++i) w[i] = b[i] + e[i];
        n = t->n_below + t->n_equal;
    } else if (side == MSIM_TAIL_ABOVE || side == MSIM_TAIL_AT_LEAST) {
        if (!total || !tail_sub_words(tail_words(total), b, w)) return MSIM_E_INVALID;
        n = n_runs - t->n_below;
        if (side == MSIM_TAIL_ABOVE) {
            if (!tail_sub_words(w, e, w)) return MSIM_E_INVALID;
            n -= t->n_equal;
        }
    } else {
        return MSIM_E_INVALID;
    }
    memcpy(out, w, sizeof(w));
    *out_n = n;
    return MSIM_OK;
}

// Widths: a first sum S < 2^32 runs * 2^64 = 2^96, counts < 2^32: S n_equal + (k - n) S_equal < 2^130, the
// shifted numerator of the division below < 2^197. 256 bits hold everything.
using TailWide = WideU<8>;

template <int W>
inline int mw_bits(const WideU<W> &a)
{
    for (int i = W - 1; i >= 0; --i)
        if (a.w[i]) {
            int b = 32;
            while (!(a.w[i] >> (b - 1))) --b;
            return 32 * i + b;
        }
    return 0;
}

// num / den as the nearest double (ties to even), den != 0: the quotient of the numerator shifted left until it
// has at least 65 bits, by long division, with a non-zero remainder folded into its lowest bit; mw_to_double then
// rounds once, and the scaling back by a power of two is exact. The shifted numerator must fit the type.
template <int W>
inline double mw_div_to_double(const WideU<W> &num, const WideU<W> &den)
{
    const int bn = mw_bits(num), bd = mw_bits(den);
    if (bn == 0) return 0.0;
    const int shift = bn >= bd + 65 ? 0 : bd + 65 - bn;
    const int top = bn + shift;  // bits of the shifted numerator, <= 32 W
    WideU<W> q, rem;
    memset(&q, 0, sizeof(q));
    memset(&rem, 0, sizeof(rem));
    for (int pos = top - 1; pos >= 0; --pos) {
        // rem = rem << 1 | bit `pos` of num << shift
        uint32_t carry = 0;
        if (pos >= shift) carry = (num.w[(pos - shift) >> 5] >> ((pos - shift) & 31)) & 1u;
        for (int i = 0; i < W; ++i) {
            const uint32_t nx = rem.w[i] >> 31;
            rem.w[i] = rem.w[i] << 1 | carry;
            carry = nx;
        }
        if (mw_cmp(rem, den) >= 0) {
            rem = mw_sub(rem, den);
            q.w[pos >> 5] |= 1u << (pos & 31);
        }
    }
    if (!mw_is_zero(rem)) q.w[0] |= 1u;  // at least 64 bits below the quotient's top bit: sticky only
    return ldexp(mw_to_double(q), -shift);
}

// The four first sums of a set of msim_moments words: found, stale, share_t, rate_t.
inline void tail_first_sums(const uint64_t *w, TailWide s[4])
{
    const uint64_t sh[2] = {w[3], w[2]}, rt[2] = {w[5], w[4]};  // msim_sums stores the high limb first
    s[0] = mw_from_u64<TailWide::W>(w[0]);
    s[1] = mw_from_u64<TailWide::W>(w[1]);
    s[2] = mw_join<TailWide::W>(sh, 2);
    s[3] = mw_join<TailWide::W>(rt, 2);
}

// mean_k of the target's found, stale, share and rate over the k smallest (upper == 0) or k largest runs of the
// condition: all of the strict side plus k - n_strict of the ties, every tie weighted (k - n_strict) / n_equal:
//   (S_strict n_equal + (k - n_strict) S_equal) / (k n_equal)
// formed exactly, then one correctly rounded division; share and rate scaled by 2^-32 (exact).
inline int tail_means(const msim_tail *t, const msim_moments *total, uint64_t n_runs, uint64_t k, int upper,
                      double out[4])
{
    if (!t || !out || (upper != 0 && upper != 1)) return MSIM_E_INVALID;
    msim_moments strict;
    uint64_t n_strict;
    const int rc = tail_side(t, total, n_runs, upper ? MSIM_TAIL_ABOVE : MSIM_TAIL_BELOW, &strict, &n_strict);
    if (rc != MSIM_OK) return rc;
    if (k <= n_strict || k - n_strict > t->n_equal) return MSIM_E_INVALID;  // k outside the tie range
    TailWide S[4], E[4];
    tail_first_sums(tail_words(&strict), S);
    tail_first_sums(tail_words(&t->equal), E);
    const TailWide ne = mw_from_u64<TailWide::W>(t->n_equal), take = mw_from_u64<TailWide::W>(k - n_strict);
    const TailWide den = mw_mul(mw_from_u64<TailWide::W>(k), ne);
    for (int q = 0; q < 4; ++q) {
        const double v = mw_div_to_double(mw_add(mw_mul(S[q], ne), mw_mul(take, E[q])), den);
        out[q] = q < 2 ? v : v * 0x1.0p-32;
    }
    return MSIM_OK;
}
}  // namespace msim

#endif  // MSIM_TAIL_H

// msim_fastdraw.h — the draw kernels' fast, exactly-checked forms of the reference's two draws.
//
// NextBlockInterval (/root/reference/simulation.h:205-210 + xoroshiro128++.h:17-20,36-39) is
//     ms = trunc(llround(6e11 * -log1p(-(u>>11) * 2^-53)) / 1e6)
// with glibc's log1p. Only the millisecond value matters, and it changes only where 6e11*E + 0.5
// crosses a multiple of 1e6. So the fast path evaluates E with a cheap table method (64-entry 1/c
// table, degree-5 log1p polynomial, FMAs allowed) whose total error against glibc's bits is < 0.05 ns
// in 6e11*E, and accepts its result only when 6e11*E + 0.5 lies at least
// MARGIN_NS = 1 ns away from every millisecond boundary; anything closer (2e-6 of draws) is recomputed
// by the bit-exact glibc sequence of msim_draws.h. The result is therefore identical to the
// reference's for every input, not just statistically.
//
// PickFinder (simulation.h:213-221) returns the first miner whose cumulative perc*PERC_MULTIPLIER
// exceeds u. With integer percentages that is lut[q], q = floor(u / PERC_MULTIPLIER), and q is
// p = floor(100 * u_hi / 2^32) (u_hi = u >> 32) unless the low word of 100 * u_hi is within 101 of
// 2^32 (then q = p or p + 1, decided exactly by u >= (p+1) * PM): one 32-bit high multiply, one
// 32-bit low multiply and one 4-byte table read replace the M-step scan; 3e-8 of draws take the
// exact two-multiply path.
//
// Table sizes are set by the LDS banking of gfx950 (MI355X_MICROARCH.md §LDS): a lane-random 16-byte
// read from a 512-entry table conflicted 3-way on average (round-3 K1 counters: 68 % of the LDS cycles
// were bank conflicts), whereas the 64-entry f64 arrays below span at most two entries per bank pair
// and the 101-word pick table at most four words per bank.
#pragma once
#include <math.h>
#include <stdint.h>

#include "msim_draws.h"

namespace msim {

constexpr int LOG_BITS = 6;
constexpr int LOG_TAB = 1 << LOG_BITS;
constexpr int PICK_TAB = 101;  // q = 0 .. 100 (q = 100: PickFinder falls through, simulation.h:220)
constexpr double MARGIN_NS = 1.0;
// Pick info word: finder k in bits 10..13 (so that info & 0x3C00 is the byte offset of owner k's row of a
// [16][256] u32 LDS counter array), fast threshold fthr in bits 14..31. FTHR_CAP bounds fthr: an honest
// network whose delays reach it does not run the pipeline (msim_api.hip); PickFinder's fall-through
// (k = 15) carries FTHR_CAP and is caught by its own counter (msim_pipeline.h combine_run).
constexpr uint32_t INFO_K_SHIFT = 10, INFO_T_SHIFT = 14;
constexpr uint32_t FTHR_NEVER = (1u << 27) - 1;  // large-network tables (msim_wide.h): > any interval
constexpr uint32_t FTHR_CAP = (1u << (32 - INFO_T_SHIFT)) - 1;  // 262 143 ms
MSIM_HD uint32_t info_finder(uint32_t info) { return (info >> INFO_K_SHIFT) & 15u; }
MSIM_HD uint32_t info_fthr(uint32_t info) { return info >> INFO_T_SHIFT; }
MSIM_HD uint32_t make_info(uint32_t k, uint32_t fthr) { return (k << INFO_K_SHIFT) | (fthr << INFO_T_SHIFT); }

// Log table, structure of arrays: entry j covers w in [1 + j/LOG_TAB, 1 + (j+1)/LOG_TAB); invc ~ 1/c_j,
// c_j = 1 + (j + 1/2)/LOG_TAB, and A = (0.5 - 6e11 * log(1/invc)) * 1e-6: the entry's share of
// z = (6e11*E + 0.5) / 1e6 in ms.
struct LogTab {
    double invc[LOG_TAB];
    double A[LOG_TAB];
};
// Pick table: info[q] = make_info(k, fthr) for q = floor(u / PERC_MULTIPLIER): k = finder (15 = fell
// through), fthr = the interval the NEXT draw must exceed for the block to be "fast" (honest finder, next
// find after its arrival).
struct PickTab {
    uint32_t info[128];
};

// Fast interval with exactness check; on `ok == false` the caller must use the exact path.
// v = 1 - (u>>11)*2^-53 is formed EXACTLY from the two 32-bit halves of u (both partial results are
// multiples of 2^-53 in (0, 1], so neither rounding loses a bit), v = 2^e * w with w in [1, 2) read off
// its bits, and z = (6e11 * E + 0.5) / 1e6 = A_j - 6e5 * (e*ln2 + log1p(r)), E = -log(v), r = w*invc_j - 1
// (|r| <= 2^-7: the degree-5 truncation r^6/6 is < 4e-14, i.e. <= 0.025 ns in 6e11*E).
// The reference's interval is floor(z) whenever frac(z) is at least MARGIN_NS/1e6 from 0 and 1.
constexpr double FD_C1 = -6e5, FD_C2 = 3e5, FD_C3 = -2e5, FD_C4 = 1.5e5, FD_C5 = -1.2e5;  // -6e5 * (-1)^(k+1) / k
constexpr double FD_CE = -6e5 * 6.93147180559945309417e-01;                              // -6e5 * ln 2
#if defined(__HIP_DEVICE_COMPILE__)
// u32 -> f64 as one v_cvt_f64_u32 (LLVM widens a converted `u >> 32` into a 64-bit conversion that adds
// a +0.0 it cannot fold away).
__device__ __forceinline__ double u32_to_f64(uint32_t x)
{
    double d;
    asm("v_cvt_f64_u32 %0, %1" : "=v"(d) : "v"(x));
    return d;
}
#else
MSIM_HD double u32_to_f64(uint32_t x) { return (double)x; }
#endif

// Polynomial constants as values the caller hoists into scalar registers once (fd_consts) and passes
// down: every Horner step is then ONE three-operand VOP3 FMA with the constant as its SGPR addend. With
// literal constants the compiler emits v_fmac, which overwrites its addend, and copies the constant into
// a fresh register pair before every draw.
// The leading coefficient (a multiplicand of the first step, beside the SGPR addend) lives in a VGPR:
// one VOP3 instruction reads at most one SGPR on gfx950.
#ifndef MSIM_FD_C5_VGPR
#define MSIM_FD_C5_VGPR 1
#endif
struct FdConsts {
    double c1, c2, c3, c4, c5;
};
MSIM_HD FdConsts fd_consts()
{
    FdConsts k{FD_C1, FD_C2, FD_C3, FD_C4, FD_C5};
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(k.c1));
    asm("" : "+s"(k.c2));
    asm("" : "+s"(k.c3));
    asm("" : "+s"(k.c4));
#if MSIM_FD_C5_VGPR
    asm("" : "+v"(k.c5));
#endif
#endif
    return k;
}
#define MSIM_FD_DEFAULT FdConsts{FD_C1, FD_C2, FD_C3, FD_C4, FD_C5}

MSIM_HD double interval_fast_z(uint64_t u, const LogTab *__restrict__ tab, FdConsts kc = MSIM_FD_DEFAULT)
{
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    const double c = __builtin_fma(u32_to_f64(lo >> 11), -0x1.0p-53, 1.0);  // exact
    const double v = __builtin_fma(u32_to_f64(hi), -0x1.0p-32, c);           // exact: 1 - (u>>11) 2^-53
    const uint64_t vb = __builtin_bit_cast(uint64_t, v);
    const uint32_t vh = (uint32_t)(vb >> 32);
    const int e = (int)(vh >> 20) - 1023;                                    // v = 2^e w, e in [-53, 0]
    const uint32_t j = (vh >> (20 - LOG_BITS)) & (LOG_TAB - 1);              // top LOG_BITS mantissa bits
    const double w = __builtin_bit_cast(double, (vb & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
#if defined(__HIP_DEVICE_COMPILE__)
    // A_j through a base the compiler cannot relate to invc_j's: two ds_read_b64 (64-bank, at most two
    // entries per bank pair) instead of one merged ds_read2st64_b64 (32-bank, up to four)
    uint32_t aoff = j * 8u;
    asm("" : "+v"(aoff));
    const double Aj = *(const double *)((const char *)tab->A + aoff);
#else
    const double Aj = tab->A[j];
#endif
    const double r = __builtin_fma(w, tab->invc[j], -1.0);
    double p = __builtin_fma(r, kc.c5, kc.c4);
    p = __builtin_fma(r, p, kc.c3);
    p = __builtin_fma(r, p, kc.c2);
    p = __builtin_fma(r, p, kc.c1);
    const double z0 = __builtin_fma(r, p, Aj);                               // A_j - 6e5 log1p(r)
    return __builtin_fma((double)e, FD_CE, z0);
}

// Acceptance on the high word of frac(z) (a positive double below 1: integer order = value order):
// strictly inside (hi(MARGIN), hi(1 - MARGIN)) implies frac in (MARGIN, 1 - MARGIN); a high word equal
// to either bound falls back to the exact path (a 2^-20 relative sliver of that band).
constexpr uint32_t FD_OK_LO = 0x3EB0C6F7u + 1u;  // hi(1e-6) + 1
constexpr uint32_t FD_OK_HI = 0x3FEFFFFDu;       // hi(1 - 1e-6) (exclusive)
constexpr uint32_t FD_OK_RANGE = FD_OK_HI - FD_OK_LO;
// Fast interval and its acceptance key: the result is the reference's iff key < FD_OK_RANGE (keys of
// several draws combine with max).
MSIM_HD int32_t interval_ms_fast_key(uint64_t u, const LogTab *__restrict__ tab, uint32_t &key,
                                     FdConsts kc = MSIM_FD_DEFAULT)
{
    const double z = interval_fast_z(u, tab, kc);
    const int32_t q = (int32_t)z;                 // z >= 0.5e-6 > 0: truncation = floor
#if defined(__HIP_DEVICE_COMPILE__)
    const double f = __builtin_amdgcn_fract(z);
#else
    const double f = z - (double)q;
#endif
    key = (uint32_t)(__builtin_bit_cast(uint64_t, f) >> 32) - FD_OK_LO;
    return q;
}
MSIM_HD int32_t interval_ms_fast(uint64_t u, const LogTab *__restrict__ tab, bool &ok, FdConsts kc = MSIM_FD_DEFAULT)
{
    uint32_t key;
    const int32_t q = interval_ms_fast_key(u, tab, key, kc);
    ok = key < FD_OK_RANGE;
    return q;
}

// ---------------------------------------------------------------- K1's form of the fast interval
// The draw kernel (msim_drawgen.hip) issues one vector instruction stream per block drawn, so its form of the
// fast interval trades table size and margin for instructions. Each item has a build switch (A/B builds:
// `make variant VFLAGS=-D...=0`); with both off K1 computes exactly interval_fast_z. K2, K3, W1 and the selfish
// engines keep the general form above. Every result is still the reference's: a draw the checks below do not
// accept is recomputed, first by the general form (k1_interval_key<false>, no exponent limit), then, within
// the margin of a millisecond boundary, by glibc's sequence.
//
// MSIM_FD_A2: the exponent term is folded into the table. The low four bits of v's biased exponent and the top
//   six mantissa bits are adjacent in its high word vh (bits 14..23), so A2[(vh >> 14) & 1023] = A_j + e*FD_CE
//   replaces the exponent's extraction, its conversion and the last FMA. Row eps = (e + 1023) & 15 holds
//   e = eps - 15, right for e in [-15, 0]; a smaller exponent (2^-15 of draws) aliases and MUST be rejected:
//   the caller checks vt = vh >> 11 (the table offset before masking, which the form computes anyway)
//   against FD_VT_MIN (K1's quad, msim_pipeline.h k1p_quad_fast, folds a min over the quad into one compare).
// MSIM_FD_DEG4: -6e5 log1p(r) as the degree-4 minimax polynomial of scripts/fit_log1p_deg4.py (Remez, 60
//   digits; k1..k4 rounded to doubles, k0 added to the table before its one rounding). Its largest error on
//   |r| <= 2^-7 is 0.2183 ns against the Taylor form's 0.025 ns, so the acceptance margin grows from 1 ns to
//   K1_MARGIN_NS = 1.25 ns: margin minus total error (truncation + the roundings of r, the Horner steps, the
//   table entry and z, together < 0.01 ns for e >= -15) stays above the general form's 1 - 0.05 ns.
//   tests/native/fastdraw2_check.cpp measures both sides of that inequality.
// Share of draws sent to the general form: 2^-15 + 2 * 1.25e-6 = 3.3e-5.
#ifndef MSIM_FD_A2
#define MSIM_FD_A2 1
#endif
#ifndef MSIM_FD_DEG4
#define MSIM_FD_DEG4 1
#endif
constexpr int K1_EROWS = 16;
constexpr int FD_VT_SHIFT = 20 - LOG_BITS - 3;  // vt = vh >> 11: entry index * 8 in bits 3..12, exponent from bit 9
constexpr uint32_t FD_VT_MIN = ((uint32_t)(1023 - (K1_EROWS - 1)) << 20) >> FD_VT_SHIFT;  // vt of 2^-15
// One entry of the packed table (below, "the packed form"): everything one fast draw reads, as one 16-byte read.
struct alignas(16) K1Pair {
    double invc;  // invc_j * 2^(15 - eps)
    double A;     // A2[eps, j] less the acceptance margin
};
struct K1Log {
    double invc[LOG_TAB];
    double A2[K1_EROWS * LOG_TAB];  // row K1_EROWS - 1 (e = 0) is the general form's A (+ the polynomial's k0)
    K1Pair P[K1_EROWS * LOG_TAB];   // the packed form's table, entry (eps, j) as A2's
};
#if MSIM_FD_DEG4
constexpr double K1_MARGIN_NS = 1.25;
constexpr long double FD4_K0 = 1.421215240674198145941903e-9L;
constexpr double FD4_K1 = -0x1.24f7fffedb037p+19, FD4_K2 = 0x1.24f7fffb0a5dbp+18, FD4_K3 = -0x1.86a493edc0716p+17,
                 FD4_K4 = 0x1.24fd57452922dp+17;
constexpr uint32_t K1_OK_LO = 0x3EB4F8B5u + 1u;  // hi(1.25e-6) + 1
#define MSIM_K1_CONSTS FdConsts{FD4_K1, FD4_K2, FD4_K3, FD4_K4, 0.0}
#define MSIM_K1_LEAD c4  // the leading coefficient: the one multiplicand of the first Horner step
#else
constexpr double K1_MARGIN_NS = MARGIN_NS;
constexpr long double FD4_K0 = 0.0L;
constexpr uint32_t K1_OK_LO = FD_OK_LO;
#define MSIM_K1_CONSTS MSIM_FD_DEFAULT
#define MSIM_K1_LEAD c5
#endif
constexpr uint32_t K1_OK_HI = 0x3FEFFFFDu;  // hi(1 - 1.25e-6) = hi(1 - 1e-6) (exclusive)
constexpr uint32_t K1_OK_RANGE = K1_OK_HI - K1_OK_LO;

// z = (6e11 E + 0.5) / 1e6 by K1's polynomial. FOLD: the table row is chosen by the exponent's low bits (valid
// only for vt >= FD_VT_MIN); otherwise the general form, for any exponent. vt = (the high word of v) >> 11.
// On the arrays themselves (K1 keeps only invc and row e = 0 in LDS): A = A2 for FOLD, row e = 0 of it otherwise.
template <bool FOLD>
MSIM_HD double k1_interval_z_on(uint64_t u, const double *__restrict__ invc, const double *__restrict__ A, uint32_t &vt,
                                FdConsts kc = MSIM_K1_CONSTS)
{
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    const double c = __builtin_fma(u32_to_f64(lo >> 11), -0x1.0p-53, 1.0);  // exact
    const double v = __builtin_fma(u32_to_f64(hi), -0x1.0p-32, c);           // exact: 1 - (u>>11) 2^-53
    const uint64_t vb = __builtin_bit_cast(uint64_t, v);
    const uint32_t vh = (uint32_t)(vb >> 32);
    const double w = __builtin_bit_cast(double, (vb & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    // byte offsets of entry j and of entry (eps, j): the two reads have different address registers, so the
    // compiler cannot merge them into one ds_read2st64_b64 (32-bank: see the table sizes above)
    vt = vh >> FD_VT_SHIFT;
    const uint32_t joff = vt & ((LOG_TAB - 1u) << 3);
    uint32_t aoff = FOLD ? vt & ((K1_EROWS * LOG_TAB - 1u) << 3) : joff;
#if defined(__HIP_DEVICE_COMPILE__)
    if (!FOLD) asm("" : "+v"(aoff));  // as interval_fast_z: keeps the general form's two reads apart
#endif
    const double Aj = *(const double *)((const char *)A + aoff);
    const double r = __builtin_fma(w, *(const double *)((const char *)invc + joff), -1.0);
#if MSIM_FD_DEG4
    double p = __builtin_fma(r, kc.c4, kc.c3);
#else
    double p = __builtin_fma(r, kc.c5, kc.c4);
    p = __builtin_fma(r, p, kc.c3);
#endif
    p = __builtin_fma(r, p, kc.c2);
    p = __builtin_fma(r, p, kc.c1);
    const double z0 = __builtin_fma(r, p, Aj);
    if (FOLD) return z0;
    return __builtin_fma((double)((int)(vt >> (20 - FD_VT_SHIFT)) - 1023), FD_CE, z0);
}
template <bool FOLD>
MSIM_HD double k1_interval_z(uint64_t u, const K1Log *__restrict__ tab, uint32_t &vt, FdConsts kc = MSIM_K1_CONSTS)
{
    return k1_interval_z_on<FOLD>(u, tab->invc, FOLD ? tab->A2 : tab->A2 + (K1_EROWS - 1) * LOG_TAB, vt, kc);
}
// Interval and acceptance key of a z (as interval_ms_fast_key): the reference's value iff key < K1_OK_RANGE and,
// for the folded table, vt >= FD_VT_MIN.
MSIM_HD int32_t k1_z_key(double z, uint32_t &key)
{
    const int32_t q = (int32_t)z;  // z >= 0.5e-6 > 0: truncation = floor
#if defined(__HIP_DEVICE_COMPILE__)
    const double f = __builtin_amdgcn_fract(z);
#else
    const double f = z - (double)q;
#endif
    key = (uint32_t)(__builtin_bit_cast(uint64_t, f) >> 32) - K1_OK_LO;
    return q;
}
template <bool FOLD>
MSIM_HD int32_t k1_interval_key(uint64_t u, const K1Log *__restrict__ tab, uint32_t &key, uint32_t &vt,
                                FdConsts kc = MSIM_K1_CONSTS)
{
    return k1_z_key(k1_interval_z<FOLD>(u, tab, vt, kc), key);
}
// The general form on K1's two small arrays (invc and row e = 0 of A2): k1_interval_general's value and flag.
MSIM_HD int32_t k1_interval_general_on(uint64_t u, const double *__restrict__ invc, const double *__restrict__ A0, bool &ok,
                                       FdConsts kc = MSIM_K1_CONSTS)
{
    uint32_t key, vt;
    const int32_t q = k1_z_key(k1_interval_z_on<false>(u, invc, A0, vt, kc), key);
    ok = key < K1_OK_RANGE;
    return q;
}
// K1's fast form alone: ok == false sends the draw to the general form.
MSIM_HD int32_t k1_interval_fast(uint64_t u, const K1Log *__restrict__ tab, bool &ok, FdConsts kc = MSIM_K1_CONSTS)
{
    uint32_t key, vt;
    const int32_t q = k1_interval_key<MSIM_FD_A2 != 0>(u, tab, key, vt, kc);
    ok = key < K1_OK_RANGE && (!MSIM_FD_A2 || vt >= FD_VT_MIN);
    return q;
}
MSIM_HD int32_t k1_interval_general(uint64_t u, const K1Log *__restrict__ tab, bool &ok, FdConsts kc = MSIM_K1_CONSTS)
{
    uint32_t key, vt;
    const int32_t q = k1_interval_key<false>(u, tab, key, vt, kc);
    ok = key < K1_OK_RANGE;
    return q;
}

// ---------------------------------------------------------------- the packed form (what K1's quad runs)
// The folded form above, with the work its result does not need taken out; k1_interval_fast above stays the
// checked definition the packed form is compared with (tests/native/k1pack_check.cpp).
//
// Packing: one 16-byte entry per draw, P[(vh >> 14) & 1023] = {invc_j * 2^(15 - eps), A2[eps, j]}, and
//   r = fma(v, P.invc, -1) on v itself. With v = w * 2^e and e = eps - 15 in [-15, 0], v * (invc_j * 2^-e) and
//   w * invc_j are the same real number (the scaling is by a power of two, at most 2^15: no overflow, no
//   underflow), so the FMA rounds to the same bits as the folded form's: r, z and the interval are identical.
//   The mantissa's rebuild (v_and, v_or), one of the two address masks and one of the two LDS reads go. For
//   e < -15 the row aliases as before, and the quad rejects on the smallest high word of its four v's.
// Folded margin: the entry's A is A2 - M, M = K1_MARGIN_NS * 1e-6 ms (80-bit, rounded once, like every entry), so
//   the form computes z' = z - M. Let f' = fract(z'). The draw is accepted iff hi(f') < K1P_OK_HI =
//   hi(1 - 2M), which implies f' < 1 - 2M, and then:
//     z' >= 0: fract of a negative z' (only z < M; u = 0 is such a draw) is just below 1 on the device and
//       negative on the host (z' - trunc(z')); both fail the test;
//     frac(z) = f' + M lies in [M, 1 - M): z is at least the margin away from both millisecond boundaries, the
//       condition under which floor(z) is the reference's interval (above);
//     floor(z') = floor(z), since z' = floor(z) + (frac(z) - M) with 0 <= frac(z) - M < 1.
//   Conversely frac(z) < M gives f' >= 1 - M: rejected. So one upper bound on the raw high word replaces the
//   two-sided test, the per-draw rebase of the key (v_add_u32) goes, and the quad's max runs on the raw high
//   words. The lower margin is now M itself (the folded form asks one high-word step more), the upper one
//   1 - 6 * 2^-21 - M = 1.61 ns; rejected share 2^-15 + 2.86e-6.
// v without conversions: the general form builds v = 1 - (u>>11) 2^-53 from two v_cvt_f64_u32 and two FMAs. The
//   packed form writes each 32-bit half of the draw into the low word of a double whose high word is a constant,
//   which IS an exact double, and subtracts twice:
//     dh = [K1V_HI_WORD : hi]       = 2^20 + hi 2^-32        (exponent 2^20: one unit in the last place is 2^-32)
//     dl = [K1V_LO_WORD : lo >> 11] = 1/2 + (lo >> 11) 2^-53 (exponent 2^-1: one unit is 2^-53; lo >> 11 < 2^21)
//     c  = K1V_BASE - dh = 1.5 - hi 2^-32      a multiple of 2^-32 in (0.5, 1.5]: representable, so the
//                                              subtraction rounds to it exactly
//     v  = c - dl        = 1 - (u>>11) 2^-53   a multiple of 2^-53 in (0, 1]: representable, exact
//   so v has the bits of the general form's v for every u (tests/native/k1v_check.cpp). Both conversions, of the
//   slow issue class, go; in their place the quad has two v_mov_b32 per draw (a half, or a high word, into its
//   pair), of the cheap class: the compiler keeps one copy of each high word in a register across the loop and
//   writes lo >> 11 of every other draw straight beside it, and K1V_BASE is a scalar addend. The instruction
//   count is unchanged and K1 is 4.8 % faster (profiles/r12/INDEX.md). Two held copies of each high word (one per
//   draw in flight, four moves a quad fewer, 100 VGPRs) measured 0.4 % SLOWER and were not kept.
constexpr uint32_t K1V_HI_WORD = 0x41300000u, K1V_LO_WORD = 0x3FE00000u;
constexpr double K1V_BASE = 0x1.0p20 + 1.5;
MSIM_HD double k1p_v(uint64_t u)
{
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    const double dh = __builtin_bit_cast(double, ((uint64_t)K1V_HI_WORD << 32) | hi);
    const double dl = __builtin_bit_cast(double, ((uint64_t)K1V_LO_WORD << 32) | (lo >> 11));
    const double c = K1V_BASE - dh;
    return c - dl;
}
constexpr uint32_t K1P_OK_HI = 0x3FEFFFFAu;  // hi(1 - 2.5e-6) (exclusive)
constexpr uint32_t K1P_VH_MIN = (uint32_t)(1023 - (K1_EROWS - 1)) << 20;  // high word of 2^-15
// z - M of the packed form; vh = the high word of v, r = the polynomial's argument.
MSIM_HD double k1p_interval_z(uint64_t u, const K1Pair *__restrict__ P, uint32_t &vh, double &r, FdConsts kc = MSIM_K1_CONSTS)
{
    const double v = k1p_v(u);
    vh = (uint32_t)(__builtin_bit_cast(uint64_t, v) >> 32);
    const uint32_t off = (vh >> (FD_VT_SHIFT + 3 - 4)) & ((K1_EROWS * LOG_TAB - 1u) << 4);
    const K1Pair en = *(const K1Pair *)((const char *)P + off);
    r = __builtin_fma(v, en.invc, -1.0);
#if MSIM_FD_DEG4
    double p = __builtin_fma(r, kc.c4, kc.c3);
#else
    double p = __builtin_fma(r, kc.c5, kc.c4);
    p = __builtin_fma(r, p, kc.c3);
#endif
    p = __builtin_fma(r, p, kc.c2);
    p = __builtin_fma(r, p, kc.c1);
    return __builtin_fma(r, p, en.A);
}
// Interval and acceptance key: the reference's value iff key < K1P_OK_HI and vh >= K1P_VH_MIN.
MSIM_HD int32_t k1p_interval_key(uint64_t u, const K1Pair *__restrict__ P, uint32_t &key, uint32_t &vh,
                                 FdConsts kc = MSIM_K1_CONSTS)
{
    double r;
    const double z = k1p_interval_z(u, P, vh, r, kc);
    const int32_t q = (int32_t)z;  // an accepted z is >= 0: truncation = floor
#if defined(__HIP_DEVICE_COMPILE__)
    const double f = __builtin_amdgcn_fract(z);
#else
    const double f = z - (double)q;
#endif
    key = (uint32_t)(__builtin_bit_cast(uint64_t, f) >> 32);
    return q;
}
// The packed form alone: ok == false sends the draw to the general form.
MSIM_HD int32_t k1p_interval_fast(uint64_t u, const K1Pair *__restrict__ P, bool &ok, FdConsts kc = MSIM_K1_CONSTS)
{
    uint32_t key, vh;
    const int32_t q = k1p_interval_key(u, P, key, vh, kc);
    ok = key < K1P_OK_HI && vh >= K1P_VH_MIN;
    return q;
}

// PickFinder's table index q = floor(u / PERC_MULTIPLIER), fast form: p = floor(100 u_hi / 2^32), exact
// unless `rare` (the low word of 100 u_hi is >= 2^32 - 128; q = p + 1 needs it >= 2^32 - 101).
constexpr uint32_t PICK_RARE_LO = 0xFFFFFF80u;  // low word of 100 u_hi at or above it: the exact path
MSIM_HD uint32_t pick_q_fast_key(uint64_t u, uint32_t &key)  // key = low word of 100 u_hi
{
    const uint32_t h = (uint32_t)(u >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t p = __umulhi(h, 100u);
#else
    const uint32_t p = (uint32_t)(((uint64_t)h * 100u) >> 32);
#endif
    key = h * 100u;
    return p;
}
MSIM_HD uint32_t pick_q_fast(uint64_t u, bool &rare)
{
    uint32_t key;
    const uint32_t p = pick_q_fast_key(u, key);
    rare = key >= PICK_RARE_LO;
    return p;
}
// Exact q for any u: p or p + 1, exactly when u >= (p+1) * PERC_MULTIPLIER.
MSIM_HD uint32_t pick_q_exact(uint64_t u)
{
    bool rare;
    const uint32_t p = pick_q_fast(u, rare);
    return p + (u >= (uint64_t)(p + 1) * PERC_MULTIPLIER ? 1u : 0u);
}
MSIM_HD uint32_t pick_info(uint64_t u, const PickTab *__restrict__ tab)
{
    bool rare;
    uint32_t q = pick_q_fast(u, rare);
    if (rare) q = pick_q_exact(u);
    return tab->info[q];
}

// K1's picker draw: the fast pick reads only the high word h of the draw, so the output step
// rotl(s0 + s1, 17) + s0 is formed in its high half alone: the 64-bit sum, the high half of the rotate, and a
// 32-bit add that leaves out the carry of the low halves. The state update is rng_next's. The result h' has
// h = h' or h' + 1 (mod 2^32). With 100 h' = p 2^32 + key and key < PICK_HI_RARE_LO = 2^32 - 256:
// 100 (h' + 1) = p 2^32 + key + 100 with key + 100 < 2^32 - 156, so h' + 1 has the same p and its low word is
// below PICK_RARE_LO: q = p for either carry. (h' = 2^32 - 1, whose successor wraps, has key = 2^32 - 100: rare.)
// A key at or above the band (6e-8 of draws) sends the quad to pick_q_exact on the full rng_next, as before.
// K1's quad takes the table offset and the key from one multiply with 400 instead (pick_off400_key below, where
// the argument is redone with its constants: band 2^32 - 1024 on the low word of 400 h').
constexpr uint32_t PICK_HI_RARE_LO = 0xFFFFFF00u;  // low word of 100 h' at or above it: the exact path
template <bool SHL64 = false>
MSIM_HD uint32_t rng_next_hi(Rng &r)
{
    const uint32_t h = (uint32_t)(rotl64(r.s0 + r.s1, 17) >> 32) + (uint32_t)(r.s0 >> 32);
    (void)rng_next<SHL64>(r);  // the state update; its own output step is unused and compiles away
    return h;
}
// p = floor(100 h / 2^32) and its key (the low word of 100 h): pick_q_fast_key on a high word.
MSIM_HD uint32_t pick_p_key(uint32_t h, uint32_t &key) { return pick_q_fast_key((uint64_t)h << 32, key); }

// What K1's quad runs instead: ONE 32 x 32 -> 64 multiply, 400 h' = t 2^32 + L (t < 400; v_mad_u64_u32), gives
// both the table's byte offset and the key; pick_p_key above stays the checked definition it is compared with
// (tests/native/k1pick400_check.cpp, over all 2^32 values of h').
//   Offset: 400 h' / 2^32 = 4 * (100 h' / 2^32), and floor(floor(x) / 4) = floor(x / 4), so t >> 2 = p and
//   t & ~3 = 4 p, the byte offset of info[p]: one v_and_b32 where the multiply with 100 needed a shift.
//   Key: write t = 4 p + j (j = 0..3). Then 100 h' = p 2^32 + (j 2^32 + L) / 4 (the division is exact), i.e.
//   pick_p_key's key is (j 2^32 + L) / 4. For L < PICK400_RARE_LO = 2^32 - 1024 that key is below
//   (3 * 2^32 + 2^32 - 1024) / 4 = 2^32 - 256 = PICK_HI_RARE_LO for every j, and the carry argument above
//   applies as it stands: q = p for h' and for h' + 1, with any low word. (Conversely pick_p_key's band,
//   j = 3 and L >= 2^32 - 1024, lies inside L >= PICK400_RARE_LO: testing L alone flags a superset, 1024 / 2^32 =
//   2.4e-7 of draws against 6e-8, next to the 3.3e-5 of the interval's check.)
//   h' = 2^32 - 1, whose successor wraps: 400 h' = 399 * 2^32 + (2^32 - 400), L = 2^32 - 400 is in the band.
constexpr uint32_t PICK400_RARE_LO = 0xFFFFFC00u;  // low word of 400 h' at or above it: the exact path
MSIM_HD uint32_t pick_off400_key(uint32_t h, uint32_t &key)  // the byte offset of info[p]; key = low word of 400 h
{
    const uint64_t m = (uint64_t)h * 400u;
    key = (uint32_t)m;
    return (uint32_t)(m >> 32) & ~3u;
}

// ---------------------------------------------------------------- host table builders
inline void build_log_table(LogTab *out)
{
    for (int j = 0; j < LOG_TAB; ++j) {
        const double c = 1.0 + (j + 0.5) / LOG_TAB;
        const double invc = 1.0 / c;
        out->invc[j] = invc;
        const long double L = -logl((long double)invc);  // log(1/invc), 80-bit
        out->A[j] = (double)((0.5L - 6e11L * L) * 1e-6L);
    }
}

// K1's log table: every entry computed in 80-bit arithmetic and rounded once.
inline void build_k1_log(K1Log *out)
{
    const long double ce = -6e5L * 6.931471805599453094172321214581766e-01L;
    for (int j = 0; j < LOG_TAB; ++j) {
        const double invc = 1.0 / (1.0 + (j + 0.5) / LOG_TAB);  // the same invc as build_log_table
        out->invc[j] = invc;
        const long double a = (0.5L - 6e11L * -logl((long double)invc)) * 1e-6L + FD4_K0;
        for (int eps = 0; eps < K1_EROWS; ++eps) {
            const long double ae = a + (eps - (K1_EROWS - 1)) * ce;
            out->A2[eps * LOG_TAB + j] = (double)ae;
            // the packed form's entry: invc scaled by 2^-e (exact), A less the acceptance margin
            out->P[eps * LOG_TAB + j] = K1Pair{ldexp(invc, K1_EROWS - 1 - eps), (double)(ae - (long double)K1_MARGIN_NS * 1e-6L)};
        }
    }
}

// perc: integer percentages summing to 100 (validated by the caller); prop: ms; selfish flags.
inline void build_pick_table(const uint64_t *perc, const int64_t *prop, const uint8_t *selfish, int m, PickTab *out)
{
    for (int q = 0; q < 128; ++q) {
        uint64_t cum = 0;
        int k = 15;
        for (int i = 0; i < m && q < PICK_TAB; ++i) {
            cum += perc[i];
            if (cum > (uint64_t)q) {
                k = i;
                break;
            }
        }
        uint32_t fthr = FTHR_CAP;
        if (k < 15 && !selfish[k]) fthr = prop[k] < (int64_t)FTHR_CAP ? (uint32_t)prop[k] : FTHR_CAP;
        out->info[q] = make_info((uint32_t)k, fthr);
    }
}

// K1's uniform-delay form (MSIM_K1_UNI): when every miner is honest with the same fast threshold (c1, c2, most
// presets), K1 compares the next interval with that one scalar and its pick table holds only the finder's
// counter row offset (k << INFO_K_SHIFT, threshold bits zero: info_finder still reads it).
// PickFinder's fall-through entries (k = 15; percentages summing below 100) have no threshold of their own in
// this form, so their "fast" bit is arbitrary. That is harmless: what sends such a run to the retry path is
// not the fast bit but the counter of owner 15, which K1 increments through the same row offset in both forms.
// combine_run (msim_pipeline.h) returns false, i.e. retry, when that counter is nonzero in a segment before
// the run's end (`ft`), in the end group's cumulative counters (gc[CNT_WORDS - 1] >> 16) or for a block of the
// redrawn end group (klast == 15); blocks after the end are in neither form's result
// (tests/test_pipeline_k1_host.py runs both forms on a network with such a gap).
#ifndef MSIM_K1_UNI
#define MSIM_K1_UNI 1
#endif
inline bool k1_uniform_fthr(const int64_t *prop, const uint8_t *selfish, int m, uint32_t *fthr)
{
    if (!MSIM_K1_UNI || m < 1) return false;
    for (int k = 0; k < m; ++k)
        if (selfish[k] || prop[k] != prop[0]) return false;
    *fthr = prop[0] < (int64_t)FTHR_CAP ? (uint32_t)prop[0] : FTHR_CAP;
    return true;
}
inline void build_k1_pick(const uint64_t *perc, const int64_t *prop, const uint8_t *selfish, int m, bool uni, PickTab *out)
{
    build_pick_table(perc, prop, selfish, m, out);
    if (uni)
        for (int q = 0; q < 128; ++q) out->info[q] &= 15u << INFO_K_SHIFT;
}

}  // namespace msim

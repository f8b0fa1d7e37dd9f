// k1v_check.cpp — TEST INFRASTRUCTURE: the packed form's v = 1 - (u>>11) 2^-53 built without integer-to-double
// conversions (msim_fastdraw.h k1p_v) against the two-conversion form of the general interval
// (interval_fast_z, k1_interval_z_on), bit for bit. A stand-alone program (built with
// -fsanitize=address,undefined by tests/test_k1pick400.py).
//
//   k1v_check [N_RANDOM]   -> prints counts as JSON
//
// Inputs: u = 0, 2^11 - 1, 2^11, 2^64 - 1, every u with a single one bit, every u with a single zero bit, and
// N_RANDOM draws of the reference's generator (half of them with their top bits set, so that v is small).
#include <stdio.h>
#include <stdlib.h>

#include "../../miningsimulation_amd/csrc/msim_fastdraw.h"

using namespace msim;

// the general form's v, as interval_fast_z writes it
static double v_two_conversions(uint64_t u)
{
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    const double c = __builtin_fma((double)(lo >> 11), -0x1.0p-53, 1.0);
    return __builtin_fma((double)hi, -0x1.0p-32, c);
}

struct Tally {
    uint64_t n, differs, differs_from_plain, out_of_range, first_bad;
};

static void check(uint64_t u, Tally *t)
{
    const double a = k1p_v(u), b = v_two_conversions(u);
    const double plain = 1.0 - (double)(u >> 11) * 0x1.0p-53;  // u >> 11 < 2^53: the conversion is exact
    bool bad = false;
    t->n++;
    if (__builtin_bit_cast(uint64_t, a) != __builtin_bit_cast(uint64_t, b)) t->differs++, bad = true;
    if (__builtin_bit_cast(uint64_t, a) != __builtin_bit_cast(uint64_t, plain)) t->differs_from_plain++, bad = true;
    if (!(a >= 0x1.0p-53 && a <= 1.0)) t->out_of_range++, bad = true;
    if (bad && !t->first_bad) t->first_bad = u;
}

static void print(const char *name, const Tally &t, const char *end)
{
    printf("\"%s\": {\"n\": %llu, \"differs\": %llu, \"differs_from_plain\": %llu, \"out_of_range\": %llu, \"first_bad\": %llu}%s",
           name, (unsigned long long)t.n, (unsigned long long)t.differs, (unsigned long long)t.differs_from_plain,
           (unsigned long long)t.out_of_range, (unsigned long long)t.first_bad, end);
}

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    Tally special{}, one_bit{}, zero_bit{}, rnd{};
    check(0, &special);
    check((1ull << 11) - 1, &special);
    check(1ull << 11, &special);
    check(~0ull, &special);
    for (int b = 0; b < 64; ++b) {
        check(1ull << b, &one_bit);
        check(~(1ull << b), &zero_bit);
    }
    Rng r = rng_seed(0x6b31765eedull);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t u = rng_next(r);
        // every other draw with 1 .. 53 leading ones: v down to 2^-53, through every exponent
        check(i & 1 ? u | ~(~0ull >> (1 + (i >> 1) % 53)) : u, &rnd);
    }
    // the held high words are the constants the subtraction's exactness rests on
    printf("{\"hi_word\": %llu, \"lo_word\": %llu, \"base\": %.17g, ", (unsigned long long)K1V_HI_WORD,
           (unsigned long long)K1V_LO_WORD, K1V_BASE);
    print("special", special, ", ");
    print("one_bit", one_bit, ", ");
    print("zero_bit", zero_bit, ", ");
    print("random", rnd, "}\n");
    return 0;
}

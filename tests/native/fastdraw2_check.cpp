// fastdraw2_check.cpp — TEST INFRASTRUCTURE: K1's form of the fast interval (msim_fastdraw.h, "K1's form":
// exponent folded into the table, degree-4 minimax polynomial, 1.25 ns margin) against glibc's sequence, i.e.
// against exactly what the reference calls, in the build-switch combination it is compiled with.
//
//   fastdraw2_check N_RANDOM THREADS    -> prints counts as JSON
//   fastdraw2_check crafted FILE        -> writes the crafted inputs as (u, reference interval) uint64 pairs
//
// An "accepted" value is one a form returns with ok == true; the chain is K1's: the fast form, then the general
// form, then glibc's sequence (msim_pipeline.h k1_quad_fast / k1_quad_exact).
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_draws.h"
#include "../../miningsimulation_amd/csrc/msim_fastdraw.h"

static msim::K1Log g_k1;
static msim::LogTab g_log;  // the general form's table (today's error, for the margin comparison)

static int64_t ref_interval(uint64_t u)
{
    const double e = -log1p((double)(u >> 11) * -0x1.0p-53);
    const long long ns = llround(msim::BLOCK_INTERVAL_NS * e);
    return (int64_t)(ns / 1000000LL);
}

// e of v = 1 - (u>>11) 2^-53 = 2^e w (exact in a double)
static int exponent_of(uint64_t u)
{
    int e;
    frexp(1.0 - (double)(u >> 11) * 0x1.0p-53, &e);
    return e - 1;
}

struct Tally {
    uint64_t n, bad_fast, bad_general, bad_chain, rejected_fast, rejected_general, low_e, low_e_accepted, first_bad_u;
    double max_err_ns;  // |K1 fast 6e11*E + 0.5 - (fl(6e11*E_glibc) + 0.5)| over inputs with e >= -15
    double general_max_err_ns;  // the same for interval_fast_z (the general form), every input
};

static void check(uint64_t u, Tally *t)
{
    const int64_t ref = ref_interval(u);
    bool okf, okg;
    const int32_t qf = msim::k1_interval_fast(u, &g_k1, okf);
    const int32_t qg = msim::k1_interval_general(u, &g_k1, okg);
    const bool low = exponent_of(u) < -(msim::K1_EROWS - 1);
    t->n++;
    if (low) t->low_e++;
    if (low && okf && MSIM_FD_A2) t->low_e_accepted++;
    if (!okf) t->rejected_fast++;
    if (!okg) t->rejected_general++;
    bool bad = false;
    if (okf && qf != ref) t->bad_fast++, bad = true;
    if (okg && qg != ref) t->bad_general++, bad = true;
    const int64_t chain = okf ? qf : okg ? qg : msim::interval_ms_of(u);
    if (chain != ref) t->bad_chain++, bad = true;
    if (bad && !t->first_bad_u) t->first_bad_u = u;
    if (!low || !MSIM_FD_A2) {
        const double e = -log1p((double)(u >> 11) * -0x1.0p-53);
        uint32_t vt;
        const double err = fabs(msim::k1_interval_z<MSIM_FD_A2 != 0>(u, &g_k1, vt) * 1e6 - (msim::BLOCK_INTERVAL_NS * e + 0.5));
        if (err > t->max_err_ns) t->max_err_ns = err;
    }
    {
        const double e = -log1p((double)(u >> 11) * -0x1.0p-53);
        const double err = fabs(msim::interval_fast_z(u, &g_log) * 1e6 - (msim::BLOCK_INTERVAL_NS * e + 0.5));
        if (err > t->general_max_err_ns) t->general_max_err_ns = err;
    }
}

static void add(Tally *a, const Tally &b)
{
    a->n += b.n;
    a->bad_fast += b.bad_fast;
    a->bad_general += b.bad_general;
    a->bad_chain += b.bad_chain;
    a->rejected_fast += b.rejected_fast;
    a->rejected_general += b.rejected_general;
    a->low_e += b.low_e;
    a->low_e_accepted += b.low_e_accepted;
    if (!a->first_bad_u) a->first_bad_u = b.first_bad_u;
    if (b.max_err_ns > a->max_err_ns) a->max_err_ns = b.max_err_ns;
    if (b.general_max_err_ns > a->general_max_err_ns) a->general_max_err_ns = b.general_max_err_ns;
}

// u whose 6e11*E + 0.5 lies within +-4 ns of a millisecond boundary (draws_check.cpp near_boundaries).
static void near_boundaries(int n, std::vector<uint64_t> *out)
{
    msim::Rng r = msim::rng_seed(99);
    for (int i = 0; i < n; ++i) {
        // every other one below 6.2e6 ms, where the exponent is inside the folded table's range
        const double qms = (double)(msim::rng_next(r) % (i & 1 ? 6200000ull : 22000000ull));
        const double off = ((double)(int64_t)(msim::rng_next(r) % 8001) - 4000.0) * 1e-3;
        const double y = qms * 1e6 - 0.5 + off;
        if (y <= 0) continue;
        const double v = exp(-y / msim::BLOCK_INTERVAL_NS);
        const double m = (1.0 - v) * 0x1.0p53;
        if (!(m >= 0 && m < 9007199254740991.0)) continue;
        const uint64_t mb = (uint64_t)m;
        for (int64_t d = -2; d <= 2; ++d) {
            const uint64_t mm = mb + (uint64_t)d;
            if (mm >= (1ull << 53)) continue;
            out->push_back((mm << 11) | (msim::rng_next(r) & 0x7FF));
        }
    }
}

// Every exponent of v (0 .. -53) x every table column x (first, middle, last) mantissa of the column.
static void exponent_grid(std::vector<uint64_t> *out)
{
    for (int e = 0; e >= -53; --e)
        for (uint64_t j = 0; j < 64; ++j)
            for (int pos = 0; pos < 3; ++pos) {
                // v = 2^e (1 + (j + f) / 64), f = 0, 1/2 and the largest below 1 for which v is a multiple of
                // 2^-53 (u>>11 = (1 - v) 2^53 is an integer); columns that small exponents cannot reach are skipped
                const int sh = -e;  // v 2^53 = wbits 2^(1 + e)
                const uint64_t mask = sh > 1 ? (1ull << (sh - 1)) - 1 : 0;
                const uint64_t frac = (pos == 0 ? 0 : pos == 1 ? (1ull << 45) : (1ull << 46) - 1) & ~mask;  // of 2^46
                const uint64_t wbits = (1ull << 52) | (j << 46) | frac;                                    // w 2^52
                if (e == 0 && (j || pos)) continue;  // v <= 1
                if (wbits & mask) continue;
                const uint64_t v53 = sh == 0 ? wbits << 1 : wbits >> (sh - 1);
                out->push_back((((1ull << 53) - v53) << 11) | 0x2A5);
            }
}

static void crafted(int near, std::vector<uint64_t> *out)
{
    near_boundaries(near, out);
    exponent_grid(out);
    out->push_back(0);
    out->push_back(~0ull);
    out->push_back(1ull << 11);
}

// The polynomial alone: K1's Horner form (the double coefficients, the FMAs of k1_interval_z) against an
// extended-precision -6e5 log1p(r) on a dense grid of |r| <= 2^-7, beside the general form's degree-5 Taylor
// polynomial. Errors in ns of 6e11*E.
static void poly_errors(double *k1_ns, double *general_ns)
{
    using namespace msim;  // the constants' macros name unqualified members
    const FdConsts k = MSIM_K1_CONSTS, g = MSIM_FD_DEFAULT;
    double ek = 0, eg = 0;
    const int N = 4000000;
    for (int i = 0; i <= N; ++i) {
        const double r = -0x1.0p-7 + 0x1.0p-6 * ((double)i / N);
        const long double want = -6e5L * log1pl((long double)r);
#if MSIM_FD_DEG4
        double p = __builtin_fma(r, k.c4, k.c3);
#else
        double p = __builtin_fma(r, k.c5, k.c4);
        p = __builtin_fma(r, p, k.c3);
#endif
        p = __builtin_fma(r, p, k.c2);
        p = __builtin_fma(r, p, k.c1);
        const long double got_k = (long double)r * (long double)p + msim::FD4_K0;
        double q = __builtin_fma(r, g.c5, g.c4);
        q = __builtin_fma(r, q, g.c3);
        q = __builtin_fma(r, q, g.c2);
        q = __builtin_fma(r, q, g.c1);
        const long double got_g = (long double)r * (long double)q;
        const double dk = (double)fabsl(got_k - want) * 1e6, dg = (double)fabsl(got_g - want) * 1e6;
        if (dk > ek) ek = dk;
        if (dg > eg) eg = dg;
    }
    *k1_ns = ek;
    *general_ns = eg;
}

struct Job {
    uint64_t n, seed;
    Tally t;
};

static void *worker(void *p)
{
    Job *j = (Job *)p;
    msim::Rng r = msim::rng_seed(j->seed);
    for (uint64_t i = 0; i < j->n; ++i) check(msim::rng_next(r), &j->t);
    return nullptr;
}

static void print_tally(const char *name, const Tally &t, const char *end)
{
    printf("\"%s\": {\"n\": %llu, \"bad_fast\": %llu, \"bad_general\": %llu, \"bad_chain\": %llu, \"rejected_fast\": %llu, "
           "\"rejected_general\": %llu, \"low_e\": %llu, \"low_e_accepted\": %llu, \"max_err_ns\": %.6g, \"general_max_err_ns\": %.6g, "
           "\"first_bad_u\": %llu}%s",
           name, (unsigned long long)t.n, (unsigned long long)t.bad_fast, (unsigned long long)t.bad_general,
           (unsigned long long)t.bad_chain, (unsigned long long)t.rejected_fast, (unsigned long long)t.rejected_general,
           (unsigned long long)t.low_e, (unsigned long long)t.low_e_accepted, t.max_err_ns, t.general_max_err_ns,
           (unsigned long long)t.first_bad_u, end);
}

int main(int argc, char **argv)
{
    msim::build_k1_log(&g_k1);
    msim::build_log_table(&g_log);
    if (argc > 2 && !strcmp(argv[1], "crafted")) {
        std::vector<uint64_t> us;
        crafted(400, &us);
        FILE *f = fopen(argv[2], "wb");
        if (!f) return 2;
        for (uint64_t u : us) {
            const uint64_t rec[2] = {u, (uint64_t)ref_interval(u)};
            if (fwrite(rec, 8, 2, f) != 2) return 2;
        }
        fclose(f);
        return 0;
    }
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000000ull;
    const int th = argc > 2 ? atoi(argv[2]) : 8;
    std::vector<Job> jobs((size_t)th);
    std::vector<pthread_t> t((size_t)th);
    for (int i = 0; i < th; ++i) {
        jobs[i] = Job{n / (uint64_t)th, 0x51ed5eedull + (uint64_t)i, Tally{}};
        pthread_create(&t[i], nullptr, worker, &jobs[i]);
    }
    Tally rnd{}, near{}, grid{}, special{};
    std::vector<uint64_t> us;
    near_boundaries(200000, &us);
    for (uint64_t u : us) check(u, &near);
    us.clear();
    exponent_grid(&us);
    for (uint64_t u : us) check(u, &grid);
    check(0, &special);
    check(~0ull, &special);
    check(1ull << 11, &special);
    double pk, pg;
    poly_errors(&pk, &pg);
    for (int i = 0; i < th; ++i) {
        pthread_join(t[i], nullptr);
        add(&rnd, jobs[i].t);
    }
    printf("{\"a2\": %d, \"deg4\": %d, \"margin_ns\": %.6g, \"general_margin_ns\": %.6g, \"poly_err_ns\": %.6g, "
           "\"general_poly_err_ns\": %.6g, ",
           MSIM_FD_A2, MSIM_FD_DEG4, msim::K1_MARGIN_NS, msim::MARGIN_NS, pk, pg);
    print_tally("random", rnd, ", ");
    print_tally("near_boundary", near, ", ");
    print_tally("exponent_grid", grid, ", ");
    print_tally("special", special, "}\n");
    return 0;
}

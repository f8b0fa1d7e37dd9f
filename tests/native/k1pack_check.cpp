// k1pack_check.cpp — TEST INFRASTRUCTURE: the forms K1's quad runs (msim_fastdraw.h "the packed form" and the
// high-word picker) against what they replace and against the reference.
//
//   k1pack_check N_RANDOM THREADS   -> prints counts as JSON
//   k1pack_check quads FILE         -> writes crafted quad start states with their expected draws (write_quads)
//
// Intervals: the packed form against glibc's sequence (llround / log1p, exactly what the reference calls) and,
// bit for bit, against the folded form k1_interval_fast, on the four input sets of fastdraw2_check.cpp (whose
// generators this file reuses by including it with its main() renamed).
// Picker: p(h') of the high-word output step against PickFinder's index u / PERC_MULTIPLIER.
#define main fastdraw2_check_main
#include "fastdraw2_check.cpp"
#undef main

using namespace msim;

static int64_t chain_interval(uint64_t u, bool *okp)
{
    bool okg;
    const int32_t qp = k1p_interval_fast(u, g_k1.P, *okp);
    if (*okp) return qp;
    const int32_t qg = k1_interval_general(u, &g_k1, okg);
    return okg ? qg : interval_ms_of(u);
}

struct PTally {
    uint64_t n, bad_packed, bad_chain, rejected, low_e, low_e_accepted, both, r_differs, q_differs, general_on_differs,
        first_bad_u;
    double max_err_ns, general_max_err_ns;
};

static void pcheck(uint64_t u, PTally *t)
{
    const int64_t ref = ref_interval(u);
    bool okp, okf, okg, okg2;
    const int32_t qp = k1p_interval_fast(u, g_k1.P, okp);
    const int32_t qf = k1_interval_fast(u, &g_k1, okf);
    const bool low = exponent_of(u) < -(K1_EROWS - 1);
    bool bad = false;
    t->n++;
    if (low) t->low_e++;
    if (low && okp) t->low_e_accepted++;
    if (!okp) t->rejected++;
    if (okp && qp != ref) t->bad_packed++, bad = true;
    bool okc;
    if (chain_interval(u, &okc) != ref) t->bad_chain++, bad = true;
    // the general form on the two small arrays K1 keeps is k1_interval_general
    const int32_t qg = k1_interval_general(u, &g_k1, okg);
    const int32_t qg2 = k1_interval_general_on(u, g_k1.invc, g_k1.A2 + (K1_EROWS - 1) * LOG_TAB, okg2);
    if (qg != qg2 || okg != okg2) t->general_on_differs++, bad = true;
    uint32_t vh, vt;
    double r;
    const double zp = k1p_interval_z(u, g_k1.P, vh, r);
    if (okp && okf) {
        // item 1 is an identity: the same r (recomputed here as the folded form does) and the same interval
        const double v = 1.0 - (double)(u >> 11) * 0x1.0p-53;
        const uint64_t vb = __builtin_bit_cast(uint64_t, v);
        const double w = __builtin_bit_cast(double, (vb & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
        const double rf = __builtin_fma(w, g_k1.invc[(vb >> 46) & 63], -1.0);
        t->both++;
        if (__builtin_bit_cast(uint64_t, rf) != __builtin_bit_cast(uint64_t, r)) t->r_differs++, bad = true;
        if (qp != qf) t->q_differs++, bad = true;
        // and the same z up to the folded margin's one rounding
        const double zf = k1_interval_z<true>(u, &g_k1, vt);
        if (fabs((zp + K1_MARGIN_NS * 1e-6) - zf) > 1e-8) t->q_differs++, bad = true;
    }
    if (bad && !t->first_bad_u) t->first_bad_u = u;
    const double e = -log1p((double)(u >> 11) * -0x1.0p-53);
    if (!low) {
        const double z = zp + K1_MARGIN_NS * 1e-6;
        const double err = fabs(z * 1e6 - (BLOCK_INTERVAL_NS * e + 0.5));
        if (err > t->max_err_ns) t->max_err_ns = err;
    }
    const double errg = fabs(interval_fast_z(u, &g_log) * 1e6 - (BLOCK_INTERVAL_NS * e + 0.5));
    if (errg > t->general_max_err_ns) t->general_max_err_ns = errg;
}

static void padd(PTally *a, const PTally &b)
{
    a->n += b.n, a->bad_packed += b.bad_packed, a->bad_chain += b.bad_chain, a->rejected += b.rejected;
    a->low_e += b.low_e, a->low_e_accepted += b.low_e_accepted, a->both += b.both, a->r_differs += b.r_differs;
    a->q_differs += b.q_differs, a->general_on_differs += b.general_on_differs;
    if (!a->first_bad_u) a->first_bad_u = b.first_bad_u;
    if (b.max_err_ns > a->max_err_ns) a->max_err_ns = b.max_err_ns;
    if (b.general_max_err_ns > a->general_max_err_ns) a->general_max_err_ns = b.general_max_err_ns;
}

static void pprint(const char *name, const PTally &t, const char *end)
{
    printf("\"%s\": {\"n\": %llu, \"bad_packed\": %llu, \"bad_chain\": %llu, \"rejected\": %llu, \"low_e\": %llu, "
           "\"low_e_accepted\": %llu, \"both\": %llu, \"r_differs\": %llu, \"q_differs\": %llu, \"general_on_differs\": %llu, "
           "\"max_err_ns\": %.6g, \"general_max_err_ns\": %.6g, \"first_bad_u\": %llu}%s",
           name, (unsigned long long)t.n, (unsigned long long)t.bad_packed, (unsigned long long)t.bad_chain,
           (unsigned long long)t.rejected, (unsigned long long)t.low_e, (unsigned long long)t.low_e_accepted,
           (unsigned long long)t.both, (unsigned long long)t.r_differs, (unsigned long long)t.q_differs,
           (unsigned long long)t.general_on_differs, t.max_err_ns, t.general_max_err_ns, (unsigned long long)t.first_bad_u, end);
}

// ---------------------------------------------------------------- picker
struct KTally {
    uint64_t n, settled, flagged, bad, state_differs;
};

// One draw's high-word key against the full draw u: h' is h or h - 1, and below the band p(h') is PickFinder's index.
static void kcheck_words(uint32_t hprime, uint64_t u, KTally *t)
{
    uint32_t key;
    const uint32_t p = pick_p_key(hprime, key);
    t->n++;
    if (key < PICK_HI_RARE_LO) {
        t->settled++;
        if (p != (uint32_t)(u / PERC_MULTIPLIER) || p != pick_q_exact(u)) t->bad++;
    } else {
        t->flagged++;
        if (pick_q_exact(u) != (uint32_t)(u / PERC_MULTIPLIER)) t->bad++;  // where the quad's redraw goes
    }
}

static void kcheck_state(Rng s, KTally *t)
{
    Rng a = s, b = s;
    const uint32_t hp = rng_next_hi(a);
    const uint64_t u = rng_next(b);
    if (a.s0 != b.s0 || a.s1 != b.s1) t->state_differs++;
    const uint32_t h = (uint32_t)(u >> 32);
    if (h != hp && h != hp + 1u) t->bad++;
    kcheck_words(hp, u, t);
}

// Every h' within +-512 of each of the 100 bucket boundaries (the smallest h with floor(100 h / 2^32) = b; b = 100:
// 2^32, reached from below only), both carries, low words 0, 1, 2^31, 2^32 - 2, 2^32 - 1 and the low word of the
// boundary b * PERC_MULTIPLIER and its two neighbours.
static void picker_boundaries(KTally *t)
{
    for (uint64_t b = 1; b <= 100; ++b) {
        const uint64_t hb = (b << 32) / 100 + ((b << 32) % 100 ? 1 : 0);
        const uint32_t blo = (uint32_t)(b * PERC_MULTIPLIER);
        const uint32_t lows[8] = {0u, 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, blo - 1u, blo, blo + 1u};
        for (int64_t d = -512; d <= 512; ++d) {
            const int64_t hp = (int64_t)hb + d;
            if (hp < 0 || hp > 0xFFFFFFFFll) continue;
            for (uint32_t carry = 0; carry < 2; ++carry)
                for (uint32_t lo : lows) kcheck_words((uint32_t)hp, ((uint64_t)((uint32_t)hp + carry) << 32) | lo, t);
        }
    }
}

// A state whose next output is u: s1 = rotr(u - s0, 17) - s0.
static Rng state_for_output(uint64_t s0, uint64_t u)
{
    const uint64_t x = u - s0;
    return Rng{s0, ((x >> 17) | (x << 47)) - s0};
}
// Crafted states: keys on both sides of the band's edge, with and without a carry out of the low halves.
// 100 h' = key (mod 2^32) has solutions only for key = 0 (mod 4): h' = (key / 4) * 25^-1 (mod 2^30), four of them.
static void picker_crafted(KTally *below, KTally *inside)
{
    uint64_t inv25 = 1;
    for (int i = 0; i < 6; ++i) inv25 = inv25 * (2 - 25 * inv25);  // Newton: 25^-1 mod 2^64
    Rng g = rng_seed(4242);
    for (int64_t dk = -64; dk < 64; ++dk) {
        const uint32_t key = PICK_HI_RARE_LO + (uint32_t)(4 * dk);  // through the band's edge up to 2^32 - 4
        for (uint32_t top = 0; top < 4; ++top) {
            const uint32_t hp = (uint32_t)((((uint64_t)(key / 4) * inv25) & 0x3FFFFFFFull) | ((uint64_t)top << 30));
            for (uint32_t carry = 0; carry < 2; ++carry)
                for (int rep = 0; rep < 4; ++rep) {
                    uint64_t s0 = rng_next(g);
                    uint32_t lo = (uint32_t)rng_next(g);
                    // a carry out of the low halves: rot_lo + s0_lo >= 2^32, i.e. u_lo < s0_lo
                    if (carry && (uint32_t)s0 == 0u) s0 |= 1u;
                    if (carry) lo %= (uint32_t)s0;
                    else if (lo < (uint32_t)s0) lo = (uint32_t)s0 + (lo % (0u - (uint32_t)s0));
                    const uint64_t u = ((uint64_t)(hp + carry) << 32) | lo;
                    const Rng s = state_for_output(s0, u);
                    Rng a = s;
                    KTally *t = key < PICK_HI_RARE_LO ? below : inside;
                    if (rng_next_hi(a) != hp) t->bad++;  // the crafting itself
                    kcheck_state(s, t);
                }
        }
    }
}

static void kprint(const char *name, const KTally &t, const char *end)
{
    printf("\"%s\": {\"n\": %llu, \"settled\": %llu, \"flagged\": %llu, \"bad\": %llu, \"state_differs\": %llu}%s", name,
           (unsigned long long)t.n, (unsigned long long)t.settled, (unsigned long long)t.flagged, (unsigned long long)t.bad,
           (unsigned long long)t.state_differs, end);
}

// ---------------------------------------------------------------- crafted quads for the device test
// The state before `s` (the inverse of xoroshiro128++'s linear update).
static Rng step_back(Rng s)
{
    const uint64_t t = (s.s1 >> 28) | (s.s1 << 36);  // rotr 28: s0 ^ s1 of the earlier state
    const uint64_t x = s.s0 ^ t ^ (t << 21);
    const uint64_t s0 = (x >> 49) | (x << 15);  // rotr 49
    return Rng{s0, t ^ s0};
}
// A start state whose draw number `pos` (0-3) is u.
static Rng start_for(uint64_t u, int pos, Rng *g)
{
    Rng s = state_for_output(rng_next(*g), u);
    for (int i = 0; i < pos; ++i) s = step_back(s);
    return s;
}
// Records of 64 bytes: ri, rp (4 x u64), then the four intervals and the four PickFinder indices
// u / PERC_MULTIPLIER (8 x u32) of sequential rng_next + interval_ms_of.
static int write_quads(const char *path)
{
    std::vector<uint64_t> iu, pu;
    near_boundaries(150, &iu);
    {
        std::vector<uint64_t> grid;
        exponent_grid(&grid);
        for (size_t i = 0; i < grid.size(); ++i)
            if (i % 5 == 0 || exponent_of(grid[i]) < -(K1_EROWS - 1) - 36) iu.push_back(grid[i]);
    }
    const size_t nreg = iu.size();
    for (int pos = 0; pos < 4; ++pos) iu.push_back(0), iu.push_back(~0ull), iu.push_back(1ull << 11);
    uint64_t inv25 = 1;
    for (int i = 0; i < 6; ++i) inv25 = inv25 * (2 - 25 * inv25);
    Rng g = rng_seed(777);
    // in-band picker draws (and the eight keys below the band's edge), without and with a carry, alternating
    for (int64_t dk = -8; dk < 64; ++dk)
        for (uint32_t top = 0; top < 4; ++top)
            for (uint32_t carry = 0; carry < 2; ++carry) {
                const uint32_t key = PICK_HI_RARE_LO + (uint32_t)(4 * dk);
                const uint32_t hp = (uint32_t)((((uint64_t)(key / 4) * inv25) & 0x3FFFFFFFull) | ((uint64_t)top << 30));
                // the low halves carry iff u_lo < s0_lo: low word 0 carries for any s0_lo != 0, 2^32 - 1 never does
                pu.push_back(((uint64_t)(hp + carry) << 32) | (carry ? 0u : 0xFFFFFFFFu));
            }
    // the top of the range: index 100, where PickFinder falls through (owner 15), and the last draw of index 99
    pu.push_back(~0ull), pu.push_back(100 * PERC_MULTIPLIER), pu.push_back(100 * PERC_MULTIPLIER - 1);
    FILE *f = fopen(path, "wb");
    if (!f) return 2;
    for (size_t i = 0; i < iu.size(); ++i) {
        const int posI = i < nreg ? (int)((i >> 3) & 3) : (int)((i - nreg) / 3), posP = (int)((i >> 1) & 3);
        const uint64_t upick = pu[i % pu.size()];
        const Rng rp = start_for(upick, posP, &g);
        const Rng ri = start_for(iu[i], posI, &g);
        Rng a = ri, b = rp;
        uint32_t out[8];
        for (int q = 0; q < 4; ++q) {
            out[q] = (uint32_t)interval_ms_of(rng_next(a));
            out[4 + q] = (uint32_t)(rng_next(b) / PERC_MULTIPLIER);
        }
        const uint64_t st[4] = {ri.s0, ri.s1, rp.s0, rp.s1};
        if (fwrite(st, 8, 4, f) != 4 || fwrite(out, 4, 8, f) != 8) return 2;
    }
    fclose(f);
    return 0;
}

struct PJob {
    uint64_t n, seed;
    PTally t;
    KTally k;
};

static void *pworker(void *p)
{
    PJob *j = (PJob *)p;
    Rng r = rng_seed(j->seed), s = rng_seed(j->seed ^ 0x9e3779b97f4a7c15ull);
    for (uint64_t i = 0; i < j->n; ++i) {
        pcheck(rng_next(r), &j->t);
        kcheck_state(s, &j->k);
        rng_next(s);
    }
    return nullptr;
}

int main(int argc, char **argv)
{
    build_k1_log(&g_k1);
    build_log_table(&g_log);
    if (argc > 2 && !strcmp(argv[1], "quads")) return write_quads(argv[2]);
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000000ull;
    const int th = argc > 2 ? atoi(argv[2]) : 8;
    std::vector<PJob> jobs((size_t)th);
    std::vector<pthread_t> t((size_t)th);
    for (int i = 0; i < th; ++i) {
        jobs[i] = PJob{n / (uint64_t)th, 0x51ed5eedull + (uint64_t)i, PTally{}, KTally{}};
        pthread_create(&t[i], nullptr, pworker, &jobs[i]);
    }
    PTally rnd{}, near{}, grid{}, special{};
    std::vector<uint64_t> us;
    near_boundaries(200000, &us);
    for (uint64_t u : us) pcheck(u, &near);
    us.clear();
    exponent_grid(&us);
    for (uint64_t u : us) pcheck(u, &grid);
    pcheck(0, &special);
    pcheck(~0ull, &special);
    pcheck(1ull << 11, &special);
    KTally kb{}, kbelow{}, kinside{}, krnd{};
    picker_boundaries(&kb);
    picker_crafted(&kbelow, &kinside);
    for (int i = 0; i < th; ++i) {
        pthread_join(t[i], nullptr);
        padd(&rnd, jobs[i].t);
        krnd.n += jobs[i].k.n, krnd.settled += jobs[i].k.settled, krnd.flagged += jobs[i].k.flagged;
        krnd.bad += jobs[i].k.bad, krnd.state_differs += jobs[i].k.state_differs;
    }
    printf("{\"margin_ns\": %.6g, \"general_margin_ns\": %.6g, ", K1_MARGIN_NS, MARGIN_NS);
    pprint("random", rnd, ", ");
    pprint("near_boundary", near, ", ");
    pprint("exponent_grid", grid, ", ");
    pprint("special", special, ", ");
    kprint("pick_boundaries", kb, ", ");
    kprint("pick_below_band", kbelow, ", ");
    kprint("pick_in_band", kinside, ", ");
    kprint("pick_random", krnd, "}\n");
    return 0;
}

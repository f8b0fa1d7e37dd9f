// sweep_shared_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over the shared-draw sweep's lane bodies
// (sweep_shared_body.h: split_segment, episode_entry with the index list, combine_run), built with AddressSanitizer
// and UBSan and run as a child process on the CPU (tests/test_sweep_shared_host.py). Every (point, run) is compared
// with the per-lane model (msim_model.h Sim::run, itself checked against the oracle by tests/test_model_host.py);
// the overflow cases must flag the runs the rules of msim_sweepsplit.h name and still give the model's counters.
#include <stdio.h>

#include "sweep_shared_body.h"

using namespace msim;

namespace {

int failures = 0;

struct Case {
    const char *name;
    int m;
    uint64_t perc[15];
    uint32_t np;
    int64_t props[6][15];
    int64_t duration;
    uint32_t n, env_cap, env_lcap, pt_cap[6], pt_lcap[6], max_group;
    int expect;  // 0: no run flagged; 1: some run flagged at every point; 2: flagged at point 0 only
};

template <int M>
void reference(const uint64_t *perc, const int64_t *prop, int64_t duration, uint32_t seed_base, uint64_t run, uint32_t *F,
               uint32_t *S)
{
    uint8_t self[15] = {0};
    SimParams sp;
    make_params(perc, prop, self, M, duration, &sp);
    RunResult rr;
    Sim<M, false, true, NX_WIDE, NG_WIDE> s;
    s.run(sp, rng_seed(seed_interval(seed_base, run)), rng_seed(seed_picker(seed_base, run)), rr);
    for (int k = 0; k < M; ++k) {
        F[k] = rr.found[k];
        S[k] = rr.stale[k];
    }
}

void run_case(const Case &c)
{
    const int m = c.m;
    std::vector<int64_t> props((size_t)c.np * m);
    for (uint32_t p = 0; p < c.np; ++p)
        for (int k = 0; k < m; ++k) props[(size_t)p * m + k] = c.props[p][k];
    std::vector<uint32_t> found((size_t)c.np * c.n * m), stale(found.size());
    std::vector<uint8_t> ok((size_t)c.np * c.n), lst(c.np);
    uint32_t ne = 0;
    const uint32_t seed = 4242;
    const int rc = sshost::shared_run_m(m, c.perc, props.data(), c.np, c.duration, seed, 7, c.n, 8192, c.env_cap, c.env_lcap,
                                        c.pt_cap, c.pt_lcap, c.max_group, found.data(), stale.data(), ok.data(), lst.data(), &ne);
    if (rc) {
        printf("FAIL %s: rc %d\n", c.name, rc);
        ++failures;
        return;
    }
    std::vector<uint32_t> flagged(c.np, 0);
    for (uint32_t p = 0; p < c.np; ++p) {
        if (!lst[p]) {
            printf("FAIL %s: point %u listing differs from its own tables'\n", c.name, p);
            ++failures;
        }
        for (uint32_t r = 0; r < c.n; ++r) {
            uint32_t F[15], S[15];
            switch (m) {
#define CASE(MM) \
    case MM:     \
        reference<MM>(c.perc, &props[(size_t)p * m], c.duration, seed, 7 + r, F, S); \
        break;
                MSIM_FOR_EACH_M(CASE)
#undef CASE
            }
            flagged[p] += ok[(size_t)p * c.n + r] != 1;
            for (int k = 0; k < m; ++k)
                if (found[((size_t)p * c.n + r) * m + k] != F[k] || stale[((size_t)p * c.n + r) * m + k] != S[k]) {
                    printf("FAIL %s: point %u run %u miner %d\n", c.name, p, r, k);
                    ++failures;
                    k = m;
                }
        }
    }
    bool shape = true;
    if (c.expect == 0)
        for (uint32_t p = 0; p < c.np; ++p) shape = shape && flagged[p] == 0;
    if (c.expect == 1)
        for (uint32_t p = 0; p < c.np; ++p) shape = shape && flagged[p] > 0;
    if (c.expect == 2)
        for (uint32_t p = 0; p < c.np; ++p) shape = shape && (p == 0 ? flagged[p] > 0 : flagged[p] == 0);
    if (!shape) {
        printf("FAIL %s: flagged runs per point:", c.name);
        for (uint32_t p = 0; p < c.np; ++p) printf(" %u", flagged[p]);
        printf(" (expected shape %d)\n", c.expect);
        ++failures;
    }
    printf("%s: %u envelope entries, flagged", c.name, ne);
    for (uint32_t p = 0; p < c.np; ++p) printf(" %u", flagged[p]);
    printf("\n");
}

}  // namespace

int main()
{
    const int64_t Y = 31556952000ll;
    static const Case cases[] = {
        {"uniform3", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 3,
         {{10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000}, {1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000},
          {100, 100, 100, 100, 100, 100, 100, 100, 100}}, Y / 12, 6, 0, 0, {0}, {0}, 0, 0},
        {"hetero", 4, {40, 30, 20, 10}, 3, {{10000, 100, 100, 100}, {100, 10000, 10000, 10000}, {0, 1000, 2000, 3000}}, Y / 12, 6,
         0, 0, {0}, {0}, 2, 0},
        {"five_in_passes_of_two", 2, {70, 30}, 5, {{60000, 60000}, {10000, 0}, {0, 10000}, {1, 1}, {0, 0}}, Y / 24, 4, 0, 0, {0},
         {0}, 2, 0},
        {"short", 1, {100}, 2, {{5000}, {0}}, 1, 4, 0, 0, {0}, {0}, 0, 0},
        {"zero", 3, {50, 25, 25}, 2, {{5000, 1, 0}, {0, 0, 0}}, 0, 4, 0, 0, {0}, {0}, 0, 0},
        {"env_cap", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 2,
         {{10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000}, {100, 100, 100, 100, 100, 100, 100, 100, 100}}, Y, 6, 1,
         0, {0}, {0}, 0, 1},
        {"env_lcap", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 2,
         {{10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000}, {100, 100, 100, 100, 100, 100, 100, 100, 100}}, Y, 6, 0,
         3, {0}, {0}, 0, 1},
        {"point_cap", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 2,
         {{10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000}, {100, 100, 100, 100, 100, 100, 100, 100, 100}}, Y, 6, 0,
         0, {1, 0}, {0}, 0, 2},
        {"point_lcap", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 2,
         {{10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000, 10000}, {100, 100, 100, 100, 100, 100, 100, 100, 100}}, Y, 6, 0,
         0, {0}, {3, 0}, 0, 2},
    };
    for (const Case &c : cases) run_case(c);
    printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

// pipe_overflow_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over the honest pipeline's lane bodies with
// capacities lowered to what tests/test_gpu_pipe_overflow.py sets on the device (MSIM_PIPE_TEST_*, include/msim.h):
// draw_segment, episode_entry and combine_run of the plain pipeline (pipeline_body.h), and the envelope's draws,
// split_segment, episode_entry with the index list and combine_run per point of a shared-draw group
// (sweep_shared_body.h). Built with AddressSanitizer and UBSan and run as a child process on the CPU
// (tests/test_pipeline_host.py). Every buffer a capacity sizes is allocated at exactly the lowered size, so an access
// the lowered capacity does not guard fails here, before the same values reach a GPU. Every run the pipeline does not
// flag must equal the per-lane model (msim_model.h Sim::run, itself checked against the oracle by
// tests/test_model_host.py), and each case names how many runs it must flag: none, some, or all.
#include <stdio.h>

#include "pipeline_body.h"
#include "sweep_shared_body.h"

using namespace msim;

namespace {

int failures = 0;
const uint32_t SEED = 1000, N = 257;

template <int M>
void reference(const uint64_t *perc, const int64_t *prop, int64_t duration, uint64_t run, uint32_t *F, uint32_t *S)
{
    uint8_t self[15] = {0};
    SimParams sp;
    make_params(perc, prop, self, M, duration, &sp);
    RunResult rr;
    Sim<M, false, true, NX_WIDE, NG_WIDE> s;
    s.run(sp, rng_seed(seed_interval(SEED, run)), rng_seed(seed_picker(SEED, run)), rr);
    for (int k = 0; k < M; ++k) {
        F[k] = rr.found[k];
        S[k] = rr.stale[k];
    }
}

// The miner counts of the cases below (each is one instantiation of every lane body: the build stays short).
#define CHECK_FOR_EACH_M(X) X(1) X(2) X(9) X(15)

void reference_m(int m, const uint64_t *perc, const int64_t *prop, int64_t duration, uint64_t run, uint32_t *F, uint32_t *S)
{
    switch (m) {
#define CASE(MM) \
    case MM:     \
        reference<MM>(perc, prop, duration, run, F, S); \
        break;
        CHECK_FOR_EACH_M(CASE)
#undef CASE
    }
}

int plain_m(int m, const uint64_t *perc, const int64_t *prop, int64_t duration, const pipehost::Overrides &ov, uint32_t *found,
            uint32_t *stale, uint8_t *ok, uint32_t *n_episodes)
{
    uint8_t self[15] = {0};
    SimParams p;
    const int rc = make_params(perc, prop, self, m, duration, &p);
    if (rc) return rc;
    const double rho = pipehost::rho_of(perc, prop, m);
    switch (m) {
#define CASE(MM) \
    case MM:     \
        return pipehost::run_pipeline<MM>(p, perc, prop, self, rho, SEED, 0, N, 8192, ov, found, stale, ok, n_episodes, nullptr, nullptr);
        CHECK_FOR_EACH_M(CASE)
#undef CASE
    }
    return -1;
}

enum Expect { NONE, SOME, ALL };

bool shape_ok(Expect e, uint32_t flagged, uint32_t n) { return e == NONE ? flagged == 0 : e == ALL ? flagged == n : flagged > 0 && flagged < n; }

// Half of a launch's natural list count is asked for by lcap = HALF.
const uint32_t HALF = 0xFFFFFFFFu;

struct Plain {
    const char *name;
    int m;
    uint64_t perc[15];
    int64_t delay, duration;
    uint32_t cap, lcap;
    int kind;
    Expect expect;
};

void run_plain(const Plain &c)
{
    const int m = c.m;
    int64_t prop[15];
    for (int k = 0; k < 15; ++k) prop[k] = c.delay;
    std::vector<uint32_t> found((size_t)N * m), stale(found.size());
    std::vector<uint8_t> ok(N);
    uint32_t ne = 0;
    pipehost::Overrides ov;
    if (c.lcap == HALF) {  // the natural launch's list count first
        const int rc = plain_m(m, c.perc, prop, c.duration, ov, found.data(), stale.data(), ok.data(), &ne);
        if (rc) {
            printf("FAIL %s: rc %d\n", c.name, rc);
            ++failures;
            return;
        }
    }
    ov.cap = c.cap;
    ov.lcap = c.lcap == HALF ? (ne / 2 ? ne / 2 : 1) : c.lcap;
    ov.k2_kind = c.kind;
    const int rc = plain_m(m, c.perc, prop, c.duration, ov, found.data(), stale.data(), ok.data(), &ne);
    if (rc) {
        printf("FAIL %s: rc %d\n", c.name, rc);
        ++failures;
        return;
    }
    uint32_t flagged = 0;
    for (uint32_t r = 0; r < N; ++r) {
        if (!ok[r]) {
            ++flagged;
            continue;
        }
        uint32_t F[15], S[15];
        reference_m(m, c.perc, prop, c.duration, r, F, S);
        for (int k = 0; k < m; ++k)
            if (found[(size_t)r * m + k] != F[k] || stale[(size_t)r * m + k] != S[k]) {
                printf("FAIL %s: unflagged run %u miner %d differs from the model\n", c.name, r, k);
                ++failures;
                break;
            }
    }
    if (!shape_ok(c.expect, flagged, N)) {
        printf("FAIL %s: %u of %u runs flagged (expected shape %d)\n", c.name, flagged, N, (int)c.expect);
        ++failures;
    }
    printf("%s: cap %u lcap %u kind %d: list count %u, %u of %u runs flagged\n", c.name, ov.cap, ov.lcap, c.kind, ne, flagged, N);
}

struct Shared {
    const char *name;
    int m;
    uint64_t perc[15];
    uint32_t env_cap, env_lcap, pt_cap, pt_lcap, max_group;  // HALF: half of the envelope's / the point's list count
    int kind;
    Expect expect[3];  // per point: 10 s, 1 s, 100 ms
};

void run_shared(const Shared &c)
{
    const int m = c.m;
    const uint32_t np = 3;
    const int64_t delays[np] = {10000, 1000, 100}, D = 1000000000ll;
    std::vector<int64_t> props((size_t)np * m);
    for (uint32_t p = 0; p < np; ++p)
        for (int k = 0; k < m; ++k) props[(size_t)p * m + k] = delays[p];
    std::vector<uint32_t> found((size_t)np * N * m), stale(found.size());
    std::vector<uint8_t> ok((size_t)np * N), lst(np);
    uint32_t ne = 0, pt_cap[np], pt_lcap[np], env_lcap = c.env_lcap;
    for (uint32_t p = 0; p < np; ++p) {
        pt_cap[p] = c.pt_cap;
        pt_lcap[p] = c.pt_lcap;
    }
    if (c.env_lcap == HALF || c.pt_lcap == HALF) {  // the list counts: the envelope's, and each point's own network's
        std::vector<uint32_t> f((size_t)N * m), s(f.size());
        std::vector<uint8_t> o(N);
        for (uint32_t p = 0; p < np; ++p) {
            uint32_t cnt = 0;
            const int rc = plain_m(m, c.perc, &props[(size_t)p * m], D, pipehost::Overrides(), f.data(), s.data(), o.data(), &cnt);
            if (rc) {
                printf("FAIL %s: rc %d\n", c.name, rc);
                ++failures;
                return;
            }
            if (p == 0 && c.env_lcap == HALF) env_lcap = cnt / 2 ? cnt / 2 : 1;  // the envelope is the 10 s network
            if (c.pt_lcap == HALF) pt_lcap[p] = cnt / 2 ? cnt / 2 : 1;
        }
    }
    int rc = -1;
    switch (m) {
#define CASE(MM)                                                                                                             \
    case MM:                                                                                                                 \
        rc = sshost::shared_run<MM>(c.perc, props.data(), np, D, SEED, 0, N, 8192, c.env_cap, env_lcap, pt_cap, pt_lcap,     \
                                    c.max_group, found.data(), stale.data(), ok.data(), lst.data(), &ne, c.kind);            \
        break;
        CHECK_FOR_EACH_M(CASE)
#undef CASE
    }
    if (rc) {
        printf("FAIL %s: rc %d\n", c.name, rc);
        ++failures;
        return;
    }
    printf("%s: %u envelope entries, flagged", c.name, ne);
    for (uint32_t p = 0; p < np; ++p) {
        if (!lst[p]) {
            printf("\nFAIL %s: point %u listing differs from its own tables'\n", c.name, p);
            ++failures;
        }
        uint32_t flagged = 0;
        for (uint32_t r = 0; r < N; ++r) {
            uint32_t F[15], S[15];
            reference_m(m, c.perc, &props[(size_t)p * m], D, r, F, S);
            flagged += ok[(size_t)p * N + r] != 1;
            for (int k = 0; k < m; ++k)
                if (found[((size_t)p * N + r) * m + k] != F[k] || stale[((size_t)p * N + r) * m + k] != S[k]) {
                    printf("\nFAIL %s: point %u run %u miner %d differs from the model\n", c.name, p, r, k);
                    ++failures;
                    break;
                }
        }
        printf(" %u", flagged);
        if (!shape_ok(c.expect[p], flagged, N)) {
            printf("\nFAIL %s: point %u: %u runs flagged (expected shape %d)\n", c.name, p, flagged, (int)c.expect[p]);
            ++failures;
        }
    }
    printf("\n");
}

}  // namespace

int main()
{
    const int64_t D = 1000000000ll;
    // caps 13 and 16: ceil(lambda + 1.3 sqrt(lambda)) and ceil(lambda + 2.3 sqrt(lambda)) at lambda = rho * 544 = 8.99,
    // the 10 s network's segment of 544 blocks
    static const Plain plain[] = {
        {"natural", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 0, 0, -1, NONE},
        {"cap1", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 1, 0, -1, ALL},
        {"cap13", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 13, 0, -1, SOME},
        {"cap16", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 16, 0, -1, SOME},
        {"lcap1", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 0, 1, -1, ALL},
        {"lcap_half", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 0, HALF, -1, SOME},
        {"cap13_lcap_half_lean", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, D, 13, HALF, 0, SOME},
        {"lean_one_miner_one_read", 1, {100}, 45000, 5 * D, 0, 0, 0, SOME},
        {"lean_one_miner_1e9", 1, {100}, 45000, D, 0, 0, 0, SOME},
        {"lean_one_miner_batched", 1, {100}, 45000, D / 10, 0, 0, 0, SOME},
        {"mid_one_miner", 1, {100}, 45000, 5 * D, 0, 0, -1, NONE},
        {"lean_two_miners_one_read", 2, {70, 30}, 45000, 5 * D, 0, 0, 0, SOME},
        {"lean_two_miners_1e9", 2, {70, 30}, 45000, D, 0, 0, 0, SOME},
        {"lean_two_miners_batched", 2, {70, 30}, 45000, D / 10, 0, 0, 0, SOME},
        {"m1_cap13", 1, {100}, 10000, D, 13, 0, -1, SOME},
        {"m1_lcap_half", 1, {100}, 10000, D, 0, HALF, -1, SOME},
        {"m2_cap13", 2, {70, 30}, 10000, D, 13, 0, -1, SOME},
        {"m2_lcap_half", 2, {70, 30}, 10000, D, 0, HALF, -1, SOME},
        {"m15_cap13", 15, {20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1}, 10000, D, 13, 0, -1, SOME},
        {"m15_lcap_half", 15, {20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1}, 10000, D, 0, HALF, -1, SOME},
    };
    for (const Plain &c : plain) run_plain(c);
    static const Shared shared[] = {
        {"shared_natural", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 0, 0, 0, 0, 0, -1, {NONE, NONE, NONE}},
        {"shared_env_cap13", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 13, 0, 0, 0, 0, -1, {SOME, SOME, SOME}},
        {"shared_env_cap13_passes_of_2", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 13, 0, 0, 0, 2, -1, {SOME, SOME, SOME}},
        {"shared_env_cap1", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 1, 0, 0, 0, 0, -1, {ALL, ALL, ALL}},
        {"shared_point_cap13", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 0, 0, 13, 0, 0, -1, {SOME, NONE, NONE}},
        {"shared_point_cap1", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 0, 0, 1, 0, 0, -1, {ALL, SOME, SOME}},
        {"shared_lcaps_half", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 0, HALF, 0, HALF, 0, -1, {SOME, SOME, SOME}},
        {"shared_env_lcap1", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 0, 1, 0, 0, 0, -1, {ALL, ALL, ALL}},
        {"shared_all_lowered_lean", 9, {30, 29, 12, 11, 8, 5, 3, 1, 1}, 13, HALF, 13, HALF, 2, 0, {SOME, SOME, SOME}},
        {"shared_m15_env_cap13", 15, {20, 15, 12, 10, 8, 7, 6, 5, 4, 4, 3, 2, 2, 1, 1}, 13, 0, 0, 0, 0, -1, {SOME, SOME, SOME}},
    };
    for (const Shared &c : shared) run_shared(c);
    printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

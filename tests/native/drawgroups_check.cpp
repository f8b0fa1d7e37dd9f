// drawgroups_check.cpp — the draw-group planner (csrc/msim_drawgroups.h) alone, with stand-in predicates, under
// AddressSanitizer and UBSan (tests/test_drawgroups_host.py builds and runs it). A point is a draw key and one delay
// per miner; an envelope is taken when the sum over miners of the group's largest delay is below a bound.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../miningsimulation_amd/csrc/msim_drawgroups.h"

typedef std::vector<std::vector<uint32_t>> Groups;

struct Instance {
    std::vector<int> key;
    std::vector<std::vector<int64_t>> delay;  // [point][miner]
    int64_t bound;
    int64_t max_delay(uint32_t i) const { return *std::max_element(delay[i].begin(), delay[i].end()); }
    bool accepts(const std::vector<uint32_t> &g) const
    {
        int64_t sum = 0;
        for (size_t k = 0; k < delay[0].size(); ++k) {
            int64_t pe = 0;
            for (uint32_t i : g) pe = std::max(pe, delay[i][k]);
            sum += pe;
        }
        return sum < bound;
    }
};

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (++fails < 20) printf("line %d: %s\n", __LINE__, #c); \
        }                                                          \
    } while (0)

// The loop of the two group builders of csrc/msim_api.hip before the planner was written once, transcribed: `work`
// grows while it is walked; a group of one is taken as it is.
static void reference(const Instance &in, Groups *groups, std::vector<int32_t> *group_of)
{
    const uint32_t np = (uint32_t)in.key.size();
    Groups work;
    for (uint32_t i = 0; i < np; ++i) {
        bool placed = false;
        for (auto &g : work) {
            if (in.key[g[0]] == in.key[i]) {
                g.push_back(i);
                placed = true;
                break;
            }
        }
        if (!placed) work.push_back({i});
    }
    group_of->assign(np, -1);
    groups->clear();
    for (size_t g = 0; g < work.size(); ++g) {
        for (;;) {
            if (work[g].size() == 1 || in.accepts(work[g])) {
                groups->push_back(work[g]);
                break;
            }
            size_t worst = 0;
            for (size_t j = 1; j < work[g].size(); ++j)
                if (in.max_delay(work[g][j]) > in.max_delay(work[g][worst])) worst = j;
            const uint32_t pt = work[g][worst];
            work[g].erase(work[g].begin() + (long)worst);
            work.push_back({pt});
        }
        for (uint32_t i : work[g]) (*group_of)[i] = (int32_t)g;
    }
}

// Runs the planner; fail_at >= 0: the fail_at-th envelope call returns error 77. Returns the planner's code.
static int plan(const Instance &in, Groups *groups, std::vector<int32_t> *group_of, int fail_at = -1, int *calls = nullptr)
{
    int n = 0;
    const int rc = msim::plan_draw_groups(
        (uint32_t)in.key.size(), [&](uint32_t i, uint32_t j) { return in.key[i] == in.key[j]; },
        [&](uint32_t i) { return in.max_delay(i); },
        [&](const std::vector<uint32_t> &pts, bool *taken) {
            CHECK(pts.size() >= 2);  // never for a group of one
            if (n++ == fail_at) return 77;
            *taken = in.accepts(pts);
            return 0;
        },
        groups, group_of);
    if (calls) *calls = n;
    return rc;
}

static void check_result(const Instance &in, const Groups &groups, const std::vector<int32_t> &group_of)
{
    const size_t np = in.key.size();
    std::vector<int> seen(np, 0);
    CHECK(group_of.size() == np);
    for (size_t g = 0; g < groups.size(); ++g) {
        CHECK(!groups[g].empty());
        CHECK(std::is_sorted(groups[g].begin(), groups[g].end()));  // the caller's point order
        for (uint32_t i : groups[g]) {
            CHECK(i < np);
            if (i >= np) continue;
            ++seen[i];
            CHECK(in.key[i] == in.key[groups[g][0]]);  // one draw key per group
            CHECK(group_of[i] == (int32_t)g);
        }
        if (groups[g].size() >= 2) CHECK(in.accepts(groups[g]));
    }
    for (size_t i = 0; i < np; ++i) CHECK(seen[i] == 1);  // a partition
}

static Instance uniform(std::vector<int> key, std::vector<int64_t> d, int64_t bound)
{
    Instance in;
    in.key = key;
    for (int64_t x : d) in.delay.push_back({x});
    in.bound = bound;
    return in;
}

int main()
{
    std::mt19937_64 rng(20240611);
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    Groups g, rg;
    std::vector<int32_t> of, rof;
    for (int it = 0; it < 4000; ++it) {
        Instance in;
        const uint32_t np = 1 + (uint32_t)below(24), nk = 1 + (uint32_t)below(4), m = 1 + (uint32_t)below(5);
        const int64_t top = 1 + (int64_t)below(it % 3 ? 6 : 60000);  // every third instance: many ties
        for (uint32_t i = 0; i < np; ++i) {
            in.key.push_back((int)below(nk));
            in.delay.emplace_back();
            for (uint32_t k = 0; k < m; ++k) in.delay.back().push_back((int64_t)below((uint64_t)top + 1));
        }
        in.bound = (int64_t)below((uint64_t)(top * m * 2 + 2));
        CHECK(plan(in, &g, &of) == 0);
        reference(in, &rg, &rof);
        CHECK(g == rg);
        CHECK(of == rof);
        check_result(in, g, of);
    }
    // all points accepted as one group
    Instance in = uniform({0, 0, 0}, {10000, 1000, 100}, 1 << 30);
    CHECK(plan(in, &g, &of) == 0 && g == Groups({{0, 1, 2}}) && of == std::vector<int32_t>({0, 0, 0}));
    // nothing accepted: every point alone, the leavers behind the group they left, largest delay first
    in = uniform({0, 0, 0, 0}, {5, 9, 7, 1}, 0);
    CHECK(plan(in, &g, &of) == 0 && g == Groups({{3}, {1}, {2}, {0}}) && of == std::vector<int32_t>({3, 1, 2, 0}));
    // test_envelope_past_the_fork_rate_limit_is_split: two miners; 60 s at either one alone is taken, at both it is not
    in.key = {0, 0, 0};
    in.delay = {{60000, 0}, {0, 60000}, {100, 100}};
    in.bound = 100000;
    CHECK(plan(in, &g, &of) == 0 && g == Groups({{1, 2}, {0}}) && of == std::vector<int32_t>({1, 0, 0}));
    // ties in max_delay: the first of the tied points leaves
    in.key = {0, 0, 0, 1};
    in.delay = {{3, 0}, {8, 0}, {0, 8}, {8, 8}};
    in.bound = 12;
    CHECK(plan(in, &g, &of) == 0 && g == Groups({{0, 2}, {3}, {1}}) && of == std::vector<int32_t>({0, 2, 0, 1}));
    // two keys interleaved; a group of one costs no envelope call
    int calls = -1;
    in = uniform({0, 1, 0, 2, 1}, {1, 1, 1, 1, 1}, 1 << 30);
    CHECK(plan(in, &g, &of, -1, &calls) == 0 && g == Groups({{0, 2}, {1, 4}, {3}}) && calls == 2);
    CHECK(of == std::vector<int32_t>({0, 1, 0, 2, 1}));
    // an error from take_envelope comes back unchanged and stops the planning
    in = uniform({0, 0, 0, 1, 1}, {5, 9, 7, 1, 1}, 0);
    for (int fail_at = 0; fail_at < 3; ++fail_at) {
        CHECK(plan(in, &g, &of, fail_at, &calls) == 77);
        CHECK(calls == fail_at + 1);
    }
    CHECK(plan(in, &g, &of, 3, &calls) == 0 && calls == 3);  // {0,1,2}, {0,2}, {3,4}: no fourth call to fail
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}

// gen_tiers_check.cpp — TEST INFRASTRUCTURE: the general engine's tiers, lane reuse and run lists on the CPU, at the
// lowered limits of the test switches MSIM_GEN_TEST_* (msim_general_launch.h GenLimits). A stand-alone program built
// with -fsanitize=address,undefined and run by tests/test_general_host.py as a child process; the CPU dry run of
// tests/test_gpu_general_tiers.py.
//
// For every case it lays the workspace out with gen_ws_layout, allocates the lists, the counters and the two chain
// arrays as separate heap blocks of exactly the sizes the tiers need (so that ASan sees an index one past any of
// them), fills them with 0xFF, and walks the tiers as launch_gen_tiers and msim_gen_kernel do: lane l takes items
// l, l + lanes, ..., every item runs Gen<GenDevStore> with the kernel's pointer arithmetic, a GERR_CAP run goes to
// the next tier's list, the list bounds count what they drop. Every run is also computed on a private, freshly
// zeroed store at the same window: the error bits, found, stale and height must be the same, i.e. what a lane's
// earlier runs left behind changes nothing. The counters must account for every run: finished + failed = runs.
// Exit status 0 = all checks held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_general_launch.h"
#include "../../miningsimulation_amd/csrc/msim_model.h"

using namespace msim;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("gen_tiers_check: line %d: %s\n", __LINE__, #c);  \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Net {
    std::vector<uint64_t> cum;
    std::vector<int64_t> prop;
    std::vector<uint8_t> self;
    std::vector<uint32_t> cls;
    GenParams g;
    Net(std::vector<uint64_t> w, int64_t delay, bool selfish0, int64_t duration)
    {
        uint64_t c = 0;
        for (size_t k = 0; k < w.size(); ++k) {
            cum.push_back(c += w[k]);
            prop.push_back(delay);
            self.push_back(k == 0 && selfish0 ? 1 : 0);
            cls.push_back((uint32_t)k);
        }
        memset(&g, 0, sizeof(g));
        g.duration_ms = duration;
        g.mult = 0xFFFFFFFFFFFFFFFFull / c;
        g.m = (uint32_t)w.size();
        g.umax = GEN_GENESIS;
    }
    GenParams params() const
    {
        GenParams p = g;
        p.cum = cum.data();
        p.prop = prop.data();
        p.self = self.data();
        p.cls = cls.data();
        return p;
    }
};

struct RunOut {
    uint32_t err = 0, height = 0;
    std::vector<uint32_t> found, stale;
    bool operator==(const RunOut &o) const { return err == o.err && height == o.height && found == o.found && stale == o.stale; }
};

// One run on the given store (the kernel's loop body, msim_general.hip).
static RunOut run_on(GenDevStore &s, const GenParams &g, uint32_t seed_base, uint64_t run)
{
    for (uint32_t k = 0; k < g.m; ++k) {
        s.st[k * s.L] = 0;
        s.pr[k * s.L] = 0;
    }
    RunOut r;
    Gen<GenDevStore> e(s, g);
    GenOut o;
    if (!e.run(rng_seed(seed_interval(seed_base, run)), rng_seed(seed_picker(seed_base, run)), o)) {
        r.err = o.err;
        return r;
    }
    e.count_best(o);
    r.height = Gen<GenDevStore>::best_height(o);
    for (uint32_t k = 0; k < g.m; ++k) {
        r.found.push_back(e.found_after_count(k));
        r.stale.push_back(s.stale(k));
    }
    return r;
}

// The same run on a private store of zeroes with one lane.
static RunOut run_private(const GenParams &g, uint32_t cap, uint32_t seed_base, uint64_t run)
{
    std::vector<uint32_t> o((size_t)g.m * cap, 0u), c(3 * (size_t)g.m, 0u);
    std::vector<int64_t> a((size_t)g.m * cap, 0);
    GenDevStore s;
    s.cap = cap;
    s.L = 1;
    s.o = o.data();
    s.a = a.data();
    s.sz = c.data();
    s.st = c.data() + g.m;
    s.pr = c.data() + 2 * (size_t)g.m;
    return run_on(s, g, seed_base, run);
}

struct Counts {
    uint32_t finished[3] = {0, 0, 0}, failed = 0, l2 = 0, l3 = 0;
};

// All tiers over one workspace, as launch_gen_tiers: `listed` gives tier 1 a list of every code (the entity
// engine's hand-over) in place of the index range.
static Counts walk(const std::vector<Net> &nets, uint32_t rpp, bool full, const GenLimits &lim, bool listed,
                   double budget = 2048.0 * (1 << 20))
{
    const uint32_t np = (uint32_t)nets.size(), runs = rpp * np, seed_base = 1000;
    uint32_t max_m = 0;
    int64_t dur = 0;
    std::vector<GenParams> pts;
    for (const Net &n : nets) {
        pts.push_back(n.params());
        max_m = n.g.m > max_m ? n.g.m : max_m;
        dur = n.g.duration_ms > dur ? n.g.duration_ms : dur;
    }
    const GenWs w = gen_ws_layout(max_m, dur, runs, budget, full, lim);
    size_t lanes = 0, chain = 0;
    for (int i = 0; i < w.nt; ++i) {
        lanes = w.tier[i].lanes > lanes ? w.tier[i].lanes : lanes;
        const size_t c = w.tier[i].lanes * (size_t)max_m * w.tier[i].cap;
        chain = c > chain ? c : chain;
        CHECK(w.tier[i].lanes >= 1 && (!lim.lanes || w.tier[i].lanes <= lim.lanes));
        CHECK(!lim.cap[i] || w.tier[i].cap <= lim.cap[i]);
    }
    CHECK(w.list_limit >= 1 && w.list_limit <= w.list_cap && w.list_cap == runs);
    // the layout's regions hold what the tiers index
    CHECK(w.sizes_off - w.lists_off >= 3 * (size_t)w.list_cap * 4);
    CHECK(w.owners_off - w.sizes_off >= 3 * (size_t)max_m * lanes * 4);
    CHECK(w.arrivals_off - w.owners_off >= chain * 4);
    CHECK(w.total - w.arrivals_off >= chain * 8);
    uint32_t *lists = new uint32_t[3 * (size_t)w.list_cap];
    uint32_t *sizes = new uint32_t[3 * (size_t)max_m * lanes];
    uint32_t *owners = new uint32_t[chain];
    int64_t *arrivals = new int64_t[chain];
    memset(lists, 0xFF, 3 * (size_t)w.list_cap * 4);
    memset(sizes, 0xFF, 3 * (size_t)max_m * lanes * 4);
    memset(owners, 0xFF, chain * 4);
    memset(arrivals, 0xFF, chain * 8);
    uint32_t counts[GEN_C_WORDS] = {0};
    uint32_t *first = lists + 2 * (size_t)w.list_cap;  // where E2 leaves its list (msim_api.hip sel_launch_impl)
    if (listed) {
        for (uint32_t c = 0; c < runs; ++c) first[c] = runs - 1 - c;  // any order
        counts[GEN_C_L1] = runs;
    }
    std::vector<int> done(runs, 0);
    Counts out;
    for (int i = 0; i < w.nt; ++i) {
        const uint32_t cap = w.tier[i].cap, list_cap = w.list_limit;
        const size_t L = w.tier[i].lanes;
        const uint32_t *list = i == 0 ? (listed ? first : nullptr) : lists + (size_t)(i - 1) * w.list_cap;
        const uint32_t *list_count = i == 0 ? counts + GEN_C_L1 : counts + GEN_C_L1 + i;
        uint32_t *next = i + 1 < w.nt ? lists + (size_t)i * w.list_cap : nullptr;
        uint32_t *next_count = i + 1 < w.nt ? counts + GEN_C_L1 + i + 1 : nullptr;
        const uint32_t n_items = list ? *list_count : runs;
        const uint32_t items = list ? (n_items < list_cap ? n_items : list_cap) : n_items;
        if (list && n_items > list_cap) counts[GEN_C_FAIL] += n_items - list_cap;
        for (size_t lane = 0; lane < L; ++lane) {
            GenDevStore s;
            s.cap = cap;
            s.L = L;
            s.sz = sizes + lane;
            s.st = sizes + (size_t)max_m * L + lane;
            s.pr = sizes + 2 * (size_t)max_m * L + lane;
            for (uint32_t it = (uint32_t)lane; it < items; it += (uint32_t)L) {
                const uint32_t code = list ? list[it] : it;
                CHECK(code < runs);
                if (code >= runs) continue;
                const uint32_t point = code / rpp, rel = code % rpp;
                const GenParams &g = pts[point];
                s.o = owners + lane * (size_t)g.m * cap;
                s.a = arrivals + lane * (size_t)g.m * cap;
                const RunOut r = run_on(s, g, seed_base, rel);
                CHECK(r == run_private(g, cap, seed_base, rel));
                if (r.err) {
                    if ((r.err & GERR_CAP) && next) {
                        const uint32_t pos = (*next_count)++;
                        if (pos < list_cap) next[pos] = code;
                    } else {
                        ++counts[GEN_C_FAIL];
                    }
                    continue;
                }
                CHECK(!done[code]);
                done[code] = 1;
                ++out.finished[i];
                uint32_t sum = 0;
                for (uint32_t f : r.found) sum += f;
                CHECK(sum == r.height);  // distinct ids, none UINT_MAX: every block of the best chain has a finder
            }
        }
    }
    out.failed = counts[GEN_C_FAIL];
    out.l2 = counts[GEN_C_L2];
    out.l3 = counts[GEN_C_L3];
    uint32_t nd = 0;
    for (int d : done) nd += (uint32_t)d;
    CHECK(nd + out.failed == runs);  // every run is finished or counted failed, once
    CHECK(nd == out.finished[0] + out.finished[1] + out.finished[2]);
    delete[] lists;
    delete[] sizes;
    delete[] owners;
    delete[] arrivals;
    return out;
}

int main()
{
    const int64_t D = 259200000;  // 3 days
    const Net A({45, 30, 25}, 1000, true, D), B({60, 25, 15}, 100, true, D);
    const Net C({30, 29, 12, 11, 8, 5, 3, 1, 1}, 3600000, false, D), Dn({30, 29, 12, 11, 8, 5, 3, 1, 1}, 10000, false, D);
    const Net N9({40, 19, 12, 11, 8, 5, 3, 1, 1}, 1000, true, D);
    const uint32_t lanes[4] = {1, 3, 64, 300}, caps[2][3] = {{8, 16, 64}, {16, 64, 256}};
    // what the tiers finish depends on the seeds and the windows alone: the same for every lane count
    for (const auto &cp : caps) {
        Counts ref[5];
        for (int li = 0; li < 4; ++li) {
            GenLimits lim;
            lim.lanes = lanes[li];
            for (int i = 0; i < 3; ++i) lim.cap[i] = cp[i];
            const uint32_t n = lanes[li] == 300 ? 700 : lanes[li] == 64 ? 200 : 17;
            const Net *nets[5] = {&A, &B, &C, &Dn, &N9};
            for (int ni = 0; ni < 5; ++ni) {
                const bool full = nets[ni]->self[0] != 0;
                const Counts c = walk({*nets[ni]}, n, full, lim, false);
                CHECK(c.failed + c.finished[0] + c.finished[1] + c.finished[2] == n);
                CHECK(c.l2 == n - c.finished[0]);
                CHECK(!full || c.l3 == c.l2 - c.finished[1]);
                CHECK(full || (c.finished[2] == 0 && c.l3 == 0 && c.failed == c.l2 - c.finished[1]));
                const Counts l = walk({*nets[ni]}, n, full, lim, true);  // through a list: the same runs
                CHECK(l.failed == c.failed && l.l2 == c.l2 && l.l3 == c.l3 && l.finished[0] == c.finished[0]);
                if (n == 17) {
                    if (li == 0) ref[ni] = c;
                    CHECK(c.failed == ref[ni].failed && c.l2 == ref[ni].l2 && c.l3 == ref[ni].l3);
                }
            }
        }
    }
    {  // a lane that takes runs of different points in turn
        GenLimits lim;
        lim.lanes = 7;
        lim.cap[0] = 16;
        lim.cap[1] = 64;
        lim.cap[2] = 1024;
        const Counts c = walk({A, B, A}, 30, true, lim, false);
        CHECK(c.failed == 0 && c.finished[2] >= 30);
    }
    {  // the told list length: half of what leaves tier 1; a lowered limit drops runs and counts each once
        GenLimits lim;
        lim.lanes = 3;
        lim.cap[0] = 16;
        lim.cap[1] = 64;
        lim.cap[2] = 1024;
        const Counts nat = walk({A}, 64, true, lim, false);
        CHECK(nat.failed == 0 && nat.l2 > 2);
        lim.list_cap = nat.l2 / 2;
        const Counts c = walk({A}, 64, true, lim, false);
        CHECK(c.l2 == nat.l2);  // the count keeps every attempt
        CHECK(c.failed == nat.l2 - nat.l2 / 2);  // tier 3's list has room for whatever tier 2 served
        lim.list_cap = 10;
        const Counts l = walk({A}, 64, true, lim, true);
        CHECK(l.failed >= 54);  // tier 1 reads 10 of E2's 64 codes
        lim.list_cap = nat.l2;
        const Counts e = walk({A}, 64, true, lim, false);
        CHECK(e.failed == 0 && e.l2 == nat.l2 && e.l3 == nat.l3);
    }
    {  // no switch: the natural geometry of a 16 MiB budget (whole waves, 256 / 4 096)
        const Counts c = walk({A}, 64, true, GenLimits(), false, 16.0 * (1 << 20));
        CHECK(c.failed == 0 && c.finished[0] + c.finished[1] == 64);
    }
    if (failures) {
        printf("gen_tiers_check: %d check(s) failed\n", failures);
        return 1;
    }
    printf("gen_tiers_check: ok\n");
    return 0;
}

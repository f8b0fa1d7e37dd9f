// msim_api.hip — the C ABI declared in include/msim.h.
//
// msim_run replaces main()'s batch loop (/root/reference/main.cpp:195-220): the reference starts one
// std::async thread per RunSimulation call, in barrier-synchronised batches of hardware_concurrency(),
// and sums MinerStats in run order on the main thread. Here one launch runs a whole shard of runs,
// one run per lane, and the per-miner sums are reduced on the device in integers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/msim.h"
#include "msim_devcache.h"
#include "msim_drawgroups.h"
#include "msim_general_launch.h"
#include "msim_host.h"
#include "msim_jump.h"
#include "msim_kernels.h"
#include "msim_sel_launch.h"
#include "msim_timing.h"
#include "msim_wide_launch.h"
#include "msim_widesplit.h"

using msim::align256;

// The per-device table cache (msim_devcache.h) over HIP. A config or a sweep holds one, on its own mutex; the
// keys name its tables.
struct HipTables {
    static bool device(int *dev) { return hipGetDevice(dev) == hipSuccess; }
    static void *alloc(size_t bytes)
    {
        void *d = nullptr;
        return hipMalloc(&d, bytes) == hipSuccess ? d : nullptr;
    }
    static bool upload(void *dst, const void *src, size_t bytes)
    {
        return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    static void release(void *ptr) { (void)hipFree(ptr); }
};
using TableCache = msim::DevCache<HipTables>;
enum TableKey : uint64_t {
    TAB_PIPE = 0,               // + segment length: pipeline tables; the entry's extent is its segment count
    TAB_WIDE = 1ull << 32,      // pick, fast-threshold, prop, log, jump tables
    TAB_SEL = 2ull << 32,       // SelParams of every point + point lists
    TAB_GEN = 3ull << 32,       // GenParams of every point + arrays
    TAB_POINTS = 4ull << 32,    // SimParams[n_points]
    TAB_SPLIT = 5ull << 32,     // shared-draw sweeps: the points' split thresholds, [16] each, in draw-group order
    TAB_WSPLIT = 6ull << 32,    // wide shared-draw sweeps: the points' delays [np][m] i64, then thresholds [np][m] u32
};

// A network as the general engine reads it (msim_general.h): integer weights summing to W.
struct GenHost {
    int64_t duration_ms = 0;
    uint64_t W = 100;
    std::vector<uint64_t> w;
    std::vector<int64_t> prop;
    std::vector<uint8_t> self;
    std::vector<uint32_t> ids;  // Miner::id (msim_general.h: blocks are identified by id class)
};

// Id classes of a miner list (msim_general.h GenParams::cls): the lowest index with the same id; the class
// of id UINT_MAX (Genesis's id, simulation.h:31-33) or GEN_GENESIS.
static void gen_id_classes(const std::vector<uint32_t> &ids, std::vector<uint32_t> &cls, uint32_t *umax)
{
    const size_t m = ids.size();
    std::vector<uint32_t> ord(m);
    for (size_t k = 0; k < m; ++k) ord[k] = (uint32_t)k;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
    cls.assign(m, 0);
    *umax = msim::GEN_GENESIS;
    for (size_t i = 0; i < m; ++i) {
        const uint32_t k = ord[i];
        cls[k] = (i > 0 && ids[ord[i - 1]] == ids[k]) ? cls[ord[i - 1]] : k;  // stable: the lowest index first
        if (ids[k] == 0xFFFFFFFFu) *umax = cls[k];
    }
}

struct msim_config {
    msim::SimParams p;
    uint32_t n;
    uint32_t ids[MSIM_MAX_MINERS];
    uint64_t perc[MSIM_MAX_MINERS];
    int64_t prop[MSIM_MAX_MINERS];
    uint8_t self[MSIM_MAX_MINERS];
    double rho;      // probability that a block is not "fast" (msim_pipeline.h)
    bool pipe_ok;    // event-skipping pipeline eligible (honest network, rare forks)
    uint32_t jobs = 1;  // launches the caller keeps in flight at once (msim_config_set_concurrent_launches)
    std::mutex mu;
    TableCache tables{mu};  // per-device tables, lazily uploaded (TableKey)
    // Large honest networks (msim_wide.h): any miner count up to WIDE_MAX_M, integer weights summing to W.
    bool wide = false;
    uint64_t total_weight = 100;
    std::vector<uint32_t> wids;
    std::vector<uint64_t> wperc;
    std::vector<int64_t> wprop;
    // Networks with selfish miners (msim_sel.h entity engine): parameter block.
    bool sel = false;
    msim::SelParams sp;
    // The segment-parallel form of E1 (msim_selseg.h: SW workers + ST stitch) serves it when asked for
    // (MSIM_SELSEG): one selfish miner, the settled form applies, long runs, rare cuts (seg_rate: expected cuts
    // per find).
    bool seg_ok = false;
    double seg_rate = 0;
    // Every network, as the general engine reads it: G finishes the runs the entity engine cannot, and
    // serves alone (`general`) the networks no fast engine covers: selfish miners in networks of more than
    // MSIM_MAX_MINERS miners, more than SEL_MAXS selfish miners, large honest networks whose fork rate the
    // wide combine cannot hold.
    GenHost gh;
    bool general = false;
    bool selfish = false;   // some miner is selfish
    bool gen_full = false;  // G keeps its full last window tier (msim_general_launch.h gen_needs_full)
};

// A parameter sweep (BASELINE configs[3]): the points' parameter blocks, uploaded per device on first use.
struct msim_sweep {
    std::vector<msim::SimParams> pts;
    uint32_t m;
    bool self;
    std::mutex mu;
    TableCache tables{mu};  // per-device tables, lazily uploaded (TableKey)
    // Entity-engine sweeps (some point has a selfish miner): every point's SelParams, the points grouped
    // by selfish class, one draw pass per slice shared by all points.
    bool sel = false;
    int64_t max_duration = 0;
    std::vector<msim::SelParams> sps;
    struct Group {
        uint32_t nscls;
        std::vector<uint32_t> points;
    };
    std::vector<Group> groups;
    // General-engine view of every point (G finishes what E2 cannot; a sweep with a general point runs on G)
    bool general = false;
    bool gen_full = false;  // some point needs G's full last window tier (gen_needs_full)
    std::vector<GenHost> gens;
    // The shared-draw form (msim_sweep_create_ex with MSIM_SWEEP_SHARED_DRAWS, every point on the honest pipeline;
    // msim_sweepsplit.h): the points partitioned into draw groups by (weights, duration), each with the config of
    // its envelope network (the group's weights, every miner at its largest delay over the group's points), which
    // supplies rho, the layout and the device tables of the group's one draw pass.
    bool shared = false;
    struct DrawGroup {
        std::vector<uint32_t> points;
        msim_config *env = nullptr;
    };
    std::vector<DrawGroup> dgroups;
    std::vector<int32_t> group_of;  // per point
    std::vector<double> rhos;       // per point (its capacities and its K2 kind follow its own rho)
    // Sweeps of large-network points (every point wide && !general; msim_widesplit.h): the sweep's own wide config
    // of every point (the plain wide launch of a group of one), and the draw groups in dgroups (env: the envelope's
    // wide config; null for a group of one). flags 0: every point a group of its own, `shared` stays false.
    bool wide = false;
    std::vector<msim_config *> wcfg;
    ~msim_sweep()
    {
        for (auto &g : dgroups) delete g.env;
        for (auto *c : wcfg) delete c;
    }
};

namespace {

uint32_t err_cap_for(uint64_t n)
{
    uint64_t c = n < 65536 ? n : 65536;
    if (c < 256) c = 256;
    return (uint32_t)align256(c);
}

struct WsLayout {
    size_t partials_off, counts_off, list_off, total;
    uint32_t err_cap;
};

WsLayout ws_layout(uint32_t m, uint64_t n)
{
    WsLayout l;
    l.err_cap = err_cap_for(n);
    l.partials_off = 0;
    l.counts_off = msim::partials_words(m, (uint32_t)n, l.err_cap) * sizeof(uint64_t);
    l.list_off = l.counts_off + 2 * sizeof(uint32_t);
    l.total = l.list_off + (size_t)l.err_cap * sizeof(uint32_t);
    l.total = align256(l.total);
    return l;
}

// Sweep workspace: per-workgroup partials, per-point retry sums, counters, retry list.
struct SweepLayout {
    size_t partials_off, retry_off, counts_off, list_off, total;
    uint32_t wpp, err_cap;
};
SweepLayout sweep_layout(uint32_t m, uint32_t n_points, uint64_t rpp)
{
    SweepLayout l;
    l.wpp = (uint32_t)((rpp + msim::TPB - 1) / msim::TPB);
    l.err_cap = err_cap_for(rpp * n_points);
    const size_t nv = 6 * (size_t)m;
    l.partials_off = 0;
    l.retry_off = (size_t)n_points * l.wpp * nv * 8;
    l.counts_off = l.retry_off + (size_t)n_points * nv * 8;
    l.list_off = l.counts_off + 256;
    l.total = align256(l.list_off + (size_t)l.err_cap * 4);
    return l;
}
constexpr double PIPE_MAX_RHO = 0.08;           // above this the per-lane kernel is cheaper
constexpr double PIPE_SLICE_BUDGET = 16.0 * (1ull << 30);  // pipeline workspace per slice (bytes)

// Test switch (MSIM_MAX_SLICE_RUNS=<n>, n > 0): a slice of the honest pipeline, the large-network pipeline and
// the entity engine (single network and sweep) holds at most n runs, rounded up to a multiple of 256, so that a
// few hundred runs take the slice loops a launch otherwise enters only past 16 GiB of workspace or 2^22 runs
// per point. 0: no cap. pipe_layout, wide_layout and sel_ws_layout apply it, and every size and launch goes
// through those three.
uint32_t max_slice_runs()
{
    const char *e = getenv("MSIM_MAX_SLICE_RUNS");
    const long long v = e ? atoll(e) : 0;
    if (v <= 0) return 0;
    return v >= (1ll << 22) ? 1u << 22 : (uint32_t)align256((size_t)v);
}

// Test switches (MSIM_PIPE_TEST_CAP, MSIM_PIPE_TEST_LCAP, MSIM_PIPE_TEST_POINT_CAP, MSIM_PIPE_TEST_POINT_LCAP,
// MSIM_PIPE_TEST_K2_KIND; msim.h): capacities of the honest pipeline lowered so that a few hundred runs overflow them
// and take the retry path, as MSIM_MAX_SLICE_RUNS makes the slice loops reachable. Read at every sizing and launch
// call. point: the per-point layouts of a shared-draw group (cap_p, lcap_p); otherwise the plain pipeline's layout and
// a group's envelope layout. The limits go into the layout computation (msim_pipeline.h PipeLimits), so offsets,
// workspace sizes and every kernel's arguments come from the same lowered values.
msim::PipeLimits pipe_test_limits(bool point)
{
    auto num = [](const char *name) {
        const char *e = getenv(name);
        const long long v = e ? atoll(e) : 0;
        return v <= 0 ? 0u : v >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
    };
    msim::PipeLimits lim;
    lim.cap = num(point ? "MSIM_PIPE_TEST_POINT_CAP" : "MSIM_PIPE_TEST_CAP");
    lim.lcap = num(point ? "MSIM_PIPE_TEST_POINT_LCAP" : "MSIM_PIPE_TEST_LCAP");
    if (const char *e = getenv("MSIM_PIPE_TEST_K2_KIND"))
        if ((e[0] == '0' || e[0] == '1') && e[1] == '\0') lim.k2_kind = e[0] - '0';
    return lim;
}

// K1 wave slots of the current device (CUs x resident K1 waves per CU); 8192 if it cannot be queried.
uint32_t draw_slots()
{
    if (const char *e = getenv("MSIM_K1_SLOTS")) return (uint32_t)atoi(e);  // measurement and test switch (msim.h)
    int dev = 0, cus = 0, blocks = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        msim::draws_blocks_per_cu(&blocks) != hipSuccess || cus <= 0 || blocks <= 0)
        return 8192;
    return (uint32_t)(cus * blocks * 4);
}

// K1's grid is planned for the launches in flight: one launch gets three rounds of resident waves (more,
// shorter segments: later rounds fill the earlier ones' ragged ends), two launches on two streams one round
// each (the other launch fills it). Measured on MI355X, c2 serial (profiles/r06/k1slots/): 3.31 / 3.13 / 3.08 /
// 3.21 / 3.21 ms per step with 1 / 2 / 3 / 5 / 6 rounds (more segments also cost K2 and K3); two streams 2.82 ms
// per step with one round each against 2.89 with 1.5 and two.
msim::PipeLayout pipe_layout(const msim_config *c, uint64_t n_runs)
{
    const uint32_t jobs = c->jobs ? c->jobs : 1u;
    uint32_t slots = jobs == 1u ? draw_slots() * 3u : draw_slots() * 2u / jobs;
    if (slots < 1u) slots = 1u;
    const msim::PipeLimits lim = pipe_test_limits(false);
    const msim::PipeLayout L = msim::pipe_layout_for(c->rho, c->n, c->p.duration_ms, n_runs, PIPE_SLICE_BUDGET, slots, lim);
    const uint32_t cap = max_slice_runs();  // the layout of a slice of exactly `cap` runs, not a smaller budget's
    return cap && L.nr > cap ? msim::pipe_layout_nr(c->rho, c->n, c->p.duration_ms, cap, slots, lim) : L;
}

// Pipeline tables for this config on the current device: pick table, log table, jump matrices for
// draw offsets j * seg.
int device_tables(msim_config *c, uint32_t seg, uint32_t nseg, msim::PipeTables *out)
{
    using namespace msim;
    // K1's pick and log tables sit between the general ones and the jump matrices (sizes are multiples of 16
    // bytes: the jump columns are read as uint4)
    const size_t pick_b = sizeof(PickTab), log_b = sizeof(LogTab), k1_b = sizeof(PickTab) + sizeof(K1Log),
                 jump_b = (size_t)nseg * 128 * 16;
    static_assert((sizeof(PickTab) + sizeof(LogTab) + sizeof(PickTab) + sizeof(K1Log)) % 16 == 0, "jump table alignment");
    // an entry with the same segment length and at least as many segments serves: its jump table is a prefix
    const char *b = (const char *)c->tables.get(
        TAB_PIPE + seg, nseg, [&](uint64_t have) { return have >= nseg; }, pick_b + log_b + k1_b + jump_b,
        [&](char *h, const char *) {
            build_pick_table(c->perc, c->prop, c->self, (int)c->n, (PickTab *)h);
            build_log_table((LogTab *)(h + pick_b));
            k1_tables_build(c->perc, c->prop, c->self, (int)c->n, (PickTab *)(h + pick_b + log_b),
                            (K1Log *)(h + pick_b + log_b + pick_b));
            build_jump_table(nseg, seg, (uint32_t *)(h + pick_b + log_b + k1_b));
        });
    if (!b) return MSIM_E_HIP;
    out->pick = (const PickTab *)b;
    out->logt = (const LogTab *)(b + pick_b);
    out->k1pick = (const PickTab *)(b + pick_b + log_b);
    out->k1log = (const K1Log *)(b + pick_b + log_b + pick_b);
    out->jump = (const uint32_t *)(b + pick_b + log_b + k1_b);
    out->k1_fthr = 0;
    out->k1_uni = k1_tables_uniform(c->prop, c->self, (int)c->n, &out->k1_fthr) ? 1u : 0u;
    return MSIM_OK;
}

// Process-wide log table (msim_fastdraw.h) per device, for msim_device_intervals and the entity engine. It
// lives as long as the process: the cache is never destroyed.
// K1's log table follows it in the same entry (msim_device_intervals checks K1's form of the interval too).
int global_log_table(const msim::LogTab **out, const msim::K1Log **k1 = nullptr)
{
    static std::mutex mu;
    static TableCache *cache = new TableCache(mu);
    static_assert(sizeof(msim::LogTab) % alignof(msim::K1Log) == 0, "K1Log alignment");
    const char *b = (const char *)cache->get(0, sizeof(msim::LogTab) + sizeof(msim::K1Log), [](char *h, const char *) {
        msim::build_log_table((msim::LogTab *)h);
        msim::k1_log_build((msim::K1Log *)(h + sizeof(msim::LogTab)));
    });
    *out = (const msim::LogTab *)b;
    if (k1) *k1 = b ? (const msim::K1Log *)(b + sizeof(msim::LogTab)) : nullptr;
    return b ? MSIM_OK : MSIM_E_HIP;
}

constexpr double WIDE_SLICE_BUDGET = 16.0 * (1ull << 30);

// Test switches (msim.h): MSIM_WIDE_TEST_RCAP=<n> lowers the candidate capacity of a plain wide launch and of a
// shared-draw group's envelope, MSIM_WIDE_TEST_POINT_RCAP=<n> every point's of such a group. They only ever lower
// (wide_rcap) and act in the layout computation, so buffers and kernel arguments agree. 0: unset.
uint32_t wide_test_rcap(bool point)
{
    const char *e = getenv(point ? "MSIM_WIDE_TEST_POINT_RCAP" : "MSIM_WIDE_TEST_RCAP");
    const long long v = e ? atoll(e) : 0;
    return v <= 0 ? 0u : v >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
}

msim::WideLayout wide_layout(const msim_config *c, uint64_t n_runs)
{
    return msim::wide_layout_for(c->rho, c->n, c->p.duration_ms, n_runs, WIDE_SLICE_BUDGET, max_slice_runs(),
                                 wide_test_rcap(false));
}

// Device tables of a wide config (msim_wide_launch.h WideArgs) on the current device, uploaded once.
int wide_tables(msim_config *c, msim::WideArgs *a)
{
    using namespace msim;
    const uint32_t m = c->n;
    const WideGeom g = wide_geom(c->p.duration_ms);
    const size_t o_cf = 0, o_bkt = o_cf + 8 * ((size_t)m + 1), o_prop = (o_bkt + 2 * (size_t)WB_N + 7) / 8 * 8;
    const size_t o_log = o_prop + 8 * (size_t)m;
    const size_t o_jm = align256(o_log + sizeof(LogTab)), o_jt = o_jm + 64 * 2048, o_js = o_jt + 64 * 2048,
                 total = o_js + 2048;
    const char *b = (const char *)c->tables.get(TAB_WIDE, total, [&](char *h, const char *) {
        std::vector<uint32_t> fthr(m);
        for (uint32_t k = 0; k < m; ++k) {
            fthr[k] = c->wprop[k] < (int64_t)FTHR_NEVER ? (uint32_t)c->wprop[k] : FTHR_NEVER;
            ((int64_t *)(h + o_prop))[k] = c->wprop[k];
        }
        build_wide_pick(c->wperc.data(), fthr.data(), m, (uint32_t)c->total_weight, (uint64_t *)(h + o_cf),
                        (uint16_t *)(h + o_bkt));
        build_log_table((LogTab *)(h + o_log));
        // jmain[l] = T^(l*S0); jtail[l] = T^(B0 + l*ST); jstep = T^(63*ST - 1)
        build_jump_table(64, g.S0, (uint32_t *)(h + o_jm));
        Mat128 step, cur, tmp;
        mat_pow(g.B0, cur);
        mat_pow(g.ST, step);
        for (uint32_t l = 0; l < 64; ++l) {
            mat_store(cur, (uint32_t *)(h + o_jt) + (size_t)l * 512);
            mat_mul(step, cur, tmp);
            cur = tmp;
        }
        mat_pow(63ull * g.ST - 1, tmp);
        mat_store(tmp, (uint32_t *)(h + o_js));
    });
    if (!b) return MSIM_E_HIP;
    a->cf = (const uint64_t *)(b + o_cf);
    a->bucket = (const uint16_t *)(b + o_bkt);
    a->prop = (const int64_t *)(b + o_prop);
    a->logt = (const LogTab *)(b + o_log);
    a->jmain = (const uint32_t *)(b + o_jm);
    a->jtail = (const uint32_t *)(b + o_jt);
    a->jstep = (const uint32_t *)(b + o_js);
    a->m = m;
    a->W = (uint32_t)c->total_weight;
    a->mult = 0xFFFFFFFFFFFFFFFFull / c->total_weight;
    a->D = c->p.duration_ms;
    a->S0 = g.S0;
    a->ST = g.ST;
    a->nch = g.nch;
    a->B0 = g.B0;
    return MSIM_OK;
}

// ---------------------------------------------------------------- entity-engine path (msim_sel_launch.h)
// E1 draws in-lane (SelFastDraw) for a single network and for sweeps alike; round 2's shared per-block word
// stream (D1) is gone: on MI355X the configs[3] grid (360 points x 8192 runs) ran 2.92 s in-lane vs 3.63 s
// reading the word stream (profiles/r03/sweep_b_*.txt).
struct SelWs {
    uint32_t nr;  // runs per slice (per point)
    uint32_t wpp, err_cap;
    size_t cold_lanes;
    size_t counts_off, partials_off, retry_off, list_off, cold_off, gen_off, total;
    msim::GenWs g;  // G, for the runs E2 cannot finish
};

// Workspace of the general engine: 512 MiB of windows when it only finishes other engines' runs, 2 GiB
// when it serves a whole network (msim_general_launch.h gen_tiers).
constexpr double GEN_FALLBACK_BUDGET = 512.0 * (1 << 20);
constexpr double GEN_BUDGET = 2048.0 * (1 << 20);

// Test switches (MSIM_GEN_TEST_LANES, MSIM_GEN_TEST_CAP1 / CAP2 / CAP3, MSIM_GEN_TEST_LIST_CAP; msim.h): G's lanes,
// windows and told list length lowered so that a few hundred short runs reach lane reuse, every tier, a last window
// that is too small and full lists. Read at every sizing and launch call, as MSIM_MAX_SLICE_RUNS; a value below the
// stated minimum is ignored. The limits go into the layout computation (msim_general_launch.h GenLimits): both
// layouts below pass them, and every size, offset and kernel argument of G comes from those two.
msim::GenLimits gen_test_limits()
{
    auto num = [](const char *name, long long least) {
        const char *e = getenv(name);
        const long long v = e ? atoll(e) : 0;
        return v < least ? 0u : v >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
    };
    msim::GenLimits lim;
    lim.lanes = num("MSIM_GEN_TEST_LANES", 1);
    lim.cap[0] = num("MSIM_GEN_TEST_CAP1", 8);
    lim.cap[1] = num("MSIM_GEN_TEST_CAP2", 8);
    lim.cap[2] = num("MSIM_GEN_TEST_CAP3", 8);
    lim.list_cap = num("MSIM_GEN_TEST_LIST_CAP", 1);
    return lim;
}

SelWs sel_ws_layout(uint32_t m, uint32_t np, uint64_t rpp, int64_t duration_ms, uint32_t max_nr = 1u << 22)
{
    SelWs w;
    // one slice of every run (up to 2^22 runs per point: cold slots ~1.4 GiB; fewer under MSIM_MAX_SLICE_RUNS,
    // which thereby caps the segment-parallel form too: its records are laid out for this nr, sel_cfg_layout)
    if (const uint32_t cap = max_slice_runs()) max_nr = cap < max_nr ? cap : max_nr;
    const uint64_t want = align256(rpp);
    w.nr = (uint32_t)(want < max_nr ? want : max_nr);
    w.wpp = (uint32_t)((rpp + msim::TPB - 1) / msim::TPB);
    w.err_cap = (uint32_t)(rpp * np);  // every lane can be retried: the list never overflows
    const size_t nv = 6 * (size_t)m;
    w.counts_off = 0;
    w.partials_off = 256;
    w.retry_off = align256(w.partials_off + (size_t)np * w.wpp * nv * 8);
    w.list_off = align256(w.retry_off + (size_t)np * nv * 8);
    // cold slots: one set per E1 lane of a slice (every point x the slice's runs, rounded to whole
    // workgroups) and per E2 lane
    const size_t e1 = (size_t)np * ((w.nr + msim::TPB - 1) / msim::TPB) * msim::TPB;
    w.cold_lanes = e1 > w.err_cap ? e1 : (size_t)w.err_cap;
    w.cold_off = align256(w.list_off + (size_t)w.err_cap * 4);
    w.gen_off = align256(w.cold_off + w.cold_lanes * msim::SEL_NC * sizeof(msim::ColdAct));
    w.g = msim::gen_ws_layout(m, duration_ms, w.err_cap, GEN_FALLBACK_BUDGET, true, gen_test_limits());
    w.total = align256(w.gen_off + w.g.total);
    return w;
}

// Geometry of the segment-parallel form (msim_selseg.h) for slices of nr runs: nseg segments of seg blocks
// covering mu + 8 sigma + 64 blocks (as K1, msim_pipeline.h), cut into whole rounds of SW's resident waves (five
// per SIMD); cap subs per (run, segment) = the expected cuts + 6 sigma + 16 (a run that exceeds it is
// recomputed by E2), qcap checkpoints (msim_sel_launch.h seg_qcap; measured on configs[2]: ~1 700 per year-long
// run, ~2/3 of the room; beyond it a worker just stores no more). Records [nr][nseg][cap], checkpoints
// [nr][nseg][qcap], counts [nseg][nr].
constexpr double SEG_MAX_RATE = 0.004;             // expected cuts per find above which E1 serves the network
constexpr double SEG_MIN_BLOCKS = 4096.0;          // shorter runs: E1
constexpr double SEG_BUDGET = 24.0 * (1ull << 30);  // records of one slice
struct SegLayout {
    uint32_t nr, nseg, seg, cap, qcap;
    size_t recs_off, cnt_off, qrecs_off, qcnt_off, total;
};
SegLayout seg_layout_nr(uint32_t m, double rate, int64_t duration_ms, uint32_t nr)
{
    SegLayout L;
    L.nr = nr;
    const double mu = (double)duration_ms / 599999.5, sd = sqrt(mu > 1.0 ? mu : 1.0);
    const double need = mu + 8.0 * sd + 64.0;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const double slots = (double)cus * 4.0 * 5.0, rows = ceil(nr / 64.0);
    uint32_t best = 1;
    double bestf = 1e300;
    for (uint32_t w = 1; w <= 64; ++w) {
        const double sg = ceil(need / w);
        if (sg < 1024.0 && w > 1) break;
        const double f = ceil(rows * w / slots) * (sg + 25.0);
        if (f < bestf * 0.999) {
            bestf = f;
            best = w;
        }
    }
    if (const char *e = getenv("MSIM_SEG_NSEG")) best = (uint32_t)atoi(e) > 0 ? (uint32_t)atoi(e) : best;
    L.nseg = best;
    L.seg = (uint32_t)ceil(need / best);
    const double lam = rate * L.seg;
    L.cap = (uint32_t)ceil(lam + 6.0 * sqrt(lam) + 16.0);
    L.qcap = msim::seg_qcap((uint32_t)ceil(lam), L.seg);
    L.recs_off = 0;
    L.cnt_off = align256((size_t)nr * L.nseg * L.cap * msim::seg_rec_bytes(m));
    L.qrecs_off = align256(L.cnt_off + (size_t)L.nseg * nr * 4);
    L.qcnt_off = align256(L.qrecs_off + (size_t)nr * L.nseg * L.qcap * msim::seg_qrec_bytes(m));
    L.total = align256(L.qcnt_off + (size_t)L.nseg * nr * 4);
    return L;
}
// Runs per slice of the segment-parallel form: the records of one slice within SEG_BUDGET.
uint32_t seg_max_nr(uint32_t m, double rate, int64_t duration_ms, uint64_t n_runs)
{
    uint64_t nr = align256(n_runs);
    if (nr > (1u << 22)) nr = 1u << 22;
    // the geometry depends on the slice size: shrink until one slice's records fit the budget
    return msim::fit_slice(nr, SEG_BUDGET, [&](uint32_t n) { return seg_layout_nr(m, rate, duration_ms, n); }).nr;
}

// The E1 workspace of a single-network launch, plus the segment-parallel form's records when it serves the config.
struct SelCfgWs {
    SelWs w;
    bool seg;
    SegLayout L;
    size_t total;
};
SelCfgWs sel_cfg_layout(const msim_config *cfg, uint64_t n_runs)
{
    SelCfgWs c;
    c.seg = cfg->seg_ok;
    const uint32_t max_nr = c.seg ? seg_max_nr(cfg->n, cfg->seg_rate, cfg->p.duration_ms, n_runs) : (1u << 22);
    c.w = sel_ws_layout(cfg->n, 1, n_runs, cfg->p.duration_ms, max_nr);
    c.total = c.w.total;
    if (c.seg) {
        c.L = seg_layout_nr(cfg->n, cfg->seg_rate, cfg->p.duration_ms, c.w.nr);
        c.total += c.L.total;
    }
    return c;
}

#ifndef MSIM_XTH_MID
#define MSIM_XTH_MID 32  // engine-phase threshold for delays of 2-10 s (build_sel_params)
#endif
#ifndef MSIM_XTH_HI
#define MSIM_XTH_HI 48  // and above 10 s
#endif

// One SelParams for a validated network (weights summing to W, <= MSIM_MAX_MINERS miners).
void build_sel_params(const msim_miner *miners, uint32_t n, int64_t duration_ms, uint64_t W, msim::SelParams *sp)
{
    using namespace msim;
    memset(sp, 0, sizeof(*sp));
    sp->duration_ms = duration_ms;
    sp->W = (uint32_t)W;
    sp->mult = 0xFFFFFFFFFFFFFFFFull / W;
    sp->m = n;
    for (int i = 0; i < SEL_MAXS; ++i) sp->sids[i] = SEL_NONE;
    uint64_t c = 0;
    for (uint32_t k = 0; k < n; ++k) {
        c += miners[k].perc;
        sp->cum[k] = c;
        sp->prop[k] = miners[k].propagation_ms;
        if (miners[k].is_selfish) sp->sids[sp->ns++] = k;
    }
    for (int k = 0; k < MAXM; ++k)
        sp->ccum[k] = (uint32_t)k < n ? (W == 100 ? (uint32_t)sp->cum[k] : (uint32_t)k + 1u) : 0xFFFFFFFFu;
    sp->uniform_prop = 1;
    for (uint32_t k = 1; k < n; ++k)
        if (miners[k].propagation_ms != miners[0].propagation_ms) sp->uniform_prop = 0;
    sp->macro = sp->ns == 1 ? 1u : 0u;
    for (uint32_t k = 0; k < n; ++k)
        if (miners[k].propagation_ms < 1) sp->macro = 0;
    if (getenv("MSIM_SEL_NO_MACRO")) sp->macro = 0;  // A/B switch: the entity engine for every find
    // Engine phases start when this many lanes of a wave wait. Long delays send more finds to the engine,
    // and larger batches then pay (measured on MI355X, SEL_XTH A/B: configs[2] at 1 s fastest with 16, the
    // configs[3] grid up to 30 s with 32; profiles/r02/xth_v.txt).
    int64_t pmax = 0;
    for (uint32_t k = 0; k < n; ++k) pmax = miners[k].propagation_ms > pmax ? miners[k].propagation_ms : pmax;
    sp->xth = pmax <= 2000 ? 16u : (pmax <= 10000 ? (uint32_t)MSIM_XTH_MID : (uint32_t)MSIM_XTH_HI);
    if (const char *e = getenv("MSIM_SEL_XTH")) sp->xth = (uint32_t)atoi(e);  // A/B override
}

struct SelGroupDev {
    uint32_t nscls, nlist;
    const uint32_t *plist;
    uint32_t uni;  // every point of the group has a uniform propagation delay
};

// G's arguments for the runs of one launch (the lists and tiers are launch_gen_tiers' business).
msim::GenArgs gen_args(const msim::GenParams *d_gpts, uint32_t m, uint64_t run_begin, uint64_t rpp, uint32_t seed_base,
                       uint64_t *sums, void *d_per_run, void *d_best_height, uint32_t *counts)
{
    msim::GenArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.pts = d_gpts;
    ga.rpp = (uint32_t)rpp;
    ga.max_m = m;
    ga.run_begin = run_begin;
    ga.seed_base = seed_base;
    ga.sums = sums;
    ga.records = (uint32_t *)d_per_run;
    ga.best_h = (uint32_t *)d_best_height;
    ga.counts = counts;
    return ga;
}

// The slice loop of one launch: E1 per group (or SW + ST for a single network the segment-parallel form serves)
// -> E2 (retries) -> G (what E2 cannot finish) -> F.
int sel_launch_impl(uint32_t m, uint32_t np, const msim::SelParams *d_pts, const msim::GenParams *d_gpts,
                    const std::vector<SelGroupDev> &groups, const msim::LogTab *logt, const SelWs &w, char *ws,
                    uint64_t run_begin, uint64_t rpp, uint32_t seed_base, void *d_sums, void *d_per_run,
                    void *d_best_height, void *d_status, hipStream_t s, std::vector<hipEvent_t> *engine_events,
                    const msim::SegArgs *seg = nullptr)
{
    using namespace msim;
    uint32_t *counts = (uint32_t *)(ws + w.counts_off);
    uint64_t *retry = (uint64_t *)(ws + w.retry_off);
    if (hipMemsetAsync(counts, 0, msim::GEN_C_WORDS * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(retry, 0, (size_t)np * 6 * m * 8, s) != hipSuccess)
        return MSIM_E_HIP;
    char *gws = ws + w.gen_off;
    uint32_t *gen_first = (uint32_t *)(gws + w.g.lists_off) + 2 * (size_t)w.g.list_cap;
    SelArgs a;
    a.pts = d_pts;
    a.rpp = (uint32_t)rpp;
    a.wpp = w.wpp;
    a.run_begin = run_begin;
    a.seed_base = seed_base;
    a.logt = logt;
    a.partials = (uint64_t *)(ws + w.partials_off);
    a.retry_sums = retry;
    a.records = (uint32_t *)d_per_run;
    a.best_h = (uint32_t *)d_best_height;
    a.counts = counts;
    a.err_list = (uint32_t *)(ws + w.list_off);
    a.err_cap = w.err_cap;
    a.force_retry = getenv("MSIM_SEL_FORCE_RETRY") != nullptr ? 1u : 0u;
    a.cold = (ColdAct *)(ws + w.cold_off);
    a.cold_lanes = w.cold_lanes;
    a.gen_list = gen_first;
    a.force_gen = getenv("MSIM_SEL_FORCE_GEN") != nullptr ? 1u : 0u;
    auto event = [&](std::vector<hipEvent_t> *v) {
        hipEvent_t e = nullptr;
        if (v && hipEventCreate(&e) == hipSuccess) {
            v->push_back(e);
            (void)hipEventRecord(e, s);
        }
    };
    uint32_t max_ns = 1;
    for (const auto &g : groups) max_ns = g.nscls > max_ns ? g.nscls : max_ns;
    for (uint64_t s0 = 0; s0 < rpp; s0 += w.nr) {
        const uint32_t sn = (uint32_t)((rpp - s0) < w.nr ? (rpp - s0) : w.nr);
        a.s0 = (uint32_t)s0;
        a.sn = sn;
        event(engine_events);
        if (seg) {  // one network: SW over (run, segment), then ST per run
            a.plist = groups[0].plist;
            a.nlist = 1;
            a.uni = groups[0].uni;
            if (launch_segwork(a, *seg, m, s) != hipSuccess || launch_stitch(a, *seg, m, s) != hipSuccess)
                return MSIM_E_HIP;
        }
        for (const auto &g : groups) {
            if (!g.nlist || seg) continue;
            a.plist = g.plist;
            a.nlist = g.nlist;
            a.uni = g.uni;
            if (launch_sel(a, m, g.nscls, s) != hipSuccess) return MSIM_E_HIP;
        }
        event(engine_events);
    }
    a.s0 = 0;
    a.sn = 0;
    if (launch_sel_retry(a, m, max_ns, s) != hipSuccess) return MSIM_E_HIP;
    const GenArgs ga = gen_args(d_gpts, m, run_begin, rpp, seed_base, retry, d_per_run, d_best_height, counts);
    if (launch_gen_tiers(ga, w.g, gws, gen_first, counts + GEN_C_L1, 0, s) != hipSuccess) return MSIM_E_HIP;
    if (launch_sel_finalize(a.partials, np, w.wpp, 6 * m, retry, (uint64_t *)d_sums, counts, (uint32_t *)d_status, s) !=
        hipSuccess)
        return MSIM_E_HIP;
    return MSIM_OK;
}

// Device GenParams of a list of networks (one per point) and their weight / delay / selfish arrays, in one
// allocation whose pointers are device addresses.
// The per-device copy is uploaded on first use (TAB_GEN of the config's or the sweep's cache).
int gen_tables(TableCache &cache, const std::vector<const GenHost *> &hs, const msim::GenParams **out)
{
    const size_t np = hs.size();
    size_t off = align256(np * sizeof(msim::GenParams));
    std::vector<size_t> o(np);
    for (size_t i = 0; i < np; ++i) {
        o[i] = off;
        off = align256(off + hs[i]->w.size() * 21);
    }
    *out = (const msim::GenParams *)cache.get(TAB_GEN, off, [&](char *h, const char *d) {
        for (size_t i = 0; i < np; ++i) {
            const GenHost &g = *hs[i];
            const size_t m = g.w.size();
            uint64_t *cum = (uint64_t *)(h + o[i]);
            int64_t *prop = (int64_t *)(h + o[i] + 8 * m);
            uint32_t *cls = (uint32_t *)(h + o[i] + 16 * m);
            uint8_t *self = (uint8_t *)(h + o[i] + 20 * m);
            std::vector<uint32_t> cv;
            uint32_t umax = msim::GEN_GENESIS;
            gen_id_classes(g.ids, cv, &umax);
            uint64_t c = 0;
            for (size_t k = 0; k < m; ++k) {
                cum[k] = (c += g.w[k]);
                prop[k] = g.prop[k];
                cls[k] = cv[k];
                self[k] = g.self[k];
            }
            msim::GenParams *gp = (msim::GenParams *)h + i;
            gp->duration_ms = g.duration_ms;
            gp->mult = 0xFFFFFFFFFFFFFFFFull / g.W;
            gp->m = (uint32_t)m;
            gp->umax = umax;
            gp->cum = (const uint64_t *)(d + o[i]);
            gp->prop = (const int64_t *)(d + o[i] + 8 * m);
            gp->cls = (const uint32_t *)(d + o[i] + 16 * m);
            gp->self = (const uint8_t *)(d + o[i] + 20 * m);
        }
    });
    return *out ? MSIM_OK : MSIM_E_HIP;
}

// Workspace of a launch served by the general engine alone: counters, then G's lists and windows.
struct GenOnlyWs {
    msim::GenWs g;
    size_t gen_off, total;
};
GenOnlyWs gen_only_layout(uint32_t m, uint32_t np, uint64_t rpp, int64_t duration_ms, bool selfish)
{
    GenOnlyWs w;
    w.g = msim::gen_ws_layout(m, duration_ms, (uint32_t)(rpp * np), GEN_BUDGET, selfish, gen_test_limits());
    w.gen_off = 256;
    w.total = w.gen_off + w.g.total;
    return w;
}

// Every run of every point on G: codes point * rpp + rel, tier 1 over the whole range.
int gen_launch_impl(uint32_t m, uint32_t np, const msim::GenParams *d_gpts, const GenOnlyWs &w, char *ws,
                    uint64_t run_begin, uint64_t rpp, uint32_t seed_base, void *d_sums, void *d_per_run,
                    void *d_best_height, void *d_status, hipStream_t s)
{
    using namespace msim;
    uint32_t *counts = (uint32_t *)ws;
    if (hipMemsetAsync(counts, 0, GEN_C_WORDS * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(d_sums, 0, (size_t)np * 6 * m * 8, s) != hipSuccess)
        return MSIM_E_HIP;
    const GenArgs ga = gen_args(d_gpts, m, run_begin, rpp, seed_base, (uint64_t *)d_sums, d_per_run, d_best_height, counts);
    if (launch_gen_tiers(ga, w.g, ws + w.gen_off, nullptr, nullptr, (uint32_t)(rpp * np), s) != hipSuccess ||
        launch_gen_status(counts, (uint32_t *)d_status, s) != hipSuccess)
        return MSIM_E_HIP;
    return MSIM_OK;
}

// Device copy of a config's SelParams and the point list {0}.
int sel_config_tables(msim_config *c, const msim::SelParams **pts, const uint32_t **plist)
{
    const size_t pb = align256(sizeof(msim::SelParams));
    const char *d = (const char *)c->tables.get(
        TAB_SEL, pb + 256, [&](char *h, const char *) { memcpy(h, &c->sp, sizeof(msim::SelParams)); });
    if (!d) return MSIM_E_HIP;
    *pts = (const msim::SelParams *)d;
    *plist = (const uint32_t *)(d + pb);
    return MSIM_OK;
}

// Validate a miner list with integer weights summing to total_weight and build the config.
// want_wide: the large-network pipeline for an honest network whatever MSIM_FORCE_WIDE says at this moment (the
// internal configs of a wide sweep: its points may be W = 100 networks that were forced wide when they were created).
int config_create_impl(const msim_miner *miners, uint32_t n, int64_t duration_ms, uint64_t total_weight,
                       msim_config **out, bool want_wide = false)
{
    if (!miners || !out || n == 0 || duration_ms < 0 || total_weight == 0) return MSIM_E_INVALID;
    if (total_weight >= (1ull << 31)) return MSIM_E_WEIGHTS;
    // Ids only name a block's creator (simulation.h:22-38); the fast engines count blocks per miner INDEX,
    // which is the reference's per-id count exactly when every id is distinct and none is Genesis's id
    // UINT_MAX (simulation.h:31-33). Any other network (two miners sharing an id: shared blocks, stale
    // counting and found counts, main.cpp:24-26, simulation.h:133; an id UINT_MAX: Genesis counted as its
    // block) runs on the general engine, whose chains hold id classes (msim_general.h).
    bool id_quirk = false;
    {
        std::vector<uint32_t> ids(n);
        for (uint32_t k = 0; k < n; ++k) ids[k] = miners[k].id;
        std::sort(ids.begin(), ids.end());
        for (uint32_t k = 1; k < n; ++k) id_quirk = id_quirk || ids[k] == ids[k - 1];
        id_quirk = id_quirk || ids[n - 1] == 0xFFFFFFFFu;
    }
    uint64_t total = 0;
    uint32_t nself = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (miners[k].propagation_ms < 0) return MSIM_E_INVALID;
        if (miners[k].perc > total_weight) return MSIM_E_WEIGHTS;
        total += miners[k].perc;
        nself += miners[k].is_selfish ? 1u : 0u;
    }
    // "Must add up to 1" (main.cpp:43); anything else makes PickFinder assert (simulation.h:220).
    if (total != total_weight) return MSIM_E_WEIGHTS;
    // Selfish miners run on the entity engine (msim_sel.h): up to SEL_MAXS of them, in networks of up to
    // MSIM_MAX_MINERS miners with any integer weights. The large-network path is honest-only.
    // The entity engine takes up to SEL_MAXS selfish miners in networks of up to MSIM_MAX_MINERS miners; any
    // other network with selfish miners runs on the general engine (msim_general.h), as does any network when
    // MSIM_FORCE_GENERAL is set (test switch).
    // Honest networks of more than WIDE_MAX_M miners (beyond the large-network pipeline's LDS tables) also
    // run on G.
    const bool gen = nself > (uint32_t)msim::SEL_MAXS || (nself && n > MSIM_MAX_MINERS) || id_quirk ||
                     n > msim::WIDE_MAX_M || getenv("MSIM_FORCE_GENERAL") != nullptr;
    // G holds every miner's explicit chain: one lane of its last window must fit (msim_general_launch.h).
    int64_t max_prop = 0;
    for (uint32_t k = 0; k < n; ++k) max_prop = miners[k].propagation_ms > max_prop ? miners[k].propagation_ms : max_prop;
    const bool gen_full = msim::gen_needs_full(nself > 0, max_prop);
    if (gen && !msim::gen_fits(n, duration_ms, gen_full)) return MSIM_E_MINERS;
    const bool sel = nself > 0 && !gen;
    const bool narrow = n <= MSIM_MAX_MINERS && (total_weight == 100 || sel);
    const bool force_wide = (want_wide || getenv("MSIM_FORCE_WIDE") != nullptr) && nself == 0;
    msim_config *c = new (std::nothrow) msim_config();
    if (!c) return MSIM_E_INVALID;
    c->n = n;
    c->total_weight = total_weight;
    c->general = gen;
    c->selfish = nself > 0;
    c->gen_full = gen_full;
    c->gh.duration_ms = duration_ms;
    c->gh.W = total_weight;
    for (uint32_t k = 0; k < n; ++k) {
        c->gh.w.push_back(miners[k].perc);
        c->gh.prop.push_back(miners[k].propagation_ms);
        c->gh.self.push_back(miners[k].is_selfish ? 1 : 0);
        c->gh.ids.push_back(miners[k].id);
    }
    c->p.duration_ms = duration_ms;
    c->p.m = (int32_t)n;
    c->p.selfish = -1;
    double rho = 0.0;
    for (uint32_t k = 0; k < n; ++k)
        rho += (double)miners[k].perc / (double)total_weight *
               (miners[k].is_selfish ? 1.0 : 1.0 - exp(-((double)miners[k].propagation_ms + 1.0) / 599999.5));
    c->rho = rho;
    if (gen && !narrow) {
        // G alone: nothing else to prepare (its tables are uploaded on first launch)
        c->pipe_ok = false;
    } else if (narrow && !force_wide) {
        for (uint32_t k = 0; k < n; ++k) {
            c->ids[k] = miners[k].id;
            c->perc[k] = miners[k].perc;
            c->prop[k] = miners[k].propagation_ms;
            c->self[k] = miners[k].is_selfish ? 1 : 0;
        }
        if (sel) {
            c->sel = true;
            build_sel_params(miners, n, duration_ms, total_weight, &c->sp);
            if (c->sp.macro && c->sp.ns == 1) {  // expected cuts per find (msim_selseg.h): honest finds that may
                const uint32_t sid = c->sp.sids[0];  // need the engine (next find within prop_k + prop_s)
                double rate = 0.0;
                for (uint32_t k = 0; k < n; ++k)
                    if (k != sid)
                        rate += (double)miners[k].perc / (double)total_weight *
                                (1.0 - exp(-((double)miners[k].propagation_ms + (double)miners[sid].propagation_ms + 1.0) /
                                           599999.5));
                c->seg_rate = rate;
                // opt-in (MSIM_SELSEG=1): exact, but slower than E1 on configs[2]
                c->seg_ok = rate <= SEG_MAX_RATE && (double)duration_ms / 599999.5 >= SEG_MIN_BLOCKS &&
                            getenv("MSIM_SELSEG") != nullptr;
            }
            c->p.duration_ms = duration_ms;
            c->p.m = (int32_t)n;
            c->p.selfish = (int32_t)c->sp.sids[0];
            for (int k = 0; k < msim::MAXM; ++k) {
                c->p.prop[k] = k < (int)n ? miners[k].propagation_ms : 0;
                c->p.thresh[k] = ~0ull;
            }
        } else if (gen) {
            c->p.m = (int32_t)n;
        } else {
            const int rc = msim::make_params(c->perc, c->prop, c->self, (int)n, duration_ms, &c->p);
            if (rc) {
                delete c;
                return rc == -3 ? MSIM_E_SELFISH : (rc == -2 ? MSIM_E_WEIGHTS : MSIM_E_INVALID);
            }
        }
        // the draw kernel's fast threshold holds delays below FTHR_CAP (262 s; msim_fastdraw.h)
        bool prop_ok = true;
        for (uint32_t k = 0; k < n; ++k) prop_ok = prop_ok && miners[k].propagation_ms < (int64_t)msim::FTHR_CAP;
        // a run longer than the draw kernel's 256 workers of 65 504 blocks cover (msim_pipeline.h pipe_fits, ~318
        // years) stays on the per-lane kernel
        c->pipe_ok = !sel && !gen && prop_ok && rho <= PIPE_MAX_RHO && msim::pipe_fits(duration_ms) &&
                     getenv("MSIM_NO_PIPELINE") == nullptr;
    } else {
        c->wide = true;
        c->pipe_ok = false;
        c->wids.resize(n);
        c->wperc.resize(n);
        c->wprop.resize(n);
        for (uint32_t k = 0; k < n; ++k) {
            c->wids[k] = miners[k].id;
            c->wperc[k] = miners[k].perc;
            c->wprop[k] = miners[k].propagation_ms;
        }
        const msim::WideLayout L = wide_layout(c, 1);
        if (msim::wide_w3_lds(n, L.rcap, L.g.nch) > 160 * 1024) c->general = true;  // fork rate too high for W3
    }
    *out = c;
    return MSIM_OK;
}

int launch_wide_cfg(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, void *d_sums,
                    void *d_per_run, void *d_best_height, void *d_status, void *d_workspace, size_t workspace_bytes,
                    void *stream, std::vector<hipEvent_t> *w1_events)
{
    const msim::WideLayout L = wide_layout(cfg, n_runs);
    const size_t head = 256;
    if (workspace_bytes < head + L.total) return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    uint32_t *counts = (uint32_t *)ws;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(d_sums, 0, 6 * sizeof(uint64_t) * cfg->n, s) != hipSuccess)
        return MSIM_E_HIP;
    msim::WideArgs a;
    int rc = wide_tables(const_cast<msim_config *>(cfg), &a);
    if (rc) return rc;
    a.seed_base = seed_base;
    a.rcap = L.rcap;
    msim::WideOut o;
    o.sums = (uint64_t *)d_sums;
    o.records = (uint32_t *)d_per_run;
    o.best_h = (uint32_t *)d_best_height;
    o.fail = counts + 1;
    o.run_begin = run_begin;
    o.n_total = n_runs;
    o.rel_begin = 0;
    if (msim::launch_wide(a, L, ws + head, o, s, w1_events) != hipSuccess) return MSIM_E_HIP;
    if (d_status && hipMemcpyAsync(d_status, counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return MSIM_E_HIP;
    return MSIM_OK;
}


// ---------------------------------------------------------------- shared-draw sweeps (msim_sweepsplit.h)
// Draw groups of an eligible sweep: points with the same weights and duration share a group; a group whose envelope
// network the pipeline does not take (heterogeneous points can push its rho past PIPE_MAX_RHO) loses its point with
// the largest delay to a group of its own until it does. A group of one is the plain pipeline on that point.
int build_draw_groups(msim_sweep *w, const msim_config *const *cfgs, uint32_t np)
{
    auto envelope = [&](const std::vector<uint32_t> &points, msim_config **env) {
        const msim_config *f = cfgs[points[0]];
        std::vector<msim_miner> ms(f->n);
        for (uint32_t k = 0; k < f->n; ++k) {
            int64_t pe = 0;
            for (uint32_t i : points) pe = cfgs[i]->prop[k] > pe ? cfgs[i]->prop[k] : pe;
            ms[k] = msim_miner{f->ids[k], f->perc[k], pe, 0};
        }
        return config_create_impl(ms.data(), f->n, f->p.duration_ms, 100u, env);
    };
    std::vector<std::vector<uint32_t>> groups;
    std::vector<std::unique_ptr<msim_config>> taken;  // the envelopes of the groups of two or more, in group order
    int rc = msim::plan_draw_groups(
        np,
        [&](uint32_t i, uint32_t j) {
            return cfgs[i]->p.duration_ms == cfgs[j]->p.duration_ms &&
                   !memcmp(cfgs[i]->perc, cfgs[j]->perc, sizeof(uint64_t) * cfgs[i]->n);
        },
        [&](uint32_t i) { return *std::max_element(cfgs[i]->prop, cfgs[i]->prop + cfgs[i]->n); },
        [&](const std::vector<uint32_t> &points, bool *ok) {
            msim_config *env = nullptr;
            const int rc = envelope(points, &env);
            *ok = rc == MSIM_OK && env->pipe_ok;
            if (*ok) taken.emplace_back(env);
            else delete env;
            return rc;
        },
        &groups, &w->group_of);
    if (rc) return rc;
    for (size_t g = 0, t = 0; g < groups.size(); ++g) {
        msim_config *env = nullptr;
        if (groups[g].size() > 1) env = taken[t++].release();
        else if ((rc = envelope(groups[g], &env)) != MSIM_OK) return rc;  // the point's own delays, whatever the pipeline says
        w->dgroups.push_back({groups[g], env});
    }
    for (uint32_t i = 0; i < np; ++i) w->rhos.push_back(cfgs[i]->rho);
    w->shared = true;
    return MSIM_OK;
}

// Points per split pass: SPLIT_MAX_POINTS, or fewer under the test switch MSIM_SWEEP_SHARED_MAX_GROUP (msim.h).
uint32_t split_bound()
{
    const char *e = getenv("MSIM_SWEEP_SHARED_MAX_GROUP");
    const long v = e ? atol(e) : 0;
    return v > 0 && v < (long)msim::SPLIT_MAX_POINTS ? (uint32_t)v : msim::SPLIT_MAX_POINTS;
}

// Workspace of a shared-draw sweep. Head: the points' counters and status words, then per point the partial sums
// and the retry list of a single network's launch (ws_layout). Then ONE group region, reused by the groups in turn:
// the envelope's pipeline layout, the points' list counts (right behind the envelope's: one memset clears them all),
// and per point nslow_p, slots_p, sel_p and recs_p at the point's own capacities.
struct SharedGroupLayout {
    msim::PipeLayout env;
    std::vector<msim::PipeLayout> pl;  // per point: cap, lcap, k2_kind, rec_words at its own rho (same nr, seg, nseg)
    std::vector<size_t> nslow_off, slots_off, sel_off, recs_off;
    size_t counts_off, total;
};
struct SharedLayout {
    size_t counts_off, status_off, point_off, point_bytes, list_off, group_off, total;
    uint32_t err_cap, slice_runs, largest;
    std::vector<SharedGroupLayout> g;
};

SharedGroupLayout shared_group_nr(const msim_sweep *sw, const msim_sweep::DrawGroup &dg, uint32_t nr, uint32_t slots)
{
    SharedGroupLayout L;
    const int64_t D = dg.env->p.duration_ms;
    L.env = msim::pipe_layout_nr(dg.env->rho, sw->m, D, nr, slots, pipe_test_limits(false));
    size_t o = L.env.total;
    L.counts_off = o;
    o = align256(o + 4 * dg.points.size());
    const msim::PipeLimits plim = pipe_test_limits(true);  // cap_p, lcap_p, K2's kind: sized below from the lowered values
    for (uint32_t pt : dg.points) {
        const msim::PipeLayout P = msim::pipe_layout_nr(sw->rhos[pt], sw->m, D, nr, slots, plim);
        L.pl.push_back(P);
        L.nslow_off.push_back(o);
        o = align256(o + (size_t)P.nseg * nr * 4);
        L.slots_off.push_back(o);
        o = align256(o + (size_t)P.nseg * P.cap * nr * 4);
        L.sel_off.push_back(o);
        o = align256(o + (size_t)P.lcap * 4);
        L.recs_off.push_back(o);
        o = align256(o + (size_t)P.lcap * P.rec_words * 4);
    }
    L.total = o;
    return L;
}

// The largest slice of the group (all runs, or fewer) that fits the slice budget, as pipe_layout_for; at most
// MSIM_MAX_SLICE_RUNS runs when that switch is set, as pipe_layout.
SharedGroupLayout shared_group_layout(const msim_sweep *sw, const msim_sweep::DrawGroup &dg, uint64_t rpp)
{
    uint32_t slots = draw_slots() * 3u;
    if (slots < 1u) slots = 1u;
    uint64_t nr = (rpp + 255) / 256 * 256;
    const uint32_t cap = max_slice_runs();
    if (cap && nr > cap) nr = cap;
    return msim::fit_slice(nr, PIPE_SLICE_BUDGET, [&](uint32_t n) { return shared_group_nr(sw, dg, n, slots); });
}

SharedLayout shared_layout(const msim_sweep *sw, uint64_t rpp)
{
    SharedLayout l;
    const uint32_t np = (uint32_t)sw->pts.size();
    l.err_cap = err_cap_for(rpp);
    l.counts_off = 0;
    l.status_off = align256((size_t)np * 8);
    l.point_off = l.status_off + align256((size_t)np * 8);
    l.list_off = align256(msim::partials_words(sw->m, (uint32_t)rpp, l.err_cap) * sizeof(uint64_t));
    l.point_bytes = l.list_off + align256((size_t)l.err_cap * 4);
    l.group_off = l.point_off + (size_t)np * l.point_bytes;
    size_t gmax = 0;
    l.slice_runs = 0;
    l.largest = 0;
    for (const auto &dg : sw->dgroups) {
        l.g.push_back(shared_group_layout(sw, dg, rpp));
        const SharedGroupLayout &G = l.g.back();
        gmax = G.total > gmax ? G.total : gmax;
        l.slice_runs = l.slice_runs == 0 || G.env.nr < l.slice_runs ? G.env.nr : l.slice_runs;
        l.largest = dg.points.size() > l.largest ? (uint32_t)dg.points.size() : l.largest;
    }
    l.total = l.group_off + gmax;
    return l;
}

// The launch: per group and slice one K1 on the envelope's tables, S1 in passes of split_bound() points, then K2
// and K3 per point; per point after its last slice the retry kernel and the finalize; the status words added up.
int shared_launch_impl(msim_sweep *sw, uint64_t run_begin, uint64_t rpp, uint32_t seed_base, void *d_sums,
                       void *d_per_run, void *d_best_height, void *d_status, char *ws, size_t workspace_bytes, hipStream_t s)
{
    using namespace msim;
    const uint32_t np = (uint32_t)sw->pts.size(), m = sw->m;
    const SharedLayout l = shared_layout(sw, rpp);
    if (workspace_bytes < l.total) return MSIM_E_INVALID;
    // every table first: the rest of the call allocates nothing and does not synchronise
    std::vector<PipeTables> tabs(sw->dgroups.size());
    for (size_t g = 0; g < sw->dgroups.size(); ++g) {
        const int rc = device_tables(sw->dgroups[g].env, l.g[g].env.seg, l.g[g].env.nseg, &tabs[g]);
        if (rc) return rc;
    }
    const uint32_t *fthr = (const uint32_t *)sw->tables.get(TAB_SPLIT, (size_t)np * 64, [&](char *h, const char *) {
        uint32_t(*f)[16] = (uint32_t(*)[16])h;
        for (const auto &dg : sw->dgroups)
            for (uint32_t pt : dg.points) split_thresholds(sw->pts[pt].prop, m, *f++);
    });
    if (!fthr) return MSIM_E_HIP;
    if (hipMemsetAsync(ws + l.counts_off, 0, (size_t)np * 8, s) != hipSuccess) return MSIM_E_HIP;
    const uint32_t bound = split_bound();
    uint32_t first = 0;  // position of the group's first point in draw-group order (the threshold table's)
    for (size_t g = 0; g < sw->dgroups.size(); ++g) {
        const msim_sweep::DrawGroup &dg = sw->dgroups[g];
        const SharedGroupLayout &G = l.g[g];
        const PipeLayout &L = G.env;
        const uint32_t ng = (uint32_t)dg.points.size();
        char *gw = ws + l.group_off;
        DrawArgs da = draw_args(L, gw, tabs[g]);
        da.seed_base = seed_base;
        std::vector<LaunchArgs> las(ng);
        std::vector<PipeArgs> pas(ng);
        std::vector<uint32_t *> sels(ng);  // sel_p
        for (uint32_t i = 0; i < ng; ++i) {
            const uint32_t pt = dg.points[i];
            const PipeLayout &P = G.pl[i];
            char *pw = ws + l.point_off + (size_t)pt * l.point_bytes;
            uint32_t *counts = (uint32_t *)(ws + l.counts_off) + 2 * pt;
            LaunchArgs &a = las[i];
            a.p = sw->pts[pt];
            a.run_begin = run_begin;
            a.n = (uint32_t)rpp;
            a.seed_base = seed_base;
            a.partials = (uint64_t *)pw;
            a.sums = (uint64_t *)d_sums + (size_t)pt * 6 * m;
            a.records = d_per_run ? (uint32_t *)d_per_run + (size_t)pt * rpp * m * 2 : nullptr;
            a.best_h = d_best_height ? (uint32_t *)d_best_height + (size_t)pt * rpp : nullptr;
            a.err_count = counts;
            a.fail_count = counts + 1;
            a.err_list = (uint32_t *)(pw + l.list_off);
            a.err_cap = l.err_cap;
            a.status = (uint32_t *)(ws + l.status_off) + 2 * pt;
            a.stream = s;
            a.pl = nullptr;
            a.pipe_ws = nullptr;
            a.tab = tabs[g];
            a.k1_events = nullptr;
            PipeArgs &pa = pas[i];
            pa = pipe_args(L, gw, tabs[g]);  // K2 and K3 read only the finder of a pick entry: the envelope's tables serve every point
            pa.cap = P.cap;
            pa.lcap = P.lcap;
            pa.rec_words = P.rec_words;
            pa.nslow = (const uint32_t *)(gw + G.nslow_off[i]);
            pa.slots = (const uint32_t *)(gw + G.slots_off[i]);
            pa.list_count = (const uint32_t *)(gw + G.counts_off) + i;
            pa.recs = (uint32_t *)(gw + G.recs_off[i]);
            sels[i] = (uint32_t *)(gw + G.sel_off[i]);
        }
        for (uint64_t off = 0; off < rpp; off += L.nr) {
            const uint32_t cn = (rpp - off) < L.nr ? (uint32_t)(rpp - off) : L.nr;
            // the envelope's list count and, right behind it, the points'
            if (hipMemsetAsync(gw + L.count_off, 0, G.counts_off - L.count_off + 4 * (size_t)ng, s) != hipSuccess)
                return MSIM_E_HIP;
            da.run_begin = run_begin + off;
            da.n = cn;
            if (launch_draws(da, s) != hipSuccess) return MSIM_E_HIP;
            for (uint32_t i0 = 0; i0 < ng; i0 += bound) {
                SplitArgs sa;
                memset(&sa, 0, sizeof(sa));
                sa.nr = L.nr;
                sa.nseg = L.nseg;
                sa.cap = L.cap;
                sa.lcap = L.lcap;
                sa.np = ng - i0 < bound ? ng - i0 : bound;
                sa.nslow = da.nslow;
                sa.slots = da.slots;
                sa.list = da.list;
                sa.fthr = fthr + (size_t)(first + i0) * 16;
                for (uint32_t i = 0; i < sa.np; ++i) {
                    const PipeArgs &pa = pas[i0 + i];
                    sa.pt[i] = SplitPoint{(uint32_t *)pa.nslow, (uint32_t *)pa.slots, sels[i0 + i],
                                          (uint32_t *)pa.list_count, pa.cap, pa.lcap};
                }
                if (launch_sweep_split(sa, s) != hipSuccess) return MSIM_E_HIP;
            }
            for (uint32_t i = 0; i < ng; ++i)
                if (launch_shared_tail(las[i], pas[i], sels[i], G.pl[i].k2_kind, (uint32_t)off, cn) != hipSuccess)
                    return MSIM_E_HIP;
        }
        for (uint32_t i = 0; i < ng; ++i)
            if (launch_shared_finish(las[i]) != hipSuccess) return MSIM_E_HIP;
        first += ng;
    }
    return launch_sweep_status((const uint32_t *)(ws + l.status_off), np, (uint32_t *)d_status, s) == hipSuccess ? MSIM_OK
                                                                                                                 : MSIM_E_HIP;
}

// ---------------------------------------------------------------- sweeps on the large-network pipeline (msim_widesplit.h)
// The sweep's own wide config of every point, and its draw groups. shared: points with equal weights, equal W and
// equal duration form a group; a group whose envelope the wide pipeline does not take (its W3 LDS is past 160 KiB:
// config_create_impl marks it general) loses its point with the largest delay to a group of its own until it is
// taken. Without `shared` every point is a group of its own. A group of one is the plain wide launch (env: null).
int build_wide_groups(msim_sweep *w, const msim_config *const *cfgs, uint32_t np, bool shared)
{
    auto wide_copy = [](const msim_config *c, const std::vector<int64_t> &prop, msim_config **out) {
        std::vector<msim_miner> ms(c->n);
        for (uint32_t k = 0; k < c->n; ++k) ms[k] = msim_miner{c->wids[k], c->wperc[k], prop[k], 0};
        const int rc = config_create_impl(ms.data(), c->n, c->p.duration_ms, c->total_weight, out, true);
        if (rc == MSIM_OK && !(*out)->wide) {  // MSIM_FORCE_GENERAL at this moment
            delete *out;
            *out = nullptr;
            return (int)MSIM_E_INVALID;
        }
        return rc;
    };
    w->wide = true;
    w->group_of.assign(np, -1);
    for (uint32_t i = 0; i < np; ++i) {
        msim_config *c = nullptr;
        const int rc = wide_copy(cfgs[i], cfgs[i]->wprop, &c);
        if (rc) return rc;
        w->wcfg.push_back(c);
        if (c->general) return MSIM_E_INVALID;
        w->rhos.push_back(c->rho);
    }
    if (!shared) {
        for (uint32_t i = 0; i < np; ++i) w->dgroups.push_back({{i}, nullptr});
        return MSIM_OK;
    }
    std::vector<std::vector<uint32_t>> groups;
    std::vector<std::unique_ptr<msim_config>> taken;  // the envelopes of the groups of two or more, in group order
    const int rc = msim::plan_draw_groups(
        np,
        [&](uint32_t i, uint32_t j) {
            return cfgs[i]->p.duration_ms == cfgs[j]->p.duration_ms && cfgs[i]->total_weight == cfgs[j]->total_weight &&
                   cfgs[i]->wperc == cfgs[j]->wperc;
        },
        [&](uint32_t i) { return *std::max_element(cfgs[i]->wprop.begin(), cfgs[i]->wprop.end()); },
        [&](const std::vector<uint32_t> &points, bool *ok) {
            const msim_config *f = cfgs[points[0]];
            std::vector<int64_t> pe(f->n, 0);
            for (uint32_t k = 0; k < f->n; ++k)
                for (uint32_t i : points) pe[k] = cfgs[i]->wprop[k] > pe[k] ? cfgs[i]->wprop[k] : pe[k];
            msim_config *env = nullptr;
            const int rc = wide_copy(f, pe, &env);
            *ok = rc == MSIM_OK && !env->general;
            if (*ok) taken.emplace_back(env);
            else delete env;
            return rc;
        },
        &groups, &w->group_of);
    if (rc) return rc;
    size_t t = 0;
    for (const auto &g : groups) w->dgroups.push_back({g, g.size() > 1 ? taken[t++].release() : nullptr});
    w->shared = true;
    return MSIM_OK;
}

// Workspace of a wide sweep: a head with the counters ([0] = 0, [1] = failed (point, run)s over all points), then ONE
// group region, reused by the groups in turn: a plain wide layout (group of one) or a WideGroupLayout.
struct WideSweepLayout {
    size_t group_off, total;
    uint32_t slice_runs, largest;
    std::vector<msim::WideLayout> one;       // per group; used when the group has one point
    std::vector<msim::WideGroupLayout> grp;  // per group; used otherwise
};
WideSweepLayout wide_sweep_layout(const msim_sweep *sw, uint64_t rpp)
{
    WideSweepLayout l;
    l.group_off = 256;
    l.slice_runs = 0;
    l.largest = 0;
    size_t gmax = 0;
    for (const auto &dg : sw->dgroups) {
        size_t tot;
        uint32_t nr;
        if (!dg.env) {
            l.one.push_back(wide_layout(sw->wcfg[dg.points[0]], rpp));
            l.grp.emplace_back();
            tot = l.one.back().total;
            nr = l.one.back().nr;
        } else {
            std::vector<double> rhos;
            for (uint32_t pt : dg.points) rhos.push_back(sw->rhos[pt]);
            l.one.emplace_back();
            l.grp.push_back(msim::wide_group_layout_for(dg.env->rho, rhos, sw->m, dg.env->p.duration_ms, rpp,
                                                        WIDE_SLICE_BUDGET, max_slice_runs(), wide_test_rcap(false),
                                                        wide_test_rcap(true)));
            tot = l.grp.back().total;
            nr = l.grp.back().nr;
        }
        gmax = tot > gmax ? tot : gmax;
        l.slice_runs = l.slice_runs == 0 || nr < l.slice_runs ? nr : l.slice_runs;
        l.largest = dg.points.size() > l.largest ? (uint32_t)dg.points.size() : l.largest;
    }
    l.total = l.group_off + gmax;
    return l;
}

int wide_sweep_launch(msim_sweep *sw, uint64_t run_begin, uint64_t rpp, uint32_t seed_base, void *d_sums, void *d_per_run,
                      void *d_best_height, void *d_status, char *ws, size_t workspace_bytes, hipStream_t s)
{
    using namespace msim;
    const uint32_t np = (uint32_t)sw->pts.size(), m = sw->m;
    const WideSweepLayout l = wide_sweep_layout(sw, rpp);
    if (workspace_bytes < l.total) return MSIM_E_INVALID;
    // every table first: the rest of the call allocates nothing and does not synchronise
    std::vector<WideArgs> tabs(sw->dgroups.size());
    for (size_t g = 0; g < sw->dgroups.size(); ++g) {
        const auto &dg = sw->dgroups[g];
        const int rc = wide_tables(dg.env ? dg.env : sw->wcfg[dg.points[0]], &tabs[g]);
        if (rc) return rc;
    }
    const char *pt_tab = nullptr;
    if (sw->shared) {
        pt_tab = (const char *)sw->tables.get(TAB_WSPLIT, (size_t)np * m * 12, [&](char *h, const char *) {
            int64_t *pr = (int64_t *)h;
            uint32_t *ft = (uint32_t *)(h + (size_t)np * m * 8);
            for (uint32_t p = 0; p < np; ++p)
                for (uint32_t k = 0; k < m; ++k) {
                    pr[(size_t)p * m + k] = sw->wcfg[p]->wprop[k];
                    ft[(size_t)p * m + k] = wsplit_fthr(sw->wcfg[p]->wprop[k]);
                }
        });
        if (!pt_tab) return MSIM_E_HIP;
    }
    uint32_t *counts = (uint32_t *)ws;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(d_sums, 0, 6 * sizeof(uint64_t) * (size_t)m * np, s) != hipSuccess)
        return MSIM_E_HIP;
    auto out_of = [&](uint32_t pt) {
        WideOut o;
        o.sums = (uint64_t *)d_sums + (size_t)pt * 6 * m;
        o.records = d_per_run ? (uint32_t *)d_per_run + (size_t)pt * rpp * m * 2 : nullptr;
        o.best_h = d_best_height ? (uint32_t *)d_best_height + (size_t)pt * rpp : nullptr;
        o.fail = counts + 1;
        o.run_begin = run_begin;
        o.n_total = rpp;
        o.rel_begin = 0;
        return o;
    };
    for (size_t g = 0; g < sw->dgroups.size(); ++g) {
        const auto &dg = sw->dgroups[g];
        WideArgs a = tabs[g];
        a.seed_base = seed_base;
        if (!dg.env) {
            a.rcap = l.one[g].rcap;
            if (launch_wide(a, l.one[g], ws + l.group_off, out_of(dg.points[0]), s, nullptr) != hipSuccess) return MSIM_E_HIP;
            continue;
        }
        std::vector<WideGroupPoint> pts;
        for (uint32_t pt : dg.points)
            pts.push_back(WideGroupPoint{(const int64_t *)pt_tab + (size_t)pt * m,
                                         (const uint32_t *)(pt_tab + (size_t)np * m * 8) + (size_t)pt * m, out_of(pt)});
        if (launch_wide_group(a, l.grp[g], pts, ws + l.group_off, run_begin, rpp, s) != hipSuccess) return MSIM_E_HIP;
    }
    return hipMemcpyAsync(d_status, counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) == hipSuccess ? MSIM_OK
                                                                                                             : MSIM_E_HIP;
}

}  // namespace

void msim::config_weights(const msim_config *cfg, std::vector<uint64_t> *w, uint32_t *total_weight)
{
    *w = cfg->gh.w;  // every config keeps its miner list there, whichever engine serves it
    *total_weight = (uint32_t)cfg->total_weight;
}

extern "C" {

int msim_config_create(const msim_miner *miners, uint32_t n, int64_t duration_ms, msim_config **out)
{
    return config_create_impl(miners, n, duration_ms, 100u, out);
}

int msim_config_create_weighted(const msim_miner *miners, uint32_t n, int64_t duration_ms, uint64_t total_weight,
                                msim_config **out)
{
    return config_create_impl(miners, n, duration_ms, total_weight, out);
}

int msim_config_is_wide(const msim_config *cfg) { return cfg && cfg->wide ? 1 : 0; }

int msim_config_set_concurrent_launches(msim_config *cfg, uint32_t n)
{
    if (!cfg || n < 1 || n > 64) return MSIM_E_INVALID;
    std::lock_guard<std::mutex> g(cfg->mu);
    cfg->jobs = n;
    return MSIM_OK;
}

void msim_config_destroy(msim_config *cfg)
{
    delete cfg;  // its table cache frees the device tables
}

uint32_t msim_config_miner_count(const msim_config *cfg) { return cfg ? cfg->n : 0; }

size_t msim_workspace_bytes(const msim_config *cfg, uint64_t n_runs)
{
    if (!cfg || n_runs == 0 || n_runs > msim::MAX_LAUNCH_RUNS) return 0;
    if (cfg->general) return gen_only_layout(cfg->n, 1, n_runs, cfg->p.duration_ms, cfg->gen_full).total;
    if (cfg->wide) return 256 + wide_layout(cfg, n_runs).total;
    if (cfg->sel) return sel_cfg_layout(cfg, n_runs).total;
    size_t t = ws_layout(cfg->n, n_runs).total;
    if (cfg->pipe_ok) t += pipe_layout(cfg, n_runs).total;
    return t;
}

int msim_launch(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, void *d_sums,
                void *d_per_run, void *d_best_height, void *d_status, void *d_workspace, size_t workspace_bytes,
                void *stream)
{
    if (!cfg || !d_sums || !d_status || !d_workspace || n_runs == 0 || n_runs > msim::MAX_LAUNCH_RUNS) return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    // Each branch brackets its launch with a LaunchTimer (msim_timing.h) once its tables are on the device.
    if (cfg->general) {
        const GenOnlyWs w = gen_only_layout(cfg->n, 1, n_runs, cfg->p.duration_ms, cfg->gen_full);
        if (workspace_bytes < w.total) return MSIM_E_INVALID;
        msim_config *c = const_cast<msim_config *>(cfg);
        const msim::GenParams *gp = nullptr;
        const int rc = gen_tables(c->tables, {&cfg->gh}, &gp);
        if (rc) return rc;
        msim::LaunchTimer timer(s);
        return gen_launch_impl(cfg->n, 1, gp, w, (char *)d_workspace, run_begin, n_runs, seed_base, d_sums, d_per_run,
                               d_best_height, d_status, s);
    }
    if (cfg->wide) {
        msim::LaunchTimer timer(s);
        return launch_wide_cfg(cfg, run_begin, n_runs, seed_base, d_sums, d_per_run, d_best_height, d_status,
                               d_workspace, workspace_bytes, stream, timer.k1());
    }
    if (cfg->sel) {
        const SelCfgWs cw = sel_cfg_layout(cfg, n_runs);
        const SelWs &w = cw.w;
        if (workspace_bytes < cw.total) return MSIM_E_INVALID;
        msim_config *c = const_cast<msim_config *>(cfg);
        msim::SegArgs plan;
        if (cw.seg) {  // the segment-parallel form: jump matrices for offsets j * seg, records after E1's workspace
            msim::PipeTables tab;
            const int rt = device_tables(c, cw.L.seg, cw.L.nseg, &tab);
            if (rt) return rt;
            plan.jump = tab.jump;
            plan.recs = (char *)d_workspace + w.total + cw.L.recs_off;
            plan.cnt = (uint32_t *)((char *)d_workspace + w.total + cw.L.cnt_off);
            plan.qrecs = (char *)d_workspace + w.total + cw.L.qrecs_off;
            plan.qcnt = (uint32_t *)((char *)d_workspace + w.total + cw.L.qcnt_off);
            plan.nr = cw.L.nr;
            plan.nseg = cw.L.nseg;
            plan.seg = cw.L.seg;
            plan.cap = cw.L.cap;
            plan.qcap = cw.L.qcap;
            plan.xth = 16;
            if (const char *e = getenv("MSIM_SEG_XTH")) plan.xth = (uint32_t)atoi(e);
        }
        const msim::SelParams *pts = nullptr;
        const uint32_t *plist = nullptr;
        int rc = sel_config_tables(c, &pts, &plist);
        if (rc) return rc;
        const msim::GenParams *gp = nullptr;
        rc = gen_tables(c->tables, {&cfg->gh}, &gp);
        if (rc) return rc;
        const msim::LogTab *lt = nullptr;
        rc = global_log_table(&lt);
        if (rc) return rc;
        std::vector<SelGroupDev> groups{{msim::sel_ns_class(cfg->sp.ns), 1u, plist, cfg->sp.uniform_prop != 0 ? 1u : 0u}};
        msim::LaunchTimer timer(s);
        return sel_launch_impl(cfg->n, 1, pts, gp, groups, lt, w, (char *)d_workspace, run_begin, n_runs, seed_base,
                               d_sums, d_per_run, d_best_height, d_status, s, timer.engine(), cw.seg ? &plan : nullptr);
    }
    const WsLayout l = ws_layout(cfg->n, n_runs);
    msim::PipeLayout pl;
    if (cfg->pipe_ok) pl = pipe_layout(cfg, n_runs);
    if (workspace_bytes < l.total + (cfg->pipe_ok ? pl.total : 0)) return MSIM_E_INVALID;
    char *ws = (char *)d_workspace;
    uint32_t *counts = (uint32_t *)(ws + l.counts_off);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s) != hipSuccess) return MSIM_E_HIP;
    msim::LaunchArgs a;
    a.p = cfg->p;
    a.run_begin = run_begin;
    a.n = (uint32_t)n_runs;
    a.seed_base = seed_base;
    a.partials = (uint64_t *)(ws + l.partials_off);
    a.sums = (uint64_t *)d_sums;
    a.records = (uint32_t *)d_per_run;
    a.best_h = (uint32_t *)d_best_height;
    a.err_count = counts;
    a.fail_count = counts + 1;
    a.err_list = (uint32_t *)(ws + l.list_off);
    a.err_cap = l.err_cap;
    a.status = (uint32_t *)d_status;
    a.stream = s;
    a.pl = nullptr;
    a.pipe_ws = nullptr;
    if (cfg->pipe_ok) {
        const int rc = device_tables(const_cast<msim_config *>(cfg), pl.seg, pl.nseg, &a.tab);
        if (rc) return rc;
        a.pl = &pl;
        a.pipe_ws = ws + l.total;
    }
    msim::LaunchTimer timer(s);
    a.k1_events = timer.k1();
    return msim::launch_runs(a) == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_device_log1p(const double *d_x, double *d_out, uint64_t n, void *stream)
{
    if (!d_x || !d_out) return MSIM_E_INVALID;
    return msim::launch_log1p(d_x, d_out, n, (hipStream_t)stream) == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_device_intervals(const uint64_t *d_uniform, int64_t *d_out_ms, uint64_t n, void *stream)
{
    if (!d_uniform || !d_out_ms) return MSIM_E_INVALID;
    const msim::LogTab *lt = nullptr;
    const msim::K1Log *kl = nullptr;
    const int rc = global_log_table(&lt, &kl);
    if (rc) return rc;
    return msim::launch_intervals(lt, kl, d_uniform, d_out_ms, n, (hipStream_t)stream) == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_device_picks(const msim_config *cfg, const uint64_t *d_uniform, int32_t *d_out_index, uint64_t n, void *stream)
{
    if (!cfg || !d_uniform || !d_out_index) return MSIM_E_INVALID;
    if (cfg->wide) {
        msim::WideArgs a;
        const int rc = wide_tables(const_cast<msim_config *>(cfg), &a);
        if (rc) return rc;
        return msim::launch_wide_picks(a, d_uniform, d_out_index, n, (hipStream_t)stream) == hipSuccess ? MSIM_OK
                                                                                                         : MSIM_E_HIP;
    }
    msim::PipeTables t;
    const msim::PipeLayout pl = pipe_layout(cfg, 1);
    const int rc = device_tables(const_cast<msim_config *>(cfg), pl.seg, pl.nseg, &t);
    if (rc) return rc;
    return msim::launch_picks(t.pick, d_uniform, d_out_index, n, (hipStream_t)stream) == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_device_k1_quads(const msim_config *cfg, const uint64_t *d_states, uint32_t *d_out, uint64_t n, void *stream)
{
    if (!cfg || !d_states || !d_out || cfg->wide) return MSIM_E_INVALID;
    msim::PipeTables t;
    const msim::PipeLayout pl = pipe_layout(cfg, 1);
    const int rc = device_tables(const_cast<msim_config *>(cfg), pl.seg, pl.nseg, &t);
    if (rc) return rc;
    static_assert(sizeof(msim::Rng) == 16, "two 64-bit words per stream state");
    return msim::launch_k1_quads(t, (const msim::Rng *)d_states, d_out, n, (hipStream_t)stream) == hipSuccess ? MSIM_OK
                                                                                                             : MSIM_E_HIP;
}

// A Q32.32 sum held as two limbs -> double with ONE rounding of the exact value (hi << 32) + lo, so the
// result does not depend on how runs were split into workgroups, slices, launches or ranks (each split
// moves value between the limbs but never changes the exact sum).
static double fx_value(uint64_t hi, uint64_t lo)
{
    const unsigned __int128 v = ((unsigned __int128)hi << 32) + lo;
    return (double)v * 0x1.0p-32;
}

void msim_sums_to_stats(const msim_sums *sums, uint32_t n, msim_stats *out)
{
    for (uint32_t k = 0; k < n; ++k) {
        out[k].blocks_found = sums[k].blocks_found;
        out[k].blocks_share = fx_value(sums[k].share_hi, sums[k].share_lo);
        out[k].stale_rate = fx_value(sums[k].rate_hi, sums[k].rate_lo);
    }
}

int msim_run(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
             msim_stats *out_sums, msim_sums *opt_sums, msim_run_record *opt_per_run, uint32_t *opt_best_height)
{
    if (!cfg || !out_sums || n_runs == 0) return MSIM_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MSIM_E_HIP;
    const uint32_t m = cfg->n;
    const uint64_t chunk = n_runs < msim::MAX_LAUNCH_RUNS ? n_runs : msim::MAX_LAUNCH_RUNS;
    const size_t wsb = msim_workspace_bytes(cfg, chunk);
    const bool want_rec = opt_per_run != nullptr;
    const bool want_bh = want_rec || opt_best_height != nullptr;
    int rc = MSIM_OK;
    std::vector<uint32_t> bh_host;
    if (want_rec && !opt_best_height) bh_host.resize(n_runs);
    uint32_t *bh_out = opt_best_height ? opt_best_height : (want_rec ? bh_host.data() : nullptr);
    std::vector<uint64_t> acc(6 * (size_t)m, 0), part(6 * (size_t)m);
    uint32_t st[2];
    // G's last window can need tens of GB for one lane of a large network (msim_general_launch.h): a
    // workspace larger than the device's free memory is the network's size limit, not a HIP failure
    if (cfg->general && !msim::workspace_fits(wsb)) return MSIM_E_MINERS;
    msim::DevBuf ws, sums, status, rec, bh;
    msim::DevStream stream;  // after the buffers: destroyed before they are freed
    if (!ws.alloc(wsb) || !sums.alloc(6 * sizeof(uint64_t) * m) || !status.alloc(2 * sizeof(uint32_t)) ||
        (want_rec && !rec.alloc(chunk * m * sizeof(msim_run_record))) || (want_bh && !bh.alloc(chunk * sizeof(uint32_t))) ||
        !stream.create())
        return MSIM_E_HIP;
    hipStream_t s = stream.get();
    for (uint64_t off = 0; off < n_runs && rc == MSIM_OK; off += chunk) {
        const uint64_t cn = (n_runs - off) < chunk ? (n_runs - off) : chunk;
        rc = msim_launch(cfg, run_begin + off, cn, seed_base, sums.get(), rec.get(), bh.get(), status.get(), ws.get(), wsb, s);
        if (rc) break;
        if (hipMemcpyAsync(part.data(), sums.get(), part.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(st, status.get(), sizeof(st), hipMemcpyDeviceToHost, s) != hipSuccess ||
            (want_rec && hipMemcpyAsync(opt_per_run + off * m, rec.get(), cn * m * sizeof(msim_run_record),
                                        hipMemcpyDeviceToHost, s) != hipSuccess) ||
            (want_bh && hipMemcpyAsync(bh_out + off, bh.get(), cn * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            rc = MSIM_E_HIP;
            break;
        }
        if (st[1] != 0) {
            rc = MSIM_E_CAPACITY;
            break;
        }
        for (size_t i = 0; i < acc.size(); ++i) acc[i] += part[i];
    }
    if (rc == MSIM_OK) {
        msim_sums *fs = (msim_sums *)acc.data();
        if (opt_sums) memcpy(opt_sums, fs, sizeof(msim_sums) * m);
        msim_sums_to_stats(fs, m, out_sums);
        if (want_rec) {
            // Exact reference aggregation: per-run MinerStats (main.cpp:22-30) summed in run order
            // (main.cpp:211-217, MinerStats::operator+= 34-40).
            for (uint32_t k = 0; k < m; ++k) {
                out_sums[k].blocks_share = 0.0;
                out_sums[k].stale_rate = 0.0;
            }
            for (uint64_t r = 0; r < n_runs; ++r)
                for (uint32_t k = 0; k < m; ++k) {
                    const msim_run_record &x = opt_per_run[r * m + k];
                    const double share = x.found == 0 ? 0.0 : (double)x.found / (double)bh_out[r];
                    const double rate = x.found == 0 ? 0.0 : (double)x.stale / (double)x.found;
                    out_sums[k].blocks_share += share;
                    out_sums[k].stale_rate += rate;
                }
        }
    }
    return rc;
}

int msim_sweep_create(const msim_config *const *cfgs, uint32_t n_points, msim_sweep **out)
{
    return msim_sweep_create_ex(cfgs, n_points, 0u, out);
}

int msim_sweep_create_ex(const msim_config *const *cfgs, uint32_t n_points, uint32_t flags, msim_sweep **out)
{
    if (!cfgs || !out || n_points == 0 || (flags & ~(uint32_t)MSIM_SWEEP_SHARED_DRAWS)) return MSIM_E_INVALID;
    msim_sweep *w = new (std::nothrow) msim_sweep();
    if (!w) return MSIM_E_INVALID;
    w->m = cfgs[0] ? cfgs[0]->n : 0;
    w->self = false;
    bool any_general = false;
    bool all_wide = true;  // every point on the large-network pipeline: a wide sweep (msim_widesplit.h)
    for (uint32_t i = 0; i < n_points; ++i) {
        any_general = any_general || (cfgs[i] && cfgs[i]->general);
        all_wide = all_wide && cfgs[i] && cfgs[i]->wide && !cfgs[i]->general;
    }
    for (uint32_t i = 0; i < n_points; ++i) {
        // one miner count per sweep; narrow networks with percentages unless the sweep runs on the general
        // engine (the per-lane and entity-engine sweeps share draws and tables between points) or every point
        // runs on the large-network pipeline
        if (!cfgs[i] || cfgs[i]->n != w->m ||
            (!any_general && !all_wide && (cfgs[i]->wide || cfgs[i]->total_weight != 100))) {
            delete w;
            return MSIM_E_INVALID;
        }
        w->pts.push_back(cfgs[i]->p);
        w->self = w->self || cfgs[i]->selfish || cfgs[i]->p.selfish >= 0;
        w->sel = w->sel || cfgs[i]->sel;
        w->general = w->general || cfgs[i]->general;
        w->gen_full = w->gen_full || cfgs[i]->gen_full;
        w->gens.push_back(cfgs[i]->gh);
        w->max_duration = cfgs[i]->p.duration_ms > w->max_duration ? cfgs[i]->p.duration_ms : w->max_duration;
    }
    if (w->general) {  // a point only the general engine serves: every point on G
        w->sel = false;
    } else if (all_wide) {
        const int rc = build_wide_groups(w, cfgs, n_points, (flags & MSIM_SWEEP_SHARED_DRAWS) != 0);
        if (rc) {
            delete w;
            return rc;
        }
    } else if (w->sel) {
        // every point on the entity engine; points grouped by selfish class
        for (uint32_t i = 0; i < n_points; ++i) {
            const msim_config *c = cfgs[i];
            msim::SelParams sp;
            if (c->sel) {
                sp = c->sp;
            } else {
                std::vector<msim_miner> ms(c->n);
                for (uint32_t k = 0; k < c->n; ++k) ms[k] = msim_miner{c->ids[k], c->perc[k], c->prop[k], 0};
                build_sel_params(ms.data(), c->n, c->p.duration_ms, 100, &sp);
            }
            w->sps.push_back(sp);
            w->max_duration = sp.duration_ms > w->max_duration ? sp.duration_ms : w->max_duration;
            const uint32_t nc = msim::sel_ns_class(sp.ns);
            bool placed = false;
            for (auto &g : w->groups)
                if (g.nscls == nc) {
                    g.points.push_back(i);
                    placed = true;
                }
            if (!placed) w->groups.push_back({nc, {i}});
        }
        // A group's workgroups are dispatched in point-list order, and a point's runs cost in proportion to its
        // engine entries: an honest find needs the engine when the next interval is below prop_k (+ prop_s while
        // the selfish miner leads). The costliest points go first, so the launch ends on cheap workgroups
        // (longest-first list scheduling); results are indexed by point, not by list position.
        auto cost = [&](uint32_t p) {
            const msim::SelParams &s = w->sps[p];
            if (!s.macro) return 1e30;  // the engine for every find
            const int64_t ps = s.prop[s.sids[0]];
            double c = 0.0;
            for (uint32_t k = 0; k < s.m; ++k)
                if (k != s.sids[0]) c += (double)(s.cum[k] - (k ? s.cum[k - 1] : 0)) * (double)(s.prop[k] + ps);
            return c / (double)s.W;
        };
        if (!getenv("MSIM_SWEEP_LISTED_ORDER"))  // A/B: the caller's point order
            for (auto &g : w->groups)
                std::stable_sort(g.points.begin(), g.points.end(), [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
    } else if (flags & MSIM_SWEEP_SHARED_DRAWS) {
        // the shared-draw form takes effect only when the honest pipeline takes every point; any other sweep keeps
        // the per-lane kernel, and the flag changes nothing
        bool all_pipe = !w->self;
        for (uint32_t i = 0; i < n_points; ++i) all_pipe = all_pipe && cfgs[i]->pipe_ok;
        if (all_pipe) {
            const int rc = build_draw_groups(w, cfgs, n_points);
            if (rc) {
                delete w;
                return rc;
            }
        }
    }
    *out = w;
    return MSIM_OK;
}

int msim_sweep_group_of(const msim_sweep *sw, uint32_t point)
{
    return sw && sw->shared && point < sw->group_of.size() ? sw->group_of[point] : -1;
}

int msim_sweep_info(const msim_sweep *sw, uint64_t runs_per_point, msim_sweep_plan *out)
{
    if (!sw || !out || runs_per_point == 0 || runs_per_point * sw->pts.size() > msim::MAX_LAUNCH_RUNS) return MSIM_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->engine = sw->general ? 4u : sw->wide ? 2u : sw->sel ? 3u : sw->shared ? 1u : 0u;
    out->slice_runs = (uint32_t)runs_per_point;
    if (sw->sel && !sw->general) out->slice_runs = sel_ws_layout(sw->m, (uint32_t)sw->pts.size(), runs_per_point, sw->max_duration).nr;
    if (sw->wide) {
        const WideSweepLayout l = wide_sweep_layout(sw, runs_per_point);
        out->draw_groups = (uint32_t)sw->dgroups.size();
        out->largest_group = l.largest;
        out->slice_runs = l.slice_runs;
    } else if (sw->shared) {
        const SharedLayout l = shared_layout(sw, runs_per_point);
        out->draw_groups = (uint32_t)sw->dgroups.size();
        out->largest_group = l.largest;
        out->slice_runs = l.slice_runs;
    }
    out->workspace_bytes = msim_sweep_workspace_bytes(sw, runs_per_point);
    return MSIM_OK;
}

void msim_sweep_destroy(msim_sweep *sw)
{
    delete sw;  // its table cache frees the device tables
}

uint32_t msim_sweep_point_count(const msim_sweep *sw) { return sw ? (uint32_t)sw->pts.size() : 0u; }
uint32_t msim_sweep_miner_count(const msim_sweep *sw) { return sw ? sw->m : 0u; }

size_t msim_sweep_workspace_bytes(const msim_sweep *sw, uint64_t runs_per_point)
{
    if (!sw || runs_per_point == 0 || runs_per_point * sw->pts.size() > msim::MAX_LAUNCH_RUNS) return 0;
    if (sw->general) return gen_only_layout(sw->m, (uint32_t)sw->pts.size(), runs_per_point, sw->max_duration, sw->gen_full).total;
    if (sw->wide) return wide_sweep_layout(sw, runs_per_point).total;
    if (sw->sel) return sel_ws_layout(sw->m, (uint32_t)sw->pts.size(), runs_per_point, sw->max_duration).total;
    if (sw->shared) return shared_layout(sw, runs_per_point).total;
    return sweep_layout(sw->m, (uint32_t)sw->pts.size(), runs_per_point).total;
}

int msim_sweep_launch(const msim_sweep *sw, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                      void *d_sums, void *d_per_run, void *d_best_height, void *d_status, void *d_workspace,
                      size_t workspace_bytes, void *stream)
{
    if (!sw || !d_sums || !d_status || !d_workspace || runs_per_point == 0) return MSIM_E_INVALID;
    const uint32_t np = (uint32_t)sw->pts.size();
    if (runs_per_point * np > msim::MAX_LAUNCH_RUNS) return MSIM_E_INVALID;
    // Stage timing brackets msim_launch only: a sweep launch takes no LaunchTimer and records nothing.
    msim_sweep *sm = const_cast<msim_sweep *>(sw);  // its table cache fills on first use
    const msim::GenParams *gp = nullptr;
    if (sw->wide)
        return wide_sweep_launch(sm, run_begin, runs_per_point, seed_base, d_sums, d_per_run, d_best_height, d_status,
                                 (char *)d_workspace, workspace_bytes, (hipStream_t)stream);
    if (sw->general || sw->sel) {
        std::vector<const GenHost *> hs;
        for (const auto &g : sm->gens) hs.push_back(&g);
        const int rc = gen_tables(sm->tables, hs, &gp);
        if (rc) return rc;
        if (sw->general) {
            const GenOnlyWs w = gen_only_layout(sw->m, np, runs_per_point, sw->max_duration, sw->gen_full);
            if (workspace_bytes < w.total) return MSIM_E_INVALID;
            return gen_launch_impl(sw->m, np, gp, w, (char *)d_workspace, run_begin, runs_per_point, seed_base, d_sums,
                                   d_per_run, d_best_height, d_status, (hipStream_t)stream);
        }
    }
    if (sw->sel) {
        const SelWs w = sel_ws_layout(sw->m, np, runs_per_point, sw->max_duration);
        if (workspace_bytes < w.total) return MSIM_E_INVALID;
        const size_t pb = align256(np * sizeof(msim::SelParams));
        const char *d = (const char *)sm->tables.get(TAB_SEL, pb + (size_t)np * 4, [&](char *h, const char *) {
            memcpy(h, sm->sps.data(), np * sizeof(msim::SelParams));
            uint32_t *pl = (uint32_t *)(h + pb);
            for (const auto &gr : sm->groups)
                for (uint32_t p : gr.points) *pl++ = p;
        });
        if (!d) return MSIM_E_HIP;
        std::vector<SelGroupDev> groups;
        const uint32_t *pl = (const uint32_t *)(d + pb);
        for (const auto &gr : sm->groups) {
            uint32_t uni = 1;
            for (uint32_t p : gr.points) uni &= sm->sps[p].uniform_prop != 0 ? 1u : 0u;
            groups.push_back({gr.nscls, (uint32_t)gr.points.size(), pl, uni});
            pl += gr.points.size();
        }
        const msim::LogTab *lt = nullptr;
        int rc = global_log_table(&lt);
        if (rc) return rc;
        return sel_launch_impl(sw->m, np, (const msim::SelParams *)d, gp, groups, lt, w, (char *)d_workspace, run_begin,
                               runs_per_point, seed_base, d_sums, d_per_run, d_best_height, d_status,
                               (hipStream_t)stream, nullptr);
    }
    if (sw->shared)
        return shared_launch_impl(sm, run_begin, runs_per_point, seed_base, d_sums, d_per_run, d_best_height, d_status,
                                  (char *)d_workspace, workspace_bytes, (hipStream_t)stream);
    const SweepLayout l = sweep_layout(sw->m, np, runs_per_point);
    if (workspace_bytes < l.total) return MSIM_E_INVALID;
    const size_t pts_b = np * sizeof(msim::SimParams);
    const void *pts = sm->tables.get(TAB_POINTS, pts_b, [&](char *h, const char *) { memcpy(h, sm->pts.data(), pts_b); });
    if (!pts) return MSIM_E_HIP;
    char *ws = (char *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws + l.retry_off, 0, l.list_off - l.retry_off, s) != hipSuccess) return MSIM_E_HIP;
    msim::SweepArgs a;
    a.pts = (const msim::SimParams *)pts;
    a.m = sw->m;
    a.self = sw->self;
    a.n_points = np;
    a.rpp = (uint32_t)runs_per_point;
    a.wpp = l.wpp;
    a.run_begin = run_begin;
    a.seed_base = seed_base;
    a.partials = (uint64_t *)(ws + l.partials_off);
    a.retry_sums = (uint64_t *)(ws + l.retry_off);
    a.sums = (uint64_t *)d_sums;
    a.records = (uint32_t *)d_per_run;
    a.best_h = (uint32_t *)d_best_height;
    a.err_count = (uint32_t *)(ws + l.counts_off);
    a.err_list = (uint32_t *)(ws + l.list_off);
    a.err_cap = l.err_cap;
    a.status = (uint32_t *)d_status;
    a.stream = s;
    return msim::launch_sweep(a) == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_sweep_run(const msim_sweep *sw, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base, int device,
                   msim_stats *out_stats, msim_sums *opt_sums, msim_run_record *opt_per_run, uint32_t *opt_best_height)
{
    if (!sw || !out_stats || runs_per_point == 0) return MSIM_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MSIM_E_HIP;
    const size_t np = sw->pts.size(), m = sw->m, nr = np * runs_per_point;
    const size_t wsb = msim_sweep_workspace_bytes(sw, runs_per_point);
    if (!wsb) return MSIM_E_INVALID;
    std::vector<msim_sums> hs(np * m);
    uint32_t st[2] = {0, 0};
    if (sw->general && !msim::workspace_fits(wsb)) return MSIM_E_MINERS;  // as in msim_run
    msim::DevBuf ws, sums, status, rec, bh;
    msim::DevStream stream;  // after the buffers: destroyed before they are freed
    if (!ws.alloc(wsb) || !sums.alloc(hs.size() * sizeof(msim_sums)) || !status.alloc(sizeof(st)) ||
        (opt_per_run && !rec.alloc(nr * m * sizeof(msim_run_record))) ||
        (opt_best_height && !bh.alloc(nr * sizeof(uint32_t))) || !stream.create())
        return MSIM_E_HIP;
    hipStream_t s = stream.get();
    const int rc = msim_sweep_launch(sw, run_begin, runs_per_point, seed_base, sums.get(), rec.get(), bh.get(),
                                     status.get(), ws.get(), wsb, s);
    if (rc) return rc;
    if (hipMemcpyAsync(hs.data(), sums.get(), hs.size() * sizeof(msim_sums), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(st, status.get(), sizeof(st), hipMemcpyDeviceToHost, s) != hipSuccess ||
        (opt_per_run && hipMemcpyAsync(opt_per_run, rec.get(), nr * m * sizeof(msim_run_record), hipMemcpyDeviceToHost, s) != hipSuccess) ||
        (opt_best_height && hipMemcpyAsync(opt_best_height, bh.get(), nr * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
        return MSIM_E_HIP;
    if (st[1] != 0) return MSIM_E_CAPACITY;
    if (opt_sums) memcpy(opt_sums, hs.data(), hs.size() * sizeof(msim_sums));
    msim_sums_to_stats(hs.data(), (uint32_t)hs.size(), out_stats);
    return MSIM_OK;
}

int msim_pipeline_info(const msim_config *cfg, uint64_t n_runs, msim_pipeline_layout *out)
{
    if (!cfg || !out || n_runs == 0) return MSIM_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->rho = cfg->rho;
    if (cfg->general) {
        const GenOnlyWs w = gen_only_layout(cfg->n, 1, n_runs, cfg->p.duration_ms, cfg->gen_full);
        out->uses_pipeline = 4;
        out->slice_runs = (uint32_t)w.g.tier[0].lanes;
        out->segment_blocks = w.g.tier[0].cap;
        out->segments = (uint32_t)w.g.nt;
        out->blocks_per_run = w.g.tier[w.g.nt - 1].cap;
        out->workspace_bytes = w.total;
        return MSIM_OK;
    }
    if (cfg->wide) {
        const msim::WideLayout L = wide_layout(cfg, n_runs);
        out->uses_pipeline = 2;
        out->slice_runs = L.nr;
        out->segment_blocks = L.g.S0;
        out->segments = 64;
        out->blocks_per_run = L.g.B0 + 64ull * L.g.ST * L.g.nch;
        out->workspace_bytes = L.total;
        return MSIM_OK;
    }
    if (cfg->sel) {
        const SelCfgWs cw = sel_cfg_layout(cfg, n_runs);
        out->slice_runs = cw.w.nr;
        out->workspace_bytes = cw.total;
        if (cw.seg) {  // the segment-parallel form (msim_selseg.h): SW segments + ST
            out->uses_pipeline = 6;
            out->segment_blocks = cw.L.seg;
            out->segments = cw.L.nseg;
            out->blocks_per_run = cw.L.nseg * cw.L.seg;
            out->rho = cfg->seg_rate;
            return MSIM_OK;
        }
        out->uses_pipeline = 3;  // E1 draws in-lane: no draw segments
        out->segment_blocks = 0;
        out->segments = 0;
        out->blocks_per_run = 0;
        return MSIM_OK;
    }
    if (!cfg->pipe_ok) return MSIM_OK;
    const msim::PipeLayout pl = pipe_layout(cfg, n_runs);
    out->uses_pipeline = 1;
    out->slice_runs = pl.nr;
    out->segment_blocks = pl.seg;
    out->segments = pl.nseg;
    out->blocks_per_run = pl.nb;
    out->workspace_bytes = pl.total;
    return MSIM_OK;
}

const char *msim_strerror(int code)
{
    switch (code) {
    case MSIM_OK: return "ok";
    case MSIM_E_INVALID: return "invalid argument";
    case MSIM_E_WEIGHTS: return "miner weights must be integers adding up to the total weight (100 for percentages)";
    case MSIM_E_SELFISH: return "reserved (not returned: every network with selfish miners runs)";
    case MSIM_E_MINERS: return "network too large for the general engine (one run's explicit chains, miners x blocks per run x 12 B, exceed 96 GiB, or the launch's workspace exceeds the device's free memory)";
    case MSIM_E_HIP: return "HIP runtime error";
    case MSIM_E_CAPACITY: return "a run exceeded the compact state capacity";
    case MSIM_E_PICK: return "PickFinder fell through its table";
    default: return "unknown error";
    }
}

const char *msim_version(void) { return "msim 0.1 (gfx950)"; }

}  // extern "C"

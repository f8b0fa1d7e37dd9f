// msim_moments.hip — second moments and histograms of the per-run terms, reduced on the device from the records
// and best heights a launch writes on request (include/msim.h: msim_moments_launch, msim_run_moments,
// msim_sweep_run_moments, msim_moments_to_errors; the host conveniences at the end also serve msim_run_contrasts
// and msim_sweep_run_contrasts, whose kernel is msim_cross.hip's, and msim_run_classes and msim_sweep_run_classes,
// whose fold kernel is msim_fold.hip's). The arithmetic is msim_moments.h's.
//
// Kernel layout. Grid = (run chunks, miner tiles, points), 256 threads. A tile holds `tm` consecutive miners
// (at most 256), and thread t owns miner t % tm of the tile on rows t / tm, t / tm + 256 / tm, ... of its run
// chunk: consecutive lanes read consecutive 8-byte records (the whole chunk is one contiguous range when the
// tile covers every miner), and a thread's twenty limb sums stay in registers over its rows. The workgroup then
// folds them into LDS (one 64-bit LDS atomic per non-zero limb and thread) and flushes with one global atomic
// per non-zero limb, as W3's flush does (msim_wide.hip). Histogram rows are 32-bit LDS counters
// [tm][2][bins + 2], bumped per record and flushed with one 64-bit global atomic per non-zero bin.
// LDS is a static pool: 16 KB where that holds a tile of at least 16 miners (or all of them), 60 KB otherwise
// (7 miners per tile at 1 024 bins), so M and bins are runtime arguments of two instantiations.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <vector>

#include "msim_cross.h"
#include "msim_host.h"
#include "msim_moments.h"

namespace msim {

struct MomArgs {
    const uint2 *rec;      // [point][run][miner] {found, stale}
    const uint32_t *bh;    // [point][run]
    unsigned long long *out;   // [point][miner][20]
    unsigned long long *hist;  // [point][miner][2][bins + 2] or null
    uint32_t m, runs, tm, rows, runs_per_wg;
    uint32_t bins, share_shift, rate_shift;
    uint64_t share_lo, rate_lo;
};

constexpr uint32_t MOM_THREADS = 256;
constexpr uint32_t MOM_POOL_SMALL = 4096;   // 32-bit words: 16 KB
constexpr uint32_t MOM_POOL_LARGE = 15360;  // 60 KB

template <uint32_t POOL_WORDS>
__global__ __launch_bounds__(MOM_THREADS) void msim_moments_kernel(MomArgs a)
{
    __shared__ unsigned long long pool[POOL_WORDS / 2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.y * a.tm;
    const uint32_t tmc = a.m - k0 < a.tm ? a.m - k0 : a.tm;  // miners of this tile
    const uint32_t p = blockIdx.z;
    const uint32_t row_w = a.hist ? a.bins + 2 : 0;
    unsigned long long *acc = pool;                                   // [tm][20]
    uint32_t *hl = (uint32_t *)(pool + (size_t)a.tm * MOM_WORDS);     // [tm][2][bins + 2]
    const uint32_t lds_words = a.tm * (2 * MOM_WORDS + 2 * row_w);    // <= POOL_WORDS (msim_moments_launch)
    for (uint32_t i = tid; i < lds_words; i += MOM_THREADS) ((uint32_t *)pool)[i] = 0;
    __syncthreads();

    const uint32_t kin = tid % a.tm, row = tid / a.tm;
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    if (row < a.rows && kin < tmc) {
        uint64_t w[MOM_WORDS];
#pragma unroll
        for (uint32_t i = 0; i < MOM_WORDS; ++i) w[i] = 0;
        const size_t base = (size_t)p * a.runs;
        uint32_t *hk = hl + (size_t)kin * 2 * row_w;
        for (uint64_t r = begin + row; r < end; r += a.rows) {
            const uint2 x = a.rec[(base + r) * a.m + k0 + kin];
            const uint32_t L = a.bh[base + r];
            const uint64_t st = mom_share_term(x.x, L), rt = mom_rate_term(x.x, x.y);
            mom_add_run(w, x.x, x.y, st, rt);
            if (a.hist) {
                atomicAdd(hk + mom_bin(st, a.share_lo, a.share_shift, a.bins), 1u);
                atomicAdd(hk + row_w + mom_bin(rt, a.rate_lo, a.rate_shift, a.bins), 1u);
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < MOM_WORDS; ++i)
            if (w[i]) atomicAdd(acc + kin * MOM_WORDS + i, (unsigned long long)w[i]);
    }
    __syncthreads();
    // flush: one global atomic per non-zero limb / bin of the workgroup
    unsigned long long *o = a.out + ((size_t)p * a.m + k0) * MOM_WORDS;
    for (uint32_t i = tid; i < tmc * MOM_WORDS; i += MOM_THREADS) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(o + i, v);
    }
    if (a.hist) {
        unsigned long long *ho = a.hist + ((size_t)p * a.m + k0) * 2 * row_w;
        for (uint32_t i = tid; i < tmc * 2 * row_w; i += MOM_THREADS) {
            const uint32_t v = hl[i];
            if (v) atomicAdd(ho + i, (unsigned long long)v);
        }
    }
}

}  // namespace msim

extern "C" {

int msim_moments_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                        const void *d_best_height, const msim_hist_spec *spec, void *d_moments, void *d_hist,
                        void *stream)
{
    using namespace msim;
    if (m == 0 || n_points == 0 || n_points > 65535 || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull ||
        !d_per_run || !d_best_height || !d_moments || (spec != nullptr) != (d_hist != nullptr))
        return MSIM_E_INVALID;
    if (spec && (spec->bins == 0 || spec->bins > MOM_MAX_BINS || spec->share_shift > 63 || spec->rate_shift > 63))
        return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t row_w = spec ? spec->bins + 2 : 0;
    const uint32_t wpm = 2 * MOM_WORDS + 2 * row_w;  // LDS words per miner of a tile
    const uint32_t cap = m < MOM_THREADS ? m : MOM_THREADS;
    uint32_t tm = MOM_POOL_SMALL / wpm < cap ? MOM_POOL_SMALL / wpm : cap;
    const bool large = tm < (cap < 16 ? cap : 16);
    if (large) tm = MOM_POOL_LARGE / wpm < cap ? MOM_POOL_LARGE / wpm : cap;
    const uint32_t tiles = (m + tm - 1) / tm;
    if (tm == 0 || tiles > 65535) return MSIM_E_INVALID;
    MomArgs a;
    a.rec = (const uint2 *)d_per_run;
    a.bh = (const uint32_t *)d_best_height;
    a.out = (unsigned long long *)d_moments;
    a.hist = (unsigned long long *)d_hist;
    a.m = m;
    a.runs = (uint32_t)runs_per_point;
    a.tm = tm;
    a.rows = MOM_THREADS / tm;
    // about 2 048 workgroups in all (eight per CU), each at least four passes over its rows
    const uint64_t want = 2048 / ((uint64_t)tiles * n_points) ? 2048 / ((uint64_t)tiles * n_points) : 1;
    uint64_t rpw = (runs_per_point + want - 1) / want;
    if (rpw < 4 * a.rows) rpw = 4 * a.rows;
    rpw = (rpw + a.rows - 1) / a.rows * a.rows;
    a.runs_per_wg = (uint32_t)(rpw > 0xFFFFFF00ull ? 0xFFFFFF00ull : rpw);
    a.bins = spec ? spec->bins : 0;
    a.share_shift = spec ? spec->share_shift : 0;
    a.rate_shift = spec ? spec->rate_shift : 0;
    a.share_lo = spec ? spec->share_lo : 0;
    a.rate_lo = spec ? spec->rate_lo : 0;
    const uint64_t chunks = (runs_per_point + a.runs_per_wg - 1) / a.runs_per_wg;
    if (hipMemsetAsync(d_moments, 0, sizeof(msim_moments) * (size_t)m * n_points, s) != hipSuccess) return MSIM_E_HIP;
    if (d_hist && hipMemsetAsync(d_hist, 0, sizeof(uint64_t) * 2 * row_w * (size_t)m * n_points, s) != hipSuccess)
        return MSIM_E_HIP;
    const dim3 grid((uint32_t)chunks, tiles, n_points);
    if (large)
        hipLaunchKernelGGL(msim_moments_kernel<MOM_POOL_LARGE>, grid, dim3(MOM_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(msim_moments_kernel<MOM_POOL_SMALL>, grid, dim3(MOM_THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

void msim_moments_to_errors(const msim_moments *moments, uint32_t m, uint64_t n_runs, msim_errors *out)
{
    if (!moments || !out || n_runs == 0) return;
    msim::mom_to_errors(moments, m, n_runs, out);
}

}  // extern "C"

// ---------------------------------------------------------------- host conveniences
namespace {

constexpr uint64_t MOM_CHUNK_BYTES = 1ull << 30;      // records of one chunk in device memory

uint64_t chunk_cap()
{
    const char *e = getenv("MSIM_MOMENTS_CHUNK_RUNS");
    if (!e) return 0;
    const long long v = atoll(e);
    return v > 0 ? (uint64_t)v : 0;
}

// Runs [run_begin, run_begin + runs) of n_points networks of m miners in chunks: launch(begin, cn, d_sums, d_rec,
// d_bh, d_status, d_ws, wsb, stream) then msim_moments_launch on the same stream; only sums, status, moments
// and histograms are copied back and added limb by limb. With `cross` (msim_run_contrasts), its pairs are checked
// and uploaded once, every chunk adds msim_cross_launch on the same stream, and the cross words come back and are
// added the same way.
struct CrossJob {
    const msim_pair *pairs;
    uint32_t n_pairs;
    msim_cross *out;
};
// With `cls` (msim_run_classes), the map is checked and uploaded once, every chunk runs msim_fold_launch between the
// launch and the reductions, and moments, histograms and cross sums are those of the folded records: mc = n_classes
// columns per point where the plain forms have m. Sums and stats stay per miner.
struct ClassJob {
    const uint32_t *class_of;
    uint32_t n_classes;
};

template <class WsBytes, class Launch>
int run_moments_impl(uint32_t m, uint32_t np, uint64_t run_begin, uint64_t runs, int device, msim_stats *out_stats,
                     msim_sums *opt_sums, msim_moments *out_moments, const msim_hist_spec *spec, uint64_t *opt_hist,
                     bool general, WsBytes ws_bytes, Launch launch, const CrossJob *cross, const ClassJob *cls = nullptr)
{
    if (!out_stats || !out_moments || runs == 0 || m == 0 || np == 0 || (spec != nullptr) != (opt_hist != nullptr))
        return MSIM_E_INVALID;
    if (spec && (spec->bins == 0 || spec->bins > msim::MOM_MAX_BINS || spec->share_shift > 63 || spec->rate_shift > 63))
        return MSIM_E_INVALID;
    if (cls && msim_classes_check(m, cls->class_of, cls->n_classes) != MSIM_OK) return MSIM_E_INVALID;
    const uint32_t mc = cls ? cls->n_classes : m;  // columns of the moments, histograms and pairs
    if (cross && (!cross->out || msim_pairs_check(mc, np, cross->pairs, cross->n_pairs) != MSIM_OK)) return MSIM_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MSIM_E_HIP;
    uint64_t chunk = msim::MAX_LAUNCH_RUNS / np;
    const uint64_t by_bytes = MOM_CHUNK_BYTES / ((uint64_t)np * m * sizeof(msim_run_record));
    if (chunk > by_bytes) chunk = by_bytes ? by_bytes : 1;
    if (const uint64_t cap = chunk_cap())
        if (chunk > cap) chunk = cap;
    if (chunk > runs) chunk = runs;
    if (chunk == 0) return MSIM_E_INVALID;
    const size_t wsb = ws_bytes(chunk);
    if (!wsb) return MSIM_E_INVALID;
    const size_t n_sums = 6 * (size_t)np * m, n_mom = msim::MOM_WORDS * (size_t)np * mc;
    const size_t n_hist = spec ? 2 * (size_t)(spec->bins + 2) * np * mc : 0;
    const size_t n_cross = cross ? msim::CROSS_WORDS * (size_t)cross->n_pairs : 0;
    std::vector<uint64_t> acc_s(n_sums, 0), part_s(n_sums), acc_m(n_mom, 0), part_m(n_mom), acc_h(n_hist, 0),
        part_h(n_hist), acc_c(n_cross, 0), part_c(n_cross);
    uint32_t st[2] = {0, 0};
    // as msim_run: a workspace beyond the device's free memory is the network's size limit
    if (general && !msim::workspace_fits(wsb)) return MSIM_E_MINERS;
    msim::DevBuf ws, sums, status, rec, bh, mom, hist, pairs, crs, map, crec;
    msim::DevStream stream;  // after the buffers: destroyed before they are freed
    if (!ws.alloc(wsb) || !sums.alloc(n_sums * sizeof(uint64_t)) || !status.alloc(sizeof(st)) ||
        !rec.alloc(chunk * np * m * sizeof(msim_run_record)) || !bh.alloc(chunk * np * sizeof(uint32_t)) ||
        !mom.alloc(n_mom * sizeof(uint64_t)) || (n_hist && !hist.alloc(n_hist * sizeof(uint64_t))) ||
        (cross && (!pairs.alloc(cross->n_pairs * sizeof(msim_pair)) || !crs.alloc(n_cross * sizeof(uint64_t)))) ||
        (cls && (!map.alloc(m * sizeof(uint32_t)) || !crec.alloc(chunk * np * mc * sizeof(msim_run_record)))) ||
        !stream.create())
        return MSIM_E_HIP;
    hipStream_t s = stream.get();
    if (cross && hipMemcpy(pairs.get(), cross->pairs, cross->n_pairs * sizeof(msim_pair), hipMemcpyHostToDevice) != hipSuccess)
        return MSIM_E_HIP;
    if (cls && hipMemcpy(map.get(), cls->class_of, m * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        return MSIM_E_HIP;
    const void *red = cls ? crec.get() : rec.get();  // the records the reductions read
    for (uint64_t off = 0; off < runs; off += chunk) {
        const uint64_t cn = runs - off < chunk ? runs - off : chunk;
        int rc = launch(run_begin + off, cn, sums.get(), rec.get(), bh.get(), status.get(), ws.get(), wsb, s);
        if (rc) return rc;
        if (cls) {
            rc = msim_fold_launch(m, np, cn, rec.get(), map.get(), mc, crec.get(), s);
            if (rc) return rc;
        }
        rc = msim_moments_launch(mc, np, cn, red, bh.get(), spec, mom.get(), hist.get(), s);
        if (rc) return rc;
        if (cross) {
            rc = msim_cross_launch(mc, np, cn, red, bh.get(), pairs.get(), cross->n_pairs, crs.get(), s);
            if (rc) return rc;
        }
        if (hipMemcpyAsync(part_s.data(), sums.get(), n_sums * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(st, status.get(), sizeof(st), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(part_m.data(), mom.get(), n_mom * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            (n_hist && hipMemcpyAsync(part_h.data(), hist.get(), n_hist * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
            (n_cross && hipMemcpyAsync(part_c.data(), crs.get(), n_cross * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess)
            return MSIM_E_HIP;
        if (st[1] != 0) return MSIM_E_CAPACITY;
        for (size_t i = 0; i < n_sums; ++i) acc_s[i] += part_s[i];
        for (size_t i = 0; i < n_mom; ++i) acc_m[i] += part_m[i];
        for (size_t i = 0; i < n_hist; ++i) acc_h[i] += part_h[i];
        for (size_t i = 0; i < n_cross; ++i) acc_c[i] += part_c[i];
    }
    if (opt_sums) memcpy(opt_sums, acc_s.data(), n_sums * sizeof(uint64_t));
    msim_sums_to_stats((const msim_sums *)acc_s.data(), np * m, out_stats);
    memcpy(out_moments, acc_m.data(), n_mom * sizeof(uint64_t));
    if (n_hist) memcpy(opt_hist, acc_h.data(), n_hist * sizeof(uint64_t));
    if (n_cross) memcpy(cross->out, acc_c.data(), n_cross * sizeof(uint64_t));
    return MSIM_OK;
}

int run_config(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
               msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments, const msim_hist_spec *spec,
               uint64_t *opt_hist, const CrossJob *cross, const ClassJob *cls = nullptr)
{
    if (!cfg) return MSIM_E_INVALID;
    msim_pipeline_layout pl;
    const bool general = msim_pipeline_info(cfg, 1, &pl) == MSIM_OK && pl.uses_pipeline == 4;
    return run_moments_impl(
        msim_config_miner_count(cfg), 1, run_begin, n_runs, device, out_stats, opt_sums, out_moments, spec, opt_hist,
        general, [&](uint64_t n) { return msim_workspace_bytes(cfg, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_launch(cfg, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        cross, cls);
}

int run_sweep(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base, int device,
              msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments, const msim_hist_spec *spec,
              uint64_t *opt_hist, const CrossJob *cross, const ClassJob *cls = nullptr)
{
    if (!sweep) return MSIM_E_INVALID;
    return run_moments_impl(
        msim_sweep_miner_count(sweep), msim_sweep_point_count(sweep), run_begin, runs_per_point, device, out_stats,
        opt_sums, out_moments, spec, opt_hist, false, [&](uint64_t n) { return msim_sweep_workspace_bytes(sweep, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_sweep_launch(sweep, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        cross, cls);
}

}  // namespace

extern "C" {

int msim_run_moments(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                     msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                     const msim_hist_spec *opt_hist_spec, uint64_t *opt_hist)
{
    return run_config(cfg, run_begin, n_runs, seed_base, device, out_stats, opt_sums, out_moments, opt_hist_spec,
                      opt_hist, nullptr);
}

int msim_sweep_run_moments(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                           int device, msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                           const msim_hist_spec *opt_hist_spec, uint64_t *opt_hist)
{
    return run_sweep(sweep, run_begin, runs_per_point, seed_base, device, out_stats, opt_sums, out_moments,
                     opt_hist_spec, opt_hist, nullptr);
}

int msim_run_contrasts(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                       const msim_pair *pairs, uint32_t n_pairs, msim_stats *out_stats, msim_sums *opt_sums,
                       msim_moments *out_moments, msim_cross *out_cross)
{
    const CrossJob job = {pairs, n_pairs, out_cross};
    return run_config(cfg, run_begin, n_runs, seed_base, device, out_stats, opt_sums, out_moments, nullptr, nullptr,
                      &job);
}

int msim_sweep_run_contrasts(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point,
                             uint32_t seed_base, int device, const msim_pair *pairs, uint32_t n_pairs,
                             msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_moments,
                             msim_cross *out_cross)
{
    const CrossJob job = {pairs, n_pairs, out_cross};
    return run_sweep(sweep, run_begin, runs_per_point, seed_base, device, out_stats, opt_sums, out_moments, nullptr,
                     nullptr, &job);
}

int msim_run_classes(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                     const uint32_t *class_of, uint32_t n_classes, const msim_pair *pairs_or_NULL, uint32_t n_pairs,
                     msim_stats *out_stats, msim_sums *opt_sums, msim_moments *out_class_moments,
                     const msim_hist_spec *opt_hist_spec, uint64_t *opt_class_hist, msim_cross *opt_cross)
{
    if ((pairs_or_NULL != nullptr) != (opt_cross != nullptr) || (!pairs_or_NULL && n_pairs)) return MSIM_E_INVALID;
    const CrossJob job = {pairs_or_NULL, n_pairs, opt_cross};
    const ClassJob cls = {class_of, n_classes};
    return run_config(cfg, run_begin, n_runs, seed_base, device, out_stats, opt_sums, out_class_moments, opt_hist_spec,
                      opt_class_hist, pairs_or_NULL ? &job : nullptr, &cls);
}

int msim_sweep_run_classes(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                           int device, const uint32_t *class_of, uint32_t n_classes, const msim_pair *pairs_or_NULL,
                           uint32_t n_pairs, msim_stats *out_stats, msim_sums *opt_sums,
                           msim_moments *out_class_moments, const msim_hist_spec *opt_hist_spec,
                           uint64_t *opt_class_hist, msim_cross *opt_cross)
{
    if ((pairs_or_NULL != nullptr) != (opt_cross != nullptr) || (!pairs_or_NULL && n_pairs)) return MSIM_E_INVALID;
    const CrossJob job = {pairs_or_NULL, n_pairs, opt_cross};
    const ClassJob cls = {class_of, n_classes};
    return run_sweep(sweep, run_begin, runs_per_point, seed_base, device, out_stats, opt_sums, out_class_moments,
                     opt_hist_spec, opt_class_hist, pairs_or_NULL ? &job : nullptr, &cls);
}

}  // extern "C"

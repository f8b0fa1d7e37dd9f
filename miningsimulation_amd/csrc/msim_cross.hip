// msim_cross.hip — cross sums of pairs of (point, miner) columns, reduced on the device from the records and best
// heights a launch writes on request (include/msim.h: msim_cross_launch, msim_pairs_check,
// msim_cross_to_contrasts). The arithmetic is msim_cross.h's.
//
// Kernel layout, msim_moments_kernel's with a tile of pairs where that kernel has a tile of miners. Grid = (run
// chunks, pair tiles), 256 threads. A tile holds `tp` consecutive pairs (at most 256), and thread t owns pair
// t % tp of the tile on rows t / tp, t / tp + 256 / tp, ... of its run chunk. It reads its pair once (16 bytes) and
// per row two records and two best heights; the canonical pair lists are miner-minor, so consecutive lanes read
// consecutive 8-byte records on both sides. A thread's twelve limb sums stay in registers over its rows. The
// workgroup then folds them into LDS (one 64-bit LDS atomic per non-zero limb and thread; 12 words x 256 pairs =
// 24 KB, so six workgroups share a CU's LDS) and flushes with one global atomic per non-zero limb. A pair outside
// the records (cross_pair_ok) is skipped before any read: its words keep the zeros the launch wrote.
//
// What bounds it: per pair and run 24 bytes are read (two records, two best heights; the heights and, for lists
// against a baseline, one side's records come from L2 after their first use) against four f64 divisions, the
// terms of both sides, each a few dozen instructions on gfx950, and two 64 x 64 -> 128-bit products. Measured on
// the configs[3] grid it moves its logical bytes at 3.9 TB/s, twice the moments kernel's rate and
// well below what HBM and L2 deliver: by its instruction mix the divisions and conversions bound it, not the
// reads (no counters were collected).
#include <hip/hip_runtime.h>

#include "msim_cross.h"

namespace msim {

struct CrossArgs {
    const uint2 *rec;      // [point][run][miner] {found, stale}
    const uint32_t *bh;    // [point][run]
    const uint4 *pairs;    // [n_pairs] {point_a, miner_a, point_b, miner_b}
    unsigned long long *out;  // [n_pairs][12]
    uint32_t m, n_points, runs, n_pairs, tp, rows, runs_per_wg;
};

constexpr uint32_t CROSS_THREADS = 256;
constexpr uint32_t CROSS_MAX_TILES = 65535;  // grid.y
static_assert(MSIM_MAX_PAIRS == CROSS_MAX_TILES * CROSS_THREADS, "MSIM_MAX_PAIRS is the grid's capacity");

__global__ __launch_bounds__(CROSS_THREADS) void msim_cross_kernel(CrossArgs a)
{
    __shared__ unsigned long long acc[CROSS_THREADS * CROSS_WORDS];  // [tp][12]
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.y * a.tp;
    const uint32_t tpc = a.n_pairs - k0 < a.tp ? a.n_pairs - k0 : a.tp;  // pairs of this tile
    for (uint32_t i = tid; i < a.tp * CROSS_WORDS; i += CROSS_THREADS) acc[i] = 0;
    __syncthreads();

    const uint32_t kin = tid % a.tp, row = tid / a.tp;
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    if (row < a.rows && kin < tpc) {
        const uint4 pq = a.pairs[k0 + kin];
        const msim_pair q = {pq.x, pq.y, pq.z, pq.w};
        if (cross_pair_ok(q, a.n_points, a.m)) {
            uint64_t w[CROSS_WORDS];
#pragma unroll
            for (uint32_t i = 0; i < CROSS_WORDS; ++i) w[i] = 0;
            const size_t base_a = (size_t)q.point_a * a.runs, base_b = (size_t)q.point_b * a.runs;
            for (uint64_t r = begin + row; r < end; r += a.rows) {
                const uint2 x = a.rec[(base_a + r) * a.m + q.miner_a];
                const uint2 y = a.rec[(base_b + r) * a.m + q.miner_b];
                const uint32_t La = a.bh[base_a + r], Lb = a.bh[base_b + r];
                cross_add_run(w, x.x, x.y, mom_share_term(x.x, La), mom_rate_term(x.x, x.y), y.x, y.y,
                              mom_share_term(y.x, Lb), mom_rate_term(y.x, y.y));
            }
#pragma unroll
            for (uint32_t i = 0; i < CROSS_WORDS; ++i)
                if (w[i]) atomicAdd(acc + kin * CROSS_WORDS + i, (unsigned long long)w[i]);
        }
    }
    __syncthreads();
    // flush: one global atomic per non-zero limb of the workgroup
    unsigned long long *o = a.out + (size_t)k0 * CROSS_WORDS;
    for (uint32_t i = tid; i < tpc * CROSS_WORDS; i += CROSS_THREADS) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(o + i, v);
    }
}

}  // namespace msim

extern "C" {

int msim_cross_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                      const void *d_best_height, const void *d_pairs, uint32_t n_pairs, void *d_cross, void *stream)
{
    using namespace msim;
    if (m == 0 || n_points == 0 || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull || n_pairs == 0 ||
        n_pairs > MSIM_MAX_PAIRS || !d_per_run || !d_best_height || !d_pairs || !d_cross)
        return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    CrossArgs a;
    a.rec = (const uint2 *)d_per_run;
    a.bh = (const uint32_t *)d_best_height;
    a.pairs = (const uint4 *)d_pairs;
    a.out = (unsigned long long *)d_cross;
    a.m = m;
    a.n_points = n_points;
    a.runs = (uint32_t)runs_per_point;
    a.n_pairs = n_pairs;
    a.tp = n_pairs < CROSS_THREADS ? n_pairs : CROSS_THREADS;
    a.rows = CROSS_THREADS / a.tp;
    const uint32_t tiles = (n_pairs + a.tp - 1) / a.tp;  // <= CROSS_MAX_TILES
    // about 2 048 workgroups in all (eight per CU), each at least four passes over its rows
    const uint64_t want = 2048 / tiles ? 2048 / tiles : 1;
    uint64_t rpw = (runs_per_point + want - 1) / want;
    if (rpw < 4 * a.rows) rpw = 4 * a.rows;
    rpw = (rpw + a.rows - 1) / a.rows * a.rows;
    a.runs_per_wg = (uint32_t)(rpw > 0xFFFFFF00ull ? 0xFFFFFF00ull : rpw);
    const uint64_t chunks = (runs_per_point + a.runs_per_wg - 1) / a.runs_per_wg;
    if (hipMemsetAsync(d_cross, 0, sizeof(msim_cross) * (size_t)n_pairs, s) != hipSuccess) return MSIM_E_HIP;
    hipLaunchKernelGGL(msim_cross_kernel, dim3((uint32_t)chunks, tiles), dim3(CROSS_THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_pairs_check(uint32_t m, uint32_t n_points, const msim_pair *pairs, uint32_t n_pairs)
{
    if (!pairs || n_pairs == 0 || n_pairs > MSIM_MAX_PAIRS) return MSIM_E_INVALID;
    for (uint32_t i = 0; i < n_pairs; ++i)
        if (!msim::cross_pair_ok(pairs[i], n_points, m)) return MSIM_E_INVALID;
    return MSIM_OK;
}

void msim_cross_to_contrasts(const msim_moments *moments, uint32_t m, const msim_pair *pairs, const msim_cross *cross,
                             uint32_t n_pairs, uint64_t n_runs, msim_contrast *out)
{
    if (!moments || !pairs || !cross || !out || n_runs == 0) return;
    msim::cross_to_contrasts(moments, m, pairs, cross, n_pairs, n_runs, out);
}

}  // extern "C"

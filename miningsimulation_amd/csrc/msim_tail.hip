// msim_tail.hip — tail statistics: per item, the moments of a target column over the runs whose condition key lies
// below, or at, a threshold, reduced on the device from the records and best heights a launch writes on request
// (include/msim.h: msim_tail_launch, msim_tail_items_check, msim_tail_side, msim_tail_means). The arithmetic is
// msim_tail.h's.
//
// Kernel layout, msim_cross_kernel's with a tile of items where that kernel has a tile of pairs. Grid = (run
// chunks, item tiles), 256 threads. A tile holds `tp` consecutive items (at most 128: 42 words x 128 items =
// 42 KB of LDS; 256 items would need 84 KB, past a workgroup's 64 KB), and thread t owns item t % tp of the tile on
// rows t / tp, t / tp + 256 / tp, ... of its run chunk. It reads its item once (32 bytes) and per row the
// condition's record (and its best height only for a share key), forms the ONE key its quantity needs and compares:
// a run above the threshold ends there, one record read and at most one division, no target read. Only a run at
// or below the threshold reads the target's record and best height (the condition's own when both are the same
// record) and adds mom_add_run's 20 addends to one of the thread's two sets of limb sums. Those stay in registers
// over the rows, every index static. The workgroup then folds them into LDS (one 64-bit LDS atomic per non-zero
// limb and thread) and flushes with one global atomic per non-zero limb. The canonical item lists are
// column-minor, so consecutive lanes read consecutive 8-byte records. An item outside the records (tail_item_ok)
// is skipped before any read: its words keep the zeros the launch wrote.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "msim_tail.h"

namespace msim {

struct TailArgs {
    const uint2 *rec;         // [point][run][column] {found, stale}
    const uint32_t *bh;       // [point][run]
    const uint4 *items;       // [n_items][2]: msim_tail_item as two 16-byte halves
    unsigned long long *out;  // [n_items][42]
    uint32_t m, n_points, runs, n_items, tp, rows, runs_per_wg;
};

constexpr uint32_t TAIL_THREADS = 256;
constexpr uint32_t TAIL_TILE = 128;         // items of a tile at most: 42 KB of LDS
constexpr uint32_t TAIL_MAX_TILES = 65535;  // grid.y
static_assert(MSIM_MAX_TAIL_ITEMS == TAIL_MAX_TILES * TAIL_TILE, "MSIM_MAX_TAIL_ITEMS is the grid's capacity");
static_assert(TAIL_TILE * TAIL_WORDS * sizeof(unsigned long long) <= 64 * 1024, "a tile's accumulators fit the LDS");

__global__ __launch_bounds__(TAIL_THREADS) void msim_tail_kernel(TailArgs a)
{
    __shared__ unsigned long long acc[TAIL_TILE * TAIL_WORDS];  // [tp][42]
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.y * a.tp;
    const uint32_t tpc = a.n_items - k0 < a.tp ? a.n_items - k0 : a.tp;  // items of this tile
    for (uint32_t i = tid; i < a.tp * TAIL_WORDS; i += TAIL_THREADS) acc[i] = 0;
    __syncthreads();

    const uint32_t kin = tid % a.tp, row = tid / a.tp;
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    if (row < a.rows && kin < tpc) {
        const uint4 lo = a.items[(size_t)(k0 + kin) * 2], hi = a.items[(size_t)(k0 + kin) * 2 + 1];
        msim_tail_item it;
        it.cond_point = lo.x;
        it.cond_column = lo.y;
        it.quantity = lo.z;
        it.target_point = lo.w;
        it.target_column = hi.x;
        it.reserved = hi.y;
        it.value = (uint64_t)hi.w << 32 | hi.z;
        if (tail_item_ok(it, a.n_points, a.m)) {
            uint64_t w[TAIL_WORDS];
#pragma unroll
            for (uint32_t i = 0; i < TAIL_WORDS; ++i) w[i] = 0;
            const size_t base_c = (size_t)it.cond_point * a.runs, base_t = (size_t)it.target_point * a.runs;
            const bool same = it.cond_point == it.target_point && it.cond_column == it.target_column;
            const bool key_needs_height = it.quantity == 2;
            for (uint64_t r = begin + row; r < end; r += a.rows) {
                const uint2 c = a.rec[(base_c + r) * a.m + it.cond_column];
                const uint32_t Lc = key_needs_height ? a.bh[base_c + r] : 0;
                const uint64_t key = tail_key(it.quantity, c.x, c.y, Lc);
                if (key > it.value) continue;
                uint32_t xf = c.x, xs = c.y;  // the same record is read once
                if (!same) {
                    const uint2 x = a.rec[(base_t + r) * a.m + it.target_column];
                    xf = x.x;
                    xs = x.y;
                }
                // the key is one of the target's own terms when both are the same record
                const uint64_t st = same && it.quantity == 2 ? key : mom_share_term(xf, a.bh[base_t + r]);
                const uint64_t rt = same && it.quantity == 3 ? key : mom_rate_term(xf, xs);
                tail_add_run(w, key < it.value, xf, xs, st, rt);
            }
#pragma unroll
            for (uint32_t i = 0; i < TAIL_WORDS; ++i)
                if (w[i]) atomicAdd(acc + kin * TAIL_WORDS + i, (unsigned long long)w[i]);
        }
    }
    __syncthreads();
    // flush: one global atomic per non-zero limb of the workgroup
    unsigned long long *o = a.out + (size_t)k0 * TAIL_WORDS;
    for (uint32_t i = tid; i < tpc * TAIL_WORDS; i += TAIL_THREADS) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(o + i, v);
    }
}

}  // namespace msim

extern "C" {

int msim_tail_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_best_height, const void *d_items, uint32_t n_items, void *d_tails, void *stream)
{
    using namespace msim;
    if (m == 0 || n_points == 0 || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull || n_items == 0 ||
        n_items > MSIM_MAX_TAIL_ITEMS || !d_per_run || !d_best_height || !d_items || !d_tails)
        return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    TailArgs a;
    a.rec = (const uint2 *)d_per_run;
    a.bh = (const uint32_t *)d_best_height;
    a.items = (const uint4 *)d_items;
    a.out = (unsigned long long *)d_tails;
    a.m = m;
    a.n_points = n_points;
    a.runs = (uint32_t)runs_per_point;
    a.n_items = n_items;
    a.tp = n_items < TAIL_TILE ? n_items : TAIL_TILE;
    a.rows = TAIL_THREADS / a.tp;
    const uint32_t tiles = (n_items + a.tp - 1) / a.tp;  // <= TAIL_MAX_TILES
    // about 2 048 workgroups in all (eight per CU), each at least four passes over its rows
    const uint64_t want = 2048 / tiles ? 2048 / tiles : 1;
    uint64_t rpw = (runs_per_point + want - 1) / want;
    if (rpw < 4 * a.rows) rpw = 4 * a.rows;
    rpw = (rpw + a.rows - 1) / a.rows * a.rows;
    if (rpw > 0xFFFFFF00ull) rpw = 0xFFFFFF00ull;
    if (const char *e = getenv("MSIM_TAIL_TEST_WG_RUNS")) {
        const long long v = atoll(e);
        if (v > 0 && (uint64_t)v < rpw) rpw = (uint64_t)v;
    }
    a.runs_per_wg = (uint32_t)rpw;
    const uint64_t chunks = (runs_per_point + rpw - 1) / rpw;
    if (chunks > 0x7FFFFFFFull) return MSIM_E_INVALID;
    if (hipMemsetAsync(d_tails, 0, sizeof(msim_tail) * (size_t)n_items, s) != hipSuccess) return MSIM_E_HIP;
    hipLaunchKernelGGL(msim_tail_kernel, dim3((uint32_t)chunks, tiles), dim3(TAIL_THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_tail_items_check(uint32_t m, uint32_t n_points, const msim_tail_item *items, uint32_t n_items)
{
    if (!items || n_items == 0 || n_items > MSIM_MAX_TAIL_ITEMS) return MSIM_E_INVALID;
    for (uint32_t i = 0; i < n_items; ++i)
        if (!msim::tail_item_ok(items[i], n_points, m)) return MSIM_E_INVALID;
    return MSIM_OK;
}

int msim_tail_side(const msim_tail *t, const msim_moments *total_or_NULL, uint64_t n_runs, int side,
                   msim_moments *out, uint64_t *out_n)
{
    return msim::tail_side(t, total_or_NULL, n_runs, side, out, out_n);
}

int msim_tail_means(const msim_tail *t, const msim_moments *total_or_NULL, uint64_t n_runs, uint64_t k, int upper,
                    double out[4])
{
    return msim::tail_means(t, total_or_NULL, n_runs, k, upper, out);
}

}  // extern "C"

// msim_fold.hip — miner classes: [point][run][miner] records folded into [point][run][class] records on the device
// (include/msim.h: msim_fold_launch, msim_classes_check). The lane's work and the tile shape are msim_fold.h's.
//
// Kernel layout. Grid = (run tiles, class tiles, points), 256 threads = four waves. A workgroup walks run tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...; in a tile each wave owns a segment of gw consecutive runs, a contiguous
// range of gw * m records that its lanes read 64 at a time (8-byte loads, four in flight per lane). For m above
// 2 048 (and for fewer runs than waves can share) gw is 1: a wave walks one run. The sums go to LDS cells
// [run of the tile][tc], found and stale in separate arrays so that neighbouring cells lie in neighbouring banks.
// A lane adds to a cell only when its cell changes (fold_lane_add) and at the end of its segment; where the whole
// wave ends on ONE cell (a wave on one run of a network whose tail is one large class) the 64 pending sums are
// added across lanes and one lane makes the add. After a barrier the workgroup writes the tile's cells out and
// zeroes them in the same pass: with one class tile the tile's output is one contiguous range of records, written
// by consecutive threads; with several class tiles each wave writes rows of tc consecutive records. Every record
// of the output is written exactly once and nothing of it is read, so what the buffer held does not matter.
#include <hip/hip_runtime.h>

#include "msim_fold.h"

namespace msim {

struct FoldArgs {
    const FoldRec *rec;        // [point][run][miner]
    const uint32_t *class_of;  // [miner]
    FoldRec *out;              // [point][run][class]
    uint32_t m, runs, n_classes, tc, gw, iters;
};

struct FoldLdsSink {
    uint32_t *found, *stale;
    __device__ void operator()(uint32_t cell, uint32_t f, uint32_t s)
    {
        if (f) atomicAdd(found + cell, f);
        if (s) atomicAdd(stale + cell, s);
    }
};

__device__ inline uint32_t fold_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = FOLD_LANES / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, FOLD_LANES);
    return v;
}

__global__ __launch_bounds__(FOLD_THREADS) void msim_fold_kernel(FoldArgs a)
{
    extern __shared__ uint32_t fold_cells[];  // found [4 gw][tc], then stale [4 gw][tc]
    const uint32_t tid = threadIdx.x, lane = tid % FOLD_LANES, wave = tid / FOLD_LANES;
    const uint32_t tile_rows = FOLD_WAVES * a.gw, n_cells = tile_rows * a.tc;  // <= FOLD_POOL (fold_plan)
    uint32_t *cf = fold_cells, *cs = fold_cells + n_cells;
    for (uint32_t i = tid; i < 2 * n_cells; i += FOLD_THREADS) fold_cells[i] = 0;
    __syncthreads();

    const uint32_t c0 = blockIdx.y * a.tc;
    const uint32_t tcc = a.n_classes - c0 < a.tc ? a.n_classes - c0 : a.tc;  // classes of this tile
    const size_t pbase = (size_t)blockIdx.z * a.runs;
    for (uint32_t it = 0; it < a.iters; ++it) {  // the same trips for every workgroup: the barriers are uniform
        const uint64_t run0 = ((uint64_t)it * gridDim.x + blockIdx.x) * tile_rows;
        const uint32_t rows = run0 < a.runs ? (a.runs - run0 < tile_rows ? (uint32_t)(a.runs - run0) : tile_rows) : 0;
        const uint32_t wr0 = wave * a.gw;
        const uint32_t wrows = rows > wr0 ? (rows - wr0 < a.gw ? rows - wr0 : a.gw) : 0;  // runs of this wave
        if (wrows) {
            FoldLane st = {FOLD_SKIP, 0, 0};
            FoldLdsSink sink = {cf + (size_t)wr0 * a.tc, cs + (size_t)wr0 * a.tc};
            fold_walk(lane, a.rec + (pbase + run0 + wr0) * a.m, wrows * a.m, a.m, a.class_of, a.n_classes, c0, tcc,
                      a.tc, st, sink);
            // the sums still pending: one cross-lane sum where every lane that has one ends on the same cell
            const bool have = st.cell != FOLD_SKIP;
            const unsigned long long mask = __ballot(have);
            if (mask) {
                const int first = __ffsll((long long)mask) - 1;
                const uint32_t cell = __shfl(st.cell, first, FOLD_LANES);
                if (__ballot(have && st.cell == cell) == mask && (mask & (mask - 1))) {
                    const uint32_t f = fold_wave_sum(have ? st.found : 0u), s = fold_wave_sum(have ? st.stale : 0u);
                    if ((int)lane == first) sink(cell, f, s);
                } else if (have) {
                    sink(st.cell, st.found, st.stale);
                }
            }
        }
        __syncthreads();
        if (rows) {
            FoldRec *o = a.out + (pbase + run0) * a.n_classes + c0;
            if (tcc == a.n_classes) {  // one class tile (tc == n_classes): the tile's rows are one contiguous range
                for (uint32_t j = tid; j < rows * a.tc; j += FOLD_THREADS) {
                    const FoldRec v = {cf[j], cs[j]};
                    cf[j] = 0;
                    cs[j] = 0;
                    o[j] = v;
                }
            } else {
                for (uint32_t row = wave; row < rows; row += FOLD_WAVES)
                    for (uint32_t col = lane; col < tcc; col += FOLD_LANES) {
                        const uint32_t j = row * a.tc + col;
                        const FoldRec v = {cf[j], cs[j]};
                        cf[j] = 0;
                        cs[j] = 0;
                        o[(size_t)row * a.n_classes + col] = v;
                    }
            }
        }
        __syncthreads();
    }
}

}  // namespace msim

extern "C" {

int msim_fold_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_class_of, uint32_t n_classes, void *d_class_run, void *stream)
{
    using namespace msim;
    if (m == 0 || n_points == 0 || n_points > FOLD_MAX_TILES || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull ||
        n_classes == 0 || n_classes > m || !d_per_run || !d_class_of || !d_class_run)
        return MSIM_E_INVALID;
    FoldArgs a;
    fold_plan(m, n_classes, runs_per_point, &a.tc, &a.gw);
    const uint32_t class_tiles = (n_classes + a.tc - 1) / a.tc;
    if (class_tiles > FOLD_MAX_TILES) return MSIM_E_INVALID;
    a.rec = (const FoldRec *)d_per_run;
    a.class_of = (const uint32_t *)d_class_of;
    a.out = (FoldRec *)d_class_run;
    a.m = m;
    a.runs = (uint32_t)runs_per_point;
    a.n_classes = n_classes;
    const uint32_t tile_rows = FOLD_WAVES * a.gw;
    const uint64_t tiles = (runs_per_point + tile_rows - 1) / tile_rows;
    // about 4 096 workgroups in all (sixteen per CU: four resident, four rounds), each zeroing its cells once
    uint64_t gx = 4096 / ((uint64_t)class_tiles * n_points) ? 4096 / ((uint64_t)class_tiles * n_points) : 1;
    if (gx > tiles) gx = tiles;
    a.iters = (uint32_t)((tiles + gx - 1) / gx);
    const size_t lds = sizeof(uint32_t) * 2 * tile_rows * a.tc;
    hipLaunchKernelGGL(msim_fold_kernel, dim3((uint32_t)gx, class_tiles, n_points), dim3(FOLD_THREADS), lds,
                       (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_classes_check(uint32_t m, const uint32_t *class_of, uint32_t n_classes)
{
    return msim::fold_map_ok(m, class_of, n_classes) ? MSIM_OK : MSIM_E_INVALID;
}

}  // extern "C"

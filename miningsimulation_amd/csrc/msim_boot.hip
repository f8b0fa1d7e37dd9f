// msim_boot.hip — the Poisson bootstrap's gfx950 kernels (include/msim.h: msim_boot_weights_launch,
// msim_boot_begin_launch, msim_boot_count_launch, msim_boot_step_launch, msim_boot_below_launch). The weight, key,
// layout and row step are msim_boot.h's; match, digit and narrowing are msim_rank.h's.
//
// Count kernel. Grid = (run chunks, replicate tiles, items), 256 threads. A workgroup owns ONE item and a tile of 32
// consecutive replicates: LDS holds the tile's [32][256] 32-bit counters (32 KB), its prefixes and its pairs'
// constants, so two workgroups fit a CU. Thread t takes runs t, t + 256, ... of the chunk; it reads the item's one
// record and forms the item's one key once (at most one division), then walks the tile two replicates at a time: one
// mix gives the 64 bits of a pair, each half a weight, and a replicate whose prefix the key carries gets one LDS
// atomic of w when w != 0. Prefixes are read from LDS (a broadcast read): no runtime-indexed register array.
// Weights are recomputed per (item, pass) rather than cached per job; DESIGN 6c-5 says why. The flush is the rank
// count kernel's: one 64-bit global atomic per non-zero counter. A workgroup takes at most 2^24 runs, so
// 13 * 2^24 cannot wrap a counter.
//
// Step kernel. One wave per row, four rows per workgroup: the rank step's prefix sum and pick, then the wave zeroes
// the row's counts (every lane has read its four before). Waves never talk to each other.
//
// Below kernel. The count kernel's shape: one item and a tile of 32 replicates per workgroup, the key formed once per
// record. LDS holds the tile's values (0 for an empty row: no key lies below 0) and per replicate the two 64-bit sums,
// eight copies of each chosen by lane so that lanes adding to one replicate collide eight times less. A record below
// neither value of a pair costs two compares: no mix, no weight, no atomic, which at q = 0.05 is 95 % of them. A
// workgroup's sums stay below 13 * 2^24 * 2^32 < 2^64. The flush adds the eight copies and issues one global atomic
// per non-zero sum.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <vector>

#include "msim_boot.h"

namespace msim {

constexpr uint32_t BOOT_THREADS = 256;
constexpr uint32_t BOOT_TILE = 32;               // replicates of a tile: 32 KB of counters
constexpr uint32_t BOOT_MAX_WG_RUNS = 1u << 24;  // 13 * 2^24 < 2^32
constexpr uint32_t BOOT_BELOW_SLOTS = 8;         // copies of a below accumulator, by lane: same-address atomics / 8

__device__ inline uint64_t boot_wave_sum(uint64_t v)
{
    for (uint32_t d = 32; d >= 1; d >>= 1) v += __shfl_down((unsigned long long)v, d, 64);
    return v;
}

// Grid = (run chunks, replicate pairs). W[b] += the weights of the chunk's runs.
__global__ __launch_bounds__(BOOT_THREADS) void msim_boot_weights_kernel(uint64_t seed, uint64_t run_begin,
                                                                         uint64_t runs, uint32_t runs_per_wg, uint32_t B,
                                                                         unsigned long long *W)
{
    const uint32_t b0 = 2 * blockIdx.y;
    const uint64_t begin = (uint64_t)blockIdx.x * runs_per_wg;
    const uint64_t end = begin + runs_per_wg < runs ? begin + runs_per_wg : runs;
    const uint64_t c = boot_pair_const(seed, b0);
    uint64_t w0 = 0, w1 = 0;
    for (uint64_t r = begin + threadIdx.x; r < end; r += BOOT_THREADS) {
        const uint64_t z = boot_pair_bits(c, run_begin + r);
        w0 += boot_weight_from(z, b0);
        w1 += boot_weight_from(z, b0 + 1);
    }
    w0 = boot_wave_sum(w0);
    w1 = boot_wave_sum(w1);
    if (threadIdx.x % 64 == 0) {
        if (w0) atomicAdd(W + b0, (unsigned long long)w0);
        if (w1 && b0 + 1 < B) atomicAdd(W + b0 + 1, (unsigned long long)w1);
    }
}

// The items and the rows' ranks are in place (copied from the host); sets the rows' state and the header.
__global__ __launch_bounds__(BOOT_THREADS) void msim_boot_begin_kernel(unsigned long long *ws, uint32_t m,
                                                                       uint32_t n_points, uint32_t n_items, uint32_t B)
{
    const BootLayout l = boot_layout(n_items, B);
    const uint64_t g = (uint64_t)blockIdx.x * BOOT_THREADS + threadIdx.x;
    if (g == 0) {
        ws[0] = boot_header0(n_items);
        ws[1] = boot_header1(B, m);
        ws[2] = n_points;
        ws[3] = 0;
    }
    if (g >= l.rows) return;
    ws[l.prefix_at + g] = 0;
    ws[l.remaining_at + g] = ws[l.rank_at + g];
}

struct BootArgs {
    const uint2 *rec;    // [point][run][column] {found, stale}
    const uint32_t *bh;  // [point][run]
    unsigned long long *ws;
    unsigned long long *rows;  // the below kernel's: [item][replicate][5]
    uint64_t seed, run_begin;
    uint32_t m, points, runs, runs_per_wg, n_items, B, pass;
};

__global__ __launch_bounds__(BOOT_THREADS) void msim_boot_count_kernel(BootArgs a)
{
    __shared__ uint32_t cnt[BOOT_TILE * RANK_BINS];
    __shared__ uint64_t prefix[BOOT_TILE], pair_c[BOOT_TILE / 2];
    __shared__ uint32_t live[BOOT_TILE];
    if (!boot_prepared(a.ws, a.m, a.points, a.n_items, a.B)) return;
    const BootLayout l = boot_layout(a.n_items, a.B);
    const uint32_t tid = threadIdx.x, item = blockIdx.z;
    const uint32_t b0 = blockIdx.y * BOOT_TILE;
    const uint32_t tn = a.B - b0 < BOOT_TILE ? a.B - b0 : BOOT_TILE;  // replicates of this tile
    const msim_boot_item it = boot_item_at(a.ws, l, item);
    if (!boot_item_ok(it, a.m, a.points, MSIM_MAX_RANKS)) return;  // uniform: begin's host check makes it unreachable
    const uint64_t row0 = (uint64_t)item * a.B + b0;
    if (tid < BOOT_TILE) {
        const bool in = tid < tn;
        prefix[tid] = in ? a.ws[l.prefix_at + row0 + tid] : 0;
        live[tid] = in && a.ws[l.rank_at + row0 + tid] != MSIM_BOOT_EMPTY;
        if (tid < BOOT_TILE / 2) pair_c[tid] = boot_pair_const(a.seed, b0 + 2 * tid);
    }
    for (uint32_t i = tid; i < BOOT_TILE * RANK_BINS; i += BOOT_THREADS) cnt[i] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    const size_t base = (size_t)it.point * a.runs;
    const uint32_t pairs = (tn + 1) / 2;
    for (uint64_t r = begin + tid; r < end; r += BOOT_THREADS) {
        const uint2 x = a.rec[(base + r) * a.m + it.column];
        const uint64_t key = boot_key(it.quantity, x.x, x.y, it.quantity == 2 ? a.bh[base + r] : 0u);
        const uint32_t d = rank_digit(key, a.pass);
        const uint64_t run = a.run_begin + r;
        for (uint32_t jp = 0; jp < pairs; ++jp) {
            const uint64_t z = boot_pair_bits(pair_c[jp], run);
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                const uint32_t j = 2 * jp + h;
                if (!live[j] || !rank_matches(key, prefix[j], a.pass)) continue;
                const uint32_t w = boot_weight_from(z, b0 + j);
                if (w) atomicAdd(&cnt[j * RANK_BINS + d], w);
            }
        }
    }
    __syncthreads();
    unsigned long long *counts = a.ws + l.counts_at + row0 * RANK_BINS;
    for (uint32_t i = tid; i < tn * RANK_BINS; i += BOOT_THREADS) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(counts + i, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(BOOT_THREADS) void msim_boot_step_kernel(unsigned long long *ws, uint32_t n_items,
                                                                      uint32_t B, uint32_t pass,
                                                                      unsigned long long *out, uint32_t *status)
{
    if (!boot_prepared(ws, 0, 0, n_items, B)) return;
    const BootLayout l = boot_layout(n_items, B);
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t row = (uint64_t)blockIdx.x * (BOOT_THREADS / 64) + threadIdx.x / 64;  // uniform over the wave
    if (row >= l.rows) return;
    unsigned long long *rowp = ws + l.counts_at + row * RANK_BINS + 4 * lane;
    const uint64_t c[4] = {rowp[0], rowp[1], rowp[2], rowp[3]};
    rowp[0] = rowp[1] = rowp[2] = rowp[3] = 0;
    const uint64_t rank = ws[l.rank_at + row];
    const bool last = pass + 1 == MSIM_RANK_PASSES;
    if (rank == MSIM_BOOT_EMPTY) {
        if (last && lane < BOOT_ROW_WORDS) out[row * BOOT_ROW_WORDS + lane] = 0;
        return;
    }
    const uint64_t s = c[0] + c[1] + c[2] + c[3];
    uint64_t incl = s;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += t;
    }
    const uint64_t rem = ws[l.remaining_at + row];
    const unsigned long long holds = __ballot(incl > rem);
    if (holds == 0) {  // the rank is not below the replicate's weight: it was not computed from W
        if (lane == 0) atomicAdd(status, 1u);
        return;
    }
    if (lane == (uint32_t)__ffsll(holds) - 1) {
        uint64_t before = incl - s, equal = c[0];
        uint32_t b = 0;
#pragma unroll
        for (uint32_t i = 0; i < 3; ++i)  // ends at b <= 3: this lane's total exceeds rem
            if (b == i && before + c[i] <= rem) {
                before += c[i];
                equal = c[i + 1];
                b = i + 1;
            }
        uint64_t words[BOOT_ROW_WORDS];
        const RankState ns = boot_row_step(RankState{ws[l.prefix_at + row], rem}, rank, 4 * lane + b, before, equal, pass,
                                           last ? words : nullptr);
        ws[l.prefix_at + row] = ns.prefix;
        ws[l.remaining_at + row] = ns.remaining;
        if (last) {
#pragma unroll
            for (uint32_t j = 0; j < BOOT_ROW_WORDS; ++j) out[row * BOOT_ROW_WORDS + j] = words[j];
        }
    }
}

__global__ __launch_bounds__(BOOT_THREADS) void msim_boot_below_kernel(BootArgs a)
{
    __shared__ unsigned long long acc[BOOT_TILE * 2 * BOOT_BELOW_SLOTS];  // [replicate][s_hi, s_lo][slot]
    __shared__ uint64_t value[BOOT_TILE], pair_c[BOOT_TILE / 2];
    if (!boot_prepared(a.ws, a.m, a.points, a.n_items, a.B)) return;
    const BootLayout l = boot_layout(a.n_items, a.B);
    const uint32_t tid = threadIdx.x, item = blockIdx.z;
    const uint32_t b0 = blockIdx.y * BOOT_TILE;
    const uint32_t tn = a.B - b0 < BOOT_TILE ? a.B - b0 : BOOT_TILE;
    const msim_boot_item it = boot_item_at(a.ws, l, item);
    if (!boot_item_ok(it, a.m, a.points, MSIM_MAX_RANKS)) return;  // uniform, and unreachable after begin's check
    unsigned long long *rows = a.rows + ((uint64_t)item * a.B + b0) * BOOT_ROW_WORDS;
    if (tid < BOOT_TILE) {
        // an empty row, and a slot past the tile, get the value 0: no key lies below it
        value[tid] = tid < tn && rows[tid * BOOT_ROW_WORDS + 2] != 0 ? rows[tid * BOOT_ROW_WORDS] : 0;
        if (tid < BOOT_TILE / 2) pair_c[tid] = boot_pair_const(a.seed, b0 + 2 * tid);
    }
    for (uint32_t i = tid; i < BOOT_TILE * 2 * BOOT_BELOW_SLOTS; i += BOOT_THREADS) acc[i] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    const size_t base = (size_t)it.point * a.runs;
    const uint32_t pairs = (tn + 1) / 2, slot = tid % BOOT_BELOW_SLOTS;
    for (uint64_t r = begin + tid; r < end; r += BOOT_THREADS) {
        const uint2 x = a.rec[(base + r) * a.m + it.column];
        const uint64_t key = boot_key(it.quantity, x.x, x.y, it.quantity == 2 ? a.bh[base + r] : 0u);
        const uint64_t hi = key >> 32, lo = key & 0xFFFFFFFFull, run = a.run_begin + r;
        for (uint32_t jp = 0; jp < pairs; ++jp) {
            const bool under0 = key < value[2 * jp], under1 = key < value[2 * jp + 1];
            if (!under0 && !under1) continue;  // most records at a low quantile: no mix, no weight
            const uint64_t z = boot_pair_bits(pair_c[jp], run);
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                if (!(h ? under1 : under0)) continue;
                const uint64_t w = boot_weight_from(z, b0 + 2 * jp + h);
                if (w == 0) continue;
                unsigned long long *at = acc + (size_t)(2 * jp + h) * 2 * BOOT_BELOW_SLOTS + slot;
                if (hi) atomicAdd(at, (unsigned long long)(w * hi));
                if (lo) atomicAdd(at + BOOT_BELOW_SLOTS, (unsigned long long)(w * lo));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < tn * 2; i += BOOT_THREADS) {  // i = replicate * 2 + {s_hi, s_lo}
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < BOOT_BELOW_SLOTS; ++k) sum += acc[(size_t)i * BOOT_BELOW_SLOTS + k];
        if (sum) atomicAdd(rows + (size_t)(i / 2) * BOOT_ROW_WORDS + 3 + i % 2, sum);
    }
}

// The grid of the count and below launches: about 2 048 workgroups in all, each at least eight runs per thread.
static bool boot_grid(uint64_t runs, uint32_t n_items, uint32_t B, uint32_t *runs_per_wg, dim3 *grid)
{
    const uint64_t tiles = ((uint64_t)B + BOOT_TILE - 1) / BOOT_TILE;
    const uint64_t want = 2048 / (tiles * n_items) ? 2048 / (tiles * n_items) : 1;
    uint64_t rpw = (runs + want - 1) / want;
    if (rpw < 8 * BOOT_THREADS) rpw = 8 * BOOT_THREADS;
    if (rpw > BOOT_MAX_WG_RUNS) rpw = BOOT_MAX_WG_RUNS;
    if (const char *e = getenv("MSIM_BOOT_TEST_WG_RUNS")) {
        const long long v = atoll(e);
        if (v > 0 && (uint64_t)v < rpw) rpw = (uint64_t)v;
    }
    const uint64_t chunks = (runs + rpw - 1) / rpw;
    if (chunks > 0x7FFFFFFFull) return false;
    *runs_per_wg = (uint32_t)rpw;
    *grid = dim3((uint32_t)chunks, (uint32_t)tiles, n_items);
    return true;
}

static bool boot_records_ok(uint32_t m, uint32_t n_points, uint64_t runs, const void *rec, const void *bh)
{
    return m != 0 && n_points != 0 && n_points <= 65535 && runs != 0 && runs <= 0xFFFFFFFFull && rec && bh;
}

}  // namespace msim

extern "C" {

size_t msim_boot_workspace_bytes(uint32_t n_items, uint32_t replicates)
{
    if (!msim::boot_shape_ok(n_items, replicates)) return 0;
    return msim::boot_layout(n_items, replicates).words * sizeof(uint64_t);
}

int msim_boot_counts_view(uint32_t n_items, uint32_t replicates, size_t *offset, size_t *words)
{
    if (!msim::boot_shape_ok(n_items, replicates) || !offset || !words) return MSIM_E_INVALID;
    const msim::BootLayout l = msim::boot_layout(n_items, replicates);
    *offset = l.counts_at * sizeof(uint64_t);
    *words = l.words - l.counts_at;
    return MSIM_OK;
}

int msim_boot_items_check(uint32_t m, uint32_t n_points, uint32_t n_q, const msim_boot_item *items, uint32_t n_items)
{
    if (!items || n_items == 0 || n_items > MSIM_MAX_BOOT_ITEMS || n_q == 0 || n_q > MSIM_MAX_RANKS) return MSIM_E_INVALID;
    for (uint32_t i = 0; i < n_items; ++i)
        if (!msim::boot_item_ok(items[i], m, n_points, n_q)) return MSIM_E_INVALID;
    return MSIM_OK;
}

uint64_t msim_boot_rank(uint64_t total_weight, double q) { return msim::boot_rank(total_weight, q); }

int msim_boot_weights_launch(uint64_t seed, uint64_t run_begin, uint64_t runs, uint32_t replicates, void *d_W,
                             void *stream)
{
    using namespace msim;
    if (runs == 0 || runs > 0xFFFFFFFFull || replicates == 0 || replicates > MSIM_MAX_BOOT_REPLICATES || !d_W)
        return MSIM_E_INVALID;
    const uint32_t pairs = (replicates + 1) / 2;
    uint64_t rpw = (runs + 63) / 64;  // at most 64 chunks per pair
    if (rpw < 8 * BOOT_THREADS) rpw = 8 * BOOT_THREADS;
    const uint64_t chunks = (runs + rpw - 1) / rpw;
    hipLaunchKernelGGL(msim_boot_weights_kernel, dim3((uint32_t)chunks, pairs), dim3(BOOT_THREADS), 0, (hipStream_t)stream,
                       seed, run_begin, runs, (uint32_t)rpw, replicates, (unsigned long long *)d_W);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_boot_begin_launch(uint32_t m, uint32_t n_points, const msim_boot_item *items, uint32_t n_items,
                           uint32_t replicates, const uint64_t *ranks, uint32_t n_q, void *d_ws, size_t ws_bytes,
                           void *stream)
{
    using namespace msim;
    if (m == 0 || n_points == 0 || n_points > 65535 || !boot_shape_ok(n_items, replicates) || !ranks || !d_ws ||
        msim_boot_items_check(m, n_points, n_q, items, n_items) != MSIM_OK ||
        ws_bytes < msim_boot_workspace_bytes(n_items, replicates))
        return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const BootLayout l = boot_layout(n_items, replicates);
    // the items' words and every row's rank, contiguous in the layout up to the ranks' end
    std::vector<uint64_t> head(l.rank_at + l.rows, 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        head[l.items_at + 2 * (size_t)i] = items[i].point | (uint64_t)items[i].column << 32;
        head[l.items_at + 2 * (size_t)i + 1] = items[i].quantity | (uint64_t)items[i].q_index << 32;
        for (uint32_t b = 0; b < replicates; ++b)
            head[l.rank_at + (size_t)i * replicates + b] = ranks[(size_t)items[i].q_index * replicates + b];
    }
    uint64_t *ws = (uint64_t *)d_ws;
    // the header stays invalid (zero) until the kernel writes it, after everything else is in place
    if (hipMemcpyAsync(ws, head.data(), head.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(ws + head.size(), 0, (l.words - head.size()) * sizeof(uint64_t), s) != hipSuccess)
        return MSIM_E_HIP;
    const uint64_t blocks = (l.rows + BOOT_THREADS - 1) / BOOT_THREADS;
    hipLaunchKernelGGL(msim_boot_begin_kernel, dim3((uint32_t)blocks), dim3(BOOT_THREADS), 0, s, (unsigned long long *)d_ws,
                       m, n_points, n_items, replicates);
    if (hipGetLastError() != hipSuccess) return MSIM_E_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? MSIM_OK : MSIM_E_HIP;  // `head` leaves scope
}

int msim_boot_count_launch(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs_per_point,
                           const void *d_per_run, const void *d_best_height, uint32_t n_items, uint32_t replicates,
                           uint32_t pass, void *d_ws, size_t ws_bytes, void *stream)
{
    using namespace msim;
    if (!boot_records_ok(m, n_points, runs_per_point, d_per_run, d_best_height) || !boot_shape_ok(n_items, replicates) ||
        pass >= MSIM_RANK_PASSES || !d_ws || ws_bytes < msim_boot_workspace_bytes(n_items, replicates))
        return MSIM_E_INVALID;
    BootArgs a = {(const uint2 *)d_per_run, (const uint32_t *)d_best_height, (unsigned long long *)d_ws, nullptr, seed,
                  run_begin, m, n_points, (uint32_t)runs_per_point, 0, n_items, replicates, pass};
    dim3 grid;
    if (!boot_grid(runs_per_point, n_items, replicates, &a.runs_per_wg, &grid)) return MSIM_E_INVALID;
    hipLaunchKernelGGL(msim_boot_count_kernel, grid, dim3(BOOT_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_boot_step_launch(uint32_t n_items, uint32_t replicates, uint32_t pass, void *d_ws, size_t ws_bytes,
                          void *d_out_or_NULL, void *d_status, void *stream)
{
    using namespace msim;
    if (!boot_shape_ok(n_items, replicates) || pass >= MSIM_RANK_PASSES || !d_ws || !d_status ||
        ws_bytes < msim_boot_workspace_bytes(n_items, replicates) || (pass + 1 == MSIM_RANK_PASSES && !d_out_or_NULL))
        return MSIM_E_INVALID;
    const uint64_t rows = (uint64_t)n_items * replicates, per = BOOT_THREADS / 64;
    hipLaunchKernelGGL(msim_boot_step_kernel, dim3((uint32_t)((rows + per - 1) / per)), dim3(BOOT_THREADS), 0,
                       (hipStream_t)stream, (unsigned long long *)d_ws, n_items, replicates, pass,
                       (unsigned long long *)d_out_or_NULL, (uint32_t *)d_status);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_boot_below_launch(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs_per_point,
                           const void *d_per_run, const void *d_best_height, uint32_t n_items, uint32_t replicates,
                           void *d_ws, size_t ws_bytes, void *d_rows, void *stream)
{
    using namespace msim;
    if (!boot_records_ok(m, n_points, runs_per_point, d_per_run, d_best_height) || !boot_shape_ok(n_items, replicates) ||
        !d_ws || !d_rows || ws_bytes < msim_boot_workspace_bytes(n_items, replicates))
        return MSIM_E_INVALID;
    BootArgs a = {(const uint2 *)d_per_run, (const uint32_t *)d_best_height, (unsigned long long *)d_ws,
                  (unsigned long long *)d_rows, seed, run_begin, m, n_points, (uint32_t)runs_per_point, 0, n_items,
                  replicates, 0};
    dim3 grid;
    if (!boot_grid(runs_per_point, n_items, replicates, &a.runs_per_wg, &grid)) return MSIM_E_INVALID;
    hipLaunchKernelGGL(msim_boot_below_kernel, grid, dim3(BOOT_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

}  // extern "C"

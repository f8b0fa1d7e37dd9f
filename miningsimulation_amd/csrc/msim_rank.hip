// msim_rank.hip — exact order statistics of the per-run terms by MSD radix selection over the records and best
// heights a launch writes on request (include/msim.h: msim_rank_begin_launch, msim_rank_count_launch,
// msim_rank_step_launch, msim_rank_launch, msim_run_order_stats, msim_sweep_run_order_stats). The key, match, digit
// and narrowing lines are msim_rank.h's.
//
// Count kernel. Grid = (run chunks, column tiles, points), 256 threads, tiled as msim_moments_kernel: a tile holds
// `tm` consecutive columns (at most 16), and thread t owns column t % tm of the tile on rows t / tm,
// t / tm + 256 / tm, ... of its run chunk, so consecutive lanes read consecutive 8-byte records. LDS holds ONE
// rank's rows of the tile, [tm][4 quantities][256] 32-bit counters: 4 KB per column, 64 KB at 16 columns. The
// ranks go over a loop inside the workgroup (the chunk's records are read again from L2), and only the ranks that
// count: ranks of a row group that still share a prefix have identical rows, so the step marks the lowest of them
// in the group's mask and the others are skipped (at pass 0 the loop runs once). A thread keeps a run of equal
// digits in a register and bumps LDS once per run, so a column of equal values, and the zero top bytes of every
// count and of shares below 1, cost one LDS atomic per thread instead of one per record. Non-zero counters are
// flushed with one 64-bit global atomic each and zeroed on the way, as the moments histogram is flushed.
// A workgroup takes at most 2^24 runs, so no 32-bit counter can wrap.
//
// Step kernel. One workgroup per (point, column, quantity) row group, one wave per rank in turn: a lane loads 4 of
// the 256 counts of the rank's counted row, a wave prefix sum finds the first bin whose running total exceeds what
// remains of the rank, and the lane that holds it narrows the state (and writes the result at the last pass). After
// a barrier the workgroup zeroes the counted rows and marks the ranks that count in the next pass.
// Count and step are separate launches on one stream: no flag, spin or counter passes between workgroups.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <memory>
#include <vector>

#include "msim_boot.h"
#include "msim_host.h"
#include "msim_rank.h"
#include "msim_tail.h"

namespace msim {

constexpr uint32_t RANK_THREADS = 256;
constexpr uint32_t RANK_TILE = 16;                  // columns of a tile at most: 64 KB of LDS
constexpr uint32_t RANK_MAX_WG_RUNS = 1u << 24;     // rows a workgroup sees per column: far below 2^32

struct RankRanks {
    uint64_t r[MSIM_MAX_RANKS];
};

// Whether the workspace is the one begin prepared for these counts; its rank count when it is, else 0.
__device__ inline uint32_t rank_header(const unsigned long long *ws, uint32_t m, uint32_t points)
{
    const uint64_t h0 = ws[0], h1 = ws[1];
    const uint32_t nr = (uint32_t)(h1 >> 32);
    if (h0 != (RANK_MAGIC | (uint64_t)m << 32) || (uint32_t)h1 != points || nr == 0 || nr > MSIM_MAX_RANKS) return 0;
    return nr;
}

__global__ __launch_bounds__(RANK_THREADS) void msim_rank_begin_kernel(unsigned long long *ws, uint32_t m,
                                                                       uint32_t points, uint32_t n_ranks, RankRanks rk)
{
    const RankLayout l = rank_layout(m, points, n_ranks);
    const uint64_t g = (uint64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    if (g == 0) {
        ws[0] = RANK_MAGIC | (uint64_t)m << 32;
        ws[1] = points | (uint64_t)n_ranks << 32;
        for (uint32_t j = 0; j < n_ranks; ++j) ws[l.ranks_at + j] = rk.r[j];
    }
    if (g >= l.groups) return;
    ws[l.mask_at + g] = 1;  // every rank shares the empty prefix: rank 0 counts for all
    for (uint32_t j = 0; j < n_ranks; ++j) {
        ws[l.state_at + (g * MSIM_MAX_RANKS + j) * 2] = 0;
        ws[l.state_at + (g * MSIM_MAX_RANKS + j) * 2 + 1] = rk.r[j];
    }
}

struct RankCountArgs {
    const uint2 *rec;        // [point][run][column] {found, stale}
    const uint32_t *bh;      // [point][run]
    unsigned long long *ws;
    uint32_t m, points, runs, tm, rows, runs_per_wg, pass;
};

__global__ __launch_bounds__(RANK_THREADS) void msim_rank_count_kernel(RankCountArgs a)
{
    extern __shared__ uint32_t lds[];  // [tm][4][256]
    const uint32_t n_ranks = rank_header(a.ws, a.m, a.points);
    if (n_ranks == 0) return;
    const RankLayout l = rank_layout(a.m, a.points, n_ranks);
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.y * a.tm;
    const uint32_t tmc = a.m - k0 < a.tm ? a.m - k0 : a.tm;  // columns of this tile
    const uint32_t p = blockIdx.z;
    const uint32_t kin = tid % a.tm, row = tid / a.tm;
    const bool active = row < a.rows && kin < tmc;
    const uint64_t g0 = ((uint64_t)p * a.m + k0) * RANK_QUANTITIES;  // the tile's first row group
    const uint64_t gk = g0 + (uint64_t)kin * RANK_QUANTITIES;         // this thread's column's
    uint32_t mask[RANK_QUANTITIES];
#pragma unroll
    for (uint32_t q = 0; q < RANK_QUANTITIES; ++q) mask[q] = active ? (uint32_t)a.ws[l.mask_at + gk + q] : 0;
    // the ranks any column of the tile counts, gathered in the first counter before the counters are cleared (the
    // 64 KB of a 16-column tile leave no room for a word of its own)
    if (tid == 0) lds[0] = 0;
    __syncthreads();
    const uint32_t any = mask[0] | mask[1] | mask[2] | mask[3];
    if (any) atomicOr(&lds[0], any);
    __syncthreads();
    const uint32_t todo = lds[0];
    __syncthreads();
    for (uint32_t i = tid; i < a.tm * RANK_QUANTITIES * RANK_BINS; i += RANK_THREADS) lds[i] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * a.runs_per_wg;
    const uint64_t end = begin + a.runs_per_wg < a.runs ? begin + a.runs_per_wg : a.runs;
    const size_t base = (size_t)p * a.runs;
    uint32_t *mine = lds + kin * RANK_QUANTITIES * RANK_BINS;
    unsigned long long *counts = a.ws + l.counts_at;
    for (uint32_t j = 0; j < n_ranks; ++j) {
        if (!(todo >> j & 1u)) continue;  // uniform over the workgroup
        if (any >> j & 1u) {
            uint64_t prefix[RANK_QUANTITIES];
            uint32_t last[RANK_QUANTITIES], cnt[RANK_QUANTITIES];
            bool on[RANK_QUANTITIES];
#pragma unroll
            for (uint32_t q = 0; q < RANK_QUANTITIES; ++q) {
                on[q] = mask[q] >> j & 1u;
                prefix[q] = on[q] ? a.ws[l.state_at + ((gk + q) * MSIM_MAX_RANKS + j) * 2] : 0;
                last[q] = 0;
                cnt[q] = 0;
            }
            for (uint64_t r = begin + row; r < end; r += a.rows) {
                const uint2 x = a.rec[(base + r) * a.m + k0 + kin];
                uint64_t key[RANK_QUANTITIES];
                key[0] = x.x;
                key[1] = x.y;
                key[2] = on[2] ? mom_share_term(x.x, a.bh[base + r]) : 0;
                key[3] = on[3] ? mom_rate_term(x.x, x.y) : 0;
#pragma unroll
                for (uint32_t q = 0; q < RANK_QUANTITIES; ++q) {
                    if (!on[q] || !rank_matches(key[q], prefix[q], a.pass)) continue;
                    const uint32_t d = rank_digit(key[q], a.pass);
                    if (d != last[q] && cnt[q]) {
                        atomicAdd(mine + q * RANK_BINS + last[q], cnt[q]);
                        cnt[q] = 0;
                    }
                    last[q] = d;
                    cnt[q] += 1;
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < RANK_QUANTITIES; ++q)
                if (cnt[q]) atomicAdd(mine + q * RANK_BINS + last[q], cnt[q]);
        }
        __syncthreads();
        // flush rank j's rows: one global atomic per non-zero bin, zeroed for the next rank
        for (uint32_t i = tid; i < tmc * RANK_QUANTITIES * RANK_BINS; i += RANK_THREADS) {
            const uint32_t v = lds[i];
            if (v) {
                lds[i] = 0;
                atomicAdd(counts + ((g0 + i / RANK_BINS) * n_ranks + j) * RANK_BINS + i % RANK_BINS, (unsigned long long)v);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RANK_THREADS) void msim_rank_step_kernel(unsigned long long *ws, uint32_t m,
                                                                      uint32_t points, uint32_t pass,
                                                                      msim_order_stat *out, uint32_t *status)
{
    __shared__ uint64_t old_prefix[MSIM_MAX_RANKS], old_rem[MSIM_MAX_RANKS], new_prefix[MSIM_MAX_RANKS];
    __shared__ uint32_t next_mask;
    const uint32_t n_ranks = rank_header(ws, m, points);
    if (n_ranks == 0) return;
    const RankLayout l = rank_layout(m, points, n_ranks);
    const uint64_t g = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
    const uint32_t counted = (uint32_t)ws[l.mask_at + g];
    unsigned long long *state = ws + l.state_at + g * MSIM_MAX_RANKS * 2;
    unsigned long long *counts = ws + l.counts_at + g * n_ranks * RANK_BINS;
    if (tid < n_ranks) {
        old_prefix[tid] = state[tid * 2];
        old_rem[tid] = state[tid * 2 + 1];
        new_prefix[tid] = old_prefix[tid];
    }
    if (tid == 0) next_mask = 0;
    __syncthreads();
    for (uint32_t j = wave; j < n_ranks; j += RANK_THREADS / 64) {  // uniform over the wave
        uint32_t rep = j;  // the lowest rank with this prefix: the one that was counted
        for (uint32_t i = 0; i < j; ++i)
            if (old_prefix[i] == old_prefix[j]) {
                rep = i;
                break;
            }
        const unsigned long long *rowp = counts + (size_t)rep * RANK_BINS + 4 * lane;
        const uint64_t c[4] = {rowp[0], rowp[1], rowp[2], rowp[3]};
        const uint64_t s = c[0] + c[1] + c[2] + c[3];
        uint64_t incl = s;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up((unsigned long long)incl, d, 64);
            if (lane >= d) incl += t;
        }
        const uint64_t rem = old_rem[j];
        const unsigned long long holds = __ballot(incl > rem);
        if (holds == 0) {  // the rank is not below the number of keys
            if (lane == 0) atomicAdd(status, 1u);
            continue;
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
            const RankState ns = rank_narrow(RankState{old_prefix[j], rem}, 4 * lane + b, before, pass);
            state[j * 2] = ns.prefix;
            state[j * 2 + 1] = ns.remaining;
            new_prefix[j] = ns.prefix;
            if (pass + 1 == MSIM_RANK_PASSES) out[g * n_ranks + j] = rank_result(ns, ws[l.ranks_at + j], equal);
        }
    }
    __syncthreads();
    for (uint32_t j = 0; j < n_ranks; ++j)
        if (counted >> j & 1u) counts[(size_t)j * RANK_BINS + tid] = 0;
    if (tid < n_ranks) {
        bool first = true;
        for (uint32_t i = 0; i < tid; ++i) first = first && new_prefix[i] != new_prefix[tid];
        if (first) atomicOr(&next_mask, 1u << tid);
    }
    __syncthreads();
    if (tid == 0) ws[l.mask_at + g] = next_mask;
}

static bool rank_shape_ok(uint32_t m, uint32_t n_points, uint32_t n_ranks)
{
    return m != 0 && n_points != 0 && n_points <= 65535 && n_ranks >= 1 && n_ranks <= MSIM_MAX_RANKS;
}

}  // namespace msim

extern "C" {

size_t msim_rank_workspace_bytes(uint32_t m, uint32_t n_points, uint32_t n_ranks)
{
    if (!msim::rank_shape_ok(m, n_points, n_ranks)) return 0;
    return msim::rank_layout(m, n_points, n_ranks).words * sizeof(uint64_t);
}

int msim_rank_counts_view(uint32_t m, uint32_t n_points, uint32_t n_ranks, size_t *offset, size_t *words)
{
    if (!msim::rank_shape_ok(m, n_points, n_ranks) || !offset || !words) return MSIM_E_INVALID;
    const msim::RankLayout l = msim::rank_layout(m, n_points, n_ranks);
    *offset = l.counts_at * sizeof(uint64_t);
    *words = l.words - l.counts_at;
    return MSIM_OK;
}

int msim_ranks_check(uint64_t n_runs, const uint64_t *ranks, uint32_t n_ranks)
{
    if (!ranks || n_ranks == 0 || n_ranks > MSIM_MAX_RANKS) return MSIM_E_INVALID;
    for (uint32_t j = 0; j < n_ranks; ++j)
        if (ranks[j] >= n_runs) return MSIM_E_INVALID;
    return MSIM_OK;
}

int msim_rank_begin_launch(uint32_t m, uint32_t n_points, const uint64_t *ranks, uint32_t n_ranks, void *d_ws,
                           size_t ws_bytes, void *stream)
{
    using namespace msim;
    if (!rank_shape_ok(m, n_points, n_ranks) || !ranks || !d_ws || ws_bytes < msim_rank_workspace_bytes(m, n_points, n_ranks))
        return MSIM_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const RankLayout l = rank_layout(m, n_points, n_ranks);
    RankRanks rk;
    for (uint32_t j = 0; j < MSIM_MAX_RANKS; ++j) rk.r[j] = j < n_ranks ? ranks[j] : 0;
    if (hipMemsetAsync(d_ws, 0, l.words * sizeof(uint64_t), s) != hipSuccess) return MSIM_E_HIP;
    const uint64_t blocks = (l.groups + RANK_THREADS - 1) / RANK_THREADS;
    hipLaunchKernelGGL(msim_rank_begin_kernel, dim3((uint32_t)blocks), dim3(RANK_THREADS), 0, s,
                       (unsigned long long *)d_ws, m, n_points, n_ranks, rk);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_rank_count_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                           const void *d_best_height, uint32_t pass, void *d_ws, size_t ws_bytes, void *stream)
{
    using namespace msim;
    // the launch does not know the rank count: the workspace of one rank is the least begin can have been given
    if (!rank_shape_ok(m, n_points, 1) || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull || !d_per_run ||
        !d_best_height || pass >= MSIM_RANK_PASSES || !d_ws || ws_bytes < msim_rank_workspace_bytes(m, n_points, 1))
        return MSIM_E_INVALID;
    RankCountArgs a;
    a.rec = (const uint2 *)d_per_run;
    a.bh = (const uint32_t *)d_best_height;
    a.ws = (unsigned long long *)d_ws;
    a.m = m;
    a.points = n_points;
    a.runs = (uint32_t)runs_per_point;
    a.tm = m < RANK_TILE ? m : RANK_TILE;
    a.rows = RANK_THREADS / a.tm;
    a.pass = pass;
    const uint64_t tiles = ((uint64_t)m + a.tm - 1) / a.tm;
    if (tiles > 65535) return MSIM_E_INVALID;
    // about 2 048 workgroups in all, each at least eight rows per thread
    const uint64_t want = 2048 / (tiles * n_points) ? 2048 / (tiles * n_points) : 1;
    uint64_t rpw = (runs_per_point + want - 1) / want;
    if (rpw < 8 * a.rows) rpw = 8 * a.rows;
    if (rpw > RANK_MAX_WG_RUNS) rpw = RANK_MAX_WG_RUNS;
    if (const char *e = getenv("MSIM_RANK_TEST_WG_RUNS")) {
        const long long v = atoll(e);
        if (v > 0 && (uint64_t)v < rpw) rpw = (uint64_t)v;
    }
    a.runs_per_wg = (uint32_t)rpw;
    const uint64_t chunks = (runs_per_point + rpw - 1) / rpw;
    if (chunks > 0x7FFFFFFFull) return MSIM_E_INVALID;
    const dim3 grid((uint32_t)chunks, (uint32_t)tiles, n_points);
    const size_t lds = (size_t)a.tm * RANK_QUANTITIES * RANK_BINS * sizeof(uint32_t);
    hipLaunchKernelGGL(msim_rank_count_kernel, grid, dim3(RANK_THREADS), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_rank_step_launch(uint32_t m, uint32_t n_points, uint32_t pass, void *d_ws, size_t ws_bytes,
                          void *d_out_or_NULL, void *d_status, void *stream)
{
    using namespace msim;
    if (!rank_shape_ok(m, n_points, 1) || pass >= MSIM_RANK_PASSES || !d_ws || !d_status ||
        ws_bytes < msim_rank_workspace_bytes(m, n_points, 1) || (pass + 1 == MSIM_RANK_PASSES && !d_out_or_NULL))
        return MSIM_E_INVALID;
    const uint64_t groups = rank_layout(m, n_points, 1).groups;
    if (groups > 0x7FFFFFFFull) return MSIM_E_INVALID;
    hipLaunchKernelGGL(msim_rank_step_kernel, dim3((uint32_t)groups), dim3(RANK_THREADS), 0, (hipStream_t)stream,
                       (unsigned long long *)d_ws, m, n_points, pass, (msim_order_stat *)d_out_or_NULL,
                       (uint32_t *)d_status);
    return hipGetLastError() == hipSuccess ? MSIM_OK : MSIM_E_HIP;
}

int msim_rank_launch(uint32_t m, uint32_t n_points, uint64_t runs_per_point, const void *d_per_run,
                     const void *d_best_height, const uint64_t *ranks, uint32_t n_ranks, void *d_out, void *d_status,
                     void *d_ws, size_t ws_bytes, void *stream)
{
    if (!msim::rank_shape_ok(m, n_points, n_ranks) || runs_per_point == 0 || runs_per_point > 0xFFFFFFFFull ||
        !d_per_run || !d_best_height || !ranks || !d_out || !d_status || !d_ws ||
        ws_bytes < msim_rank_workspace_bytes(m, n_points, n_ranks))
        return MSIM_E_INVALID;
    int rc = msim_rank_begin_launch(m, n_points, ranks, n_ranks, d_ws, ws_bytes, stream);
    for (uint32_t pass = 0; rc == MSIM_OK && pass < MSIM_RANK_PASSES; ++pass) {
        rc = msim_rank_count_launch(m, n_points, runs_per_point, d_per_run, d_best_height, pass, d_ws, ws_bytes, stream);
        if (rc == MSIM_OK) rc = msim_rank_step_launch(m, n_points, pass, d_ws, ws_bytes, d_out, d_status, stream);
    }
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------- host conveniences
namespace {

constexpr uint64_t RANK_CHUNK_BYTES = 1ull << 30;  // records of one chunk, as msim_run_moments'

uint64_t chunk_cap()
{
    const char *e = getenv("MSIM_MOMENTS_CHUNK_RUNS");
    if (!e) return 0;
    const long long v = atoll(e);
    return v > 0 ? (uint64_t)v : 0;
}

struct Resident {
    msim::DevBuf rec, bh;  // one chunk's (folded) records and best heights
    uint64_t runs;
    uint64_t begin;  // the absolute index of the chunk's first run
};

// What msim_run_tails adds to the order statistics' job (null for the order statistics alone): the columns' total
// moments, summed per chunk, and the tails at the selected order statistics, summed per resident buffer.
struct TailJob {
    const msim_tail_spec *specs;
    uint32_t n_specs;
    msim_moments *out_moments;  // [np][columns]
    msim_tail *out_tails;       // [n_specs]
};

// What msim_run_bootstrap adds (null otherwise): the replicates' total weights, summed per chunk, and after the order
// statistics the bootstrap's own selection and below pass over every resident buffer.
struct BootJob {
    const msim_boot_item *items;
    uint32_t n_items;
    const double *qs;
    uint32_t n_q, replicates;
    uint64_t seed;
    uint64_t *out_W;          // [replicates]
    msim_boot_row *out_rows;  // [n_items][replicates]
};

// Begin, eight rounds of count-per-buffer and step, then the below pass, on the stream `s`; W has been summed.
int run_boot_job(const BootJob &job, uint32_t mc, uint32_t np, const std::vector<Resident> &kept, msim::DevBuf &dW,
                 hipStream_t s)
{
    const uint32_t B = job.replicates;
    const size_t bwsb = msim_boot_workspace_bytes(job.n_items, B);
    const size_t n_rows = (size_t)job.n_items * B;
    msim::DevBuf bws, rows, bstatus;
    if (!bwsb || !bws.alloc(bwsb) || !rows.alloc(n_rows * sizeof(msim_boot_row)) || !bstatus.alloc(sizeof(uint32_t)))
        return MSIM_E_HIP;
    std::vector<uint64_t> ranks((size_t)job.n_q * B);
    if (hipMemcpyAsync(job.out_W, dW.get(), B * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(bstatus.get(), 0, sizeof(uint32_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return MSIM_E_HIP;
    for (uint32_t j = 0; j < job.n_q; ++j)
        for (uint32_t b = 0; b < B; ++b) ranks[(size_t)j * B + b] = msim_boot_rank(job.out_W[b], job.qs[j]);
    int rc = msim_boot_begin_launch(mc, np, job.items, job.n_items, B, ranks.data(), job.n_q, bws.get(), bwsb, s);
    for (uint32_t pass = 0; rc == MSIM_OK && pass < MSIM_RANK_PASSES; ++pass) {
        for (size_t i = 0; rc == MSIM_OK && i < kept.size(); ++i)
            rc = msim_boot_count_launch(mc, np, job.seed, kept[i].begin, kept[i].runs, kept[i].rec.get(), kept[i].bh.get(),
                                        job.n_items, B, pass, bws.get(), bwsb, s);
        if (rc == MSIM_OK) rc = msim_boot_step_launch(job.n_items, B, pass, bws.get(), bwsb, rows.get(), bstatus.get(), s);
    }
    for (size_t i = 0; rc == MSIM_OK && i < kept.size(); ++i)
        rc = msim_boot_below_launch(mc, np, job.seed, kept[i].begin, kept[i].runs, kept[i].rec.get(), kept[i].bh.get(),
                                    job.n_items, B, bws.get(), bwsb, rows.get(), s);
    if (rc) return rc;
    uint32_t bad = 0;
    if (hipMemcpyAsync(job.out_rows, rows.get(), n_rows * sizeof(msim_boot_row), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&bad, bstatus.get(), sizeof(bad), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return MSIM_E_HIP;
    return bad ? MSIM_E_INVALID : MSIM_OK;  // unreachable: the ranks come from W
}

// Runs [run_begin, run_begin + runs) of n_points networks of m miners in chunks, each launched once into a record
// buffer that stays resident (with a class map: launched into one per-miner buffer and folded into the chunk's own);
// then begin, and per pass one count launch per chunk and one step. With a TailJob every chunk also runs
// msim_moments_launch, and after the last step the specs become items (value = the spec's order statistic) and
// msim_tail_launch runs on every resident buffer. With a BootJob every chunk also adds its weights to W, and
// run_boot_job follows the order statistics.
template <class WsBytes, class Launch>
int run_order_impl(uint32_t m, uint32_t np, uint64_t run_begin, uint64_t runs, int device, const uint32_t *class_of,
                   uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks, msim_stats *out_stats,
                   msim_sums *opt_sums, msim_order_stat *out_order, bool general, WsBytes ws_bytes, Launch launch,
                   const TailJob *tail = nullptr, const BootJob *boot = nullptr)
{
    if (!out_stats || !out_order || runs == 0 || m == 0 || np == 0 || np > 65535) return MSIM_E_INVALID;
    if ((class_of == nullptr) != (n_classes == 0)) return MSIM_E_INVALID;
    if (class_of && msim_classes_check(m, class_of, n_classes) != MSIM_OK) return MSIM_E_INVALID;
    if (msim_ranks_check(runs, ranks, n_ranks) != MSIM_OK) return MSIM_E_INVALID;
    const uint32_t mc = class_of ? n_classes : m;  // columns of the selection
    if (tail) {
        if (!tail->specs || !tail->out_moments || !tail->out_tails || tail->n_specs == 0 ||
            tail->n_specs > MSIM_MAX_TAIL_ITEMS)
            return MSIM_E_INVALID;
        for (uint32_t i = 0; i < tail->n_specs; ++i) {
            const msim_tail_spec &sp = tail->specs[i];
            if (sp.cond_point >= np || sp.target_point >= np || sp.cond_column >= mc || sp.target_column >= mc ||
                sp.quantity >= msim::RANK_QUANTITIES || sp.rank_index >= n_ranks)
                return MSIM_E_INVALID;
        }
    }
    if (boot) {
        if (!boot->qs || !boot->out_W || !boot->out_rows || runs >= MSIM_BOOT_MAX_RUNS ||
            boot->replicates == 0 || boot->replicates > MSIM_MAX_BOOT_REPLICATES ||
            msim_boot_items_check(mc, np, boot->n_q, boot->items, boot->n_items) != MSIM_OK)
            return MSIM_E_INVALID;
        for (uint32_t j = 0; j < boot->n_q; ++j)
            if (!(boot->qs[j] >= 0.0 && boot->qs[j] <= 1.0)) return MSIM_E_INVALID;
    }
    if (hipSetDevice(device) != hipSuccess) return MSIM_E_HIP;
    uint64_t chunk = msim::MAX_LAUNCH_RUNS / np;
    const uint64_t by_bytes = RANK_CHUNK_BYTES / ((uint64_t)np * m * sizeof(msim_run_record));
    if (chunk > by_bytes) chunk = by_bytes ? by_bytes : 1;
    if (const uint64_t cap = chunk_cap())
        if (chunk > cap) chunk = cap;
    if (chunk > runs) chunk = runs;
    if (chunk == 0) return MSIM_E_INVALID;
    const size_t wsb = ws_bytes(chunk);
    if (!wsb) return MSIM_E_INVALID;
    const size_t rwsb = msim_rank_workspace_bytes(mc, np, n_ranks);
    if (!rwsb) return MSIM_E_INVALID;
    const size_t n_sums = 6 * (size_t)np * m, n_out = (size_t)np * mc * msim::RANK_QUANTITIES * n_ranks;
    std::vector<uint64_t> acc_s(n_sums, 0), part_s(n_sums);
    const size_t n_mom = tail ? (size_t)np * mc * msim::MOM_WORDS : 0;
    const size_t n_tw = tail ? (size_t)tail->n_specs * msim::TAIL_WORDS : 0;
    std::vector<uint64_t> acc_m(n_mom, 0), part_m(n_mom), acc_t(n_tw, 0), part_t(n_tw);
    uint32_t st[2] = {0, 0}, bad = 0;
    if (general && !msim::workspace_fits(wsb)) return MSIM_E_MINERS;
    msim::DevBuf ws, sums, status, rec, map, rws, order, rstatus, mom, items, tails, bootW;
    std::vector<Resident> kept((runs + chunk - 1) / chunk);
    msim::DevStream stream;  // after the buffers: destroyed before they are freed
    if (!ws.alloc(wsb) || !sums.alloc(n_sums * sizeof(uint64_t)) || !status.alloc(sizeof(st)) ||
        (class_of && (!map.alloc(m * sizeof(uint32_t)) || !rec.alloc(chunk * np * m * sizeof(msim_run_record)))) ||
        !rws.alloc(rwsb) || !order.alloc(n_out * sizeof(msim_order_stat)) || !rstatus.alloc(sizeof(uint32_t)) ||
        (tail && (!mom.alloc(n_mom * sizeof(uint64_t)) || !items.alloc(tail->n_specs * sizeof(msim_tail_item)) ||
                  !tails.alloc(n_tw * sizeof(uint64_t)))) ||
        (boot && !bootW.alloc(boot->replicates * sizeof(uint64_t))) || !stream.create())
        return MSIM_E_HIP;
    hipStream_t s = stream.get();
    if (boot && hipMemsetAsync(bootW.get(), 0, boot->replicates * sizeof(uint64_t), s) != hipSuccess) return MSIM_E_HIP;
    if (class_of && hipMemcpy(map.get(), class_of, m * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        return MSIM_E_HIP;
    size_t at = 0;
    for (uint64_t off = 0; off < runs; off += chunk, ++at) {
        const uint64_t cn = runs - off < chunk ? runs - off : chunk;
        Resident &k = kept[at];
        k.runs = cn;
        k.begin = run_begin + off;
        if (!k.rec.alloc(cn * np * mc * sizeof(msim_run_record)) || !k.bh.alloc(cn * np * sizeof(uint32_t)))
            return MSIM_E_HIP;
        void *into = class_of ? rec.get() : k.rec.get();
        int rc = launch(run_begin + off, cn, sums.get(), into, k.bh.get(), status.get(), ws.get(), wsb, s);
        if (rc) return rc;
        if (class_of) {
            rc = msim_fold_launch(m, np, cn, rec.get(), map.get(), mc, k.rec.get(), s);
            if (rc) return rc;
        }
        if (boot) {
            rc = msim_boot_weights_launch(boot->seed, run_begin + off, cn, boot->replicates, bootW.get(), s);
            if (rc) return rc;
        }
        if (tail) {
            rc = msim_moments_launch(mc, np, cn, k.rec.get(), k.bh.get(), nullptr, mom.get(), nullptr, s);
            if (rc) return rc;
            if (hipMemcpyAsync(part_m.data(), mom.get(), n_mom * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess)
                return MSIM_E_HIP;
        }
        if (hipMemcpyAsync(part_s.data(), sums.get(), n_sums * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(st, status.get(), sizeof(st), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return MSIM_E_HIP;
        if (st[1] != 0) return MSIM_E_CAPACITY;
        for (size_t i = 0; i < n_sums; ++i) acc_s[i] += part_s[i];
        for (size_t i = 0; i < n_mom; ++i) acc_m[i] += part_m[i];
    }
    if (hipMemsetAsync(rstatus.get(), 0, sizeof(uint32_t), s) != hipSuccess) return MSIM_E_HIP;
    int rc = msim_rank_begin_launch(mc, np, ranks, n_ranks, rws.get(), rwsb, s);
    for (uint32_t pass = 0; rc == MSIM_OK && pass < MSIM_RANK_PASSES; ++pass) {
        for (size_t i = 0; rc == MSIM_OK && i < kept.size(); ++i)
            rc = msim_rank_count_launch(mc, np, kept[i].runs, kept[i].rec.get(), kept[i].bh.get(), pass, rws.get(), rwsb, s);
        if (rc == MSIM_OK) rc = msim_rank_step_launch(mc, np, pass, rws.get(), rwsb, order.get(), rstatus.get(), s);
    }
    if (rc) return rc;
    std::vector<msim_order_stat> got(n_out);
    if (hipMemcpyAsync(got.data(), order.get(), n_out * sizeof(msim_order_stat), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&bad, rstatus.get(), sizeof(bad), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return MSIM_E_HIP;
    if (bad) return MSIM_E_INVALID;  // unreachable after msim_ranks_check
    if (tail) {
        std::vector<msim_tail_item> its(tail->n_specs);
        for (uint32_t i = 0; i < tail->n_specs; ++i) {
            const msim_tail_spec &sp = tail->specs[i];
            const size_t at_o = (((size_t)sp.cond_point * mc + sp.cond_column) * msim::RANK_QUANTITIES + sp.quantity) * n_ranks;
            its[i] = msim_tail_item{sp.cond_point, sp.cond_column, sp.quantity, sp.target_point, sp.target_column, 0,
                                    got[at_o + sp.rank_index].value};
        }
        if (hipMemcpyAsync(items.get(), its.data(), its.size() * sizeof(msim_tail_item), hipMemcpyHostToDevice, s) != hipSuccess)
            return MSIM_E_HIP;
        for (size_t i = 0; i < kept.size(); ++i) {
            rc = msim_tail_launch(mc, np, kept[i].runs, kept[i].rec.get(), kept[i].bh.get(), items.get(), tail->n_specs,
                                  tails.get(), s);
            if (rc) return rc;
            if (hipMemcpyAsync(part_t.data(), tails.get(), n_tw * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return MSIM_E_HIP;
            for (size_t j = 0; j < n_tw; ++j) acc_t[j] += part_t[j];
        }
        memcpy(tail->out_moments, acc_m.data(), n_mom * sizeof(uint64_t));
        memcpy(tail->out_tails, acc_t.data(), n_tw * sizeof(uint64_t));
    }
    if (boot) {
        rc = run_boot_job(*boot, mc, np, kept, bootW, s);
        if (rc) return rc;
    }
    if (opt_sums) memcpy(opt_sums, acc_s.data(), n_sums * sizeof(uint64_t));
    msim_sums_to_stats((const msim_sums *)acc_s.data(), np * m, out_stats);
    memcpy(out_order, got.data(), n_out * sizeof(msim_order_stat));
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_run_order_stats(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                         const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                         msim_stats *out_stats, msim_sums *opt_sums, msim_order_stat *out_order)
{
    if (!cfg) return MSIM_E_INVALID;
    msim_pipeline_layout pl;
    const bool general = msim_pipeline_info(cfg, 1, &pl) == MSIM_OK && pl.uses_pipeline == 4;
    return run_order_impl(
        msim_config_miner_count(cfg), 1, run_begin, n_runs, device, class_of_or_NULL, n_classes, ranks, n_ranks,
        out_stats, opt_sums, out_order, general, [&](uint64_t n) { return msim_workspace_bytes(cfg, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_launch(cfg, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        });
}

int msim_sweep_run_order_stats(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point,
                               uint32_t seed_base, int device, const uint32_t *class_of_or_NULL, uint32_t n_classes,
                               const uint64_t *ranks, uint32_t n_ranks, msim_stats *out_stats, msim_sums *opt_sums,
                               msim_order_stat *out_order)
{
    if (!sweep) return MSIM_E_INVALID;
    return run_order_impl(
        msim_sweep_miner_count(sweep), msim_sweep_point_count(sweep), run_begin, runs_per_point, device,
        class_of_or_NULL, n_classes, ranks, n_ranks, out_stats, opt_sums, out_order, false,
        [&](uint64_t n) { return msim_sweep_workspace_bytes(sweep, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_sweep_launch(sweep, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        });
}

int msim_run_tails(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                   const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                   const msim_tail_spec *specs, uint32_t n_specs, msim_stats *out_stats, msim_sums *opt_sums,
                   msim_order_stat *out_order, msim_moments *out_moments, msim_tail *out_tails)
{
    if (!cfg) return MSIM_E_INVALID;
    msim_pipeline_layout pl;
    const bool general = msim_pipeline_info(cfg, 1, &pl) == MSIM_OK && pl.uses_pipeline == 4;
    const TailJob job = {specs, n_specs, out_moments, out_tails};
    return run_order_impl(
        msim_config_miner_count(cfg), 1, run_begin, n_runs, device, class_of_or_NULL, n_classes, ranks, n_ranks,
        out_stats, opt_sums, out_order, general, [&](uint64_t n) { return msim_workspace_bytes(cfg, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_launch(cfg, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        &job);
}

int msim_sweep_run_tails(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                         int device, const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks,
                         uint32_t n_ranks, const msim_tail_spec *specs, uint32_t n_specs, msim_stats *out_stats,
                         msim_sums *opt_sums, msim_order_stat *out_order, msim_moments *out_moments,
                         msim_tail *out_tails)
{
    if (!sweep) return MSIM_E_INVALID;
    const TailJob job = {specs, n_specs, out_moments, out_tails};
    return run_order_impl(
        msim_sweep_miner_count(sweep), msim_sweep_point_count(sweep), run_begin, runs_per_point, device,
        class_of_or_NULL, n_classes, ranks, n_ranks, out_stats, opt_sums, out_order, false,
        [&](uint64_t n) { return msim_sweep_workspace_bytes(sweep, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_sweep_launch(sweep, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        &job);
}

int msim_run_bootstrap(const msim_config *cfg, uint64_t run_begin, uint64_t n_runs, uint32_t seed_base, int device,
                       const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks, uint32_t n_ranks,
                       const msim_boot_item *items, uint32_t n_items, const double *qs, uint32_t n_q,
                       uint32_t replicates, uint64_t boot_seed, msim_stats *out_stats, msim_sums *opt_sums,
                       msim_order_stat *out_order, uint64_t *out_W, msim_boot_row *out_rows)
{
    if (!cfg) return MSIM_E_INVALID;
    msim_pipeline_layout pl;
    const bool general = msim_pipeline_info(cfg, 1, &pl) == MSIM_OK && pl.uses_pipeline == 4;
    const BootJob job = {items, n_items, qs, n_q, replicates, boot_seed, out_W, out_rows};
    return run_order_impl(
        msim_config_miner_count(cfg), 1, run_begin, n_runs, device, class_of_or_NULL, n_classes, ranks, n_ranks,
        out_stats, opt_sums, out_order, general, [&](uint64_t n) { return msim_workspace_bytes(cfg, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_launch(cfg, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        nullptr, &job);
}

int msim_sweep_run_bootstrap(const msim_sweep *sweep, uint64_t run_begin, uint64_t runs_per_point, uint32_t seed_base,
                             int device, const uint32_t *class_of_or_NULL, uint32_t n_classes, const uint64_t *ranks,
                             uint32_t n_ranks, const msim_boot_item *items, uint32_t n_items, const double *qs,
                             uint32_t n_q, uint32_t replicates, uint64_t boot_seed, msim_stats *out_stats,
                             msim_sums *opt_sums, msim_order_stat *out_order, uint64_t *out_W,
                             msim_boot_row *out_rows)
{
    if (!sweep) return MSIM_E_INVALID;
    const BootJob job = {items, n_items, qs, n_q, replicates, boot_seed, out_W, out_rows};
    return run_order_impl(
        msim_sweep_miner_count(sweep), msim_sweep_point_count(sweep), run_begin, runs_per_point, device,
        class_of_or_NULL, n_classes, ranks, n_ranks, out_stats, opt_sums, out_order, false,
        [&](uint64_t n) { return msim_sweep_workspace_bytes(sweep, n); },
        [&](uint64_t b, uint64_t n, void *sums, void *rec, void *bh, void *status, void *ws, size_t wsb, hipStream_t s) {
            return msim_sweep_launch(sweep, b, n, seed_base, sums, rec, bh, status, ws, wsb, s);
        },
        nullptr, &job);
}

}  // extern "C"

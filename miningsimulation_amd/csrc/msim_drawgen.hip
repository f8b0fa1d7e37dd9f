// msim_drawgen.hip — K1 of the event-skipping pipeline (msim_pipeline.h): every block's draws.
//
// One lane = (run, segment): both of the run's xoroshiro128++ streams (main.cpp:134) are jumped to
// draw j*SEG (msim_jump.h), then the lane produces SEG blocks exactly as the reference's sequential
// loop would draw them (simulation.h:205-221): interval I_i (ms), finder k_i, and the "fast" bit
// I_{i+1} > prop_{k_i} (honest finders only). A wave = 64 consecutive runs at one segment, so the
// jump matrix columns are wave-uniform scalar loads. Nothing is stored per block: a non-fast block is
// listed with both RNG states (K2 redraws its episode), and each group of the band where a run can end
// keeps its first word and RNG states (K3 redraws the last group). Roofline: VALU issue (FP64 log +
// 64-bit integer RNG).
#include <hip/hip_runtime.h>

#include "msim_jump.h"
#include "msim_kernels.h"
#include "msim_pipeline.h"

namespace msim {

__device__ __noinline__ int32_t interval_ms_exact_dev(uint64_t u) { return (int32_t)interval_ms_of(u); }


// Side effects of one K1 lane (msim_pipeline.h draw_segment): LDS per-owner counters (one u32 per owner
// and lane, [owner][lane]: conflict-free, and the increment is one ds_add_u32 of a constant), wave-
// aggregated appends to the dense episode list, the band's group records.
constexpr uint32_t K1_OWNERS = 2 * CNT_WORDS;  // 15 miners + PickFinder's fall-through (index 15)
constexpr uint32_t K1_NSL = K1_OWNERS;         // LDS row after the owners: the lane's slow-block count
constexpr uint32_t K1_ROWS = K1_NSL + 1;

// The slow path keeps no per-lane register across the draw loop: its lane-dependent values are rebuilt from
// the ballot mask (mbcnt), wave-uniform SGPRs and LDS (the per-lane list count), so the loop's register
// budget (K1_WAVES below) goes to the draws. Measured on MI355X (profiles/r03/INDEX.md): with the lane id,
// its bit, the list count and the counter address held across the loop, the compiler reloaded them from
// scratch once per quad (six scratch loads and two vmcnt(0) waits per quad).
struct DevCtx {
    const DrawArgs &a;
    uint32_t (*cnt)[256];
    uint64_t amask;  // active lanes of the wave (runs < n)
    uint32_t tid, r0, seg, jb;  // r0: the wave's first run (wave-uniform)
    uint32_t cbase;             // tid * 4, the lane's byte offset in a counter row (hold())
    // The one lane-dependent value held across the loop: at 4 waves per SIMD the budget has the register, and
    // rebuilding it (two v_mbcnt and a shift-add per quad, as the 5- and 6-wave budgets needed) cost 0.75 VALU a block.
    __device__ __forceinline__ void hold()
    {
        cbase = tid * 4u;
        asm volatile("" : "+v"(cbase));  // a register of its own, not an expression to rebuild at each use
    }
    // row = the byte offset of owner k's counter row, k << 10 (K1Draws::row: info & (15 << INFO_K_SHIFT), or the
    // pick entry itself in the uniform-delay form)
    __device__ __forceinline__ void count(uint32_t row)
    {
        // the array's base is a constant the compiler folds into the instruction's offset field
        const uint32_t ad = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&cnt[0][0] + (row | cbase);
        __atomic_fetch_add((__attribute__((address_space(3))) uint32_t *)(uintptr_t)ad, 1u, __ATOMIC_RELAXED);
    }
    __device__ __forceinline__ bool vote(bool s) const { return (__builtin_amdgcn_ballot_w64(s) & amask) != 0ull; }
    // the owner counters packed as the u16 pairs of the workspace layout (msim_pipeline.h CNT_WORDS)
    __device__ __forceinline__ uint32_t packed(uint32_t w) const { return cnt[2 * w][tid] | (cnt[2 * w + 1][tid] << 16); }
    // The wave's reserved chunk of the episode list, [lend - lleft, lend) still free (wave-uniform).
    uint32_t lend, lleft;
    // Mark the unused tail of the wave's chunk (K2 skips EP_HOLE slots; no run's slots point there). A chunk
    // holds up to max(lchunk, 64) slots, so the tail can be longer than the wave: every slot of it is marked,
    // 64 per pass (K2 reads every slot below the list count, and the workspace is not cleared between launches).
    __device__ void holes()
    {
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(lane));
        const uint32_t lo = lend - lleft;
        for (uint32_t i = lane; i < lleft; i += 64u)
            if (lo + i < a.lcap) a.list[lo + i].run = EP_HOLE;
    }
    __device__ void slow(bool s, uint32_t block, uint64_t offset, uint32_t w0, uint32_t w1, const Rng &ri, const Rng &rp,
                         uint32_t skip)
    {
        const uint64_t mask = __builtin_amdgcn_ballot_w64(s) & amask;
        // rank of this lane among the slow ones (asm volatile: computed here, not hoisted out of the loop)
        uint32_t below;
        asm volatile("v_mbcnt_lo_u32_b32 %0, %1, 0\n\tv_mbcnt_hi_u32_b32 %0, %2, %0"
                     : "=&v"(below) : "s"((uint32_t)mask), "s"((uint32_t)(mask >> 32)));
        const uint32_t nsel = (uint32_t)__popcll(mask);
        if (nsel > lleft) {  // wave-uniform: a new chunk (the old one's tail becomes holes)
            holes();
            const uint32_t need = nsel > a.lchunk ? nsel : a.lchunk;
            uint32_t base = 0;
            if (s & (below == 0u)) base = atomicAdd(a.list_count, need);
            base = __builtin_amdgcn_readlane(base, (uint32_t)(__ffsll((unsigned long long)mask) - 1));
            lend = base + need;
            lleft = need;
        }
        const uint32_t base = lend - lleft;
        lleft -= nsel;
        if (!s) return;
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(lane));
        if (!((amask >> lane) & 1ull)) return;
        const uint32_t r = r0 + lane;
        const uint32_t idx = base + below;
        if (idx < a.lcap) {
            EpEntry e;
            e.run = r;
            e.block = block;
            e.offset = offset;
            e.w0 = w0;
            e.w1 = w1;
            e.skip = skip;
            e.pad = 0;
            e.ri = ri;
            e.rp = rp;
            a.list[idx] = e;
        }
        uint32_t *nsl = &cnt[K1_NSL][r & 255u];
        const uint32_t c = *nsl;
        if (c < a.cap) a.slots[((size_t)seg * a.cap + c) * a.nr + r] = idx;
        *nsl = c + 1u;
    }
    __device__ __forceinline__ uint32_t run() const { return r0 + (tid & 63u); }
    __device__ void group_start(uint32_t g, uint32_t w0, const Rng &ri, const Rng &rp)
    {
        const uint32_t r = run();
        const size_t gi = (size_t)jb * a.gps + g;
        GroupRec gr;
        gr.ri = ri;
        gr.rp = rp;
        gr.w0 = w0;
        gr.pad = 0;
        a.grec[gi * a.nr + r] = gr;
#pragma unroll
        for (uint32_t w = 0; w < CNT_WORDS; ++w) a.gcum[(gi * CNT_WORDS + w) * a.nr + r] = packed(w);
    }
    __device__ void group(uint32_t g, uint32_t sum, uint64_t end)
    {
        a.gsum[((size_t)jb * a.gps + g) * a.nr + run()] = sum;
        if (g % SGROUP == SGROUP - 1 || g + 1 == a.gps) {
            const uint32_t nsg = (a.gps + SGROUP - 1) / SGROUP;
            a.gend[((size_t)jb * nsg + g / SGROUP) * a.nr + run()] = end;
        }
    }
};

// Resident K1 waves per SIMD the register budget is sized for (VGPRs <= 512 / waves). Measured on MI355X
// (c2, profiles/r03/INDEX.md): 4 waves (113 VGPRs) 4.17 ms, 5 (96) 4.02 ms, 6 (80) 3.75 ms, 7 (72) 7.3 ms and
// 8 (64) 13.7 ms, where the spills reach the draw loop's hot values. Re-measured on round 5's K1 (chunked list
// reservation; profiles/r05/k1waves): 4 waves (104 VGPRs) 3.27 ms, 5 (96, 10 spills) 3.17-3.21 ms, 6 (80, 23
// spills) 3.27 ms serial, same box, alternating. Re-measured on round 7's loop (K1's own interval form, 12 fewer
// VALU instructions per block; profiles/r07/INDEX.md): 4 waves (102 VGPRs, no scratch) 11.40 M run-years/s serial
// and 12.41 M on two streams, 5 (96, 8 spills) 11.38 M / 12.32 M, 6 (80) 11.01 M / 12.48 M: 4 is the only budget
// that is at or near the top of both lines. Round 8's loop spends the slack of that budget on values held across the
// loop (DevCtx::hold, K1Draws::begin): 105 VGPRs, no scratch (profiles/r08/INDEX.md). Round 12's quad (one 64-bit
// shift in the state update, the picker by one multiply, v without conversions) needs 96, still at this budget
// (profiles/r12/INDEX.md).
#ifndef MSIM_K1_WAVES
#define MSIM_K1_WAVES 4
#endif
// UNI: the uniform-delay form (K1Draws<true>; launch_draws picks it from the tables' k1_uni).
template <bool UNI>
#if MSIM_K1_WAVES
__global__ __launch_bounds__(256, MSIM_K1_WAVES) void msim_draws_kernel(const DrawArgs a)
#else
__global__ __launch_bounds__(256) void msim_draws_kernel(const DrawArgs a)
#endif
{
    // one LDS block: the packed log table, invc and row e = 0 of A2 (the general-form redraw), pick table, owner
    // counters (34.5 KB: four workgroups per CU, the register budget's count, fit in 160 KB)
    __shared__ struct {
        K1Pair P[K1_EROWS * LOG_TAB];
        double invc[LOG_TAB], A0[LOG_TAB];
        PickTab pick;
        uint32_t cnt[K1_ROWS][256];
    } sm;
    const uint32_t tid = threadIdx.x;
    const K1Log *kl = a.tab.k1log;
    for (uint32_t i = tid; i < sizeof(PickTab) / 4; i += 256) ((uint32_t *)&sm.pick)[i] = ((const uint32_t *)a.tab.k1pick)[i];
    for (uint32_t i = tid; i < K1_EROWS * LOG_TAB; i += 256) sm.P[i] = kl->P[i];
    if (tid < LOG_TAB) {
        sm.invc[tid] = kl->invc[tid];
        sm.A0[tid] = kl->A2[(K1_EROWS - 1) * LOG_TAB + tid];
    }
    auto s_cnt = sm.cnt;
#pragma unroll
    for (uint32_t w = 0; w < K1_ROWS; ++w) s_cnt[w][tid] = 0;
    __syncthreads();

    const uint32_t r = blockIdx.x * 256 + tid;  // slice-local run (< nr)
    const uint32_t seg = blockIdx.y;
    const uint64_t run = a.run_begin + r;
    Rng ri = rng_seed(seed_interval(a.seed_base, run));
    Rng rp = rng_seed(seed_picker(a.seed_base, run));
    if (seg) jump2(reinterpret_cast<const uint4 *>(a.tab.jump) + (size_t)seg * 128, ri, rp);

    const uint32_t b0 = seg * a.seg;
    DevCtx cx{a, s_cnt, __builtin_amdgcn_ballot_w64(r < a.n), tid, (uint32_t)__builtin_amdgcn_readfirstlane(r & ~63u), seg,
              seg - a.band_lo, 0u, 0u, 0u};
    cx.hold();
    const uint64_t tsum =
        draw_segment_k1_on<UNI, DevCtx>(cx, ri, rp, sm.P, sm.invc, sm.A0, &sm.pick, a.tab.k1_fthr, b0, a.seg, seg >= a.band_lo);
    cx.holes();
    a.segsum[(size_t)seg * a.nr + r] = tsum;
#pragma unroll
    for (uint32_t w = 0; w < CNT_WORDS; ++w) a.segcnt[((size_t)seg * CNT_WORDS + w) * a.nr + r] = cx.packed(w);
    a.nslow[(size_t)seg * a.nr + r] = s_cnt[K1_NSL][tid];
}

// Intervals of given uniforms by K1's chain (its fast form, then the general form, then glibc's sequence); every
// eighth input takes the general tables' chain (interval_ms_fast, what K2, K3 and the engines draw with) instead,
// so a test over crafted inputs covers both.
__global__ void msim_interval_kernel(const LogTab *__restrict__ lt, const K1Log *__restrict__ kl,
                                     const uint64_t *__restrict__ u, int64_t *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok;
    int32_t q;
    if ((i & 7u) == 7u) {
        q = interval_ms_fast(u[i], lt, ok);
    } else {
        q = k1p_interval_fast(u[i], kl->P, ok);
        if (!ok) q = k1_interval_general(u[i], kl, ok);
    }
    out[i] = ok ? q : interval_ms_exact_dev(u[i]);
}

__global__ void msim_pick_kernel(const PickTab *__restrict__ pt, const uint64_t *__restrict__ u,
                                 int32_t *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = info_finder(pick_info(u[i], pt));
    out[i] = k == 15u ? -1 : (int32_t)k;
}

// K1's quad from given start states (msim_device_k1_quads, a test entry): the draw form's quad_fast, then its
// quad_exact when flagged, exactly as the lane body calls them. st[2 i], st[2 i + 1]: the interval and the picker
// stream; out[8 i ..]: the four intervals, then the four finders (15: PickFinder fell through).
template <bool UNI>
__global__ void msim_k1_quads_kernel(const PickTab *__restrict__ kp, const K1Log *__restrict__ kl, uint32_t fthr,
                                     const Rng *__restrict__ st, uint32_t *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    K1Draws<UNI> d{kl->P, kl->invc, kl->A2 + (K1_EROWS - 1) * LOG_TAB, kp, fthr, MSIM_K1_CONSTS};
    d.begin();
    Rng ri = st[2 * i], rp = st[2 * i + 1];
    const Rng ri0 = ri, rp0 = rp;
    uint32_t I[K1_QB], info[K1_QB];
    if (d.quad_fast(ri, rp, I, info)) d.quad_exact(ri0, rp0, I, info);
#pragma unroll
    for (int q = 0; q < K1_QB; ++q) {
        out[8 * i + q] = I[q];
        out[8 * i + K1_QB + q] = info_finder(info[q]);
    }
}

hipError_t launch_k1_quads(const PipeTables &t, const Rng *st, uint32_t *out, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (t.k1_uni) hipLaunchKernelGGL(msim_k1_quads_kernel<true>, grid, dim3(256), 0, s, t.k1pick, t.k1log, t.k1_fthr, st, out, n);
    else hipLaunchKernelGGL(msim_k1_quads_kernel<false>, grid, dim3(256), 0, s, t.k1pick, t.k1log, t.k1_fthr, st, out, n);
    return hipGetLastError();
}

hipError_t launch_intervals(const LogTab *lt, const K1Log *kl, const uint64_t *u, int64_t *out, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(msim_interval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lt, kl, u, out, n);
    return hipGetLastError();
}

hipError_t launch_picks(const PickTab *pt, const uint64_t *u, int32_t *out, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(msim_pick_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pt, u, out, n);
    return hipGetLastError();
}

hipError_t draws_blocks_per_cu(int *blocks)
{
    int u = 0, g = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&u, msim_draws_kernel<true>, 256, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&g, msim_draws_kernel<false>, 256, 0);
    *blocks = u < g ? u : g;
    return e;
}

hipError_t launch_draws(const DrawArgs &a, hipStream_t s)
{
    if (a.tab.k1_uni) hipLaunchKernelGGL(msim_draws_kernel<true>, dim3(a.nr / 256, a.nseg), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(msim_draws_kernel<false>, dim3(a.nr / 256, a.nseg), dim3(256), 0, s, a);
    return hipGetLastError();
}

// K1's tables are built here, in K1's translation unit, so that a variant build of this file alone (Makefile
// `variant`) gets tables that match its switches (MSIM_FD_A2, MSIM_FD_DEG4, MSIM_K1_UNI).
void k1_tables_build(const uint64_t *perc, const int64_t *prop, const uint8_t *selfish, int m, PickTab *pick, K1Log *log)
{
    uint32_t fthr = 0;
    build_k1_pick(perc, prop, selfish, m, k1_uniform_fthr(prop, selfish, m, &fthr), pick);
    build_k1_log(log);
}
bool k1_tables_uniform(const int64_t *prop, const uint8_t *selfish, int m, uint32_t *fthr)
{
    return k1_uniform_fthr(prop, selfish, m, fthr);
}
void k1_log_build(K1Log *log) { build_k1_log(log); }

}  // namespace msim

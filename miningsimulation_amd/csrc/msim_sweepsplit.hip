// msim_sweepsplit.hip — S1 of the shared-draw sweep (msim_sweepsplit.h): one envelope list -> every point's listing.
//
// One lane = (run, segment), a wave = 64 consecutive runs of one segment (as K1), so the envelope's counts and slot
// rows are read coalesced; the list entries are gathers of 8 bytes. Roofline: memory latency (two dependent reads
// per listed block, twice); the kernel moves ~(4 + 4 + 8) bytes per listed block and pass against K1's ~100 VALU
// instructions per DRAWN block, and only rho of the blocks are listed.
#include <hip/hip_runtime.h>

#include "msim_kernels.h"
#include "msim_sweepsplit.h"

namespace msim {

// Wave-aggregated reservation: an inclusive scan of the lanes' wants, one atomic per wave and point.
struct DevReserve {
    uint32_t lane;
    __device__ uint32_t reserve(uint32_t *count, uint32_t n) const
    {
        uint32_t x = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= (uint32_t)o) x += y;
        }
        const uint32_t total = __shfl(x, 63, 64);
        uint32_t base = 0;
        if (lane == 63u && total) base = atomicAdd(count, total);
        base = __shfl(base, 63, 64);
        return base + x - n;
    }
};

__global__ __launch_bounds__(256) void msim_sweep_split_kernel(const SplitArgs a)
{
    __shared__ uint32_t s_fthr[SPLIT_MAX_POINTS * 16];
    if (threadIdx.x < a.np * 16u) s_fthr[threadIdx.x] = a.fthr[threadIdx.x];
    __syncthreads();
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;  // < nr: the grid covers the slice exactly (nr % 256 == 0)
    DevReserve res{threadIdx.x & 63u};
    split_segment(a, s_fthr, r, blockIdx.y, res);
}

hipError_t launch_sweep_split(const SplitArgs &a, hipStream_t s)
{
    if (a.np == 0 || a.np > SPLIT_MAX_POINTS || a.nr % 256u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(msim_sweep_split_kernel, dim3(a.nr / 256, a.nseg), dim3(256), 0, s, a);
    return hipGetLastError();
}

// d_status of a shared-draw sweep: the points' status words added up.
__global__ void msim_sweep_status_kernel(const uint32_t *__restrict__ st, uint32_t np, uint32_t *__restrict__ status)
{
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (uint32_t p = 0; p < np; ++p) s += st[2 * p + threadIdx.x];
        status[threadIdx.x] = s;
    }
}

hipError_t launch_sweep_status(const uint32_t *st, uint32_t np, uint32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(msim_sweep_status_kernel, dim3(1), dim3(64), 0, s, st, np, status);
    return hipGetLastError();
}

}  // namespace msim

// msim_host.h — what the host side of the C ABI shares between its translation units (msim_api.hip,
// msim_sample.hip, msim_moments.hip, msim_multi.hip): the launch limit, 256-byte alignment, and owners for the
// device buffers and the stream of a blocking run.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/msim.h"

namespace msim {

constexpr uint64_t MAX_LAUNCH_RUNS = 1ull << 26;  // msim_launch / msim_sweep_launch limit (runs x points of one call)

constexpr size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// Whether a workspace of `bytes` fits the current device's free memory (hipMemGetInfo).
inline bool workspace_fits(size_t bytes)
{
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return true;  // let the allocation report it
    return bytes <= fr;
}

// A move-only HIP handle released with its owner.
template <class T, hipError_t (*Release)(T)>
class DevOwner {
public:
    DevOwner() = default;
    DevOwner(DevOwner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevOwner &operator=(DevOwner &&o) noexcept  // what this held goes with `o`
    {
        std::swap(h_, o.h_);
        return *this;
    }
    ~DevOwner()
    {
        if (h_) (void)Release(h_);
    }
    T get() const { return h_; }

protected:
    T h_ = nullptr;
};
// A device allocation, freed on the device current at that time.
struct DevBuf : DevOwner<void *, hipFree> {
    bool alloc(size_t bytes) { return hipMalloc(&h_, bytes) == hipSuccess; }
};
// A stream. Declare it after the buffers it works on: it is then destroyed before they are freed.
struct DevStream : DevOwner<hipStream_t, hipStreamDestroy> {
    bool create() { return hipStreamCreate(&h_) == hipSuccess; }
};

// A config's miner weights and their total, for the samplers (msim_sample.hip); defined beside the struct.
void config_weights(const msim_config *cfg, std::vector<uint64_t> *w, uint32_t *total_weight);

}  // namespace msim

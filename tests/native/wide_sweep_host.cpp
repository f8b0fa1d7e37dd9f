// wide_sweep_host.cpp — TEST INFRASTRUCTURE: the shared-draw form of large-network sweeps on the host
// (wide_sweep_body.h) as a shared library for tests/test_wide_sweep_host.py and tests/test_gpu_wide_sweep.py (which
// takes the per-run candidate counts from it). Never part of the product path (libmsim.so is GPU-only).
#include "wide_sweep_body.h"

extern "C" int wide_sweep_run(const uint64_t *w, const int64_t *props, uint32_t m, uint32_t np, uint64_t W, int64_t D,
                              uint32_t seed_base, uint64_t run_begin, uint32_t n, uint32_t rcap_env,
                              const uint32_t *rcap_pt, uint32_t *found, uint32_t *stale, uint8_t *ok, uint32_t *counts)
{
    return wsweep::run_group(w, props, m, np, W, D, seed_base, run_begin, n, rcap_env, rcap_pt, found, stale, ok, counts);
}

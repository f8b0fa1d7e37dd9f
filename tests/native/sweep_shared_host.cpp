// sweep_shared_host.cpp — TEST INFRASTRUCTURE: the shared-draw sweep on the host (sweep_shared_body.h) behind a C
// entry point for tests/test_sweep_shared_host.py. Never part of the product path (libmsim.so is GPU-only).
#include "sweep_shared_body.h"

extern "C" int sweep_shared_run(const uint64_t *perc, const int64_t *props, int m, uint32_t np, int64_t duration_ms,
                                uint32_t seed_base, uint64_t run_begin, uint32_t n, uint32_t wave_slots, uint32_t env_cap,
                                uint32_t env_lcap, const uint32_t *pt_cap, const uint32_t *pt_lcap, uint32_t max_group,
                                uint32_t *found, uint32_t *stale, uint8_t *ok, uint8_t *listing_ok, uint32_t *n_env_entries)
{
    return sshost::shared_run_m(m, perc, props, np, duration_ms, seed_base, run_begin, n, wave_slots, env_cap, env_lcap,
                                pt_cap, pt_lcap, max_group, found, stale, ok, listing_ok, n_env_entries);
}

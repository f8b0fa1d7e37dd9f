// pipeline_host.cpp — TEST INFRASTRUCTURE: the C entry of the host (CPU) execution of the event-skipping pipeline
// (pipeline_body.h), loaded by tests/test_pipeline_host.py and tests/test_gpu_pipe_overflow.py.
#include "pipeline_body.h"

// cap_override, lcap_override: 0 for the layout's capacities. nseg, seg: 0, 0 for the geometry the layout picks for
// wave_slots wave slots, or the workers per run and their length (-102 when the layout gives those workers another
// length). k2_kind: -1 for the network's own, or 0 / 1 / 2. listed, onepath: per run, or null (pipeline_body.h).
extern "C" int pipeline_run_ex(const uint64_t *perc, const int64_t *prop, const uint8_t *selfish, int m,
                               int64_t duration_ms, uint32_t seed_base, uint64_t run_begin, uint32_t n,
                               uint32_t cap_override, uint32_t wave_slots, uint32_t nseg, uint32_t seg, uint32_t lcap_override,
                               int32_t k2_kind, uint32_t *found, uint32_t *stale, uint8_t *ok, uint32_t *n_episodes,
                               uint32_t *listed, uint8_t *onepath)
{
    pipehost::Overrides ov;
    ov.cap = cap_override;
    ov.lcap = lcap_override;
    ov.nseg = nseg;
    ov.seg = seg;
    ov.k2_kind = k2_kind;
    return pipehost::run_pipeline_m(perc, prop, selfish, m, duration_ms, seed_base, run_begin, n, wave_slots, ov, found,
                                    stale, ok, n_episodes, listed, onepath);
}

// The same without the later overrides: the layout's geometry, list capacity and K2 kind.
extern "C" int pipeline_run(const uint64_t *perc, const int64_t *prop, const uint8_t *selfish, int m,
                            int64_t duration_ms, uint32_t seed_base, uint64_t run_begin, uint32_t n,
                            uint32_t cap_override, uint32_t wave_slots, uint32_t *found, uint32_t *stale, uint8_t *ok,
                            uint32_t *n_episodes)
{
    return pipeline_run_ex(perc, prop, selfish, m, duration_ms, seed_base, run_begin, n, cap_override, wave_slots, 0, 0, 0, -1,
                           found, stale, ok, n_episodes, nullptr, nullptr);
}

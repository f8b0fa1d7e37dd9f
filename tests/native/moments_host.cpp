// moments_host.cpp — TEST INFRASTRUCTURE: msim_moments.h's accumulation over a record array on the host (CPU), the
// same term, square and bin lines the gfx950 reduction kernel (msim_moments.hip) runs, checked against
// tests/moments_reference.py on machines without a GPU (tests/test_moments_host.py). Never part of the product
// path (libmsim.so is GPU-only).
#include "../../miningsimulation_amd/csrc/msim_moments.h"

// rec [n_runs][m]; best_height [n_runs]; out: m msim_moments; hist with spec: [m][2][bins + 2], or both NULL
extern "C" int moments_host_accumulate(const msim_run_record *rec, const uint32_t *best_height, uint64_t n_runs,
                                       uint32_t m, const msim_hist_spec *spec, msim_moments *out, uint64_t *hist)
{
    if (!rec || !best_height || !out || (spec != nullptr) != (hist != nullptr)) return -1;
    if (spec && (spec->bins == 0 || spec->bins > msim::MOM_MAX_BINS || spec->share_shift > 63 || spec->rate_shift > 63))
        return -1;
    msim::mom_accumulate_host(rec, best_height, n_runs, m, spec, out, hist);
    return 0;
}

extern "C" void moments_host_to_errors(const msim_moments *mo, uint32_t m, uint64_t n_runs, msim_errors *out)
{
    msim::mom_to_errors(mo, m, n_runs, out);
}

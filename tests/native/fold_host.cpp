// fold_host.cpp — TEST INFRASTRUCTURE: msim_fold.h's lane body over a record array on the host (CPU), the same
// lookup, pending-sum and walk lines the gfx950 fold kernel (msim_fold.hip) runs, checked against
// tests/classes_reference.py on machines without a GPU (tests/test_classes_host.py). Never part of the product path
// (libmsim.so is GPU-only).
#include "../../miningsimulation_amd/csrc/msim_fold.h"

// rec [n_runs][m] -> out [n_runs][n_classes]; tc / gw: the tile shape (classes per class tile, runs per wave
// segment), or 0 / 0 for the launch's own choice (fold_plan)
extern "C" int fold_host_run(const msim_run_record *rec, uint64_t n_runs, uint32_t m, const uint32_t *class_of,
                             uint32_t n_classes, msim_run_record *out, uint32_t tc, uint32_t gw)
{
    if (!rec || !class_of || !out || m == 0 || n_runs == 0 || n_classes == 0 || n_classes > m) return -1;
    if (tc == 0 || gw == 0) msim::fold_plan(m, n_classes, n_runs, &tc, &gw);
    if (tc > n_classes || (uint64_t)gw * m > 0xFFFFFFFFull) return -1;
    msim::fold_host(rec, n_runs, m, class_of, n_classes, out, tc, gw);
    return 0;
}

extern "C" void fold_host_plan(uint32_t m, uint32_t n_classes, uint64_t n_runs, uint32_t *tc, uint32_t *gw)
{
    msim::fold_plan(m, n_classes, n_runs, tc, gw);
}

extern "C" int fold_host_map_ok(uint32_t m, const uint32_t *class_of, uint32_t n_classes)
{
    return msim::fold_map_ok(m, class_of, n_classes) ? 1 : 0;
}

// cross_host.cpp — TEST INFRASTRUCTURE: msim_cross.h's accumulation over a record array on the host (CPU), the same
// product, per-run add and pair guard the gfx950 reduction kernel (msim_cross.hip) runs, checked against
// tests/cross_reference.py on machines without a GPU (tests/test_cross_host.py). Never part of the product path
// (libmsim.so is GPU-only).
#include "../../miningsimulation_amd/csrc/msim_cross.h"

// rec [n_points][runs][m]; best_height [n_points][runs]; out: n_pairs msim_cross
extern "C" int cross_host_accumulate(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                     uint64_t runs, uint32_t m, const msim_pair *pairs, uint32_t n_pairs,
                                     msim_cross *out)
{
    if (!rec || !best_height || !pairs || !out) return -1;
    msim::cross_accumulate_host(rec, best_height, n_points, runs, m, pairs, n_pairs, out);
    return 0;
}

// p[4]: the pieces of a * b; q[4]: mom_square_pieces(a)
extern "C" void cross_host_pieces(uint64_t a, uint64_t b, uint64_t *p, uint64_t *q)
{
    msim::cross_mul_pieces(a, b, p);
    msim::mom_square_pieces(a, q);
}

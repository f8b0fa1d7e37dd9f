// tail_host.cpp — TEST INFRASTRUCTURE: msim_tail.h's sequential accumulation over a record array and its host
// arithmetic (sides and means) on the CPU, the same item guard, key and per-run add the gfx950 kernel
// (msim_tail.hip) runs, checked against tests/tail_reference.py on machines without a GPU
// (tests/test_tail_host.py). Never part of the product path (libmsim.so is GPU-only).
#include "../../miningsimulation_amd/csrc/msim_tail.h"

// rec [n_points][runs][m]; best_height [n_points][runs]; items [n_items]; out: n_items msim_tail (overwritten).
extern "C" int tail_host_accumulate(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                    uint64_t runs, uint32_t m, const msim_tail_item *items, uint32_t n_items,
                                    msim_tail *out)
{
    if (!rec || !best_height || !items || !out || m == 0 || n_points == 0 || n_items == 0) return -1;
    msim::tail_accumulate_host(rec, best_height, n_points, runs, m, items, n_items, out);
    return 0;
}

// out += the tails of one more record buffer: what the drivers do with the chunks' words.
extern "C" int tail_host_accumulate_add(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                        uint64_t runs, uint32_t m, const msim_tail_item *items, uint32_t n_items,
                                        msim_tail *out)
{
    if (!rec || !best_height || !items || !out || m == 0 || n_points == 0 || n_items == 0) return -1;
    msim_tail *part = new msim_tail[n_items];
    msim::tail_accumulate_host(rec, best_height, n_points, runs, m, items, n_items, part);
    for (size_t i = 0; i < (size_t)n_items * msim::TAIL_WORDS; ++i) ((uint64_t *)out)[i] += ((const uint64_t *)part)[i];
    delete[] part;
    return 0;
}

extern "C" int tail_host_items_check(uint32_t m, uint32_t n_points, const msim_tail_item *items, uint32_t n_items)
{
    for (uint32_t i = 0; i < n_items; ++i)
        if (!msim::tail_item_ok(items[i], n_points, m)) return MSIM_E_INVALID;
    return MSIM_OK;
}

extern "C" int tail_host_side(const msim_tail *t, const msim_moments *total, uint64_t n_runs, int side,
                              msim_moments *out, uint64_t *out_n)
{
    return msim::tail_side(t, total, n_runs, side, out, out_n);
}

extern "C" int tail_host_means(const msim_tail *t, const msim_moments *total, uint64_t n_runs, uint64_t k, int upper,
                               double *out)
{
    return msim::tail_means(t, total, n_runs, k, upper, out);
}

extern "C" void tail_host_to_errors(const msim_moments *mo, uint64_t n_runs, msim_errors *out)
{
    msim::mom_to_errors(mo, 1, n_runs, out);
}

// num / den of two 128-bit numbers given as {lo, hi}: the division behind msim_tail_means.
extern "C" double tail_host_div(uint64_t num_lo, uint64_t num_hi, uint64_t den_lo, uint64_t den_hi)
{
    const uint64_t n[2] = {num_lo & 0xFFFFFFFFull, num_lo >> 32}, nh[2] = {num_hi & 0xFFFFFFFFull, num_hi >> 32};
    const uint64_t d[2] = {den_lo & 0xFFFFFFFFull, den_lo >> 32}, dh[2] = {den_hi & 0xFFFFFFFFull, den_hi >> 32};
    const uint64_t nn[4] = {n[0], n[1], nh[0], nh[1]}, dd[4] = {d[0], d[1], dh[0], dh[1]};
    return msim::mw_div_to_double(msim::mw_join<msim::TailWide::W>(nn, 4), msim::mw_join<msim::TailWide::W>(dd, 4));
}

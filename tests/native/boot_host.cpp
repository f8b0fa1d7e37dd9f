// boot_host.cpp — TEST INFRASTRUCTURE: msim_boot.h's weight function, sequential selection and the host mirrors of
// the begin, count, step and below launches on the CPU, the same lines the gfx950 kernels (msim_boot.hip) run,
// checked against tests/boot_reference.py on machines without a GPU (tests/test_boot_host.py). Never part of the
// product path (libmsim.so is GPU-only).
#include "../../miningsimulation_amd/csrc/msim_boot.h"

extern "C" uint32_t boot_host_weight(uint64_t seed, uint32_t b, uint64_t run) { return msim::boot_weight(seed, b, run); }

// sum of the weights of replicate b over the runs 0..n-1
extern "C" uint64_t boot_host_weight_sum(uint64_t seed, uint32_t b, uint64_t n)
{
    uint64_t W = 0;
    for (uint64_t r = 0; r < n; ++r) W += msim::boot_weight(seed, b, r);
    return W;
}

extern "C" uint32_t boot_host_threshold_weight(uint32_t u) { return msim::boot_weight_of(u); }

extern "C" uint64_t boot_host_rank(uint64_t W, double q) { return msim::boot_rank(W, q); }

extern "C" uint64_t boot_host_workspace_words(uint32_t n_items, uint32_t B)
{
    return msim::boot_shape_ok(n_items, B) ? msim::boot_layout(n_items, B).words : 0;
}

// rec [n_points][runs][m]; best_height [n_points][runs]; out_W [B]; out_rows [n_items][B][5]
extern "C" long long boot_host_select(const msim_run_record *rec, const uint32_t *best_height, uint32_t n_points,
                                      uint64_t run_begin, uint64_t runs, uint32_t m, const msim_boot_item *items,
                                      uint32_t n_items, const double *qs, uint32_t n_q, uint32_t B, uint64_t seed,
                                      uint64_t *out_W, uint64_t *out_rows)
{
    if (!rec || !best_height || !items || !qs || !out_W || !out_rows || m == 0 || n_points == 0) return -1;
    return msim::boot_select_host(rec, best_height, n_points, run_begin, runs, m, items, n_items, qs, n_q, B, seed, out_W,
                                  out_rows);
}

// Raw keys [runs] of one column (m = 1, one point): values no record gives.
struct RawKeys {
    const uint64_t *keys;
    uint64_t operator()(const msim_boot_item &, uint64_t r) const { return keys[r]; }
};

extern "C" long long boot_host_select_keys(const uint64_t *keys, uint64_t runs, uint32_t quantity, const double *qs,
                                           uint32_t n_q, uint32_t B, uint64_t seed, uint64_t *out_W, uint64_t *out_rows)
{
    if (!keys || !qs || !out_W || !out_rows || n_q == 0 || n_q > MSIM_MAX_RANKS) return -1;
    std::vector<msim_boot_item> items(n_q);
    for (uint32_t j = 0; j < n_q; ++j) items[j] = msim_boot_item{0, 0, quantity, j};
    return msim::boot_select_keys_host(RawKeys{keys}, 1, 0, runs, 1, items.data(), n_q, qs, n_q, B, seed, out_W, out_rows);
}

// The launches' mirrors over TWO buffers, runs [run_begin, run_begin + runs_a) and the runs_b after them, on the
// caller's workspace (which may hold anything): W from both, begin, eight passes of two counts and a step, two belows.
extern "C" long long boot_host_select_split(const msim_run_record *rec_a, const uint32_t *bh_a, uint64_t runs_a,
                                            const msim_run_record *rec_b, const uint32_t *bh_b, uint64_t runs_b,
                                            uint32_t n_points, uint64_t run_begin, uint32_t m,
                                            const msim_boot_item *items, uint32_t n_items, const double *qs, uint32_t n_q,
                                            uint32_t B, uint64_t seed, uint64_t *ws, uint64_t *out_W, uint64_t *out_rows)
{
    using namespace msim;
    if (!boot_shape_ok(n_items, B) || n_q == 0 || n_q > MSIM_MAX_RANKS) return -1;
    for (uint32_t i = 0; i < n_items; ++i)
        if (!boot_item_ok(items[i], m, n_points, n_q)) return -1;
    for (uint32_t b = 0; b < B; ++b) out_W[b] = 0;
    boot_weights_host(seed, run_begin, runs_a, B, out_W);
    boot_weights_host(seed, run_begin + runs_a, runs_b, B, out_W);
    std::vector<uint64_t> ranks((size_t)n_q * B);
    for (uint32_t j = 0; j < n_q; ++j)
        for (uint32_t b = 0; b < B; ++b) ranks[(size_t)j * B + b] = boot_rank(out_W[b], qs[j]);
    const BootRecordKeys ka = {rec_a, bh_a, runs_a, m}, kb = {rec_b, bh_b, runs_b, m};
    boot_begin_host(m, n_points, items, n_items, B, ranks.data(), ws);
    uint64_t bad = 0;
    for (uint32_t pass = 0; pass < MSIM_RANK_PASSES; ++pass) {
        boot_count_host(m, n_points, seed, run_begin, runs_a, ka, n_items, B, pass, ws);
        boot_count_host(m, n_points, seed, run_begin + runs_a, runs_b, kb, n_items, B, pass, ws);
        bad += boot_step_host(n_items, B, pass, ws, out_rows);
    }
    boot_below_host(m, n_points, seed, run_begin, runs_a, ka, n_items, B, ws, out_rows);
    boot_below_host(m, n_points, seed, run_begin + runs_a, runs_b, kb, n_items, B, ws, out_rows);
    return (long long)bad;
}

// A count and a step on a workspace no begin prepared: returns 1 when they left every word as it was.
extern "C" int boot_host_unprepared_is_noop(const msim_run_record *rec, const uint32_t *bh, uint64_t runs, uint32_t m,
                                            uint32_t n_items, uint32_t B, uint64_t fill)
{
    using namespace msim;
    std::vector<uint64_t> ws(boot_layout(n_items, B).words, fill), rows((size_t)n_items * B * BOOT_ROW_WORDS, fill);
    boot_count_host(m, 1, 1, 0, runs, BootRecordKeys{rec, bh, runs, m}, n_items, B, 0, ws.data());
    boot_step_host(n_items, B, MSIM_RANK_PASSES - 1, ws.data(), rows.data());
    boot_below_host(m, 1, 1, 0, runs, BootRecordKeys{rec, bh, runs, m}, n_items, B, ws.data(), rows.data());
    for (uint64_t w : ws)
        if (w != fill) return 0;
    for (uint64_t w : rows)
        if (w != fill) return 0;
    return 1;
}

// The launches' mirrors one by one, for stand-ins of the launches on CPU ranks (tests/test_boot_distributed.py).
extern "C" int boot_host_weights(uint64_t seed, uint64_t run_begin, uint64_t runs, uint32_t B, uint64_t *W)
{
    msim::boot_weights_host(seed, run_begin, runs, B, W);
    return 0;
}

extern "C" int boot_host_begin(uint32_t m, uint32_t n_points, const msim_boot_item *items, uint32_t n_items, uint32_t B,
                               const uint64_t *ranks, uint32_t n_q, uint64_t *ws)
{
    if (!msim::boot_shape_ok(n_items, B)) return -1;
    for (uint32_t i = 0; i < n_items; ++i)
        if (!msim::boot_item_ok(items[i], m, n_points, n_q)) return -1;
    msim::boot_begin_host(m, n_points, items, n_items, B, ranks, ws);
    return 0;
}

extern "C" int boot_host_count(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs,
                               const msim_run_record *rec, const uint32_t *bh, uint32_t n_items, uint32_t B,
                               uint32_t pass, uint64_t *ws)
{
    msim::boot_count_host(m, n_points, seed, run_begin, runs, msim::BootRecordKeys{rec, bh, runs, m}, n_items, B, pass, ws);
    return 0;
}

extern "C" int boot_host_step(uint32_t n_items, uint32_t B, uint32_t pass, uint64_t *ws, uint64_t *rows, uint32_t *status)
{
    *status += (uint32_t)msim::boot_step_host(n_items, B, pass, ws, pass + 1 == MSIM_RANK_PASSES ? rows : nullptr);
    return 0;
}

extern "C" int boot_host_below(uint32_t m, uint32_t n_points, uint64_t seed, uint64_t run_begin, uint64_t runs,
                               const msim_run_record *rec, const uint32_t *bh, uint32_t n_items, uint32_t B,
                               const uint64_t *ws, uint64_t *rows)
{
    msim::boot_below_host(m, n_points, seed, run_begin, runs, msim::BootRecordKeys{rec, bh, runs, m}, n_items, B, ws, rows);
    return 0;
}

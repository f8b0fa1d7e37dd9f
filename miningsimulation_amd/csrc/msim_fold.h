// msim_fold.h — miner classes: per run, the records of the miners of each class added into one record per class
// (include/msim.h: msim_fold_launch, msim_classes_check). Pure integer arithmetic, sums modulo 2^32.
//
// Everything a lane does is here and __host__ __device__: the class lookup with its NONE skip (fold_column), the
// lane's pending sum over consecutive records of one cell (fold_lane_add) and the lane's walk over a segment of
// records (fold_walk). The gfx950 kernel (msim_fold.hip) runs them with LDS atomics as the sink; fold_host below
// runs the same lines for every lane of every wave in turn with a plain array as the sink (tests/native/fold_host.cpp,
// tests/native/fold_check.cpp), at any tile shape the launch can choose (fold_plan).
//
// Shape of the work. A workgroup of FOLD_WAVES waves owns a tile of FOLD_WAVES * gw consecutive runs, each wave a
// segment of gw of them: gw * m consecutive records, walked FOLD_LANES at a time, so consecutive lanes read
// consecutive 8-byte records. For m past FOLD_SEGMENT_RECORDS, gw is 1: a wave walks one run's records. The
// sums of the tile live in `cells` [run of the tile][tc] (found and stale apart), tc = the classes of one class
// tile: all of them while FOLD_WAVES * n_classes cells fit FOLD_POOL, else the grid's y covers the classes in
// tiles of FOLD_POOL / FOLD_WAVES and every tile reads the records again.
//
// Large classes. A lane keeps the sum of its records in registers for as long as they fall on one cell, and adds
// to the cell when the cell changes and at the end of its segment. Lane l of a wave walking one run sees miners
// l, l + 64, ...: in a network of a few large classes (configs[4]: 1, 1, 1 024) that is one cell for the whole
// run, so the run costs one add per lane, not one per record; the kernel then joins those 64 adds into one
// cross-lane sum where the whole wave ends on one cell. With one miner per class every record changes the cell,
// but then no two lanes of a wave share a cell and the adds do not collide.
#ifndef MSIM_FOLD_H
#define MSIM_FOLD_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/msim.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define MSIM_FHD __host__ __device__ inline
#else
#define MSIM_FHD inline
#endif

namespace msim {

constexpr uint32_t FOLD_LANES = 64;
constexpr uint32_t FOLD_WAVES = 4;
constexpr uint32_t FOLD_THREADS = FOLD_LANES * FOLD_WAVES;
constexpr uint32_t FOLD_UNROLL = 4;                // records a lane has in flight
constexpr uint32_t FOLD_POOL = 4608;               // cells of a workgroup: 36 KB of LDS, four workgroups per CU
constexpr uint32_t FOLD_SEGMENT_RECORDS = 2048;    // a wave's segment holds at most this many records, or one run
constexpr uint32_t FOLD_SKIP = 0xFFFFFFFFu;        // the cell of a record that is not added
constexpr uint32_t FOLD_MAX_TILES = 65535;         // grid y (class tiles) and z (points)

struct alignas(8) FoldRec {  // msim_run_record, read and written as one 8-byte word
    uint32_t found, stale;
};
static_assert(sizeof(FoldRec) == sizeof(msim_run_record), "FoldRec is msim_run_record");

// The column of class `cls` in the class tile [c0, c0 + tc), or FOLD_SKIP: MSIM_CLASS_NONE, an entry outside the
// map's classes (read as NONE) and a class of another tile are all skipped.
MSIM_FHD uint32_t fold_column(uint32_t cls, uint32_t n_classes, uint32_t c0, uint32_t tc)
{
    if (cls >= n_classes) return FOLD_SKIP;
    const uint32_t col = cls - c0;  // wraps for a class below the tile
    return col < tc ? col : FOLD_SKIP;
}

// A lane's pending sum: consecutive records of one cell.
struct FoldLane {
    uint32_t cell, found, stale;
};

// One record into the lane's pending sum; sink(cell, found, stale) receives the sum when the cell changes.
template <class Sink>
MSIM_FHD void fold_lane_add(FoldLane &st, uint32_t cell, uint32_t found, uint32_t stale, Sink &sink)
{
    if (cell == FOLD_SKIP) return;
    if (cell != st.cell) {
        if (st.cell != FOLD_SKIP) sink(st.cell, st.found, st.stale);
        st.cell = cell;
        st.found = 0;
        st.stale = 0;
    }
    st.found += found;  // modulo 2^32 (include/msim.h)
    st.stale += stale;
}

// Lane `lane` of a wave over a segment of n = (runs of the segment) * m records at rec: records lane, lane + 64,
// ... The cell of record i is (i / m) * row_cells + the column of miner i % m's class; the division is done once,
// then run and miner advance by 64 / m and 64 % m. The sum still pending at the end stays in st (the caller adds
// it). Every lane of a wave makes the same number of trips.
template <class Sink>
MSIM_FHD void fold_walk(uint32_t lane, const FoldRec *rec, uint32_t n, uint32_t m, const uint32_t *class_of,
                        uint32_t n_classes, uint32_t c0, uint32_t tc, uint32_t row_cells, FoldLane &st, Sink &sink)
{
    uint32_t row = lane / m, k = lane % m;
    const uint32_t dq = FOLD_LANES / m, dk = FOLD_LANES % m;
    for (uint64_t i0 = 0; i0 < n; i0 += (uint64_t)FOLD_LANES * FOLD_UNROLL) {
        FoldRec x[FOLD_UNROLL];
        uint32_t cell[FOLD_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < FOLD_UNROLL; ++u) {
            const uint64_t i = i0 + u * FOLD_LANES + lane;
            cell[u] = FOLD_SKIP;
            x[u].found = 0;
            x[u].stale = 0;
            if (i < n) {
                x[u] = rec[i];
                const uint32_t col = fold_column(class_of[k], n_classes, c0, tc);
                if (col != FOLD_SKIP) cell[u] = row * row_cells + col;
            }
            row += dq;
            if (k >= m - dk) {  // k + dk >= m, without leaving 32 bits
                k -= m - dk;
                ++row;
            } else {
                k += dk;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < FOLD_UNROLL; ++u) fold_lane_add(st, cell[u], x[u].found, x[u].stale, sink);
    }
}

// The launch's tile shape: tc classes per class tile and gw runs per wave segment.
inline void fold_plan(uint32_t m, uint32_t n_classes, uint64_t runs_per_point, uint32_t *tc, uint32_t *gw)
{
    const uint32_t cap = FOLD_POOL / FOLD_WAVES;
    *tc = n_classes < cap ? n_classes : cap;
    uint64_t g = cap / *tc;                                            // what the cells hold
    if (g > FOLD_SEGMENT_RECORDS / m) g = FOLD_SEGMENT_RECORDS / m;    // a segment of a few dozen trips
    const uint64_t spread = (runs_per_point + 2047) / 2048;            // at least 512 tiles where the runs allow
    if (g > spread) g = spread;
    *gw = g ? (uint32_t)g : 1;
}

inline bool fold_map_ok(uint32_t m, const uint32_t *class_of, uint32_t n_classes)
{
    if (!class_of || m == 0 || n_classes == 0 || n_classes > m) return false;
    for (uint32_t k = 0; k < m; ++k)
        if (class_of[k] >= n_classes && class_of[k] != MSIM_CLASS_NONE) return false;
    return true;
}

// ---------------------------------------------------------------- host: the kernel's work, sequentially
// rec [n_runs][m] -> out [n_runs][n_classes] (overwritten), in tiles of tc classes and segments of gw runs as the
// kernel walks them: every lane of a segment in turn through fold_walk, the cells a plain array.
struct FoldHostSink {
    uint32_t *found, *stale;
    void operator()(uint32_t cell, uint32_t f, uint32_t s)
    {
        found[cell] += f;
        stale[cell] += s;
    }
};

inline void fold_host(const msim_run_record *rec, uint64_t n_runs, uint32_t m, const uint32_t *class_of,
                      uint32_t n_classes, msim_run_record *out, uint32_t tc, uint32_t gw)
{
    std::vector<uint32_t> cf((size_t)gw * tc), cs((size_t)gw * tc);
    FoldHostSink sink = {cf.data(), cs.data()};
    for (uint32_t c0 = 0; c0 < n_classes; c0 += tc) {
        const uint32_t tcc = n_classes - c0 < tc ? n_classes - c0 : tc;
        for (uint64_t r0 = 0; r0 < n_runs; r0 += gw) {
            const uint32_t rows = n_runs - r0 < gw ? (uint32_t)(n_runs - r0) : gw;
            memset(cf.data(), 0, sizeof(uint32_t) * cf.size());
            memset(cs.data(), 0, sizeof(uint32_t) * cs.size());
            for (uint32_t lane = 0; lane < FOLD_LANES; ++lane) {
                FoldLane st = {FOLD_SKIP, 0, 0};
                fold_walk(lane, (const FoldRec *)(rec + r0 * m), rows * m, m, class_of, n_classes, c0, tcc, tc, st, sink);
                if (st.cell != FOLD_SKIP) sink(st.cell, st.found, st.stale);
            }
            for (uint32_t row = 0; row < rows; ++row)
                for (uint32_t col = 0; col < tcc; ++col)
                    out[(r0 + row) * n_classes + c0 + col] = {cf[(size_t)row * tc + col], cs[(size_t)row * tc + col]};
        }
    }
}

}  // namespace msim

#endif  // MSIM_FOLD_H

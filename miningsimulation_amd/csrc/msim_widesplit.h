// msim_widesplit.h — the shared-draw form of sweeps on the large-network pipeline (msim_wide.h): one W1 pass per
// draw group, on the group's ENVELOPE network (the group's weights, every miner at its largest delay over the
// group's points), then the split kernel WS, then W2 and W3 per point.
//
// Exactness. Of what W1 writes, the histogram, info[0..1] (n_end, last finder), tlast, lanes[].t0 and every field
// of a WideCand except the rank in lane_seq are functions of the draws alone: the draws depend on the seeds, the
// weights, W and the duration, which the points of a group share. Only the LISTING
//     { i : f_i < m and I_{i+1} <= min(prop[f_i], FTHR_NEVER) }
// depends on the delays, and with it info[2], lanes[].count and the rank. The listing is monotone in the delay, so
// the envelope's list is a superset of every point's; WS puts the envelope's candidates into block order (W3's
// scan of the (phase, lane) counts plus the rank) and keeps, per point, the entries that pass the point's own
// thresholds: exactly the blocks, in block order, that W1 would have listed on the point's own tables (blocks
// past the end of the run included, so a point's count is its own launch's count).
//
// Which parts of the envelope's tables serve every point:
//   (1) cf / bucket: wide_pick returns the finder from the cumulative-weight half of a cf entry; the threshold
//       half is read by W1 alone (w1_segment's `thcur`). W2's WideSrc::next and W1's removal loops discard it.
//       So every consumer after W1 may read the envelope's cf / bucket.
//   (2) W2 and W3 read the delays only through `prop`: each point passes its own.
//   (3) logt and the jump matrices do not depend on the network.
//
// Failed runs. The wide pipeline has no retry kernel, so a failed run stays failed. An envelope failure (an error
// bit of W1, or its list past rcap_env) fails the run at every point of the group; a point's own list past its
// rcap_p fails the run at that point only, exactly when its own launch would have failed it.
#pragma once
#include <stdint.h>

#include "msim_wide.h"

namespace msim {

// A sorted envelope entry: envelope slot c (< 32 768) in the low half, finder (< WIDE_MAX_M) above it.
MSIM_HD uint32_t wsplit_pack(uint32_t c, uint32_t f) { return c | (f << 16); }
// The listing test of W1 (w1_segment: `slow = Inext <= thcur`) on a point's thresholds.
MSIM_HD bool wsplit_keep(uint32_t packed, uint32_t inext, const uint32_t *__restrict__ fthr)
{
    return inext <= fthr[packed >> 16];
}
MSIM_HD uint32_t wsplit_fthr(int64_t prop) { return prop < (int64_t)FTHR_NEVER ? (uint32_t)prop : FTHR_NEVER; }

// Host form of WS's per-point pass over one run: `packed` / `inext` are the envelope's cc candidates in block
// order. Writes sel[j] (envelope slots, block order) for j < rcap and returns the count, or WIDE_NONE when the
// point's list exceeds rcap. The device walks the same entries 64 at a time with a ballot and a prefix popcount.
inline uint32_t wsplit_select(const uint32_t *packed, const uint32_t *inext, uint32_t cc, const uint32_t *fthr,
                              uint32_t rcap, uint32_t *sel)
{
    uint32_t n = 0;
    for (uint32_t i = 0; i < cc; ++i) {
        if (!wsplit_keep(packed[i], inext[i], fthr)) continue;
        if (n < rcap) sel[n] = packed[i] & 0xFFFFu;
        ++n;
    }
    return n > rcap ? WIDE_NONE : n;
}

}  // namespace msim

// msim_drawgroups.h — the partition of a sweep's points into draw groups (msim_sweepsplit.h, msim_widesplit.h).
// Host only, no HIP and no config type: the caller says what a point is.
#pragma once
#include <stdint.h>

#include <vector>

namespace msim {

// Points that draw the same blocks share a group and one draw pass on the group's envelope network (every miner at
// its largest delay over the group). same_draws(i, j): a point joins the first group, in creation order, whose FIRST
// member it matches. take_envelope(points, &taken) -> error code: builds and judges the envelope of a group of two or
// more points (never fewer) and keeps it when it sets `taken`; an error ends the planning and is returned unchanged.
// A group that is not taken loses the first of its points with the strictly largest max_delay(i), whose group of one
// goes to the end of the list, until the rest is taken. groups: every group's points in point order; group_of: per point.
template <class SameDraws, class MaxDelay, class TakeEnvelope>
int plan_draw_groups(uint32_t n_points, SameDraws same_draws, MaxDelay max_delay, TakeEnvelope take_envelope,
                     std::vector<std::vector<uint32_t>> *groups, std::vector<int32_t> *group_of)
{
    std::vector<std::vector<uint32_t>> &work = *groups;
    work.clear();
    for (uint32_t i = 0; i < n_points; ++i) {
        size_t g = 0;
        while (g < work.size() && !same_draws(work[g][0], i)) ++g;
        if (g == work.size()) work.emplace_back();
        work[g].push_back(i);
    }
    group_of->assign(n_points, -1);
    for (size_t g = 0; g < work.size(); ++g) {  // `work` grows while groups are split
        while (work[g].size() > 1) {
            bool taken = false;
            const int rc = take_envelope(work[g], &taken);
            if (rc) return rc;
            if (taken) break;
            size_t worst = 0;
            for (size_t j = 1; j < work[g].size(); ++j)
                if (max_delay(work[g][j]) > max_delay(work[g][worst])) worst = j;
            const uint32_t pt = work[g][worst];
            work[g].erase(work[g].begin() + (long)worst);
            work.push_back({pt});
        }
        for (uint32_t i : work[g]) (*group_of)[i] = (int32_t)g;
    }
    return 0;
}

}  // namespace msim

// msim_timing.h — stage timing (msim_timing.hip): the launch bracket for the launch paths of msim_api.hip, and
// the pure part of the busy time, which tests/native/devcache_host.cpp checks on the host.
#pragma once
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

namespace msim {

// Length of the union of (begin, end) intervals: sorted by begin, overlapping or touching ones merged.
inline double interval_union(std::vector<std::pair<double, double>> iv)
{
    if (iv.empty()) return 0;
    std::sort(iv.begin(), iv.end());
    double lo = iv[0].first, hi = iv[0].second, acc = 0;
    for (const auto &p : iv) {
        if (p.first > hi) {
            acc += hi - lo;
            lo = p.first;
            hi = p.second;
        } else if (p.second > hi) {
            hi = p.second;
        }
    }
    return acc + (hi - lo);
}

#if defined(__HIPCC__)
// HIP events recorded on the launch stream (msim_timing_enable / msim_timing_read*).
struct Timing {
    std::mutex mu;
    bool on = false;
    std::vector<hipEvent_t> k1;      // (begin, end) pairs around each draw kernel (K1 / W1)
    std::vector<hipEvent_t> launch;  // (begin, end) pairs around msim_launch
    std::vector<hipEvent_t> engine;  // (begin, end) pairs around the entity engine (E1) of each slice
    uint32_t launches = 0;
};
Timing &timing();

// One msim_launch under stage timing. It takes the timing lock; with timing off it lets go at once. With timing
// on it records the launch's begin event, counts the launch and keeps the lock for its whole scope, because the
// launch code appends to the stage vectors it hands out (k1(), engine(): null with timing off); its destructor
// records the end event.
class LaunchTimer {
public:
    explicit LaunchTimer(hipStream_t s) : tm_(timing()), lk_(tm_.mu), s_(s)
    {
        if (!tm_.on) {
            lk_.unlock();
            return;
        }
        hipEvent_t begin = nullptr;
        if (hipEventCreate(&begin) == hipSuccess && hipEventCreate(&end_) == hipSuccess) {
            tm_.launch.push_back(begin);
            tm_.launch.push_back(end_);
            (void)hipEventRecord(begin, s_);
        }
        tm_.launches++;
    }
    ~LaunchTimer()
    {
        if (end_) (void)hipEventRecord(end_, s_);
    }
    std::vector<hipEvent_t> *k1() { return lk_.owns_lock() ? &tm_.k1 : nullptr; }
    std::vector<hipEvent_t> *engine() { return lk_.owns_lock() ? &tm_.engine : nullptr; }

private:
    Timing &tm_;
    std::unique_lock<std::mutex> lk_;
    hipStream_t s_;
    hipEvent_t end_ = nullptr;
};
#endif

}  // namespace msim

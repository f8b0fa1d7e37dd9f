// msim_timing.hip — stage timing (msim_timing_enable / msim_timing_read*): HIP events recorded on the launch
// stream around every msim_launch (LaunchTimer, msim_timing.h) and around the stages inside it.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/msim.h"
#include "msim_timing.h"

msim::Timing &msim::timing()
{
    static Timing t;
    return t;
}

namespace {

using msim::Timing;
using msim::timing;

// Destroys every event and zeroes the launch count (under tm.mu).
void reset(Timing &tm)
{
    for (std::vector<hipEvent_t> *v : {&tm.k1, &tm.launch, &tm.engine}) {
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
        v->clear();
    }
    tm.launches = 0;
}

// Union length of (begin, end) event pairs. Events are timed against an anchor of their own device: a pair
// whose begin cannot be timed against an existing anchor (hipEventElapsedTime fails across devices) starts a
// new group with its begin as the anchor. The result is the largest group's busy time (one device's), so a
// timed run over several devices reads instead of failing.
int busy_ms(const std::vector<hipEvent_t> &v, double *out)
{
    *out = 0;
    std::vector<hipEvent_t> anchors;
    std::vector<std::vector<std::pair<double, double>>> groups;
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
        if (hipEventSynchronize(v[i + 1]) != hipSuccess) return MSIM_E_HIP;
        bool placed = false;
        for (size_t g = 0; g < anchors.size() && !placed; ++g) {
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, anchors[g], v[i]) != hipSuccess) continue;
            if (hipEventElapsedTime(&b, anchors[g], v[i + 1]) != hipSuccess) return MSIM_E_HIP;
            groups[g].emplace_back(a, b);
            placed = true;
        }
        if (!placed) {
            float b = 0;
            if (hipEventElapsedTime(&b, v[i], v[i + 1]) != hipSuccess) return MSIM_E_HIP;
            anchors.push_back(v[i]);
            groups.push_back({{0.0, (double)b}});
        }
    }
    if (!anchors.empty()) (void)hipGetLastError();  // the failed cross-device queries leave an error behind
    for (const auto &iv : groups) {
        const double busy = msim::interval_union(iv);
        *out = busy > *out ? busy : *out;
    }
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_timing_enable(int on)
{
    Timing &tm = timing();
    std::lock_guard<std::mutex> g(tm.mu);
    reset(tm);
    tm.on = on != 0;
    return MSIM_OK;
}

int msim_timing_read_stages(double *draws_ms, double *engine_ms, double *launch_ms, uint32_t *launches)
{
    if (!draws_ms || !engine_ms || !launch_ms || !launches) return MSIM_E_INVALID;
    Timing &tm = timing();
    std::lock_guard<std::mutex> g(tm.mu);
    double acc[3] = {0, 0, 0};
    int rc = MSIM_OK;
    std::vector<hipEvent_t> *vs[3] = {&tm.k1, &tm.engine, &tm.launch};
    for (int pass = 0; pass < 3; ++pass) {
        std::vector<hipEvent_t> &v = *vs[pass];
        for (size_t i = 0; i + 1 < v.size(); i += 2) {
            float ms = 0;
            if (hipEventSynchronize(v[i + 1]) != hipSuccess || hipEventElapsedTime(&ms, v[i], v[i + 1]) != hipSuccess)
                rc = MSIM_E_HIP;
            acc[pass] += ms;
        }
    }
    *draws_ms = acc[0];
    *engine_ms = acc[1];
    *launch_ms = acc[2];
    *launches = tm.launches;
    reset(tm);
    return rc;
}

int msim_timing_read_all(msim_timing *out)
{
    if (!out) return MSIM_E_INVALID;
    memset(out, 0, sizeof(*out));
    int rc = MSIM_OK;
    {
        Timing &tm = timing();
        std::lock_guard<std::mutex> g(tm.mu);
        const std::vector<hipEvent_t> *vs[3] = {&tm.k1, &tm.engine, &tm.launch};
        double *busy[3] = {&out->draws_busy_ms, &out->engine_busy_ms, &out->launch_busy_ms};
        for (int i = 0; i < 3; ++i)
            if (busy_ms(*vs[i], busy[i]) != MSIM_OK) rc = MSIM_E_HIP;
    }
    const int r2 = msim_timing_read_stages(&out->draws_ms, &out->engine_ms, &out->launch_ms, &out->launches);
    return rc ? rc : r2;
}

int msim_timing_read(double *draws_ms, double *launch_ms, uint32_t *launches)
{
    double e = 0;
    return msim_timing_read_stages(draws_ms, &e, launch_ms, launches);
}

}  // extern "C"

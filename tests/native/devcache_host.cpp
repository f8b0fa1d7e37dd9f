// Host test of msim_devcache.h (the per-device table cache behind every lazily uploaded table of msim_api.hip)
// with a stand-in backend: a "current device" per thread, counted allocations, copies and frees, and a switch
// that makes the next copy fail. Launches race on the cache from several streams and from one thread per
// device (bench.py's two streams, msim_run_multi), so threads x calls over several devices and two keys must
// upload each (device, key) once and hand every caller the same base pointer. Also checks the pure part of
// stage timing's busy time (msim_timing.h). Prints "OK <gets> <allocs> <frees>"; exits non-zero otherwise.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../miningsimulation_amd/csrc/msim_devcache.h"
#include "../../miningsimulation_amd/csrc/msim_timing.h"

namespace {

std::atomic<long> g_allocs{0}, g_copies{0}, g_frees{0}, g_bad{0};
std::atomic<bool> g_fail_next_copy{false};
thread_local int t_device = 0;

struct FakeBackend {
    static bool device(int *dev)
    {
        *dev = t_device;
        return true;
    }
    static void *alloc(size_t bytes)
    {
        ++g_allocs;
        return malloc(bytes);
    }
    static bool upload(void *dst, const void *src, size_t bytes)
    {
        if (g_fail_next_copy.exchange(false)) return false;
        ++g_copies;
        memcpy(dst, src, bytes);
        return true;
    }
    static void release(void *ptr)
    {
        ++g_frees;
        free(ptr);
    }
};
using Cache = msim::DevCache<FakeBackend>;

void check(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAIL %s\n", what);
        ++g_bad;
    }
}

// The table of (device, key): its own device base address, then the key (a table that points into itself).
struct Table {
    const char *self;
    uint64_t key;
};
void *get_table(Cache &c, uint64_t key)
{
    return c.get(key, sizeof(Table), [&](char *h, const char *dev_base) {
        Table t{dev_base, key};
        memcpy(h, &t, sizeof(t));
    });
}

// T threads x N gets over D devices and two keys: one upload per (device, key), one base pointer each.
void test_race(int threads, int calls)
{
    const int D = 3;
    std::mutex mu;
    const long a0 = g_allocs.load(), f0 = g_frees.load(), c0 = g_copies.load();
    {
        Cache cache(mu);
        std::atomic<void *> seen[D][2];
        for (auto &row : seen)
            for (auto &p : row) p = nullptr;
        std::vector<std::thread> ts;
        for (int t = 0; t < threads; ++t)
            ts.emplace_back([&, t] {
                unsigned x = 12345u + 977u * (unsigned)t;
                for (int i = 0; i < calls; ++i) {
                    x = x * 1103515245u + 12345u;
                    const int dev = (int)((x >> 16) % D), key = (int)((x >> 24) & 1u);
                    t_device = dev;
                    void *p = get_table(cache, (uint64_t)key);
                    if (!p) {
                        ++g_bad;
                        continue;
                    }
                    void *first = nullptr;
                    if (!seen[dev][key].compare_exchange_strong(first, p) && first != p) ++g_bad;  // two base pointers
                    const Table *tab = (const Table *)p;  // the build callback saw the address get() returned
                    if (tab->self != (const char *)p || tab->key != (uint64_t)key) ++g_bad;
                    if ((x >> 8) % 64 == 0) {  // a caller of the borrowed mutex that is not inside a get()
                        std::lock_guard<std::mutex> g(mu);
                    }
                }
            });
        for (auto &t : ts) t.join();
        long want = 0;
        for (auto &row : seen)
            for (auto &p : row) want += p.load() != nullptr;
        check(g_allocs.load() - a0 == want && g_copies.load() - c0 == want, "one upload per (device, key)");
        check(g_frees.load() == f0, "nothing freed while cached");
        cache.clear();
        check(g_frees.load() - f0 == g_allocs.load() - a0, "clear() frees every allocation");
        t_device = 0;
        check(get_table(cache, 0) != nullptr && g_allocs.load() - a0 == want + 1, "a cleared cache uploads again");
    }
    check(g_frees.load() - f0 == g_allocs.load() - a0, "the destructor frees what is left");
}

// The "covers" predicate (device_tables: same segment length, at least as many segments): nseg 12, then 8
// (served by the 12), then 16 (a second upload), then 12 again (no third).
void test_covers()
{
    std::mutex mu;
    Cache cache(mu);
    t_device = 1;
    const long a0 = g_allocs.load();
    auto get = [&](uint64_t seg, uint64_t nseg) {
        return cache.get(seg, nseg, [&](uint64_t have) { return have >= nseg; }, 64 * nseg, [](char *, const char *) {});
    };
    void *p12 = get(1024, 12), *p8 = get(1024, 8);
    check(p12 && p8 == p12 && g_allocs.load() - a0 == 1, "a larger entry serves a smaller request");
    void *p16 = get(1024, 16);
    check(p16 && p16 != p12 && g_allocs.load() - a0 == 2, "a larger request uploads");
    void *q12 = get(1024, 12);
    check((q12 == p12 || q12 == p16) && g_allocs.load() - a0 == 2, "both entries keep serving");
    check(get(2048, 8) != p12 && g_allocs.load() - a0 == 3, "another segment length is another table");
    t_device = 2;
    check(get(1024, 8) != p12 && g_allocs.load() - a0 == 4, "another device is another table");
    t_device = 0;
}

// A failed copy frees its allocation and inserts nothing; the next get() uploads.
void test_failed_copy()
{
    std::mutex mu;
    Cache cache(mu);
    const long a0 = g_allocs.load(), f0 = g_frees.load(), c0 = g_copies.load();
    g_fail_next_copy = true;
    check(get_table(cache, 7) == nullptr, "a failed copy returns null");
    check(g_allocs.load() - a0 == 1 && g_frees.load() - f0 == 1 && g_copies.load() == c0, "and frees its allocation");
    void *p = get_table(cache, 7);
    check(p != nullptr && g_allocs.load() - a0 == 2 && g_copies.load() - c0 == 1, "the next get uploads");
    check(get_table(cache, 7) == p && g_allocs.load() - a0 == 2, "and is cached");
}

void test_interval_union()
{
    using IV = std::vector<std::pair<double, double>>;
    check(msim::interval_union(IV{}) == 0.0, "union: empty");
    check(msim::interval_union(IV{{2.0, 5.0}}) == 3.0, "union: one interval");
    check(msim::interval_union(IV{{0.0, 1.0}, {2.0, 4.0}, {10.0, 10.5}}) == 3.5, "union: disjoint");
    check(msim::interval_union(IV{{0.0, 10.0}, {2.0, 3.0}, {4.0, 9.0}}) == 10.0, "union: nested");
    check(msim::interval_union(IV{{0.0, 1.0}, {1.0, 2.0}, {2.0, 4.0}}) == 4.0, "union: touching");
    check(msim::interval_union(IV{{6.0, 8.0}, {0.0, 2.0}, {7.0, 9.0}, {1.0, 3.0}}) == 6.0, "union: unsorted, overlapping");
}

}  // namespace

int main(int argc, char **argv)
{
    const int threads = argc > 1 ? atoi(argv[1]) : 4;
    const int calls = argc > 2 ? atoi(argv[2]) : 2000;
    test_race(threads, calls);
    test_covers();
    test_failed_copy();
    test_interval_union();
    if (g_bad.load()) {
        fprintf(stderr, "FAIL bad=%ld\n", g_bad.load());
        return 1;
    }
    printf("OK %ld %ld %ld\n", (long)threads * calls, g_allocs.load(), g_frees.load());
    return 0;
}

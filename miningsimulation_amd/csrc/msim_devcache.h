// msim_devcache.h — "upload this table once per device": the cache behind every lazily uploaded device table
// of a config, of a sweep and of the process (msim_api.hip).
//
// get() finds the entry of the current device and a small key, or sizes, allocates, builds, copies and inserts
// one, all under one mutex, so that launches racing on several streams or devices upload each table once and
// all see the same base pointer; carving tables out of it stays with the caller. The cache BORROWS its mutex: a
// config or a sweep lends its single mutex, the process-wide log table has one of its own. Under the mutex get()
// calls only the backend and the build callback, so code that takes the same mutex elsewhere (never around a
// get() or inside a build callback) cannot deadlock with it. Templated over the backend so that the host test
// (tests/native/devcache_host.cpp) drives the same code with counting stand-ins and racing threads.
//
// Backend B: static bool device(int *dev); static void *alloc(size_t bytes);
//            static bool upload(void *dst, const void *src, size_t bytes); static void release(void *ptr).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <vector>

namespace msim {

template <class B>
class DevCache {
public:
    explicit DevCache(std::mutex &mu) : mu_(mu) {}
    DevCache(const DevCache &) = delete;
    DevCache &operator=(const DevCache &) = delete;
    ~DevCache() { clear(); }

    // The device base address of table `key` on the current device, or nullptr when the device cannot be queried,
    // the allocation fails or the copy fails (the allocation is then freed, nothing is inserted and the next call
    // tries again). An entry serves when its key matches and covers(its extent) holds; the last such entry wins.
    // A new entry is `bytes` long, stored with `extent` and filled by build(host, dev_base): the zeroed host image
    // and the address it will have on the device, for tables that hold device pointers into themselves.
    template <class Covers, class Build>
    void *get(uint64_t key, uint64_t extent, Covers covers, size_t bytes, Build build)
    {
        int dev = 0;
        if (!B::device(&dev)) return nullptr;
        std::lock_guard<std::mutex> g(mu_);
        void *d = nullptr;
        for (const Entry &e : entries_)
            if (e.dev == dev && e.key == key && covers(e.extent)) d = e.ptr;
        if (d) return d;
        if (!(d = B::alloc(bytes))) return nullptr;
        std::vector<char> h(bytes, 0);
        build(h.data(), (const char *)d);
        if (!B::upload(d, h.data(), bytes)) {
            B::release(d);
            return nullptr;
        }
        entries_.push_back({dev, key, extent, d});
        return d;
    }
    // One table per (device, key).
    template <class Build>
    void *get(uint64_t key, size_t bytes, Build build)
    {
        return get(key, 0, [](uint64_t) { return true; }, bytes, build);
    }

    // Free every entry (the owner's destroy function; no launch may be using the tables).
    void clear()
    {
        std::lock_guard<std::mutex> g(mu_);
        for (const Entry &e : entries_) B::release(e.ptr);
        entries_.clear();
    }

private:
    struct Entry {
        int dev;
        uint64_t key, extent;
        void *ptr;
    };
    std::mutex &mu_;
    std::vector<Entry> entries_;
};

}  // namespace msim

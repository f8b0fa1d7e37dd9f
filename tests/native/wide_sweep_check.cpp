// wide_sweep_check.cpp — TEST INFRASTRUCTURE: the lane bodies of the shared-draw form of large-network sweeps
// (wide_sweep_body.h: listing, wsplit_select, wide_episode, combine) as a stand-alone program, built with
// -fsanitize=address,undefined and run as a child process by tests/test_wide_sweep_host.py. Checks the split's
// selection against every point's own listing and both overflow rules; prints "ok".
#include <stdio.h>

#include "wide_sweep_body.h"

static int fail(const char *what, int code)
{
    printf("FAILED %s (%d)\n", what, code);
    return 1;
}

int main()
{
    const uint32_t n = 4;
    const int64_t day = 86400000;
    struct Case {
        uint32_t m, np;
        int64_t D;
    } cases[] = {{3, 2, 40 * day}, {17, 3, 20 * day}, {300, 4, 10 * day}, {17, 2, 0}, {17, 2, 1}, {3, 3, 600000}};
    for (const Case &c : cases) {
        std::vector<uint64_t> w(c.m);
        uint64_t W = 0;
        for (uint32_t k = 0; k < c.m; ++k) {
            w[k] = k % 5 == 3 ? 0 : 1 + (k * 7) % 11;
            W += w[k];
        }
        std::vector<int64_t> props((size_t)c.np * c.m);
        const int64_t menu[] = {0, 1, 250, 2000, 12000, 60000};
        for (uint32_t p = 0; p < c.np; ++p)
            for (uint32_t k = 0; k < c.m; ++k) props[(size_t)p * c.m + k] = menu[(p * 3 + k) % 6];
        std::vector<uint32_t> f((size_t)c.np * n * c.m), s(f.size()), counts((size_t)(1 + c.np) * n);
        std::vector<uint8_t> ok((size_t)c.np * n);
        int rc = wsweep::run_group(w.data(), props.data(), c.m, c.np, W, c.D, 1000, 5, n, 0, nullptr, f.data(), s.data(),
                                   ok.data(), counts.data());
        if (rc) return fail("selection differs from the point's listing", rc);
        for (uint8_t x : ok)
            if (!x) return fail("a run failed at natural capacities", (int)c.m);
        // the envelope's capacity at the smallest of its counts fails the other runs at every point; a point's
        // capacity fails that point alone
        uint32_t lo = counts[0], hi = counts[0];
        for (uint32_t r = 0; r < n; ++r) {
            lo = counts[r] < lo ? counts[r] : lo;
            hi = counts[r] > hi ? counts[r] : hi;
        }
        if (lo == hi || lo == 0) continue;
        std::vector<uint8_t> ok2(ok.size());
        rc = wsweep::run_group(w.data(), props.data(), c.m, c.np, W, c.D, 1000, 5, n, lo, nullptr, f.data(), s.data(),
                               ok2.data(), counts.data());
        if (rc) return fail("envelope capacity: selection", rc);
        for (uint32_t p = 0; p < c.np; ++p)
            for (uint32_t r = 0; r < n; ++r)
                if (ok2[(size_t)p * n + r] != (counts[r] <= lo ? 1 : 0)) return fail("envelope capacity rule", (int)r);
        std::vector<uint32_t> rp(c.np, 0);
        rp[1] = 1;
        rc = wsweep::run_group(w.data(), props.data(), c.m, c.np, W, c.D, 1000, 5, n, 0, rp.data(), f.data(), s.data(),
                               ok2.data(), counts.data());
        if (rc) return fail("point capacity: selection", rc);
        for (uint32_t p = 0; p < c.np; ++p)
            for (uint32_t r = 0; r < n; ++r) {
                const uint8_t want = p == 1 ? (counts[(size_t)2 * n + r] <= 1 ? 1 : 0) : 1;
                if (ok2[(size_t)p * n + r] != want) return fail("point capacity rule", (int)p);
            }
    }
    printf("ok\n");
    return 0;
}

// k1pick400_check.cpp — TEST INFRASTRUCTURE: the draw kernel's picker by one multiply with 400
// (msim_fastdraw.h pick_off400_key) over ALL 2^32 high words, as a stand-alone program (built with
// -fsanitize=address,undefined by tests/test_k1pick400.py).
//
//   k1pick400_check [THREADS]   -> prints counts as JSON
//
// The claim (msim_fastdraw.h, above rng_next_hi): with 400 h' = t 2^32 + L, whenever L < PICK400_RARE_LO both
// h' and h' + 1 (mod 2^32), with any low word, have pick_q_exact equal to t >> 2, and t & ~3 is the byte
// offset of that table entry. pick_q_exact is nondecreasing in u, so "any low word" is settled by the smallest
// draw (h', 0) and the largest one (h' + 1, 2^32 - 1). Also: the band holds every h' the key of the
// multiply with 100 (pick_p_key, PICK_HI_RARE_LO) sends to the exact path, and h' = 2^32 - 1, whose successor wraps.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../miningsimulation_amd/csrc/msim_fastdraw.h"

using namespace msim;

struct Tally {
    uint64_t n, settled, flagged, bad, bad_offset, bad_division, not_superset, old_flagged, first_bad;
};

static void check(uint32_t hp, bool divide, Tally *t)
{
    uint32_t key, key100;
    const uint32_t off = pick_off400_key(hp, key);
    const uint32_t p = pick_p_key(hp, key100);
    t->n++;
    bool bad = false;
    if (off != 4u * p || (off & 3u) || off > 4u * 99u) t->bad_offset++, bad = true;
    if (key100 >= PICK_HI_RARE_LO) {
        t->old_flagged++;
        if (key < PICK400_RARE_LO) t->not_superset++, bad = true;
    }
    if (key >= PICK400_RARE_LO) {
        t->flagged++;
    } else {
        t->settled++;
        const uint64_t umin = (uint64_t)hp << 32, umax = ((uint64_t)(hp + 1u) << 32) | 0xFFFFFFFFull;
        if (hp == 0xFFFFFFFFu) t->bad++, bad = true;  // its successor wraps: must be in the band
        if (pick_q_exact(umin) != off >> 2 || pick_q_exact(umax) != off >> 2) t->bad++, bad = true;
        if (divide && ((uint32_t)(umin / PERC_MULTIPLIER) != off >> 2 || (uint32_t)(umax / PERC_MULTIPLIER) != off >> 2))
            t->bad_division++, bad = true;
    }
    if (bad && !t->first_bad) t->first_bad = 0x100000000ull | hp;
}

struct Job {
    uint64_t lo, hi;
    Tally t;
};

static void *worker(void *p)
{
    Job *j = (Job *)p;
    for (uint64_t h = j->lo; h < j->hi; ++h) check((uint32_t)h, false, &j->t);
    return nullptr;
}

static void add(Tally *a, const Tally &b)
{
    a->n += b.n, a->settled += b.settled, a->flagged += b.flagged, a->bad += b.bad, a->bad_offset += b.bad_offset;
    a->bad_division += b.bad_division, a->not_superset += b.not_superset, a->old_flagged += b.old_flagged;
    if (!a->first_bad) a->first_bad = b.first_bad;
}

static void print(const char *name, const Tally &t, const char *end)
{
    printf("\"%s\": {\"n\": %llu, \"settled\": %llu, \"flagged\": %llu, \"bad\": %llu, \"bad_offset\": %llu, "
           "\"bad_division\": %llu, \"not_superset\": %llu, \"old_flagged\": %llu, \"first_bad\": %llu}%s",
           name, (unsigned long long)t.n, (unsigned long long)t.settled, (unsigned long long)t.flagged,
           (unsigned long long)t.bad, (unsigned long long)t.bad_offset, (unsigned long long)t.bad_division,
           (unsigned long long)t.not_superset, (unsigned long long)t.old_flagged, (unsigned long long)t.first_bad, end);
}

int main(int argc, char **argv)
{
    const int th = argc > 1 ? atoi(argv[1]) : 8;
    if (th < 1 || th > 64) return 2;
    std::vector<Job> jobs((size_t)th);
    std::vector<pthread_t> t((size_t)th);
    const uint64_t all = 1ull << 32;
    for (int i = 0; i < th; ++i) {
        jobs[i] = Job{all * (uint64_t)i / (uint64_t)th, all * (uint64_t)(i + 1) / (uint64_t)th, Tally{}};
        pthread_create(&t[i], nullptr, worker, &jobs[i]);
    }
    // every high word within 2^12 of each of the 100 multiples of 2^32 / 100 (and of 2^32 itself, from below), once
    // more with PickFinder's own division u / PERC_MULTIPLIER beside pick_q_exact
    Tally edges{};
    for (uint64_t b = 0; b <= 100; ++b) {
        const int64_t hb = (int64_t)((b << 32) / 100);
        for (int64_t d = -4096; d <= 4096; ++d)
            if (hb + d >= 0 && hb + d <= 0xFFFFFFFFll) check((uint32_t)(hb + d), true, &edges);
    }
    // the wrap: h' = 2^32 - 1 must be in the band
    uint32_t kw;
    (void)pick_off400_key(0xFFFFFFFFu, kw);
    Tally every{};
    for (int i = 0; i < th; ++i) {
        pthread_join(t[i], nullptr);
        add(&every, jobs[i].t);
    }
    printf("{\"band_lo\": %llu, \"wrap_key\": %llu, \"wrap_rejected\": %s, ", (unsigned long long)PICK400_RARE_LO,
           (unsigned long long)kw, kw >= PICK400_RARE_LO ? "true" : "false");
    print("every_high_word", every, ", ");
    print("edges", edges, "}\n");
    return 0;
}

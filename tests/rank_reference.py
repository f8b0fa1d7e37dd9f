"""Exact reference of the device's order statistics (msim_order_stat), from per-run counters, and the synthetic
records the rank tests (CPU and GPU) select from.

The four keys of a record are found, stale and the two terms of tests/moments_reference.py; a column's keys are
sorted, the r-th one is the value, and `below` and `equal` are counted. Plain NumPy and Python integers; nothing here
imports the library under test.

synthetic(): column k carries pattern (k + shift) % 9 over its runs r:
  0  all zero
  1  all equal, (6, 2): equal == N for found, stale and rate
  2  f = L                     (share term 2^32, bit 32; 0 in the runs with L = 0)
  3  (1, 2^32 - 1) on odd runs (rate term 2^64 - 2^32: top byte 0xFF), (7, 3) on even ones
  4  f = 5, s = r % 7          (with the runs of L = 0: a found block and no best chain)
  5  two values that differ only in the lowest byte (found), three (stale)
  6  two values that differ only in the highest non-zero byte
  7  strictly increasing: f = r + 1, s = 2 r
  8  random
and L is random in 1000..2999 but 0 in every fifth run."""
import numpy as np

import moments_reference as ref

U32 = 0xFFFFFFFF
QUANTITIES = 4


def synthetic(n_runs, m, shift=0, seed=0):
    """(found [n, M] uint32, stale [n, M] uint32, best_height [n] uint32)."""
    rng = np.random.default_rng(9000 + seed)
    r = np.arange(n_runs, dtype=np.int64)
    L = rng.integers(1000, 3000, size=n_runs, dtype=np.int64)
    L[r % 5 == 4] = 0
    f = np.zeros((n_runs, m), dtype=np.int64)
    s = np.zeros((n_runs, m), dtype=np.int64)
    for k in range(m):
        e = (k + shift) % 9
        if e == 1:
            f[:, k], s[:, k] = 6, 2
        elif e == 2:
            f[:, k], s[:, k] = L, r % 3
        elif e == 3:
            f[:, k] = np.where(r % 2 == 1, 1, 7)
            s[:, k] = np.where(r % 2 == 1, U32, 3)
        elif e == 4:
            f[:, k], s[:, k] = 5, r % 7
        elif e == 5:
            f[:, k], s[:, k] = 0x01020300 | (r % 2), 0xA0B0C000 | (r % 3)
        elif e == 6:
            f[:, k] = 0x01000000 + ((r % 2) << 24)
            s[:, k] = np.where(r % 2 == 1, 0x80000000, 0x40000000)
        elif e == 7:
            f[:, k], s[:, k] = r + 1, 2 * r
        elif e == 8:
            f[:, k] = rng.integers(0, 2000, size=n_runs)
            s[:, k] = rng.integers(0, 20, size=n_runs)
    return f.astype(np.uint32), s.astype(np.uint32), L.astype(np.uint32)


def records(found, stale):
    """[n, M, 2] uint32 in msim_run_record's layout."""
    return np.ascontiguousarray(np.stack([found, stale], axis=-1).astype(np.uint32))


def keys(found, stale, best_height):
    """[4, n, M] uint64: found, stale, share_t, rate_t."""
    st, rt = ref.terms(found, stale, best_height)
    return np.stack([np.asarray(found).astype(np.uint64), np.asarray(stale).astype(np.uint64), st, rt])


def select(found, stale, best_height, ranks):
    """order[column][quantity][j] = (value, below, equal) as Python ints, or None for a rank that is not below the
    run count."""
    k4 = np.sort(keys(found, stale, best_height), axis=1)  # every column's keys in order
    n, m = k4.shape[1], k4.shape[2]
    ok = [0 <= r < n for r in ranks]
    at = np.array([r if good else 0 for r, good in zip(ranks, ok)], dtype=np.int64)
    out = []
    for k in range(m):
        col = []
        for q in range(QUANTITIES):
            srt = np.ascontiguousarray(k4[q, :, k])
            v = srt[at]
            lo = np.searchsorted(srt, v, side="left")
            hi = np.searchsorted(srt, v, side="right")
            col.append([(int(a), int(b), int(c - b)) if good else None for a, b, c, good in zip(v, lo, hi, ok)])
        out.append(col)
    return out


def rank_lists(n):
    """The rank lists of the tests for n runs, by length: each but the shortest two holds 0, n - 1 and the median,
    has a duplicated rank and is unsorted."""
    mid = n // 2
    spread = [(31 - j) * (n - 1) // 31 for j in range(32)]  # n - 1 down to 0
    spread[5], spread[17], spread[20] = mid, mid, 0
    return {1: [mid], 3: [n - 1, mid, 0], 5: [mid, 0, n - 1, 0, mid], 32: spread}


def diff(got, want):
    """Mismatches between two order[column][quantity][j] nests as strings; `want` entries of None are skipped."""
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} columns on the device, {len(want)} in the reference"]
    for k, (gc, wc) in enumerate(zip(got, want)):
        for q in range(QUANTITIES):
            for j, (g, w) in enumerate(zip(gc[q], wc[q])):
                if w is not None and tuple(int(x) for x in g) != w:
                    bad.append(f"column {k} quantity {q} rank #{j}: got {tuple(int(x) for x in g)} reference {w}")
    return bad

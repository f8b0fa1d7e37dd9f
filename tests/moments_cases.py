"""Synthetic per-run records for the moments tests (CPU and GPU): random rows with L = sum(found), and in between
every extreme the term and limb arithmetic has to survive. No simulation is run, so values no network produces
(f > L, s = 2^32 - 1) are reachable.

Row r of a case carries pattern r % 9 on miner (r // 9) % M:
  0  f = 0 with stale blocks (both terms 0)
  1  L = 0 with f > 0 (share term 0 by definition, rate term counted)
  2  f = L              (share term 2^32, its square 2^64: past one uint64)
  3  f = L + 1          (share term above 2^32)
  4  s > f; in odd groups f = 2^32 - 1 with L = 1 (share term 2^64 - 2^32)
  5  f = 1, s = 2^32 - 1 (rate term 2^64 - 2^32, its square just below 2^128)
  6  a random row, which rows 7 and 8 repeat (all-equal rows)."""
import numpy as np

U32 = 0xFFFFFFFF


def synthetic(n_runs, m, seed=0):
    """(found [n, M] uint32, stale [n, M] uint32, best_height [n] uint32)."""
    rng = np.random.default_rng(1000 + seed)
    f = rng.integers(0, 2000, size=(n_runs, m), dtype=np.int64)
    f[rng.random((n_runs, m)) < 0.2] = 0
    s = rng.integers(0, 20, size=(n_runs, m), dtype=np.int64)
    L = f.sum(axis=1)
    for r in range(n_runs):
        e, g = r % 9, r // 9
        t = g % m
        if e == 0:
            f[r, t], s[r, t] = 0, 7
        elif e == 1:
            L[r] = 0
            f[r, t], s[r, t] = 5, 0
        elif e == 2:
            L[r] = max(L[r], 10)
            f[r, t], s[r, t] = L[r], 3
        elif e == 3:
            L[r] = max(L[r], 10)
            f[r, t], s[r, t] = L[r] + 1, 2
        elif e == 4:
            if g % 2:
                L[r] = 1
                f[r, t], s[r, t] = U32, 1
            else:
                f[r, t], s[r, t] = 3, 9
        elif e == 5:
            f[r, t], s[r, t] = 1, U32
        elif e in (7, 8):
            f[r], s[r], L[r] = f[r - e + 6], s[r - e + 6], L[r - e + 6]
    return f.astype(np.uint32), s.astype(np.uint32), L.astype(np.uint32)


def records(found, stale):
    """[n, M, 2] uint32 in msim_run_record's layout."""
    return np.ascontiguousarray(np.stack([found, stale], axis=-1).astype(np.uint32))

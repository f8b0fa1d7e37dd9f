"""Exact reference of the Poisson bootstrap (msim_boot_row), written from the definitions: Python integers, Fraction
and decimal only; nothing here imports the library under test or reads its header.

Replicate b gives the absolute run r the weight weight(seed, b, r); a replicate's quantile is read off the explicitly
sorted weighted multiset of a column's keys. The keys are tests/rank_reference.py's (found, stale and the two terms of
tests/moments_reference.py)."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

import rank_reference as rr

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
T = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
     4294966817, 4294967252, 4294967292, 4294967295)


def thresholds():
    """floor(2^32 * sum_{i<=k} e^-1 / i!) for k = 0..12, with 80-digit decimals."""
    getcontext().prec = 80
    e_inv = Decimal(1) / Decimal(1).exp()
    out, acc, fact = [], Decimal(0), Decimal(1)
    for k in range(13):
        if k:
            fact *= k
        acc += e_inv / fact
        out.append(int((acc * (1 << 32)).to_integral_value(rounding="ROUND_FLOOR")))
    return tuple(out)


def mix(z):
    """SplitMix64's output function."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def weight(seed, b, run):
    if b == 0:
        return 1
    c = mix((seed & M64) ^ (((b >> 1) * G) & M64))
    z = mix((c + G * (run + 1)) & M64)
    u = z >> 32 if b & 1 else z & 0xFFFFFFFF
    return sum(1 for t in T if u >= t)


def weights(seed, b, run_begin, n):
    return [weight(seed, b, run_begin + r) for r in range(n)]


def quantile_rank(W, q):
    return max(1, math.ceil(q * W)) - 1


def select_weighted(keys, ws, rank):
    """(value, below, equal, s_hi, s_lo) at the 0-based `rank` of the multiset that holds keys[r] ws[r] times."""
    pairs = sorted((int(k), int(w)) for k, w in zip(keys, ws) if w)
    run, value = 0, None
    for k, w in pairs:
        run += w
        if run > rank:
            value = k
            break
    assert value is not None, "the rank is not below the total weight"
    below = sum(w for k, w in pairs if k < value)
    equal = sum(w for k, w in pairs if k == value)
    s_hi = sum(w * (k >> 32) for k, w in pairs if k < value)
    s_lo = sum(w * (k & 0xFFFFFFFF) for k, w in pairs if k < value)
    return (value, below, equal, s_hi & M64, s_lo & M64)


def bootstrap(keys4, items, qs, B, seed, run_begin=0):
    """keys4: per point a [4][n][M] array of keys (rank_reference.keys). items: (point, column, quantity, q_index).
    Returns (W [B], rows[i][b] = 5-tuples, all zero for an empty replicate)."""
    n = int(np.asarray(keys4[0]).shape[1])
    wts = [weights(seed, b, run_begin, n) for b in range(B)]
    W = [sum(w) for w in wts]
    rows = []
    for (p, col, qu, qi) in items:
        ks = [int(x) for x in np.asarray(keys4[p])[qu, :, col].tolist()]
        rows.append([(0, 0, 0, 0, 0) if W[b] == 0 else select_weighted(ks, wts[b], quantile_rank(W[b], qs[qi]))
                     for b in range(B)])
    return W, rows


def point_keys(found, stale, best_height):
    """[4, n, M] uint64 keys of one point."""
    return rr.keys(found, stale, best_height)


def shortfall(row, W_b, q):
    """(S_below + (k - below) value) / k, or None for an empty replicate."""
    value, below, equal, s_hi, s_lo = row
    if equal == 0:
        return None
    k = quantile_rank(W_b, q) + 1
    return Fraction((s_hi << 32) + s_lo + (k - below) * value, k)


def variance(xs):
    """The sample variance of the entries that are not None, b >= 1 only (xs[0] is the data)."""
    v = [Fraction(x) for x in xs[1:] if x is not None]
    mean = sum(v) / len(v)
    return sum((x - mean) ** 2 for x in v) / (len(v) - 1)


def interval(xs, level):
    v = sorted(x for x in xs[1:] if x is not None)
    a = (1.0 - level) / 2.0
    return v[quantile_rank(len(v), a)], v[quantile_rank(len(v), 1.0 - a)]


def difference(xs, ys, level):
    d = [None if x is None or y is None else Fraction(x) - Fraction(y) for x, y in zip(xs, ys)]
    return d[0], [x for x in d[1:] if x is not None], variance(d), interval(d, level)


def diff_rows(got, want):
    """Mismatches between rows[i][b] nests as strings."""
    bad = []
    for i, (gi, wi) in enumerate(zip(got, want)):
        for b, (g, w) in enumerate(zip(gi, wi)):
            if tuple(int(x) for x in g) != tuple(w):
                bad.append(f"item {i} replicate {b}: got {tuple(int(x) for x in g)} reference {tuple(w)}")
    if len(got) != len(want):
        bad.append(f"{len(got)} items against {len(want)}")
    return bad


def extreme_columns(n):
    """(found, stale, L) of three columns: all equal; found alternating 0 / 2^32 - 1; a rate key of 2^64 - 2^32."""
    r = np.arange(n)
    f = np.stack([np.full(n, 6), np.where(r % 2 == 0, 0, 0xFFFFFFFF), np.where(r % 3 == 0, 1, 7)], axis=1)
    s = np.stack([np.full(n, 2), np.where(r % 2 == 0, 0xFFFFFFFF, 0), np.where(r % 3 == 0, 0xFFFFFFFF, 3)], axis=1)
    return f.astype(np.uint32), s.astype(np.uint32), np.full(n, 1000, dtype=np.uint32)

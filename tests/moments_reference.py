"""Exact reference of the device's second moments and histograms (msim_moments, msim_hist_spec, msim_errors), from
per-run counters.

Terms as tests/sums_reference.py computes them (one f64 division, the exact product by 2^32, one rounded + 0.5,
truncation), but without its < 2^53 bound: synthetic records reach 2^64 - 2^32, which still fits a uint64; terms
from 2^63 up are converted with int(float) on their own. Squares, cross products and sums are Python integers,
bins are integer shifts, and the error bars are fractions.Fraction until the final square root.

Plain NumPy and Python integers; nothing here imports the library under test."""
import math
from fractions import Fraction

import numpy as np

_TWO32 = 4294967296.0
ONE = 1 << 32
NAMES = ("found", "stale", "share", "rate", "found_sq", "stale_sq", "found_stale", "share_sq", "rate_sq")


def _to_int_terms(x, mask):
    """floor of the non-negative float64 array x as uint64, 0 outside mask. Values below 2^63 convert with NumPy's
    cast (exact: they are integers already); the few at or above it go through int(float) one by one."""
    v = np.where(mask, np.floor(x), 0.0)
    assert np.isfinite(v).all() and (v >= 0).all() and (v < 2.0 ** 64).all()
    big = v >= 2.0 ** 63
    t = np.where(big, 0.0, v).astype(np.uint64)
    for idx in np.argwhere(big):
        t[tuple(idx)] = int(v[tuple(idx)])
    return t


def terms(found, stale, best_height):
    """(share_t, rate_t) as uint64 arrays [n, M] (the largest term, 2^64 - 2^32, still fits); share_t = 0 where
    found == 0 or L == 0."""
    f = np.asarray(found).astype(np.int64)
    s = np.asarray(stale).astype(np.int64)
    L = np.asarray(best_height).astype(np.int64)
    assert f.ndim == 2 and s.shape == f.shape and L.shape == (f.shape[0],)
    fd, sd, Ld = f.astype(np.float64), s.astype(np.float64), L.astype(np.float64)
    some = f > 0
    ok = some & (L[:, None] > 0)
    share = np.where(ok, fd / np.where(ok, Ld[:, None], 1.0), 0.0) * _TWO32 + 0.5
    rate = np.where(some, sd / np.where(some, fd, 1.0), 0.0) * _TWO32 + 0.5
    return _to_int_terms(share, ok), _to_int_terms(rate, some)


def expected(found, stale, best_height):
    """Per miner a dict of the nine joined sums (NAMES) over the runs, as Python ints (object arrays: no overflow)."""
    st, rt = terms(found, stale, best_height)
    f = np.asarray(found).astype(np.int64).astype(object)
    s = np.asarray(stale).astype(np.int64).astype(object)
    st, rt = st.astype(object), rt.astype(object)
    cols = {"found": f, "stale": s, "share": st, "rate": rt, "found_sq": f * f, "stale_sq": s * s,
            "found_stale": f * s, "share_sq": st * st, "rate_sq": rt * rt}
    tot = {name: a.sum(axis=0) for name, a in cols.items()}
    return [{name: int(tot[name][k]) for name in NAMES} for k in range(f.shape[1])]


def bin_of(t, lo, shift, bins):
    if t < lo:
        return 0
    q = (t - lo) >> shift
    return bins + 1 if q >= bins else 1 + q


def _bins(t, lo, shift, bins):
    """bin_of over a uint64 array."""
    below = t < np.uint64(lo)
    q = (np.where(below, np.uint64(lo), t) - np.uint64(lo)) >> np.uint64(shift)
    return np.where(below, 0, np.where(q >= np.uint64(bins), bins + 1, q.astype(np.int64) % (bins + 1) + 1)).astype(np.int64)


def expected_hist(found, stale, best_height, bins, share_shift, rate_shift, share_lo, rate_lo):
    """[M, 2, bins + 2] uint64 counts."""
    st, rt = terms(found, stale, best_height)
    m = st.shape[1]
    h = np.zeros((m, 2, bins + 2), dtype=np.uint64)
    for w, (t, lo, sh) in enumerate(((st, share_lo, share_shift), (rt, rate_lo, rate_shift))):
        b = _bins(t, lo, sh, bins)
        for k in range(m):
            h[k, w] = np.bincount(b[:, k], minlength=bins + 2).astype(np.uint64)
    return h


def diff(got, want):
    """Mismatches between two lists of dicts as strings naming the miner, the field and both integers."""
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} miners on the device, {len(want)} in the reference"]
    for k, (g, w) in enumerate(zip(got, want)):
        for name in NAMES:
            if int(g[name]) != int(w[name]):
                bad.append(f"miner {k} {name}: got {int(g[name])} reference {int(w[name])}")
    return bad


def _se(s1, s2, n, scale):
    """(mean, se^2) as Fractions: se^2 = (N S2 - S1^2) / (N^2 (N - 1)), scaled."""
    mean = Fraction(s1, n) * scale
    if n < 2:
        return mean, None
    return mean, Fraction(n * s2 - s1 * s1, n * n * (n - 1)) * scale * scale


def errors(mo, n):
    """One miner's msim_errors from its joined sums: a dict name -> (exact Fraction of the mean, or of the SQUARE
    of a standard error; None where it is NaN). Compare with rel_error()."""
    q = Fraction(1, ONE)
    out = {}
    out["found_mean"], out["found_se"] = _se(mo["found"], mo["found_sq"], n, Fraction(1))
    out["share_mean"], out["share_se"] = _se(mo["share"], mo["share_sq"], n, q)
    out["rate_mean"], out["rate_se"] = _se(mo["rate"], mo["rate_sq"], n, q)
    F, S = mo["found"], mo["stale"]
    out["pooled_rate"] = Fraction(S, F) if F else Fraction(0)
    if n < 2:
        out["pooled_rate_se"] = None
    elif F == 0:
        out["pooled_rate_se"] = Fraction(0)
    else:
        x = F * F * mo["stale_sq"] - 2 * S * F * mo["found_stale"] + S * S * mo["found_sq"]
        out["pooled_rate_se"] = Fraction(n * x, (n - 1) * F ** 4)
    return out


def rel_error(got, want, squared):
    """|got - v| / v for v = want (a Fraction), or v = sqrt(want) when `squared`; 0.0 when both are zero. The
    square root is taken in 200-bit integer arithmetic, far below the tolerance of any comparison."""
    if want == 0:
        return 0.0 if got == 0.0 else math.inf
    if squared:
        scale = 1 << 400
        root = Fraction(math.isqrt(want.numerator * scale // want.denominator), 1 << 200)
    else:
        root = want
    return float(abs(Fraction(got) - root) / root)

"""Exact reference of the device's cross sums and contrasts (msim_pair, msim_cross, msim_contrast), from per-run
counters.

Terms are tests/moments_reference.py's. The products and their sums are Python integers; the contrasts are
fractions.Fraction (the SQUARE of every standard error, as moments_reference.errors does), compared through
moments_reference.rel_error. A correlation is a signed square root, so it is given as (sign, square).

Plain NumPy and Python integers; nothing here imports the library under test."""
from fractions import Fraction

import numpy as np

import moments_reference as ref

NAMES = ("found_found", "stale_stale", "share_share", "rate_rate")
ONE = 1 << 32
FIELDS = ("found_diff", "found_diff_se", "found_corr", "found_ratio", "found_ratio_se",
          "stale_diff", "stale_diff_se", "stale_corr",
          "share_diff", "share_diff_se", "share_corr", "share_ratio", "share_ratio_se",
          "rate_diff", "rate_diff_se", "rate_corr")


def columns(data):
    """data: per point (found [n, M], stale [n, M], best_height [n]). Per point the four object arrays [n, M] of
    Python ints (found, stale, share_t, rate_t) every sum below is built from."""
    out = []
    for f, s, L in data:
        st, rt = ref.terms(f, s, L)
        out.append((np.asarray(f).astype(np.int64).astype(object), np.asarray(s).astype(np.int64).astype(object),
                    st.astype(object), rt.astype(object)))
    return out


def in_range(q, n_points, m):
    return q[0] < n_points and q[2] < n_points and q[1] < m and q[3] < m


def expected(cols, pairs):
    """Per pair a dict of the four joined cross sums (NAMES) over the runs; all zero for a pair outside the
    records."""
    n_points, m = len(cols), cols[0][0].shape[1]
    out = []
    for q in pairs:
        if not in_range(q, n_points, m):
            out.append({name: 0 for name in NAMES})
            continue
        pa, ma, pb, mb = q
        out.append({name: int((cols[pa][i][:, ma] * cols[pb][i][:, mb]).sum()) for i, name in enumerate(NAMES)})
    return out


def diff(got, want):
    """Mismatches between two lists of dicts as strings naming the pair, the field and both integers."""
    if len(got) != len(want):
        return [f"{len(got)} pairs on the device, {len(want)} in the reference"]
    return [f"pair {i} {name}: got {int(g[name])} reference {int(w[name])}"
            for i, (g, w) in enumerate(zip(got, want)) for name in NAMES if int(g[name]) != int(w[name])]


def _quantity(A, B, Saa, Sbb, Sab, n, scale, ratio):
    """diff; diff_se^2; corr as (sign, corr^2); ratio; ratio_se^2. None where the value is NaN."""
    out = [Fraction(A - B, n) * scale]
    if n < 2:
        out += [None, None]
    else:
        out.append(Fraction(n * (Saa - 2 * Sab + Sbb) - (A - B) ** 2, n * n * (n - 1)) * scale * scale)
        va, vb, cov = n * Saa - A * A, n * Sbb - B * B, n * Sab - A * B
        out.append(None if va == 0 or vb == 0 else ((cov > 0) - (cov < 0), Fraction(cov * cov, va * vb)))
    if ratio:
        out.append(Fraction(A, B) if B else None)
        out.append(None if (B == 0 or n < 2) else
                   Fraction(n * (B * B * Saa - 2 * A * B * Sab + A * A * Sbb), (n - 1) * B ** 4))
    return out


def contrast(mo_a, mo_b, cr, n):
    """One pair's msim_contrast from the sides' joined moments (moments_reference.expected dicts) and its joined
    cross sums: a dict over FIELDS."""
    q = Fraction(1, ONE)
    vals = (_quantity(mo_a["found"], mo_b["found"], mo_a["found_sq"], mo_b["found_sq"], cr["found_found"], n, 1, True) +
            _quantity(mo_a["stale"], mo_b["stale"], mo_a["stale_sq"], mo_b["stale_sq"], cr["stale_stale"], n, 1, False) +
            _quantity(mo_a["share"], mo_b["share"], mo_a["share_sq"], mo_b["share_sq"], cr["share_share"], n, q, True) +
            _quantity(mo_a["rate"], mo_b["rate"], mo_a["rate_sq"], mo_b["rate_sq"], cr["rate_rate"], n, q, False))
    return dict(zip(FIELDS, vals))


def field_error(name, got, want):
    """The relative error of one msim_contrast field against contrast()'s value (inf for a NaN mismatch)."""
    import math

    if want is None:
        return 0.0 if math.isnan(got) else math.inf
    if math.isnan(got):
        return math.inf
    if name.endswith("_corr"):
        sign, sq = want
        if sign == 0:
            return 0.0 if got == 0.0 else math.inf
        return ref.rel_error(got * sign, sq, squared=True) if got * sign > 0 else math.inf
    if name.endswith("_se"):
        return ref.rel_error(got, want, squared=True)
    if want < 0:
        return ref.rel_error(-got, -want, squared=False)
    return ref.rel_error(got, want, squared=False)

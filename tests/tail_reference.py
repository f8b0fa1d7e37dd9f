"""Exact reference of the device's tail statistics (msim_tail), from per-run counters.

An item is (cond_point, cond_column, quantity, target_point, target_column, reserved, value). Its key per run is one
of tests/rank_reference.py's four keys of the condition's record; the runs with key < value and key == value form the
two sets, and over each the target column's 20 msim_moments words are summed exactly as the device defines them: word
by word, the sum of every run's 32-bit pieces (no limb is normalised, so the 42 words are a property of the data).
The sides and mean_k are Python integers and fractions.Fraction.

Plain NumPy and Python integers; nothing here imports the library under test."""
from fractions import Fraction

import numpy as np

import moments_reference as ref
import rank_reference as rr

M32 = 0xFFFFFFFF
WORDS, MOM_WORDS = 42, 20
SIDES = ("below", "at_most", "above", "at_least")
# joined sums of 20 words: name -> [(word, shift)]
_JOIN = {"found": [(0, 0)], "stale": [(1, 0)], "share": [(2, 32), (3, 0)], "rate": [(4, 32), (5, 0)],
         "found_sq": [(6, 0), (7, 32)], "stale_sq": [(8, 0), (9, 32)], "found_stale": [(10, 0), (11, 32)],
         "share_sq": [(12 + i, 32 * i) for i in range(4)], "rate_sq": [(16 + i, 32 * i) for i in range(4)]}


def join(words20):
    """The nine sums of moments_reference.NAMES from 20 unnormalised words."""
    w = [int(x) for x in words20]
    return {name: sum(w[i] << sh for i, sh in parts) for name, parts in _JOIN.items()}


def addends(found, stale, best_height):
    """[n, M, 20] uint64: what one run's record adds to each msim_moments word (every addend is below 2^32)."""
    st, rt = ref.terms(found, stale, best_height)
    f = np.asarray(found).astype(np.uint64)
    s = np.asarray(stale).astype(np.uint64)
    fo, so, sto, rto = (x.astype(object) for x in (f, s, st, rt))
    cols = [fo, so, sto >> 32, sto & M32, rto >> 32, rto & M32]
    for prod in (fo * fo, so * so, fo * so):
        cols += [prod & M32, prod >> 32]
    for sq in (sto * sto, rto * rto):
        cols += [sq & M32, (sq >> 32) & M32, (sq >> 64) & M32, sq >> 96]
    out = np.stack([np.asarray(c, dtype=object) for c in cols], axis=-1)
    assert all(0 <= int(x) <= M32 for x in out.reshape(-1)[:: max(1, out.size // 997)])
    return out.astype(np.uint64)


def item_ok(item, n_points, m):
    cp, cc, q, tp, tc, reserved, _ = item
    return cp < n_points and tp < n_points and cc < m and tc < m and q < 4 and reserved == 0


class Reference:
    """found, stale [P, n, M] and best_height [P, n] (or [n, M] and [n] for one point)."""

    def __init__(self, found, stale, best_height):
        f, s, L = np.asarray(found), np.asarray(stale), np.asarray(best_height)
        if f.ndim == 2:
            f, s, L = f[None], s[None], L[None]
        self.n_points, self.n_runs, self.m = f.shape
        self.keys = [rr.keys(f[p], s[p], L[p]) for p in range(self.n_points)]       # [4, n, M] uint64
        self.add = [addends(f[p], s[p], L[p]) for p in range(self.n_points)]        # [n, M, 20] uint64

    def total(self, point, column):
        """The column's 20 words over all runs."""
        return [int(x) for x in self.add[point][:, column].sum(axis=0, dtype=np.uint64)]

    def words(self, item):
        """The item's 42 words; all zero for an item outside the records."""
        if not item_ok(item, self.n_points, self.m):
            return [0] * WORDS
        cp, cc, q, tp, tc, _, value = item
        key = self.keys[cp][q][:, cc]
        below, equal = key < np.uint64(value), key == np.uint64(value)
        a = self.add[tp][:, tc]
        return ([int(below.sum()), int(equal.sum())] + [int(x) for x in a[below].sum(axis=0, dtype=np.uint64)] +
                [int(x) for x in a[equal].sum(axis=0, dtype=np.uint64)])

    def all_words(self, items):
        return [self.words(it) for it in items]


def sides(words42, total20, n_runs):
    """{side: (20 words, run count)}: the complements are word-wise differences from the total."""
    nb, ne = words42[0], words42[1]
    b, e = words42[2:22], words42[22:42]
    return {"below": (list(b), nb), "at_most": ([x + y for x, y in zip(b, e)], nb + ne),
            "above": ([t - x - y for t, x, y in zip(total20, b, e)], n_runs - nb - ne),
            "at_least": ([t - x for t, x in zip(total20, b)], n_runs - nb)}


def mean_k(words42, total20, n_runs, k, upper=False):
    """(found, stale, share, rate) means over the k smallest (largest) runs as Fractions, share and rate scaled by
    2^-32, every tie weighted (k - n_strict) / n_equal; None when k lies outside the tie range."""
    sd = sides(words42, total20, n_runs)
    strict, n_strict = sd["above" if upper else "below"]
    ne = words42[1]
    if not n_strict < k <= n_strict + ne:
        return None
    s, e = join(strict), join(words42[22:42])
    out = []
    for name, scale in (("found", 1), ("stale", 1), ("share", 1 << 32), ("rate", 1 << 32)):
        out.append(Fraction(s[name] * ne + (k - n_strict) * e[name], k * ne * scale))
    return tuple(out)


def item_words(items):
    """[n, 8] uint32: msim_tail_item's memory layout."""
    out = np.zeros((len(items), 8), dtype=np.uint32)
    for i, (cp, cc, q, tp, tc, reserved, value) in enumerate(items):
        out[i] = (cp, cc, q, tp, tc, reserved, value & M32, value >> 32)
    return out


def thresholds(keys_column):
    """0, the column's minimum, its (upper) median, its maximum and 2^64 - 1."""
    srt = np.sort(np.asarray(keys_column))
    return [0, int(srt[0]), int(srt[len(srt) // 2]), int(srt[-1]), 2**64 - 1]


def make_items(r, with_bad=True):
    """Every column x quantity x threshold (0, minimum, median, maximum, 2^64 - 1), conditioned on itself and as the
    condition of another column at the last point; then the out-of-range items among valid neighbours."""
    P, m = r.n_points, r.m
    items = []
    for p in range(P):
        for k in range(m):
            for q in range(4):
                for v in thresholds(r.keys[p][q][:, k]):
                    items.append((p, k, q, p, k, 0, v))
                    items.append((p, k, q, P - 1 - p, (k + 1) % m, 0, v))
    if with_bad:
        v = items[0][6]
        items[3:3] = [(P, 0, 0, 0, 0, 0, v), (0, m, 0, 0, 0, 0, v)]
        items += [(0, 0, 4, 0, 0, 0, v), (0, 0, 0, P, 0, 0, v), (0, 0, 0, 0, m, 0, v), (0, 0, 0, 0, 0, 1, v),
                  (0, 0, 0, 0, 0, 0, v)]
    return items


def synthetic_points(n_points, n_runs, m, shift=0, seed=0):
    """rank_reference.synthetic per point, stacked: ([P, n, M], [P, n, M], [P, n])."""
    sets = [rr.synthetic(n_runs, m, shift=shift, seed=seed + 31 * p) for p in range(n_points)]
    return tuple(np.stack([x[i] for x in sets]) for i in range(3))


def diff(got, want):
    """Mismatches between two lists of 42-word rows as strings."""
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} items on the device, {len(want)} in the reference"]
    for i, (g, w) in enumerate(zip(got, want)):
        for j, (x, y) in enumerate(zip(g, w)):
            if int(x) != int(y):
                bad.append(f"item {i} word {j}: got {int(x)} reference {int(y)}")
    return bad

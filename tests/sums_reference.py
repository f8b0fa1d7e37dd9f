"""Exact reference of the device's fixed-point sums (msim_sums), from the oracle's per-run counters.

Every engine adds, per run and miner, the terms
    found, stale, (uint64)(share * 2^32 + 0.5), (uint64)(rate * 2^32 + 0.5)
with share = found / L and rate = stale / found, each ONE correctly rounded f64 division of two integers (0 where
found == 0; L = |best chain| - 1). The product by 2^32 is exact, the + 0.5 is one rounded f64 addition and the
conversion truncates, so NumPy's float64 gives every term bit for bit. A sum's combined value (hi << 32) + lo does
not depend on how the runs were split into waves, workgroups, slices or atomics: only the limb split moves. The
reference is therefore compared for exact integer equality.

Plain NumPy and Python integers; nothing here imports the library under test."""
import numpy as np

FIELDS = ("blocks_found", "stale_blocks", "share", "rate")
_TWO32 = 4294967296.0
_MASK64 = (1 << 64) - 1


def _terms(x):
    """(uint64)(x * 2^32 + 0.5) elementwise: x >= 0, so the truncating conversion is floor. Terms stay below 2^53
    (x < 2^21: no miner has 2^21 stale blocks per found block), where float64 -> uint64 is exact."""
    t = np.floor(x * _TWO32 + 0.5)
    assert np.isfinite(t).all() and (t < 2.0 ** 53).all()
    return t.astype(np.uint64)


def _columns(found, stale, st, rt):
    """Per miner (sum found, sum stale, sum share terms, sum rate terms); the terms are added as Python ints."""
    m = found.shape[1]
    return [(int(found[:, k].sum()), int(stale[:, k].sum()), sum(int(x) for x in st[:, k]), sum(int(x) for x in rt[:, k]))
            for k in range(m)]


def expected(found, stale, best_height):
    """Per miner the tuple (sum found, sum stale, sum share_term, sum rate_term) of runs given as found [n, M],
    stale [n, M] and best_height [n] (integers)."""
    f = np.asarray(found).astype(np.int64)
    s = np.asarray(stale).astype(np.int64)
    L = np.asarray(best_height).astype(np.int64)
    assert f.ndim == 2 and s.shape == f.shape and L.shape == (f.shape[0],)
    fd = f.astype(np.float64)
    some = f > 0
    # the divisors where found == 0 are replaced by 1: those quotients are discarded (and L may be 0 there)
    share = np.where(some, fd / np.where(some, L[:, None].astype(np.float64), 1.0), 0.0)
    rate = np.where(some, s.astype(np.float64) / np.where(some, fd, 1.0), 0.0)
    return _columns(f, s, _terms(share), _terms(rate))


def expected_from_doubles(found, stale, share, rate):
    """The same tuples from the oracle's own per-run doubles: for networks where sum(found) is not the best height
    (miners sharing an id, or holding Genesis's), the oracle's share is the authority."""
    f = np.asarray(found).astype(np.int64)
    s = np.asarray(stale).astype(np.int64)
    sh = np.asarray(share, dtype=np.float64)
    rt = np.asarray(rate, dtype=np.float64)
    assert f.ndim == 2 and s.shape == f.shape and sh.shape == f.shape and rt.shape == f.shape
    return _columns(f, s, _terms(sh), _terms(rt))


def combined(sums):
    """A list of MsimSums (anything with the six msim_sums fields), or an [M, 6] int64 tensor / array of them
    (uint64 limbs read as int64), as the tuples of expected(): limbs joined as (hi << 32) + lo."""
    out = []
    if hasattr(sums, "tolist"):
        for row in sums.tolist():
            fo, st, sh, sl, rh, rl = (int(x) for x in row)
            out.append((fo, st, ((sh & _MASK64) << 32) + (sl & _MASK64), ((rh & _MASK64) << 32) + (rl & _MASK64)))
        return out
    for x in sums:
        out.append((int(x.blocks_found), int(x.stale_blocks), (int(x.share_hi) << 32) + int(x.share_lo),
                    (int(x.rate_hi) << 32) + int(x.rate_lo)))
    return out


def diff(got, want, fields=range(4)):
    """The mismatches between two lists of tuples as strings naming the miner, the field and both integers."""
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} miners on the device, {len(want)} in the reference"]
    for k, (g, w) in enumerate(zip(got, want)):
        for i in fields:
            if g[i] != w[i]:
                bad.append(f"miner {k} {FIELDS[i]}: device {g[i]} reference {w[i]} (device - reference {g[i] - w[i]})")
    return bad

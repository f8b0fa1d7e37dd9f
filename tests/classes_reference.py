"""Exact reference of the device's class fold (MSIM_CLASS_NONE, msim_fold_launch), from per-run counters.

fold() adds the counters of each class's miners per run, modulo 2^32; its output feeds moments_reference.expected,
moments_reference.expected_hist and cross_reference as any launch's counters do (the best heights stay the runs' own).

Plain NumPy; nothing here imports the library under test."""
import numpy as np

NONE = 0xFFFFFFFF


def fold(found, stale, class_of, n_classes):
    """(found [n, C], stale [n, C]) uint32: per run the sums over the miners of each class, modulo 2^32. An entry
    that is NONE, or that is not below n_classes, belongs to no class."""
    f = np.asarray(found).astype(np.uint64)
    s = np.asarray(stale).astype(np.uint64)
    assert f.ndim == 2 and s.shape == f.shape and len(class_of) == f.shape[1]
    cf = np.zeros((f.shape[0], n_classes), dtype=np.uint64)
    cs = np.zeros((f.shape[0], n_classes), dtype=np.uint64)
    for k, c in enumerate(class_of):
        c = int(c)
        if 0 <= c < n_classes:
            cf[:, c] += f[:, k]
            cs[:, c] += s[:, k]
    mask = np.uint64(0xFFFFFFFF)
    return (cf & mask).astype(np.uint32), (cs & mask).astype(np.uint32)


def records(found, stale):
    """[n, M, 2] uint32 in msim_run_record's layout."""
    return np.ascontiguousarray(np.stack([found, stale], axis=-1).astype(np.uint32))


def maps(m, seed=0):
    """Named class maps (class_of, n_classes) of m miners that every fold test uses: one class, two classes, the
    identity, NONE entries with an entry outside the classes, one empty class, all miners but one in one class,
    and all NONE."""
    rng = np.random.default_rng(77 + seed + m)
    out = {"one": ([0] * m, 1), "identity": (list(range(m)), m), "all_none": ([NONE] * m, 1)}
    if m >= 2:
        out["two"] = ([k % 2 for k in range(m)], 2)
        out["all_but_one"] = ([0] * (m - 1) + [1], 2)
        with_none = [int(x) for x in rng.integers(0, 2, size=m)]
        with_none[0] = NONE
        with_none[m - 1] = 2  # not below n_classes: read as NONE
        out["with_none"] = (with_none, 2)
    if m >= 3:
        c = min(m, 4)
        out["one_empty"] = ([int(x) if x != 1 else 0 for x in rng.integers(0, c, size=m)], c)  # class 1 is empty
    return out

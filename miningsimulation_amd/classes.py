"""Miner classes: statistics of groups of miners (include/msim.h: MSIM_CLASS_NONE, msim_fold_launch,
msim_run_classes; kernel in csrc/msim_fold.hip).

The reference prints three means per miner (main.cpp:224-234); the questions a simulation is run for are about
groups: the 1 024 small miners of the two-pools network as one column, everyone but the selfish miner, miners 7 and
8 as one pool. A class total's variance, quantiles and paired contrasts need the per-run class sums, so the device
adds, per run, the records of each class's miners into one record per class; moments, histograms and cross sums of
those records follow from the kernels that serve single miners, and the per-run records never leave device memory.

A class map is one entry per miner: a class index below n_classes, or NONE for a miner in no class. A class's share
and stale rate are those of the class as one miner (one rounded division of the class's counts per run), not sums
of its members' terms."""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

from ._lib import MSIM_CLASS_NONE, MSIM_OK, lib

NONE = MSIM_CLASS_NONE


def classes_of(miners) -> Tuple[List[int], List[List[int]]]:
    """(class_of, members): miners with equal (perc, propagation_ms, is_selfish) share a class, classes numbered by
    first appearance. c5_network() gives classes of 1, 1 and 1 024 miners."""
    index, class_of, members = {}, [], []
    for k, mn in enumerate(miners):
        key = (mn.perc, mn.propagation_ms, bool(mn.is_selfish))
        if key not in index:
            index[key] = len(members)
            members.append([])
        class_of.append(index[key])
        members[index[key]].append(k)
    return class_of, members


def classes_from_groups(m: int, groups: Sequence[Sequence[int]]) -> Tuple[List[int], List[List[int]]]:
    """(class_of, members) from explicit lists of miner indices: class c holds groups[c] (it may be empty), every
    miner not listed is in no class (NONE). A miner outside 0..m-1 or listed twice is a ValueError."""
    if not 1 <= len(groups) <= m:
        raise ValueError(f"{len(groups)} classes for {m} miners")
    class_of = [NONE] * m
    for c, g in enumerate(groups):
        for k in g:
            if not 0 <= int(k) < m:
                raise ValueError(f"miner {k} outside 0..{m - 1}")
            if class_of[int(k)] != NONE:
                raise ValueError(f"miner {k} is listed twice")
            class_of[int(k)] = c
    return class_of, [sorted(int(k) for k in g) for g in groups]


def members_of(class_of: Sequence[int], n_classes: int) -> List[List[int]]:
    """The miners of each class of a map."""
    out = [[] for _ in range(n_classes)]
    for k, c in enumerate(class_of):
        if c != NONE:
            out[c].append(k)
    return out


def class_map_struct(class_of: Sequence[int], m: int, n_classes: int):
    """The map as a uint32 array, checked with msim_classes_check against m miners and n_classes classes."""
    if len(class_of) != m or any(not 0 <= int(c) <= 0xFFFFFFFF for c in class_of):
        raise ValueError(f"a class map has one uint32 entry per miner ({m})")
    arr = (ctypes.c_uint32 * m)(*[int(c) for c in class_of])
    if not 0 <= n_classes <= 0xFFFFFFFF or lib.msim_classes_check(m, arr, n_classes) != MSIM_OK:
        raise ValueError(f"1..{m} classes, and every entry below the class count ({n_classes}) or NONE")
    return arr


def class_count(class_of: Sequence[int]) -> int:
    """The smallest class count a map fits: one past its largest class (1 for a map that is all NONE)."""
    return max([int(c) + 1 for c in class_of if c != NONE], default=1)


def class_line(c: int, n_members: int, hashrate_pct: float, e: dict) -> str:
    """One class's report line (host/msim_main --classes prints the same) from its msim_errors fields."""
    from .moments import _pm

    return (f"  - Class {c} ({n_members} miners, {hashrate_pct:g}% of network hashrate) found "
            f"{e['found_mean']:g} ± {_pm(e['found_se'])} blocks i.e. {e['share_mean'] * 100:g}% ± "
            f"{_pm(e['share_se'], 100.0, '%')} of blocks. Stale rate: {e['rate_mean'] * 100:g}% ± "
            f"{_pm(e['rate_se'], 100.0, '%')}.")


def report_classes(miners, members: Sequence[Sequence[int]], result) -> str:
    """One line per class of a run_classes result: member count, total hashrate, then the class's mean found
    blocks, share and stale rate per run, each with its standard error."""
    from .moments import error_bars

    errs = error_bars(result)
    if len(errs) != len(members):
        raise ValueError(f"{len(errs)} classes in the result, {len(members)} member lists")
    total = sum(mn.perc for mn in miners)
    return "\n".join(class_line(c, len(g), sum(miners[k].perc for k in g) * 100.0 / total, e)
                     for c, (g, e) in enumerate(zip(members, errs)))

"""Multi-GPU sharding of runs: one process per GPU, one all-reduce of integer sums.

The reference's only parallelism is one std::async thread per run (main.cpp:205-220), with the per-miner
MinerStats summed on the main thread. Runs are independent and their seeds are a pure function of the run
index, so here rank r of W takes a contiguous run range and the ranks combine their per-miner sums with a
single all-reduce (backend "nccl" = RCCL over xGMI on MI355X; "gloo" in CPU tests). The sums are integers
(msim_sums: found, stale and Q32.32 fixed-point share/stale-rate limbs), so the result is bit-identical
for every W and every partition.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

FIXED_ONE = 4294967296.0  # 2^32: per-run share / stale_rate are summed as round(x * 2^32)


def shard(n_total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous partition of runs [0, n_total): rank r gets [begin, begin + n)."""
    base, rem = divmod(n_total, world)
    begin = rank * base + min(rank, rem)
    return begin, base + (1 if rank < rem else 0)


def fixed_point(x: float) -> Tuple[int, int]:
    """The device's per-run conversion (msim_kernels.hip): v = (uint64)(x * 2^32 + 0.5) -> (v >> 32, v & 0xffffffff)."""
    v = int(x * FIXED_ONE + 0.5)
    return v >> 32, v & 0xFFFFFFFF


def sums_rows_from_runs(found, stale, share, rate) -> List[List[int]]:
    """msim_sums rows [found, stale, share_hi, share_lo, rate_hi, rate_lo] from per-run values [n, M]."""
    n, m = found.shape
    rows = [[0] * 6 for _ in range(m)]
    for r in range(n):
        for k in range(m):
            sh, sl = fixed_point(float(share[r, k]))
            rh, rl = fixed_point(float(rate[r, k]))
            row = rows[k]
            row[0] += int(found[r, k])
            row[1] += int(stale[r, k])
            row[2] += sh
            row[3] += sl
            row[4] += rh
            row[5] += rl
    return rows


def allreduce_sums(local_rows, device=None):
    """SUM all-reduce of the [M, 6] int64 sums over the default process group; returns the global rows."""
    import torch
    import torch.distributed as dist

    t = torch.as_tensor(local_rows, dtype=torch.int64, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t)
    return t.cpu().tolist()


MAX_LAUNCH_RUNS = 1 << 26  # msim_launch's per-call limit (msim_api.hip); larger shards run in chunks


def run_sharded(sim, n_total: int, seed_base: int, run_begin: int = 0, stream=None,
                launch: Optional[Callable] = None, device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """This rank's shard through msim_launch on the current device, then one all-reduce (RCCL on GPUs) of the
    sums with the status words packed behind them.

    Returns the global [M, 6] int64 sums as a tensor on `device` (identical on every rank). `launch`
    replaces sim.launch (same signature, workspace None) so that the partition, chunking, status check and
    all-reduce can be exercised on CPU ranks with a gloo group (tests/test_distributed.py)."""
    import contextlib

    import torch
    import torch.distributed as dist

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    begin, n = shard(n_total, world, rank)
    m = len(sim.miners)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    # the sums and the two status words in one buffer: ONE all-reduce per job
    buf = torch.zeros(6 * m + 2, dtype=torch.int64, device=dev)
    sums = buf[: 6 * m].view(m, 6)
    status = buf[6 * m:]
    part = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    pst = torch.zeros(2, dtype=torch.int32, device=dev)
    chunk = min(n, max_chunk)
    ws = None
    if n and launch is None:
        ws = torch.empty(sim.workspace_bytes(chunk), dtype=torch.uint8, device=dev)
    # Everything that touches the launch's outputs runs on the launch stream: the adds read `part` / `pst`
    # after the kernels that wrote them, the next chunk's launch overwrites them only after the adds, and
    # the all-reduce (RCCL enqueues on the current stream) sees the final sums.
    # The buffers above were zeroed on the caller's current stream: the launch stream waits for that first.
    ctx = torch.cuda.stream(stream) if (stream is not None and dev.type == "cuda") else contextlib.nullcontext()
    if stream is not None and dev.type == "cuda":
        stream.wait_stream(torch.cuda.current_stream(dev))
    with ctx:
        for off in range(0, n, max(chunk, 1)):
            cn = min(chunk, n - off)
            (launch or sim.launch)(cn, run_begin + begin + off, seed_base, part, ws, pst, stream=stream)
            sums += part
            status += pst
        if world > 1:
            dist.all_reduce(buf)
    if stream is not None and dev.type == "cuda":
        torch.cuda.current_stream(dev).wait_stream(stream)  # the caller's stream sees the result
    if int(status[1].item()) != 0:
        raise RuntimeError(f"{int(status[1].item())} runs exceeded the compact state capacity")
    return sums


def run_sharded_moments(sim, n_total: int, seed_base: int, run_begin: int = 0, stream=None,
                        launch: Optional[Callable] = None, launch_moments: Optional[Callable] = None, device=None,
                        max_chunk: int = MAX_LAUNCH_RUNS, hist=None):
    """run_sharded plus the second moments (and, with a HistSpec `hist`, the histograms) of the per-run terms:
    every chunk runs msim_launch with device-resident records and then msim_moments_launch on the launch stream,
    and sums, status, moments and histogram travel in ONE int64 buffer with ONE all-reduce. All of them are
    integer sums over runs, so the result is bit-identical for every world size and partition.

    Returns a SimulationResult (stats_total, sums, moments, hist, n_runs = n_total), identical on every rank.
    `launch` / `launch_moments` replace sim.launch / sim.launch_moments (same signatures, workspace None) so
    that the partition, chunking, packing and all-reduce can be exercised on CPU ranks with a gloo group."""
    return _run_sharded_moments(sim, n_total, seed_base, run_begin, stream, launch, launch_moments, device, max_chunk,
                                hist, None, None)[0]


def run_sharded_contrasts(sim, n_total: int, seed_base: int, pairs, run_begin: int = 0, stream=None,
                          launch: Optional[Callable] = None, launch_moments: Optional[Callable] = None,
                          launch_cross: Optional[Callable] = None, device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """run_sharded_moments plus the cross sums of `pairs` (contrasts.Pair, every one within point 0 of `sim`): every
    chunk also runs msim_cross_launch on the launch stream, and the cross words are appended to the ONE int64
    buffer of the ONE all-reduce. They are integer sums over runs too, so the result is bit-identical for every
    world size and partition.

    Returns a ContrastResult (points = [the SimulationResult of run_sharded_moments], pairs, cross), identical on
    every rank. `launch_cross` replaces sim.launch_cross as `launch_moments` replaces sim.launch_moments."""
    from .contrasts import Pair
    from .simulation import ContrastResult

    pairs = [Pair(*q) for q in pairs]
    res, cross = _run_sharded_moments(sim, n_total, seed_base, run_begin, stream, launch, launch_moments, device,
                                      max_chunk, None, pairs, launch_cross)
    return ContrastResult(points=[res], pairs=pairs, cross=cross, n_runs=n_total)


def run_sharded_classes(sim, n_total: int, seed_base: int, class_of, n_classes: Optional[int] = None, pairs=None,
                        hist=None, run_begin: int = 0, stream=None, launch: Optional[Callable] = None,
                        launch_fold: Optional[Callable] = None, launch_moments: Optional[Callable] = None,
                        launch_cross: Optional[Callable] = None, device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """run_sharded_moments / run_sharded_contrasts per class of a class map (classes.classes_of,
    classes_from_groups): every chunk runs msim_launch, msim_fold_launch into a device-resident [chunk, n_classes]
    record buffer, then msim_moments_launch (and msim_cross_launch when `pairs` of (point 0, class) columns are
    given) on the folded records, and everything travels in the ONE int64 buffer of the ONE all-reduce. Integer
    sums over runs, so the result is bit-identical for every world size and partition.

    Returns what Simulation.run_classes returns: a SimulationResult (stats_total and sums per miner, moments and
    hist per class), inside a ContrastResult when pairs were given; identical on every rank. `launch_fold` replaces
    sim.launch_fold as `launch_moments` replaces the moments launch (same signatures; the moments and cross
    launches are given the folded records)."""
    from .classes import class_count, class_map_struct
    from .contrasts import Pair
    from .simulation import ContrastResult

    nc = class_count(class_of) if n_classes is None else int(n_classes)
    class_map_struct(class_of, len(sim.miners), nc)  # ValueError for a map that does not fit
    if pairs is not None:
        pairs = [Pair(*q) for q in pairs]
    res, cross = _run_sharded_moments(sim, n_total, seed_base, run_begin, stream, launch, launch_moments, device,
                                      max_chunk, hist, pairs, launch_cross, ([int(c) for c in class_of], nc, launch_fold))
    return res if pairs is None else ContrastResult(points=[res], pairs=pairs, cross=cross, n_runs=n_total)


def _run_sharded_moments(sim, n_total, seed_base, run_begin, stream, launch, launch_moments, device, max_chunk, hist,
                         pairs, launch_cross, classes=None):
    """(SimulationResult, cross sums or None): the body of run_sharded_moments, with the pairs' cross words behind
    the histogram in the same buffer when `pairs` is given. With `classes` = (class_of, n_classes, launch_fold or
    None) every chunk is folded first, and moments, histogram and cross sums have mc = n_classes columns."""
    import contextlib

    import torch
    import torch.distributed as dist

    from ._lib import MsimSums
    from .contrasts import CROSS_WORDS, cross_from_words, pairs_struct
    from .moments import MOMENT_WORDS, moments_from_words
    from .simulation import SimulationResult, _launch_cross, _launch_fold, _launch_moments, sums_to_stats

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    begin, n = shard(n_total, world, rank)
    m = len(sim.miners)
    mc = classes[1] if classes is not None else m
    row = hist.bins + 2 if hist is not None else 0
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    o_status, o_mom, o_hist = 6 * m, 6 * m + 2, 6 * m + 2 + MOMENT_WORDS * mc
    o_cross = o_hist + 2 * row * mc
    n_pairs = len(pairs) if pairs is not None else 0
    buf = torch.zeros(o_cross + CROSS_WORDS * n_pairs, dtype=torch.int64, device=dev)
    if pairs is not None:
        import numpy as np

        pairs_struct(pairs, 1, mc)  # ValueError for a pair outside the network
        d_pairs = torch.from_numpy(np.asarray(pairs, dtype=np.uint32).reshape(-1, 4).view(np.int32)).to(dev)
        pcross = torch.zeros((n_pairs, CROSS_WORDS), dtype=torch.int64, device=dev)
    part = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    pst = torch.zeros(2, dtype=torch.int32, device=dev)
    pmom = torch.zeros((mc, MOMENT_WORDS), dtype=torch.int64, device=dev)
    phist = torch.zeros((mc, 2, row), dtype=torch.int64, device=dev) if hist is not None else None
    chunk = min(n, max_chunk)
    rec = torch.zeros((max(chunk, 1), m, 2), dtype=torch.int32, device=dev)
    red = rec  # the records the reductions read
    if classes is not None:
        import numpy as np

        d_map = torch.from_numpy(np.asarray(classes[0], dtype=np.uint32).view(np.int32)).to(dev)
        red = torch.zeros((max(chunk, 1), mc, 2), dtype=torch.int32, device=dev)
        fold = classes[2] or sim.launch_fold
        # sim.launch_moments / launch_cross size their launches by the network; the folded records have mc columns
        launch_moments = launch_moments or (lambda cn, r, b, o, hs, oh, stream=None: _launch_moments(
            mc, 1, cn, r, b, o, hs, oh, stream))
        launch_cross = launch_cross or (lambda cn, r, b, q, nq, o, stream=None: _launch_cross(
            mc, 1, cn, r, b, q, nq, o, stream))
    bh = torch.zeros(max(chunk, 1), dtype=torch.int32, device=dev)
    ws = None
    if n and launch is None:
        ws = torch.empty(sim.workspace_bytes(chunk), dtype=torch.uint8, device=dev)
    # as in run_sharded: everything that touches the launches' outputs runs on the launch stream
    ctx = torch.cuda.stream(stream) if (stream is not None and dev.type == "cuda") else contextlib.nullcontext()
    if stream is not None and dev.type == "cuda":
        stream.wait_stream(torch.cuda.current_stream(dev))
    with ctx:
        for off in range(0, n, max(chunk, 1)):
            cn = min(chunk, n - off)
            (launch or sim.launch)(cn, run_begin + begin + off, seed_base, part, ws, pst, d_per_run=rec,
                                   d_best_height=bh, stream=stream)
            if classes is not None:
                fold(cn, rec, d_map, mc, red, stream=stream)
            (launch_moments or sim.launch_moments)(cn, red, bh, pmom, hist, phist, stream=stream)
            buf[:o_status] += part.view(-1)
            buf[o_status:o_mom] += pst
            buf[o_mom:o_hist] += pmom.view(-1)
            if hist is not None:
                buf[o_hist:o_cross] += phist.view(-1)
            if pairs is not None:
                (launch_cross or sim.launch_cross)(cn, red, bh, d_pairs, n_pairs, pcross, stream=stream)
                buf[o_cross:] += pcross.view(-1)
        if world > 1:
            dist.all_reduce(buf)
    if stream is not None and dev.type == "cuda":
        torch.cuda.current_stream(dev).wait_stream(stream)
    host = buf.cpu()
    if int(host[o_status + 1]) != 0:
        raise RuntimeError(f"{int(host[o_status + 1])} runs exceeded the compact state capacity")
    rows = host[:o_status].view(m, 6).tolist()
    u64 = (lambda v: int(v) & 0xFFFFFFFFFFFFFFFF)
    cross = cross_from_words(host[o_cross:].view(n_pairs, CROSS_WORDS).numpy()) if pairs is not None else None
    return SimulationResult(
        stats_total=sums_to_stats([[u64(x) for x in r] for r in rows]),
        sums=[MsimSums(r[0], r[1], u64(r[2]), u64(r[3]), u64(r[4]), u64(r[5])) for r in rows],
        n_runs=n_total,
        moments=moments_from_words(host[o_mom:o_hist].view(mc, MOMENT_WORDS).numpy()),
        hist=host[o_hist:o_cross].view(mc, 2, row).numpy().astype("uint64") if hist is not None else None,
    ), cross


def run_sharded_quantiles(sim, n_total: int, seed_base: int, qs=(0.05, 0.5, 0.95), ranks=None, run_begin: int = 0,
                          stream=None, launch: Optional[Callable] = None, launch_rank_begin: Optional[Callable] = None,
                          launch_rank_count: Optional[Callable] = None, launch_rank_step: Optional[Callable] = None,
                          device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """run_sharded plus the exact order statistics of the per-run terms over ALL n_total runs (quantiles.py): this
    rank's shard runs through msim_launch in chunks whose records stay resident in device buffers of their own; then
    msim_rank_begin_launch and, per pass, msim_rank_count_launch on every buffer, ONE all-reduce of the workspace's
    counts view, and msim_rank_step_launch. Ranks (quantile_rank of `qs`, or `ranks` as given) are relative to
    n_total. The digit counts are integer sums over runs and every rank steps on the same totals, so the result is
    identical on every rank and for every world size. The sums and status words travel behind the counts in the
    first pass's all-reduce: eight all-reduces per job.

    Returns a QuantileResult (points = [the SimulationResult of run_sharded's sums], order[0][miner][quantity][j]).
    `launch` / `launch_rank_begin` / `launch_rank_count` / `launch_rank_step` replace sim.launch and
    sim.launch_rank_* (same signatures, workspace None for the launch) so that the partition, the resident buffers
    and the eight all-reduces can be exercised on CPU ranks with a gloo group."""
    import contextlib

    import torch
    import torch.distributed as dist

    from ._lib import MsimSums
    from .quantiles import (RANK_PASSES, QuantileResult, order_stats_from_words, rank_counts_view, rank_workspace_bytes,
                            ranks_array, ranks_of)
    from .simulation import SimulationResult, sums_to_stats

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    begin, n = shard(n_total, world, rank)
    m = len(sim.miners)
    sel = ranks_of(n_total, qs, ranks)
    ranks_array(sel, n_total)  # ValueError for a rank that is not below n_total
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    ws_words = rank_workspace_bytes(m, 1, len(sel)) // 8
    c_off, c_words = rank_counts_view(m, 1, len(sel))
    assert c_off % 8 == 0 and c_off // 8 + c_words == ws_words  # the counts end the workspace
    # the workspace with the sums and the two status words behind its counts: they join the first all-reduce
    buf = torch.zeros(ws_words + 6 * m + 2, dtype=torch.int64, device=dev)
    d_ws = buf[:ws_words]
    sums = buf[ws_words:ws_words + 6 * m].view(m, 6)
    status = buf[ws_words + 6 * m:]
    part = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    pst = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.zeros((m, 4, len(sel), 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)
    chunk = min(n, max_chunk)
    ws = None
    if n and launch is None:
        ws = torch.empty(sim.workspace_bytes(chunk), dtype=torch.uint8, device=dev)
    kept = []
    ctx = torch.cuda.stream(stream) if (stream is not None and dev.type == "cuda") else contextlib.nullcontext()
    if stream is not None and dev.type == "cuda":
        stream.wait_stream(torch.cuda.current_stream(dev))
    with ctx:
        for off in range(0, n, max(chunk, 1)):
            cn = min(chunk, n - off)
            rec = torch.zeros((cn, m, 2), dtype=torch.int32, device=dev)
            bh = torch.zeros(cn, dtype=torch.int32, device=dev)
            (launch or sim.launch)(cn, run_begin + begin + off, seed_base, part, ws, pst, d_per_run=rec,
                                   d_best_height=bh, stream=stream)
            sums += part
            status += pst
            kept.append((cn, rec, bh))
        (launch_rank_begin or sim.launch_rank_begin)(sel, d_ws, stream=stream)
        for p in range(RANK_PASSES):
            for cn, rec, bh in kept:
                (launch_rank_count or sim.launch_rank_count)(cn, rec, bh, p, d_ws, stream=stream)
            if world > 1:
                dist.all_reduce(buf[c_off // 8:] if p == 0 else buf[c_off // 8:ws_words])
            (launch_rank_step or sim.launch_rank_step)(p, d_ws, out, rst, stream=stream)
    if stream is not None and dev.type == "cuda":
        torch.cuda.current_stream(dev).wait_stream(stream)
    host = buf[ws_words:].cpu()
    if int(host[6 * m + 1]) != 0:
        raise RuntimeError(f"{int(host[6 * m + 1])} runs exceeded the compact state capacity")
    if int(rst.cpu()[0]) != 0:
        raise RuntimeError("a rank was not below the run count")
    rows = host[:6 * m].view(m, 6).tolist()
    u64 = (lambda v: int(v) & 0xFFFFFFFFFFFFFFFF)
    res = SimulationResult(
        stats_total=sums_to_stats([[u64(x) for x in r] for r in rows]),
        sums=[MsimSums(r[0], r[1], u64(r[2]), u64(r[3]), u64(r[4]), u64(r[5])) for r in rows],
        n_runs=n_total,
    )
    return QuantileResult(points=[res], ranks=sel, qs=None if ranks is not None else [float(q) for q in qs],
                          order=order_stats_from_words(out.cpu().numpy(), 1, m, len(sel)), n_runs=n_total)


def run_sharded_tails(sim, n_total: int, seed_base: int, q=0.05, ranks=None, specs=None, run_begin: int = 0,
                      stream=None, launch: Optional[Callable] = None, launch_rank_begin: Optional[Callable] = None,
                      launch_rank_count: Optional[Callable] = None, launch_rank_step: Optional[Callable] = None,
                      launch_moments: Optional[Callable] = None, launch_tails: Optional[Callable] = None,
                      device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """run_sharded_quantiles plus the tail statistics at the selected order statistics (tails.py) over ALL n_total
    runs. Two things are added to that job. Every chunk also runs msim_moments_launch, and the columns' total moments
    ride behind the sums and status words in the first pass's all-reduce. After the last step every rank holds the
    same order statistics, builds the same items from `specs` (tails.own_tails by default), runs msim_tail_launch on
    each of its resident buffers and adds the words; ONE more all-reduce of the tails' words follows: nine
    all-reduces per job. Everything reduced is an integer sum over runs, so the result is identical on every rank
    and for every world size.

    Returns a TailResult. The `launch*` callables replace sim.launch, sim.launch_rank_*, sim.launch_moments and
    sim.launch_tails (same signatures, workspace None for the launch) so that CPU ranks with a gloo group can
    exercise the job."""
    import contextlib

    import numpy as np
    import torch
    import torch.distributed as dist

    from ._lib import MsimSums
    from .moments import MOMENT_WORDS
    from .quantiles import (RANK_PASSES, order_stats_from_words, quantile_rank, rank_counts_view, rank_workspace_bytes,
                            ranks_array)
    from .simulation import SimulationResult, sums_to_stats
    from .tails import TAIL_WORDS, _q_list, items_from_specs, items_words, make_result, own_tails, specs_struct

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    begin, n = shard(n_total, world, rank)
    m = len(sim.miners)
    qs = None if ranks is not None else _q_list(q)
    sel = [int(r) for r in ranks] if ranks is not None else [quantile_rank(n_total, x) for x in qs]
    ranks_array(sel, n_total)  # ValueError for a rank that is not below n_total
    specs, _ = specs_struct(own_tails(1, m) if specs is None else specs, 1, m, len(sel))
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    ws_words = rank_workspace_bytes(m, 1, len(sel)) // 8
    c_off, c_words = rank_counts_view(m, 1, len(sel))
    assert c_off % 8 == 0 and c_off // 8 + c_words == ws_words  # the counts end the workspace
    # the workspace with the sums, the two status words and the total moments behind its counts: they join the first
    # all-reduce
    o_status, o_mom = ws_words + 6 * m, ws_words + 6 * m + 2
    buf = torch.zeros(o_mom + MOMENT_WORDS * m, dtype=torch.int64, device=dev)
    d_ws = buf[:ws_words]
    sums = buf[ws_words:o_status].view(m, 6)
    status = buf[o_status:o_mom]
    moments = buf[o_mom:].view(m, MOMENT_WORDS)
    part = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    pst = torch.zeros(2, dtype=torch.int32, device=dev)
    pmom = torch.zeros((m, MOMENT_WORDS), dtype=torch.int64, device=dev)
    out = torch.zeros((m, 4, len(sel), 3), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)
    tails = torch.zeros((len(specs), TAIL_WORDS), dtype=torch.int64, device=dev)
    ptail = torch.zeros((len(specs), TAIL_WORDS), dtype=torch.int64, device=dev)
    chunk = min(n, max_chunk)
    ws = None
    if n and launch is None:
        ws = torch.empty(sim.workspace_bytes(chunk), dtype=torch.uint8, device=dev)
    kept = []
    ctx = torch.cuda.stream(stream) if (stream is not None and dev.type == "cuda") else contextlib.nullcontext()
    if stream is not None and dev.type == "cuda":
        stream.wait_stream(torch.cuda.current_stream(dev))
    with ctx:
        for off in range(0, n, max(chunk, 1)):
            cn = min(chunk, n - off)
            rec = torch.zeros((cn, m, 2), dtype=torch.int32, device=dev)
            bh = torch.zeros(cn, dtype=torch.int32, device=dev)
            (launch or sim.launch)(cn, run_begin + begin + off, seed_base, part, ws, pst, d_per_run=rec,
                                   d_best_height=bh, stream=stream)
            (launch_moments or sim.launch_moments)(cn, rec, bh, pmom, None, None, stream=stream)
            sums += part
            status += pst
            moments += pmom
            kept.append((cn, rec, bh))
        (launch_rank_begin or sim.launch_rank_begin)(sel, d_ws, stream=stream)
        for p in range(RANK_PASSES):
            for cn, rec, bh in kept:
                (launch_rank_count or sim.launch_rank_count)(cn, rec, bh, p, d_ws, stream=stream)
            if world > 1:
                dist.all_reduce(buf[c_off // 8:] if p == 0 else buf[c_off // 8:ws_words])
            (launch_rank_step or sim.launch_rank_step)(p, d_ws, out, rst, stream=stream)
        # the order statistics are the same on every rank, and so are the items built from them
        if int(rst.cpu()[0]) != 0:
            raise RuntimeError("a rank was not below the run count")
        order = order_stats_from_words(out.cpu().numpy(), 1, m, len(sel))
        items = items_from_specs(specs, order)
        d_items = torch.from_numpy(items_words(items).view(np.int32)).to(dev)
        for cn, rec, bh in kept:
            (launch_tails or sim.launch_tails)(cn, rec, bh, d_items, len(items), ptail, stream=stream)
            tails += ptail
        if world > 1:
            dist.all_reduce(tails)
    if stream is not None and dev.type == "cuda":
        torch.cuda.current_stream(dev).wait_stream(stream)
    host = buf[ws_words:].cpu()
    if int(host[6 * m + 1]) != 0:
        raise RuntimeError(f"{int(host[6 * m + 1])} runs exceeded the compact state capacity")
    rows = host[:6 * m].view(m, 6).tolist()
    u64 = (lambda v: int(v) & 0xFFFFFFFFFFFFFFFF)
    res = SimulationResult(
        stats_total=sums_to_stats([[u64(x) for x in r] for r in rows]),
        sums=[MsimSums(r[0], r[1], u64(r[2]), u64(r[3]), u64(r[4]), u64(r[5])) for r in rows],
        n_runs=n_total,
    )
    return make_result([res], sel, qs, order, n_total, specs, host[6 * m + 2:].numpy(), tails.cpu().numpy())


def run_sharded_bootstrap(sim, n_total: int, seed_base: int, items=None, qs=(0.05,), replicates: int = 200,
                          boot_seed: Optional[int] = None, run_begin: int = 0, stream=None,
                          launch: Optional[Callable] = None, launch_boot_weights: Optional[Callable] = None,
                          launch_boot_begin: Optional[Callable] = None, launch_boot_count: Optional[Callable] = None,
                          launch_boot_step: Optional[Callable] = None, launch_boot_below: Optional[Callable] = None,
                          device=None, max_chunk: int = MAX_LAUNCH_RUNS):
    """run_sharded plus the Poisson bootstrap of `items` (bootstrap.py) over ALL n_total runs: this rank's shard runs
    through msim_launch in chunks whose records stay resident, and every chunk adds its weights to W with
    msim_boot_weights_launch. W rides behind the sums and status words in the FIRST all-reduce; every rank then
    computes the same ranks from the complete W and begins the same workspace. Per pass msim_boot_count_launch runs on
    every resident buffer, ONE all-reduce of the workspace's counts view follows, and msim_boot_step_launch; after
    the last step msim_boot_below_launch runs on every buffer and ONE all-reduce adds the rows' s_hi and s_lo: ten
    all-reduces per job. A weight depends on the absolute run index alone and everything reduced is an integer sum
    over runs, so the result is identical on every rank and for every world size.

    Returns a BootstrapResult whose `order` is empty (replicate 0 of an item is its order statistic over all runs).
    The `launch*` callables replace sim.launch, bootstrap.launch_boot_weights and sim.launch_boot_* (same
    signatures, workspace None for the launch) so that CPU ranks with a gloo group can exercise the job."""
    import contextlib

    import torch
    import torch.distributed as dist

    from . import bootstrap as bs
    from ._lib import MsimSums
    from .quantiles import RANK_PASSES, quantile_rank
    from .simulation import SimulationResult, sums_to_stats

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    begin, n = shard(n_total, world, rank)
    m = len(sim.miners)
    B = int(replicates)
    qs = bs._check_call(n_total, qs, B)
    seed = bs.DEFAULT_BOOT_SEED if boot_seed is None else int(boot_seed) & (2 ** 64 - 1)
    items, _ = bs.items_struct(bs.own_bootstrap(1, m) if items is None else items, 1, m, len(qs))
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    ws_words = bs.boot_workspace_bytes(len(items), B) // 8
    c_off, c_words = bs.boot_counts_view(len(items), B)
    assert c_off % 8 == 0 and c_off // 8 + c_words == ws_words  # the counts end the workspace
    # the sums, the two status words and W in one buffer: the first all-reduce
    head = torch.zeros(6 * m + 2 + B, dtype=torch.int64, device=dev)
    sums, status, d_W = head[:6 * m].view(m, 6), head[6 * m:6 * m + 2], head[6 * m + 2:]
    part = torch.zeros((m, 6), dtype=torch.int64, device=dev)
    pst = torch.zeros(2, dtype=torch.int32, device=dev)
    d_ws = torch.zeros(ws_words, dtype=torch.int64, device=dev)
    rows = torch.zeros((len(items), B, bs.ROW_WORDS), dtype=torch.int64, device=dev)
    rst = torch.zeros(1, dtype=torch.int32, device=dev)
    chunk = min(n, max_chunk)
    ws = None
    if n and launch is None:
        ws = torch.empty(sim.workspace_bytes(chunk), dtype=torch.uint8, device=dev)
    kept = []
    ctx = torch.cuda.stream(stream) if (stream is not None and dev.type == "cuda") else contextlib.nullcontext()
    if stream is not None and dev.type == "cuda":
        stream.wait_stream(torch.cuda.current_stream(dev))
    with ctx:
        for off in range(0, n, max(chunk, 1)):
            cn = min(chunk, n - off)
            first = run_begin + begin + off
            rec = torch.zeros((cn, m, 2), dtype=torch.int32, device=dev)
            bh = torch.zeros(cn, dtype=torch.int32, device=dev)
            (launch or sim.launch)(cn, first, seed_base, part, ws, pst, d_per_run=rec, d_best_height=bh, stream=stream)
            (launch_boot_weights or bs.launch_boot_weights)(seed, first, cn, B, d_W, stream=stream)
            sums += part
            status += pst
            kept.append((cn, first, rec, bh))
        if world > 1:
            dist.all_reduce(head)
        W = [int(w) & (2 ** 64 - 1) for w in d_W.cpu().tolist()]  # complete, and the same on every rank
        (launch_boot_begin or sim.launch_boot_begin)(items, B, bs.boot_ranks(W, qs), len(qs), d_ws, stream=stream)
        for p in range(RANK_PASSES):
            for cn, first, rec, bh in kept:
                (launch_boot_count or sim.launch_boot_count)(cn, rec, bh, seed, first, len(items), B, p, d_ws, stream=stream)
            if world > 1:
                dist.all_reduce(d_ws[c_off // 8:])
            (launch_boot_step or sim.launch_boot_step)(len(items), B, p, d_ws, rows, rst, stream=stream)
        # every rank holds the same rows {value, below, equal, 0, 0}; the below words are sums over its own runs
        for cn, first, rec, bh in kept:
            (launch_boot_below or sim.launch_boot_below)(cn, rec, bh, seed, first, len(items), B, d_ws, rows, stream=stream)
        if world > 1:
            below = rows[:, :, 3:].contiguous()
            dist.all_reduce(below)
            rows[:, :, 3:] = below
    if stream is not None and dev.type == "cuda":
        torch.cuda.current_stream(dev).wait_stream(stream)
    host = head.cpu()
    if int(host[6 * m + 1]) != 0:
        raise RuntimeError(f"{int(host[6 * m + 1])} runs exceeded the compact state capacity")
    if int(rst.cpu()[0]) != 0:
        raise RuntimeError("a replicate's rank was not below its weight")
    srows = host[:6 * m].view(m, 6).tolist()
    u64 = (lambda v: int(v) & 0xFFFFFFFFFFFFFFFF)
    res = SimulationResult(
        stats_total=sums_to_stats([[u64(x) for x in r] for r in srows]),
        sums=[MsimSums(r[0], r[1], u64(r[2]), u64(r[3]), u64(r[4]), u64(r[5])) for r in srows],
        n_runs=n_total,
    )
    return bs.make_result([res], [quantile_rank(n_total, q) for q in qs], qs, [], n_total, items, B, seed, W,
                          rows.cpu().numpy())

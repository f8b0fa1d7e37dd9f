"""run_sharded_bootstrap under gloo with host stand-ins for the launches (the pattern of
tests/test_tails_distributed.py): world sizes 1, 2 and 3 over the same 257 runs give identical words, equal to the
reference, with ten all-reduces per job."""
import ctypes
import os
import socket

import numpy as np
import torch.multiprocessing as mp

import boot_reference as br
import rank_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TOTAL, M_SH, CHUNK, B = 257, 5, 60, 33
QS = (0.05, 0.5)
BOOT_SEED = 0x5EEDB007
RUN_BEGIN = 4000


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _tp(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib():
    import __graft_entry__ as ge

    path = os.path.join(ROOT, "build", "libboot_host.so")
    src = os.path.join(ROOT, "tests", "native", "boot_host.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        ge.build_boot_tests()
    h = ctypes.CDLL(path)
    for n in ("boot_host_weights", "boot_host_begin", "boot_host_count", "boot_host_step", "boot_host_below"):
        getattr(h, n).restype = ctypes.c_int
    return h


def _items():
    import miningsimulation_amd as msim

    return msim.own_bootstrap(1, M_SH, "share", 0) + msim.own_bootstrap(1, M_SH, "found", 1) + \
        msim.own_bootstrap(1, [1, 3], "rate", 1)


class _FakeSim:
    """Stands in for Simulation on a CPU rank: launch fills the records of the absolute runs [begin, begin + n) of one
    fixed synthetic data set (and their first sums); the bootstrap launches are the host library's mirrors on the
    same buffers."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = rr.synthetic(N_TOTAL, M_SH, shift=4, seed=11)
        self.h = _lib()
        self.count_launches = []

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        import moments_reference as ref

        assert ws is None and 0 < n <= CHUNK
        a = begin - RUN_BEGIN
        f, s, L = self.f[a:a + n], self.s[a:a + n], self.L[a:a + n]
        d_per_run[:n] = torch.from_numpy(rr.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        st, rt = ref.terms(f, s, L)
        tot = (lambda x: [int(v) for v in x.astype(object).sum(axis=0)])
        lo = np.uint64(0xFFFFFFFF)
        rows = [list(r) for r in zip(tot(f), tot(s), tot(st >> np.uint64(32)), tot(st & lo), tot(rt >> np.uint64(32)),
                                     tot(rt & lo))]
        sums.copy_(torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)))
        status.zero_()

    def launch_boot_weights(self, seed, run_begin, n, replicates, d_W, stream=None):
        assert self.h.boot_host_weights(ctypes.c_uint64(seed), ctypes.c_uint64(run_begin), ctypes.c_uint64(n),
                                        ctypes.c_uint32(replicates), _tp(d_W)) == 0

    def launch_boot_begin(self, items, replicates, ranks, n_q, d_ws, stream=None):
        iw = np.ascontiguousarray(np.asarray(items, dtype=np.uint32).reshape(-1, 4))
        rk = np.asarray(ranks, dtype=np.uint64)
        assert self.h.boot_host_begin(ctypes.c_uint32(M_SH), ctypes.c_uint32(1), _vp(iw), ctypes.c_uint32(len(items)),
                                      ctypes.c_uint32(replicates), _vp(rk), ctypes.c_uint32(n_q), _tp(d_ws)) == 0

    def launch_boot_count(self, n, d_per_run, d_best_height, seed, run_begin, n_items, replicates, pass_, d_ws,
                          stream=None):
        self.count_launches.append((pass_, n))
        assert self.h.boot_host_count(ctypes.c_uint32(M_SH), ctypes.c_uint32(1), ctypes.c_uint64(seed),
                                      ctypes.c_uint64(run_begin), ctypes.c_uint64(n), _tp(d_per_run), _tp(d_best_height),
                                      ctypes.c_uint32(n_items), ctypes.c_uint32(replicates), ctypes.c_uint32(pass_),
                                      _tp(d_ws)) == 0

    def launch_boot_step(self, n_items, replicates, pass_, d_ws, d_rows, d_status, stream=None):
        assert self.h.boot_host_step(ctypes.c_uint32(n_items), ctypes.c_uint32(replicates), ctypes.c_uint32(pass_),
                                     _tp(d_ws), _tp(d_rows), _tp(d_status)) == 0

    def launch_boot_below(self, n, d_per_run, d_best_height, seed, run_begin, n_items, replicates, d_ws, d_rows,
                          stream=None):
        assert self.h.boot_host_below(ctypes.c_uint32(M_SH), ctypes.c_uint32(1), ctypes.c_uint64(seed),
                                      ctypes.c_uint64(run_begin), ctypes.c_uint64(n), _tp(d_per_run), _tp(d_best_height),
                                      ctypes.c_uint32(n_items), ctypes.c_uint32(replicates), _tp(d_ws), _tp(d_rows)) == 0


def _run_fake():
    import torch

    from miningsimulation_amd.distributed import run_sharded_bootstrap

    sim = _FakeSim()
    res = run_sharded_bootstrap(sim, N_TOTAL, 1000, items=_items(), qs=QS, replicates=B, boot_seed=BOOT_SEED,
                                run_begin=RUN_BEGIN, launch=sim.launch, launch_boot_weights=sim.launch_boot_weights,
                                launch_boot_begin=sim.launch_boot_begin, launch_boot_count=sim.launch_boot_count,
                                launch_boot_step=sim.launch_boot_step, launch_boot_below=sim.launch_boot_below,
                                device=torch.device("cpu"), max_chunk=CHUNK)
    out = {"W": res.W, "rows": res.rows.tolist(), "ranks": res.ranks, "qs": res.qs, "n_runs": res.n_runs,
           "items": [tuple(i) for i in res.items],
           "sums": [[getattr(x, f) for f, _ in x._fields_] for x in res.points[0].sums],
           "se2": [str(res.variance(i)) for i in range(len(res.items))],
           "shortfall_se2": [str(res.variance(i, shortfall=True)) for i in range(len(res.items))]}
    return out, [n for p, n in sim.count_launches if p == 0]


def _worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce

    def counted(t, *a, **kw):
        calls.append(t.numel())
        return real(t, *a, **kw)

    dist.all_reduce = counted
    try:
        res, launches = _run_fake()
    finally:
        dist.all_reduce = real
    out_q.put((rank, res, launches, calls))
    dist.destroy_process_group()


def _spawn(world):
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def test_gloo_run_sharded_bootstrap_is_the_same_for_every_world_size(msim_lib_path):
    from miningsimulation_amd import quantile_rank

    _lib()
    want, launches = _run_fake()  # no process group: world 1
    f, s, L = rr.synthetic(N_TOTAL, M_SH, shift=4, seed=11)
    items = [tuple(it) for it in _items()]
    W, rows = br.bootstrap([br.point_keys(f, s, L)], items, QS, B, BOOT_SEED, RUN_BEGIN)
    assert want["W"] == W and W[0] == N_TOTAL == want["n_runs"]
    assert not br.diff_rows(want["rows"], rows)
    assert want["ranks"] == [quantile_rank(N_TOTAL, q) for q in QS] and want["items"] == items
    for i, it in enumerate(items):
        assert want["se2"][i] == str(br.variance([r[0] for r in rows[i]]))
        assert want["shortfall_se2"][i] == str(br.variance([br.shortfall(r, W[b], QS[it[3]]) for b, r in enumerate(rows[i])]))
    assert launches == [60, 60, 60, 60, 17]  # five resident buffers

    n_items = len(items)
    for world in (2, 3):
        for rank, res, launches, calls in _spawn(world):
            assert res == want, (world, rank)
            # the sums, status words and W first; eight of the counts view; one of the rows' s_hi and s_lo
            assert calls == [6 * M_SH + 2 + B] + [n_items * B * 256] * 8 + [n_items * B * 2], (world, rank, calls)
            assert sum(launches) in (N_TOTAL // world, N_TOTAL // world + 1) and max(launches) <= CHUNK

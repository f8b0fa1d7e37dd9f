"""run_sharded_tails under gloo with host stand-ins for the launches (the pattern of tests/test_rank_host.py's sharded
quantiles): world sizes 1, 2 and 3 over the same 257 runs give identical TailResults, equal to the reference, with
nine all-reduces per job."""
import ctypes
import os
import socket

import numpy as np
import torch.multiprocessing as mp

import rank_reference as rr
import tail_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TOTAL, M_SH, CHUNK = 257, 5, 60
Q = 0.05


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _tp(t):
    return ctypes.c_void_p(t.data_ptr())


def _libs():
    import __graft_entry__ as ge

    paths = [os.path.join(ROOT, "build", n) for n in ("librank_host.so", "libtail_host.so", "libmoments_host.so")]
    for p, build in zip(paths, (ge.build_rank_tests, ge.build_tail_tests, ge.build_moments_tests)):
        if not os.path.exists(p):
            build()
    libs = [ctypes.CDLL(p) for p in paths]
    for h, names in zip(libs, (("rank_host_begin", "rank_host_count", "rank_host_step"), ("tail_host_accumulate",),
                               ("moments_host_accumulate",))):
        for n in names:
            getattr(h, n).restype = ctypes.c_int
    return libs


def _specs():
    import miningsimulation_amd as msim

    return msim.own_tails(1, M_SH) + msim.tails_given(0, 4, "found", M_SH) + msim.tails_given(0, 2, "rate", M_SH)


class _FakeSim:
    """Stands in for Simulation on a CPU rank: launch fills the records of runs [begin, begin + n) of one fixed
    synthetic data set (and their first sums); the rank, moments and tail launches are the host libraries' functions on
    the same buffers."""

    miners = list(range(M_SH))

    def __init__(self):
        self.f, self.s, self.L = rr.synthetic(N_TOTAL, M_SH, shift=4, seed=11)
        self.rank, self.tail, self.mom = _libs()
        self.tail_launches = []

    def launch(self, n, begin, seed_base, sums, ws, status, d_per_run=None, d_best_height=None, stream=None):
        import torch

        import moments_reference as ref

        assert ws is None and 0 < n <= CHUNK
        f, s, L = self.f[begin:begin + n], self.s[begin:begin + n], self.L[begin:begin + n]
        d_per_run[:n] = torch.from_numpy(rr.records(f, s).view(np.int32))
        d_best_height[:n] = torch.from_numpy(L.view(np.int32))
        st, rt = ref.terms(f, s, L)
        tot = (lambda a: [int(x) for x in a.astype(object).sum(axis=0)])
        lo = np.uint64(0xFFFFFFFF)
        rows = [list(r) for r in zip(tot(f), tot(s), tot(st >> np.uint64(32)), tot(st & lo), tot(rt >> np.uint64(32)),
                                     tot(rt & lo))]
        sums.copy_(torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)))
        status.zero_()

    def launch_moments(self, n, d_per_run, d_best_height, d_moments, hist_spec, d_hist, stream=None):
        assert hist_spec is None and d_hist is None
        assert self.mom.moments_host_accumulate(_tp(d_per_run), _tp(d_best_height), ctypes.c_uint64(n),
                                                ctypes.c_uint32(M_SH), None, _tp(d_moments), None) == 0

    def launch_rank_begin(self, ranks, d_ws, stream=None):
        rk = np.asarray(ranks, dtype=np.uint64)
        assert self.rank.rank_host_begin(ctypes.c_uint32(M_SH), _vp(rk), ctypes.c_uint32(len(ranks)), _tp(d_ws)) == 0

    def launch_rank_count(self, n, d_per_run, d_best_height, pass_, d_ws, stream=None):
        assert self.rank.rank_host_count(_tp(d_per_run), _tp(d_best_height), ctypes.c_uint64(n), ctypes.c_uint32(M_SH),
                                         ctypes.c_uint32(pass_), _tp(d_ws)) == 0

    def launch_rank_step(self, pass_, d_ws, d_out, d_status, stream=None):
        assert self.rank.rank_host_step(ctypes.c_uint32(M_SH), ctypes.c_uint32(pass_), _tp(d_ws), _tp(d_out),
                                        _tp(d_status)) == 0

    def launch_tails(self, n, d_per_run, d_best_height, d_items, n_items, d_tails, stream=None):
        self.tail_launches.append(n)
        assert self.tail.tail_host_accumulate(_tp(d_per_run), _tp(d_best_height), ctypes.c_uint32(1), ctypes.c_uint64(n),
                                              ctypes.c_uint32(M_SH), _tp(d_items), ctypes.c_uint32(n_items),
                                              _tp(d_tails)) == 0


def _run_fake():
    import torch

    from miningsimulation_amd.distributed import run_sharded_tails

    sim = _FakeSim()
    res = run_sharded_tails(sim, N_TOTAL, 1000, q=Q, specs=_specs(), launch=sim.launch,
                            launch_rank_begin=sim.launch_rank_begin, launch_rank_count=sim.launch_rank_count,
                            launch_rank_step=sim.launch_rank_step, launch_moments=sim.launch_moments,
                            launch_tails=sim.launch_tails, device=torch.device("cpu"), max_chunk=CHUNK)
    out = {"order": [[[list(o) for o in row] for row in col] for col in res.order[0]], "ranks": res.ranks, "qs": res.qs,
           "sums": [[getattr(x, f) for f, _ in x._fields_] for x in res.points[0].sums], "n_runs": res.n_runs,
           "tail_words": res.tail_words.tolist(), "moment_words": res.moment_words.tolist(), "tails": res.tails,
           "moments": res.moments, "items": [tuple(i) for i in res.items],
           "means": [list(res.means(i).values()) for i in range(len(res.specs))],
           "shortfall": [str(res.expected_shortfall(k)) for k in range(M_SH)]}
    return out, sim.tail_launches


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


def test_gloo_run_sharded_tails_is_the_same_for_every_world_size(msim_lib_path):
    from miningsimulation_amd import quantile_rank

    _libs()
    want, launches = _run_fake()  # no process group: world 1
    f, s, L = rr.synthetic(N_TOTAL, M_SH, shift=4, seed=11)
    r = tr.Reference(f, s, L)
    specs = _specs()
    assert want["ranks"] == [quantile_rank(N_TOTAL, Q)] == [12] and want["n_runs"] == N_TOTAL
    assert not rr.diff(want["order"], rr.select(f, s, L, want["ranks"]))
    items = [(cp, cc, q, tp, tc, 0, v) for cp, cc, q, tp, tc, v in want["items"]]
    assert [it[6] for it in items] == [want["order"][sp.cond_column][sp.quantity][0][0] for sp in specs]
    assert not tr.diff(want["tail_words"], r.all_words(items))
    assert want["moment_words"] == [[r.total(0, k) for k in range(M_SH)]]
    for sp, row in zip(specs, want["tail_words"]):
        assert row[:2] == want["order"][sp.cond_column][sp.quantity][0][1:]   # n_below, n_equal = below, equal
    for i, sp in enumerate(specs):
        assert want["means"][i] == [float(x) for x in tr.mean_k(want["tail_words"][i], r.total(0, sp.target_column),
                                                                N_TOTAL, 13)]
    assert launches == [60, 60, 60, 60, 17]  # five resident buffers

    words = M_SH * 4 * 256
    for world in (2, 3):
        for rank, res, launches, calls in _spawn(world):
            assert res == want, (world, rank)
            # eight all-reduces of the counts view, the sums, status words and total moments behind the first; then
            # one of the tails' words
            assert calls == [words + 6 * M_SH + 2 + 20 * M_SH] + [words] * 7 + [42 * len(specs)], (world, rank, calls)
            assert sum(launches) in (N_TOTAL // world, N_TOTAL // world + 1) and max(launches) <= CHUNK

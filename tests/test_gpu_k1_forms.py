"""The draw kernel's own forms on the device (msim_fastdraw.h "K1's form", msim_drawgen.hip): its interval chain on
crafted inputs bit for bit against the host, and the pipeline built on it against the oracle for the
uniform-delay instantiation (c2), the per-finder one (three different delays), one miner and fifteen."""
import ctypes
import subprocess

import numpy as np
import pytest

import k1_native
import sums_reference

pytestmark = pytest.mark.gpu

D = 31_556_952_000
MONTH = 30 * 86_400_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def test_gpu_k1_intervals_crafted(msim, tmp_path):
    """msim_device_intervals (K1's fast form, then the general form, then glibc's sequence; every eighth input the
    general tables' chain) on the crafted set of tests/native/fastdraw2_check.cpp: inputs within +-4 ns of a
    millisecond boundary, every exponent x table column x (first, middle, last mantissa), u = 0, 2^64 - 1 and
    bit 11 alone. Expected values: glibc's on the host, which the host build of the same chain reproduces
    (tests/test_fastdraw2.py)."""
    import torch
    from miningsimulation_amd import _lib

    path = tmp_path / "crafted.bin"
    subprocess.run([k1_native.ensure()["fastdraw2_check"], "crafted", str(path)], check=True)
    rec = np.fromfile(path, dtype=np.uint64).reshape(-1, 2)
    assert 5_000 < rec.shape[0] < 20_000
    u = np.repeat(rec[:, 0], 8)  # eight consecutive copies: every input meets both chains' lanes
    du = torch.from_numpy(u.view(np.int64).copy()).cuda()
    di = torch.empty(u.size, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib.msim_device_intervals(ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(di.data_ptr()), u.size, None))
    torch.cuda.synchronize()
    got = di.cpu().numpy().view(np.uint64).reshape(-1, 8)
    bad = np.nonzero((got != rec[:, 1:2]).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], rec[bad[:8]], got[bad[:8]])


def _parity(msim, oracle, percs, props, duration, n, begin=0, seed=1000):
    miners = [msim.Miner(k, percs[k], props[k], False) for k in range(len(percs))]
    res = msim.Simulation(miners, duration).run(n, begin, seed, 0, per_run=True)
    f, st, sh, r = oracle.run_batch(percs, props, [0] * len(percs), duration, n, begin, seed, threads=16)
    assert np.array_equal(res.found.astype(np.int64), f), (percs, props)
    assert np.array_equal(res.stale.astype(np.int64), st), (percs, props)
    bad = sums_reference.diff(sums_reference.combined(res.sums), sums_reference.expected(f, st, f.sum(axis=1)))
    assert not bad, (percs, props, bad[:8])


@pytest.mark.parametrize("name,percs,props", [
    ("c2_uniform", H, [100] * 9),
    ("three_delays", H, [100, 100, 100, 1000, 1000, 1000, 10_000, 10_000, 0]),
    ("one_miner", [100], [1000]),
    ("fifteen_miners", [7] * 14 + [2], [250] * 15),
])
def test_gpu_k1_pipeline_month(msim, oracle, name, percs, props):
    """512 runs x 1 month: counters run by run and the fixed-point sums against the oracle."""
    _parity(msim, oracle, percs, props, MONTH, 512, begin=2048)


def test_gpu_k1_pipeline_year(msim, oracle):
    """256 runs x 1 year of c2: a full band segment and every segment's jump."""
    _parity(msim, oracle, H, [100] * 9, D, 256, begin=8192)

"""The draw kernel's hot quad on the device (msim_pipeline.h K1Draws::quad_fast / quad_exact on the packed interval
form and the high-word picker, msim_fastdraw.h) from crafted stream states, word for word against sequential
rng_next + interval_ms_of + PickFinder's index on the host, in both instantiations; and the pipeline built on it
against the oracle on a network with no propagation delay.

A network whose percentages sum below 100 cannot be created (msim_config_create returns MSIM_E_WEIGHTS: the
reference asserts there), so PickFinder's fall-through (owner 15) is reached here the way a valid network
reaches it: picker draws in the top sixteen values, index 100, crafted into the quads at every position."""
import ctypes
import subprocess

import numpy as np
import pytest

import k1pack_native
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


@pytest.fixture(scope="module")
def quads(tmp_path_factory):
    """Crafted quads (tests/native/k1pack_check.cpp write_quads): the interval stream produces, at each of the four
    positions, inputs within +-4 ns of a millisecond boundary, low-exponent inputs, u = 0 and u = 2^64 - 1; the
    picker stream produces draws in the rare band and just below it, with and without a carry out of the low
    halves, and the top of the range. Positions 2-4 are reached by stepping the crafted state back."""
    path = tmp_path_factory.mktemp("k1quads") / "quads.bin"
    subprocess.run([k1pack_native.ensure(), "quads", str(path)], check=True)
    raw = np.fromfile(path, dtype=np.uint8).reshape(-1, 64)
    states = raw[:, :32].copy().view(np.uint64).reshape(-1, 4)
    want = raw[:, 32:].copy().view(np.uint32).reshape(-1, 8)
    assert 2_000 < states.shape[0] < 5_000
    assert (want[:, 4:] == 100).any(axis=0).all()  # the fall-through index at every position
    return states, want


@pytest.mark.parametrize("name,percs,props", [
    ("uniform", H, [100] * 9),                                                    # msim_draws_kernel<true>'s form
    ("per_finder", H, [100, 100, 100, 1000, 1000, 1000, 10_000, 10_000, 0]),      # <false>'s
])
def test_gpu_k1_quads_crafted(msim, quads, name, percs, props):
    import torch
    from miningsimulation_amd import _lib

    states, want = quads
    n = states.shape[0]
    sim = msim.Simulation([msim.Miner(k, percs[k], props[k], False) for k in range(len(percs))], D)
    fn = _lib.lib.msim_device_k1_quads
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    ds = torch.from_numpy(states.view(np.int64).copy()).cuda()
    do = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
    _lib.check(fn(sim.handle, ctypes.c_void_p(ds.data_ptr()), ctypes.c_void_p(do.data_ptr()), n, None))
    torch.cuda.synchronize()
    got = do.cpu().numpy().view(np.uint32)
    # finder of a PickFinder index: the first miner whose cumulative percentage exceeds it, 15 when none does
    finder = np.full(101, 15, dtype=np.uint32)
    finder[:100] = np.searchsorted(np.cumsum(percs), np.arange(100), side="right")
    exp = want.copy()
    exp[:, 4:] = finder[want[:, 4:]]
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (name, bad[:8], states[bad[:8]], exp[bad[:8]], got[bad[:8]])


def test_gpu_k1_pipeline_month_no_delay(msim, oracle):
    """512 runs x 1 month of a network with 0 ms delays (only a 0 ms interval makes a block slow): counters run by
    run and the fixed-point sums against the oracle."""
    percs, props = H, [0] * 9
    miners = [msim.Miner(k, percs[k], props[k], False) for k in range(len(percs))]
    res = msim.Simulation(miners, MONTH).run(512, 4096, 1000, 0, per_run=True)
    f, st, sh, r = oracle.run_batch(percs, props, [0] * len(percs), MONTH, 512, 4096, 1000, threads=16)
    assert np.array_equal(res.found.astype(np.int64), f)
    assert np.array_equal(res.stale.astype(np.int64), st)
    bad = sums_reference.diff(sums_reference.combined(res.sums), sums_reference.expected(f, st, f.sum(axis=1)))
    assert not bad, bad[:8]

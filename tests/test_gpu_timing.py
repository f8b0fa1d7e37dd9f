"""Stage timing (msim_timing_enable / msim_timing_read_all) around each branch of msim_launch: the honest
pipeline, the entity engine, the large-network pipeline and the general engine. Timing brackets every launch
with HIP events on the launch stream (draw kernels and the entity engine get brackets of their own inside it),
and must not change what a launch computes."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DAY = 86_400_000

# name -> (uses_pipeline of msim_pipeline_info, has a draw stage, has an entity-engine stage)
BRANCHES = {
    "pipeline": (1, True, False),
    "entity": (3, False, True),
    "wide": (2, True, False),
    "general": (4, False, False),
}


@pytest.fixture(scope="module")
def msim(msim_lib_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as m

    return m


def _network(msim, name, monkeypatch):
    """(Simulation, runs): one small network per branch of msim_launch."""
    if name == "wide":
        return msim.Simulation(msim.c5_network(), 30 * DAY, total_weight=msim.C5_TOTAL_WEIGHT), 16
    if name == "general":
        monkeypatch.setenv("MSIM_FORCE_GENERAL", "1")  # read when the config is created
    return msim.Simulation(msim.PRESETS["c3" if name == "entity" else "c2"](), DAY), 256


def _int_sums(res):
    return [tuple(getattr(s, f) for f, _ in s._fields_) for s in res.sums]


@pytest.mark.parametrize("name", list(BRANCHES))
def test_gpu_timing_brackets(msim, monkeypatch, name):
    path, draws, engine = BRANCHES[name]
    sim, n = _network(msim, name, monkeypatch)
    assert sim.pipeline_info(n)["uses_pipeline"] == path
    slices = -(-n // sim.pipeline_info(n)["slice_runs"])  # one draw or engine bracket per slice of a launch
    want = _int_sums(sim.run(n, 0, 1000, 0))  # timing off
    t0 = time.perf_counter()
    msim.timing_enable(True)
    try:
        timed = [_int_sums(sim.run(n, 0, 1000, 0)) for _ in range(2)]
        t = msim.timing_read()
        again = msim.timing_read()
        window_ms = (time.perf_counter() - t0) * 1e3
    finally:
        msim.timing_enable(False)
    print(name, {k: repr(v) for k, v in t.items()})
    assert t["launches"] == 2
    # the draw and engine brackets nest inside the launch bracket on one stream
    assert t["launch_ms"] > 0
    assert t["launch_ms"] >= t["draws_ms"]
    assert t["launch_ms"] >= t["engine_ms"]
    assert (t["draws_ms"] > 0) == draws
    assert (t["engine_ms"] > 0) == engine
    # Busy time is the union of the intervals that the summed time adds up, so it cannot exceed the sum, up to
    # float32 rounding: hipEventElapsedTime returns float32 milliseconds, the union takes both ends of a bracket
    # against the first event (two roundings of at most half an ulp at the window's length) and the sum takes the
    # bracket's length directly (one more, smaller). Per bracket that is at most 1.5 ulp of the time since
    # timing_enable; a stage has at most `slices` brackets per launch.
    slack = 2 * slices * 1.5 * float(np.spacing(np.float32(window_ms)))
    for stage in ("draws", "engine", "launch"):
        assert t[stage + "_busy_ms"] <= t[stage + "_ms"] + slack, (stage, slack)
    assert timed == [want, want]  # timing does not change the integer sums
    assert again["launches"] == 0 and all(v == 0 for v in again.values())  # a read consumes the events

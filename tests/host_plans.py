"""What the host side of the C ABI plans, without a device: tests/golden/host_plans.json and its generator.

compute() asks the library, through the host-only entry points (msim_workspace_bytes, msim_pipeline_info,
msim_sweep_create_ex, msim_sweep_info, msim_sweep_workspace_bytes, msim_sweep_group_of), for the plan of a list of
single networks and sweeps, under the test switches that change a plan. tests/test_host_plans.py compares it with the
recorded file for equality: a change of the host code that moves a slice size, a workspace size, an engine or a draw
group shows there.

The file is recorded from the commit BEFORE a change of the host code, never from the code under test:

    python tests/host_plans.py            # rewrites tests/golden/host_plans.json

MSIM_K1_SLOTS is pinned, so the plan does not depend on whether a device is visible."""
import contextlib
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_plans.json")

Y = 31_556_952_000
DAY = 86_400_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]
PIN = {"MSIM_K1_SLOTS": "8192"}
# every switch that changes a plan: cleared unless a case sets it
SWITCHES = ("MSIM_K1_SLOTS", "MSIM_SELSEG", "MSIM_SEG_NSEG", "MSIM_MAX_SLICE_RUNS", "MSIM_PIPE_TEST_CAP",
            "MSIM_PIPE_TEST_LCAP", "MSIM_PIPE_TEST_POINT_CAP", "MSIM_PIPE_TEST_POINT_LCAP", "MSIM_PIPE_TEST_K2_KIND",
            "MSIM_WIDE_TEST_RCAP", "MSIM_WIDE_TEST_POINT_RCAP", "MSIM_FORCE_WIDE", "MSIM_FORCE_GENERAL",
            "MSIM_NO_PIPELINE", "MSIM_SWEEP_SHARED_MAX_GROUP", "MSIM_GEN_TEST_LANES", "MSIM_GEN_TEST_CAP1",
            "MSIM_GEN_TEST_CAP2", "MSIM_GEN_TEST_CAP3", "MSIM_GEN_TEST_LIST_CAP")

CONFIG_RUNS = (1, 257, 32_768, 1 << 22, 1 << 26)
SWEEP_RUNS = (257, 8_192, 1 << 20)
MAX_SLICE = {"MSIM_MAX_SLICE_RUNS": "256"}
PIPE_TEST = {"MSIM_PIPE_TEST_CAP": "1", "MSIM_PIPE_TEST_LCAP": "1024", "MSIM_PIPE_TEST_K2_KIND": "1"}
WIDE_TEST = {"MSIM_WIDE_TEST_RCAP": "8"}
SWEEP_TEST = {"MSIM_MAX_SLICE_RUNS": "256", "MSIM_PIPE_TEST_POINT_CAP": "1", "MSIM_WIDE_TEST_POINT_RCAP": "4"}


@contextlib.contextmanager
def _env(extra=None):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(PIN)
    os.environ.update(extra or {})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _net(msim, w, props, ids=None):
    return [msim.Miner(ids[k] if ids else k, w[k], props[k]) for k in range(len(w))]


def _configs(msim):
    """name -> (miners, duration, total weight, forced wide, kind)"""
    W5 = msim.C5_TOTAL_WEIGHT
    rng = random.Random(11)  # the 5 000-miner and 100-miner networks of tests/test_gpu_general.py
    big = [2000, 1500] + [rng.randint(1, 3) for _ in range(4998)]
    rng = random.Random(5)
    cuts = sorted(rng.sample(range(1, 700), 98))
    hundred = [300] + [b - a for a, b in zip([0] + cuts, cuts + [700])]
    return {
        "g_5000_honest": (_net(msim, big, [1000] * 5000), DAY, sum(big), False, "general"),
        "g_100_one_selfish": ([msim.Miner(k, hundred[k], 1000, k == 0) for k in range(100)], 7 * DAY, 1000, False, "general"),
        "c1": (msim.PRESETS["c1"](), Y, 100, False, "honest"),
        "c2": (msim.PRESETS["c2"](), Y, 100, False, "honest"),
        "c3": (msim.PRESETS["c3"](), Y, 100, False, "selfish"),
        "c5_30d": (msim.c5_network(), 30 * DAY, W5, False, "wide"),
        "c5_year": (msim.c5_network(), Y, W5, False, "wide"),
        "two_miners_60s": (_net(msim, [50, 50], [60_000, 0]), Y, 100, False, "honest"),
        "c2_forced_wide": (msim.PRESETS["c2"](), Y, 100, True, "wide"),
    }


def _sim(msim, miners, duration, total_weight=100, force_wide=False):
    with _env({"MSIM_FORCE_WIDE": "1"} if force_wide else None):
        return msim.Simulation(miners, duration, total_weight)


def _config_plans(msim, _lib):
    out = {}
    for name, (miners, dur, W, fw, kind) in _configs(msim).items():
        sim = _sim(msim, miners, dur, W, fw)
        variants = {"base": None, "max_slice_256": MAX_SLICE}
        if kind == "honest":
            variants["pipe_test"] = PIPE_TEST
        if kind == "wide":
            variants["wide_test_rcap_8"] = WIDE_TEST
        for vname, env in variants.items():
            with _env(env):
                for n in CONFIG_RUNS:
                    pl = _lib.MsimPipelineLayout()
                    rc = _lib.lib.msim_pipeline_info(sim.handle, n, ctypes.byref(pl))
                    out[f"{name}/{vname}/{n}"] = [int(_lib.lib.msim_workspace_bytes(sim.handle, n)), rc] + [
                        getattr(pl, f).hex() if f == "rho" else int(getattr(pl, f)) for f, _ in pl._fields_]
    return out


def _sweeps(msim):
    """name -> list of (miners, duration, total weight, forced wide), one per point"""
    W5 = msim.C5_TOTAL_WEIGHT
    net5 = msim.c5_network()
    pt = lambda miners, dur=Y, W=100, fw=False: (miners, dur, W, fw)
    c5 = lambda d: [msim.Miner(mn.id, mn.perc, d) for mn in net5]
    w2 = [20, 20, 20, 10, 10, 10, 5, 4, 1]
    by_weights = [_net(msim, H, [1000] * 9), _net(msim, w2, [100] * 9), _net(msim, H, [100] * 9),
                  _net(msim, w2, [5000] * 9), _net(msim, H, [10] * 9)]
    tail = [7, 1, 1, 2, 5, 3, 0, 6, 4, 9, 8, 2, 1, 6, 5]
    wc, wb, ws = [41, 0] + tail, [20, 21] + tail, [19, 22] + tail
    a5 = [msim.Miner(mn.id, mn.perc, 25_000 if mn.id < 2 else 0) for mn in net5]
    b5 = [msim.Miner(mn.id, mn.perc, 0 if mn.id < 2 else 36_000) for mn in net5]
    w4 = [3, 0, 7, 10]
    delays20 = [100 + 450 * k for k in range(20)]
    return {
        # tests/test_sweep_shared_host.py
        "one_default_point": [pt(msim.setup_miners())],
        "by_weights_and_duration": [pt(p, 10**9) for p in by_weights],
        "two_durations": [pt(by_weights[0], 10**9), pt(by_weights[2], 10**8), pt(by_weights[4], 10**9)],
        "honest_uniform_3": [pt(msim.setup_miners(p)) for p in (10_000, 1_000, 100)],  # flags 0: a per-lane sweep
        "a_selfish_point": [pt(msim.setup_miners(1000)), pt(msim.setup_miners(1000, 30))],
        "a_600s_point": [pt(msim.setup_miners(1000)), pt(msim.setup_miners(600_000))],
        "envelope_past_the_fork_rate_limit": [pt(_net(msim, [50, 50], [60_000, 0])), pt(_net(msim, [50, 50], [0, 60_000])),
                                              pt(_net(msim, [50, 50], [100, 100]))],
        # tests/test_wide_sweep_host.py
        "c5_uniform_3": [pt(c5(d), Y, W5) for d in (10_000, 1_000, 100)],
        "wide_two_groups_and_a_singleton": [pt(_net(msim, wc, [10_000] * 17), 10**9, 101), pt(_net(msim, wb, [1_000] * 17), 10**9, 101),
                                            pt(_net(msim, wc, [100] * 17), 10**9, 101), pt(_net(msim, ws, [2_000] * 17), 10**9, 101),
                                            pt(_net(msim, wb, [50] * 17), 10**9, 101)],
        "wide_two_durations": [pt(_net(msim, w4, [1000] * 4), 10**9, 20), pt(_net(msim, w4, [100] * 4), 10**8, 20),
                               pt(_net(msim, w4, [10] * 4), 10**9, 20)],
        "c5_envelope_not_taken_2": [pt(a5, Y, W5), pt(b5, Y, W5)],
        "c5_envelope_not_taken_3": [pt(a5, Y, W5), pt(b5, Y, W5), pt(c5(100), Y, W5)],
        "narrow_and_forced_wide": [pt(msim.setup_miners(1000)), pt(msim.setup_miners(100), Y, 100, True)],
        "forced_wide_twice": [pt(msim.setup_miners(100), Y, 100, True)] * 2,
        "c5_with_a_general_point": [pt(net5, Y, W5), pt(c5(60_000), Y, W5)],
        # further engines and the split passes
        "selfish_grid_360": [pt(p) for p in msim.c4_grid()],
        "six_selfish_c3_c2": [pt([msim.Miner(k, w, 1000, k < 5) for k, w in enumerate([10] * 7 + [15, 15])], 30 * DAY),
                              pt(msim.PRESETS["c3"](), 30 * DAY), pt(msim.PRESETS["c2"](), 30 * DAY)],
        "a_shared_id_point": [pt(msim.setup_miners(1000)), pt(_net(msim, H, [1000] * 9, ids=[0, 0, 2, 3, 4, 5, 6, 7, 8]))],
        "honest_uniform_20": [pt(msim.setup_miners(d)) for d in delays20],
        "wide_uniform_20": [pt(_net(msim, wc, [d] * 17), 10**9, 101) for d in delays20],
    }


def _sweep_plans(msim, _lib):
    out = {}
    for name, points in _sweeps(msim).items():
        sims = [_sim(msim, *p) for p in points]
        hs = (ctypes.c_void_p * len(sims))(*[s.handle.value for s in sims])
        for flags in (0, 1):
            h = ctypes.c_void_p()
            with _env():
                rc = _lib.lib.msim_sweep_create_ex(hs, len(sims), flags, ctypes.byref(h))
            rec = {"create_rc": rc}
            if rc == _lib.MSIM_OK:
                rec["group_of"] = [int(_lib.lib.msim_sweep_group_of(h, p)) for p in range(len(sims) + 1)]
                for vname, env in (("base", None), ("sweep_test", SWEEP_TEST)):
                    with _env(env):
                        for rpp in SWEEP_RUNS:
                            pl = _lib.MsimSweepPlan()
                            irc = _lib.lib.msim_sweep_info(h, rpp, ctypes.byref(pl))
                            rec[f"{vname}/{rpp}"] = [irc] + [int(getattr(pl, f)) for f, _ in pl._fields_] + [
                                int(_lib.lib.msim_sweep_workspace_bytes(h, rpp))]
                _lib.lib.msim_sweep_destroy(h)
            out[f"{name}/flags_{flags}"] = rec
    return out


def compute():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    with _env():
        return {"config_plan_fields": ["msim_workspace_bytes", "info_rc"] + [f for f, _ in _lib.MsimPipelineLayout._fields_],
                "sweep_plan_fields":["info_rc"] + [f for f, _ in _lib.MsimSweepPlan._fields_] + ["msim_sweep_workspace_bytes"],
                "configs": _config_plans(msim, _lib), "sweeps": _sweep_plans(msim, _lib)}


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(compute(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")

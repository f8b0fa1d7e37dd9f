"""The plans of the C ABI's host side equal the recorded ones (tests/golden/host_plans.json), value for value.

The file holds what the library answered, without a device, for single networks and sweeps on every engine: workspace
sizes, slice sizes, segment geometry, engines, draw groups and every point's group, with and without the test switches
that change a plan (tests/host_plans.py lists the cases and regenerates the file). It was recorded from the commit
before the sweep planning, the launch-argument builders and the slice-fitting loop were each written once
(5484533), so that rewrite, and any later one of the host code, has to reproduce every value. The general engine's
networks (5 000 honest miners, 100 miners with one selfish, a sweep with a point only it serves) were added to the
file from the commit before its test switches MSIM_GEN_TEST_* were written (f7767df): unset, they change no plan.
CPU only."""
import json

import host_plans


def test_every_recorded_plan_is_reproduced(msim_lib_path):
    with open(host_plans.GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(host_plans.compute()))
    assert sorted(got) == sorted(want)
    for section in ("config_plan_fields", "sweep_plan_fields"):
        assert got[section] == want[section]
    for section in ("configs", "sweeps"):
        assert sorted(got[section]) == sorted(want[section]), section
        assert len(want[section]) > 30
        diff = {k: (want[section][k], got[section][k]) for k in want[section] if got[section][k] != want[section][k]}
        assert not diff, (section, diff)

"""The draw-group planner of the two shared-draw sweep forms (csrc/msim_drawgroups.h) alone, on the host.

tests/native/drawgroups_check.cpp includes that header only and supplies stand-in points (a draw key and a delay per
miner; an envelope is taken when the sum of the group's per-miner largest delays is below a bound). Built here with
AddressSanitizer and UBSan and run as a child process, it checks a few thousand random instances against a
transcription of the loop the planner replaced (same groups, same order, same group_of), that every result is a
partition into groups of one key whose envelopes were accepted, the fixed cases the ABI tests assert through real
configs (tests/test_sweep_shared_host.py, tests/test_wide_sweep_host.py), that an envelope error comes back unchanged and
ends the planning, and that no envelope is asked for a group of one."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "drawgroups_check.cpp")


def test_planner_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drawgroups_check")
        b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.strip().endswith("ok")

"""The per-device table cache of the C ABI (csrc/msim_devcache.h, used by csrc/msim_api.hip) on the host, with a
counting stand-in backend: threads racing over several devices and two keys upload each table once and all see
one base pointer; a larger cached entry serves a smaller request; a failed copy frees its allocation and caches
nothing; clear() frees everything. The same program checks the interval union behind stage timing's busy time
(csrc/msim_timing.h). The reference's counterpart is main.cpp:205-209's std::async fan-out, whose tasks share
no tables."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "devcache_host.cpp")


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ok, gets, allocs, frees = r.stdout.split()
    assert ok == "OK"
    assert int(allocs) == int(frees)  # every stand-in allocation freed exactly once
    return int(gets)


def test_devcache_one_upload_per_device_and_key():
    exe = os.path.join(ROOT, "build", "devcache_host")
    if not os.path.exists(exe):
        pytest.skip("build() not run")
    assert _run(exe, 8, 4000) == 32000


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_devcache_thread_sanitizer():
    """The same driver under ThreadSanitizer (host code only): no data race on the entries."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "dc_tsan")
        b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", SRC, "-o", exe],
                           capture_output=True, text=True)
        if b.returncode != 0:
            pytest.skip("ThreadSanitizer unavailable: " + b.stderr[-300:])
        assert _run(exe, 4, 1500) == 6000

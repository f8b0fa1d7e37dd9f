"""Test-only host builds of the draw kernel's own forms (build/fastdraw2_check, build/libpipeline_k1_host.so):
built on demand, like conftest's native_tests, by __graft_entry__.build_k1_tests()."""
import fcntl
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "fastdraw2_check")
PIPE = os.path.join(ROOT, "build", "libpipeline_k1_host.so")


def _newest_source() -> float:
    srcs = []
    for d, exts in ((os.path.join(ROOT, "miningsimulation_amd", "csrc"), (".h",)),
                    (os.path.join(ROOT, "tests", "native"), (".cpp", ".h"))):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts)]
    return max(os.path.getmtime(f) for f in srcs)


def ensure() -> dict:
    import __graft_entry__ as ge

    outs = (CHECK, PIPE)
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".k1_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not all(os.path.exists(p) for p in outs) or min(os.path.getmtime(p) for p in outs) < _newest_source():
            ge.build_k1_tests()
    return {"fastdraw2_check": CHECK, "pipeline_k1_host": PIPE}

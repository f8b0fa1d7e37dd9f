"""Test-only host builds of the shared-draw sweep's lane bodies (tests/native/sweep_shared_body.h):
build/libsweep_shared_host.so and build/sweep_shared_check, built on demand by
__graft_entry__.build_sweep_shared_tests()."""
import fcntl
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "build", "libsweep_shared_host.so")
CHECK = os.path.join(ROOT, "build", "sweep_shared_check")


def _newest_source() -> float:
    srcs = []
    for d, exts in ((os.path.join(ROOT, "miningsimulation_amd", "csrc"), (".h",)),
                    (os.path.join(ROOT, "tests", "native"), (".cpp", ".h"))):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts)]
    return max(os.path.getmtime(f) for f in srcs)


def ensure() -> dict:
    import __graft_entry__ as ge

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".sweep_shared_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (LIB, CHECK)
        if not all(os.path.exists(p) for p in outs) or min(os.path.getmtime(p) for p in outs) < _newest_source():
            ge.build_sweep_shared_tests()
    return {"lib": LIB, "check": CHECK}

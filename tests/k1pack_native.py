"""Test-only host build of the forms the draw kernel's quad runs (build/k1pack_check: the packed interval form and
the high-word picker, tests/native/k1pack_check.cpp): built on demand by __graft_entry__.build_k1pack_tests()."""
import fcntl
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "k1pack_check")


def _newest_source() -> float:
    srcs = []
    for d, exts in ((os.path.join(ROOT, "miningsimulation_amd", "csrc"), (".h",)),
                    (os.path.join(ROOT, "tests", "native"), (".cpp", ".h"))):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts)]
    return max(os.path.getmtime(f) for f in srcs)


def ensure() -> str:
    import __graft_entry__ as ge

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".k1pack_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(CHECK) or os.path.getmtime(CHECK) < _newest_source():
            ge.build_k1pack_tests()
    return CHECK

"""ctypes wrapper of tests/native/pipeline_host.cpp (pipeline_run_ex): the honest pipeline's lane bodies run on the CPU.
Shared by tests/test_pipeline_host.py and tests/test_gpu_pipe_overflow.py."""
import ctypes
import fcntl
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "pipe_overflow_check")


def ensure_check() -> str:
    """build/pipe_overflow_check (tests/native/pipe_overflow_check.cpp under ASan and UBSan), built on demand."""
    import __graft_entry__ as ge

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".pipe_overflow_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        srcs = []
        for d, exts in ((os.path.join(ROOT, "miningsimulation_amd", "csrc"), (".h",)),
                        (os.path.join(ROOT, "tests", "native"), (".cpp", ".h"))):
            srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts)]
        if not os.path.exists(CHECK) or os.path.getmtime(CHECK) < max(os.path.getmtime(f) for f in srcs):
            ge.build_pipe_overflow_tests()
    return CHECK


def sigma_cap(lam: float, k: float) -> int:
    """ceil(lam + k sqrt(lam)): a slot capacity k standard deviations above a segment's mean count of listed blocks."""
    return math.ceil(lam + k * math.sqrt(lam))


def load(path):
    lib = ctypes.CDLL(path)

    def run(percs, props, duration, n, base=1000, begin=0, cap=0, slots=8192, nseg=0, seg=0, lcap=0, kind=-1,
            detail=False):
        """found [n, m], stale [n, m], ok [n] (False: the run goes to the retry kernel) and the list count; with
        detail also the listed blocks K3 counts per run and whether K3 takes its one-read path for them.
        cap, lcap: capacity overrides (0: the layout's). nseg, seg: the workers per run and their length (0, 0: what
        the layout picks for `slots` wave slots). kind: K2's state machine (-1: the network's own)."""
        m = len(percs)
        f = (ctypes.c_uint32 * (n * m))()
        s = (ctypes.c_uint32 * (n * m))()
        ok = (ctypes.c_uint8 * n)()
        ne = ctypes.c_uint32()
        listed = (ctypes.c_uint32 * n)()
        onepath = (ctypes.c_uint8 * n)()
        rc = lib.pipeline_run_ex((ctypes.c_uint64 * m)(*percs), (ctypes.c_int64 * m)(*props), (ctypes.c_uint8 * m)(),
                              m, ctypes.c_int64(duration), ctypes.c_uint32(base), ctypes.c_uint64(begin),
                              ctypes.c_uint32(n), ctypes.c_uint32(cap), ctypes.c_uint32(slots), ctypes.c_uint32(nseg),
                              ctypes.c_uint32(seg), ctypes.c_uint32(lcap), ctypes.c_int32(kind), f, s, ok,
                              ctypes.byref(ne), listed, onepath)
        assert rc == 0, (f"pipeline_run_ex rc={rc} (-100: jump-ahead state differs from sequential stepping; -101, -102: "
                         "nseg and seg are not a geometry of the layout)")
        out = (np.array(f, dtype=np.int64).reshape(n, m), np.array(s, dtype=np.int64).reshape(n, m),
               np.array(ok, dtype=bool), ne.value)
        if detail:
            out += (np.array(listed, dtype=np.int64), np.array(onepath, dtype=bool))
        return out

    return run

"""Test-only host builds of the lane bodies of the shared-draw form of large-network sweeps
(tests/native/wide_sweep_body.h): build/libwide_sweep_host.so and build/wide_sweep_check, built on demand by
__graft_entry__.build_wide_sweep_tests()."""
import ctypes
import fcntl
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "build", "libwide_sweep_host.so")
CHECK = os.path.join(ROOT, "build", "wide_sweep_check")


def _newest_source() -> float:
    srcs = []
    for d, exts in ((os.path.join(ROOT, "miningsimulation_amd", "csrc"), (".h",)),
                    (os.path.join(ROOT, "tests", "native"), (".cpp", ".h"))):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts)]
    return max(os.path.getmtime(f) for f in srcs)


def ensure() -> dict:
    import __graft_entry__ as ge

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".wide_sweep_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        outs = (LIB, CHECK)
        if not all(os.path.exists(p) for p in outs) or min(os.path.getmtime(p) for p in outs) < _newest_source():
            ge.build_wide_sweep_tests()
    return {"lib": LIB, "check": CHECK}


def run_group(weights, props, W, duration, n, base=1000, begin=0, rcap_env=0, rcap_pt=None):
    """One draw group on the host. props: [points][m]. Returns found, stale [points, n, m], ok [points, n] and counts
    [1 + points, n] (row 0: the envelope's candidates per run, then every point's own)."""
    lib = ctypes.CDLL(ensure()["lib"])
    m, np_ = len(weights), len(props)
    flat = [d for pt in props for d in pt]
    f = (ctypes.c_uint32 * (np_ * n * m))()
    s = (ctypes.c_uint32 * (np_ * n * m))()
    ok = (ctypes.c_uint8 * (np_ * n))()
    cnt = (ctypes.c_uint32 * ((1 + np_) * n))()
    rc = lib.wide_sweep_run((ctypes.c_uint64 * m)(*weights), (ctypes.c_int64 * len(flat))(*flat), ctypes.c_uint32(m),
                            ctypes.c_uint32(np_), ctypes.c_uint64(W), ctypes.c_int64(duration), ctypes.c_uint32(base),
                            ctypes.c_uint64(begin), ctypes.c_uint32(n), ctypes.c_uint32(rcap_env),
                            (ctypes.c_uint32 * np_)(*(rcap_pt or [0] * np_)), f, s, ok, cnt)
    assert rc == 0, f"point {rc - 1}: the split's selection differs from the listing on the point's own thresholds"
    return (np.array(f, dtype=np.int64).reshape(np_, n, m), np.array(s, dtype=np.int64).reshape(np_, n, m),
            np.array(ok, dtype=np.int64).reshape(np_, n), np.array(cnt, dtype=np.int64).reshape(1 + np_, n))

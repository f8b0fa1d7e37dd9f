"""The draw kernel's picker by one multiply with 400 (msim_fastdraw.h pick_off400_key: table byte offset and
exactness key from the two words of 400 h'), over all 2^32 high words, and the packed interval form's v built
without integer-to-double conversions (k1p_v) against the two-conversion form, bit for bit: host builds under
AddressSanitizer and UBSan (tests/native/k1pick400_check.cpp, k1v_check.cpp: stand-alone programs run as child
processes). The GPU build of the same header is checked in tests/test_gpu_k1_pickband.py."""
import fcntl
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "k1pick400_check")
VCHECK = os.path.join(ROOT, "build", "k1v_check")


def ensure() -> str:
    import __graft_entry__ as ge

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "native", "k1pick400_check.cpp"),
            os.path.join(ROOT, "tests", "native", "k1v_check.cpp"),
            os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_fastdraw.h"),
            os.path.join(ROOT, "miningsimulation_amd", "csrc", "msim_draws.h")]
    with open(os.path.join(ROOT, "build", ".k1pick400_tests.lock"), "w") as lk:  # one builder at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        newest = max(os.path.getmtime(f) for f in srcs)
        if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in (CHECK, VCHECK)):
            ge.build_k1pick400_tests()
    return CHECK


def _run(path, *args):
    out = subprocess.run([path, *args], capture_output=True, text=True, check=True)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    res = json.loads(out.stdout)
    print(json.dumps(res, indent=1))
    return res


@pytest.fixture(scope="module")
def report():
    return _run(ensure(), "16")


@pytest.fixture(scope="module")
def vreport():
    ensure()
    return _run(VCHECK, "10000000")


def test_every_high_word(report):
    """All 2^32 values of h': whenever the low word of 400 h' is below the band, h' and h' + 1 with any low word
    (pick_q_exact is monotone: the smallest and the largest such draw) have PickFinder's index hi(400 h') >> 2,
    and hi(400 h') & ~3 is four times the index of the multiply with 100."""
    t = report["every_high_word"]
    assert t["n"] == 1 << 32, t
    assert t["bad"] == 0 and t["bad_offset"] == 0 and t["first_bad"] == 0, t
    assert t["settled"] + t["flagged"] == t["n"]


def test_band_is_a_superset_and_stays_small(report):
    """Every h' the multiply with 100 sends to the exact path is in the new band, and the band stays at
    1024 / 2^32 = 2.4e-7 of the high words (a broken key must not hide as "always the exact path")."""
    t = report["every_high_word"]
    assert t["not_superset"] == 0 and t["old_flagged"] > 0, t
    assert 0 < t["flagged"] <= 1024, t
    assert t["old_flagged"] <= t["flagged"]


def test_band_rejects_the_wrap(report):
    """h' = 2^32 - 1, whose successor wraps to 0, is in the band."""
    assert report["band_lo"] == 0xFFFFFC00
    assert report["wrap_rejected"] is True and report["wrap_key"] == (1 << 32) - 400, report


def test_edges_against_the_division(report):
    """Every high word within 2^12 of each of the 100 multiples of 2^32 / 100 (and of 2^32): the same, and
    against u / PERC_MULTIPLIER itself."""
    t = report["edges"]
    assert t["n"] > 800_000 and t["bad"] == 0 and t["bad_offset"] == 0 and t["bad_division"] == 0, t
    assert t["flagged"] > 0 and t["not_superset"] == 0, t


@pytest.mark.parametrize("part,n", [("special", 4), ("one_bit", 64), ("zero_bit", 64), ("random", 10_000_000)])
def test_v_without_conversions_is_bit_equal(vreport, part, n):
    """u = 0, 2^11 - 1, 2^11 and 2^64 - 1; every single-bit u; every u with a single zero bit; 10 M random draws,
    half of them with 1 to 53 leading ones: k1p_v has the bits of the two-conversion v and of
    1 - (u >> 11) 2^-53 computed plainly, and lies in [2^-53, 1]."""
    t = vreport[part]
    assert t["n"] == n, t
    assert t["differs"] == 0 and t["differs_from_plain"] == 0 and t["out_of_range"] == 0, t


def test_v_constants(vreport):
    """The high words are those of 2^20 and 1/2, the addend 2^20 + 1.5."""
    assert vreport["hi_word"] == 0x41300000 and vreport["lo_word"] == 0x3FE00000
    assert vreport["base"] == 2.0 ** 20 + 1.5

"""The forms the draw kernel's quad runs (msim_fastdraw.h "the packed form": one 16-byte table entry per draw with
invc pre-scaled and the acceptance margin folded in; the high-word picker), host build
(tests/native/k1pack_check.cpp), against glibc's log1p/llround, the folded form k1_interval_fast and PickFinder's
index u / PERC_MULTIPLIER. The GPU build of the same header is checked in tests/test_gpu_k1_quads.py."""
import json
import subprocess

import pytest

import k1pack_native

PARTS = ["random", "near_boundary", "exponent_grid", "special"]


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([k1pack_native.ensure(), "20000000", "8"], capture_output=True, text=True, check=True)
    res = json.loads(out.stdout)
    print(json.dumps(res, indent=1))
    return res


@pytest.mark.parametrize("part", PARTS)
def test_no_accepted_value_differs(report, part):
    """20 M random u; ~1 M u within +-4 ns of a millisecond boundary; every exponent x table column x (first,
    middle, last mantissa); u = 0, 2^64 - 1 and bit 11 alone. A value the packed form accepts is llround/log1p's,
    and so is the end of the chain packed form -> general form -> glibc's sequence; the general form on the two
    small arrays K1 keeps is k1_interval_general."""
    t = report[part]
    assert t["bad_packed"] == 0 and t["bad_chain"] == 0 and t["general_on_differs"] == 0, t
    assert t["n"] >= {"random": 19_999_992, "near_boundary": 900_000, "exponent_grid": 9_000, "special": 3}[part]


@pytest.mark.parametrize("part", PARTS)
def test_small_exponents_are_rejected(report, part):
    """v below 2^-15 aliases in the 16-row table: the packed form must never accept one."""
    t = report[part]
    assert t["low_e_accepted"] == 0, t
    if part != "random":
        assert t["low_e"] > 0


@pytest.mark.parametrize("part", PARTS)
def test_packing_is_an_identity(report, part):
    """For every input both forms accept, the packed form's r and interval equal the folded form's bit for bit
    (v * invc_j 2^-e and w * invc_j are the same real number), and its z is the folded z less the margin."""
    t = report[part]
    assert t["r_differs"] == 0 and t["q_differs"] == 0, t
    if part != "special":  # u = 0, 2^64 - 1 and bit 11 alone are rejected by both
        assert t["both"] > 0.25 * t["n"], t


def test_rejected_share_stays_small(report):
    """The cap that keeps a broken check from hiding as "always the exact path": at most 1e-4 of random draws
    leave the packed form (design: 2^-15 + 2.86e-6 = 3.3e-5)."""
    t = report["random"]
    assert t["rejected"] <= 1e-4 * t["n"], t
    assert t["rejected"] >= t["low_e"] > 0


def test_margin(report):
    """Margin minus the worst measured error (the packed z plus the margin against glibc's 6e11 E + 0.5, every
    input with e >= -15) is at least the general form's: the inequality of test_fastdraw2.test_polynomial_margin."""
    worst = max(report[p]["max_err_ns"] for p in PARTS)
    worst_general = max(report[p]["general_max_err_ns"] for p in PARTS)
    assert report["margin_ns"] - worst >= report["general_margin_ns"] - worst_general, (worst, worst_general)


def test_picker_boundaries(report):
    """Every h' within +-512 of each of the 100 bucket boundaries, both carries, extreme low words and the low
    words around the boundary b * PERC_MULTIPLIER: whenever the key is below the band, p(h') is PickFinder's index."""
    t = report["pick_boundaries"]
    assert t["bad"] == 0 and t["settled"] > 1_600_000 and t["flagged"] > 0, t


def test_picker_from_states(report):
    """From stream states against rng_next + pick_q_exact: 20 M random states, and crafted ones (s0 chosen, s1 solved
    for the target output) whose keys lie on both sides of the band's edge, without and with a carry out of the low
    halves. The state after the high-word step is rng_next's."""
    for part in ("pick_random", "pick_below_band", "pick_in_band"):
        t = report[part]
        assert t["bad"] == 0 and t["state_differs"] == 0, (part, t)
    assert report["pick_below_band"]["flagged"] == 0 and report["pick_below_band"]["settled"] == 2048
    assert report["pick_in_band"]["settled"] == 0 and report["pick_in_band"]["flagged"] == 2048
    t = report["pick_random"]
    assert t["n"] >= 19_999_992 and t["flagged"] <= 1e-6 * t["n"], t  # design: 256 / 2^32 = 6e-8

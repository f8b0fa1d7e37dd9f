"""The draw kernel's own form of the fast interval (msim_fastdraw.h, "K1's form": exponent folded into the log
table, degree-4 minimax polynomial, 1.25 ns margin; host build, tests/native/fastdraw2_check.cpp) against
glibc's log1p/llround, i.e. exactly what the reference calls. The GPU build of the same header is checked in
tests/test_gpu_k1_forms.py."""
import json
import subprocess

import pytest

import k1_native


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([k1_native.ensure()["fastdraw2_check"], "20000000", "8"], capture_output=True, text=True,
                         check=True)
    res = json.loads(out.stdout)
    print(json.dumps(res, indent=1))
    return res


def test_ships_both_table_items(report):
    """The combination under test is the shipped one: folded exponent and the degree-4 polynomial."""
    assert report["a2"] == 1 and report["deg4"] == 1


@pytest.mark.parametrize("part", ["random", "near_boundary", "exponent_grid", "special"])
def test_no_accepted_value_differs(report, part):
    """20 M random u; ~1 M u within +-4 ns of a millisecond boundary; every exponent x table column x (first,
    middle, last mantissa); u = 0, 2^64 - 1 and bit 11 alone. A value a form accepts is the reference's, and so
    is the end of the chain fast form -> general form -> glibc's sequence."""
    t = report[part]
    assert t["bad_fast"] == 0 and t["bad_general"] == 0 and t["bad_chain"] == 0, t
    assert t["n"] >= {"random": 19_999_992, "near_boundary": 900_000, "exponent_grid": 9_000, "special": 3}[part]


@pytest.mark.parametrize("part", ["random", "near_boundary", "exponent_grid", "special"])
def test_small_exponents_are_rejected(report, part):
    """v below 2^-15 aliases in the 16-row table: the fast form must never accept one."""
    t = report[part]
    assert t["low_e_accepted"] == 0, t
    if part != "random":
        assert t["low_e"] > 0  # the crafted sets do reach below 2^-15 (u = 2^64 - 1 among the special ones)


def test_rejected_share_stays_small(report):
    """The cap that keeps a broken check from hiding as "always the exact path": at most 1e-4 of random draws
    leave the fast form (design: 2^-15 + 2 x 1.25e-6 = 3.3e-5), and the general form keeps its 2e-6 x 1.25."""
    t = report["random"]
    assert t["rejected_fast"] <= 1e-4 * t["n"], t
    assert t["rejected_fast"] >= t["low_e"] > 0
    assert t["rejected_general"] <= 5e-6 * t["n"], t


def test_polynomial_margin(report):
    """Margin minus error is at least the general form's, for the polynomial alone (double Horner form against
    an 80-bit log1p on 4 M points of |r| <= 2^-7) and for the whole interval against glibc on every input above."""
    k1_margin, margin = report["margin_ns"], report["general_margin_ns"]
    assert report["poly_err_ns"] < 0.2184  # scripts/fit_log1p_deg4.py: 0.218298 ns
    assert k1_margin - report["poly_err_ns"] >= margin - report["general_poly_err_ns"]
    worst = max(report[p]["max_err_ns"] for p in ("random", "near_boundary", "exponent_grid", "special"))
    worst_general = max(report[p]["general_max_err_ns"] for p in ("random", "near_boundary", "exponent_grid", "special"))
    assert k1_margin - worst >= margin - worst_general, (worst, worst_general)

"""tests/golden/long_runs.json against the oracle: two of the cheap cases recomputed (the first 8 runs of each; the
file's other cases take the oracle up to a minute), and the file's shape for every case."""
import numpy as np
import pytest

import long_runs


@pytest.mark.parametrize("name", long_runs.CHEAP)
def test_recorded_counters_are_the_oracles(oracle, name):
    c = long_runs.CASES[name]
    f, s, L = long_runs.oracle_counters(oracle, c, runs=8, threads=8)
    ef, es, eL = long_runs.expected(name, runs=8)
    assert np.array_equal(f, ef) and np.array_equal(s, es) and np.array_equal(L, eL)


def test_every_case_is_recorded_in_full():
    for name, c in long_runs.CASES.items():
        f, s, L = long_runs.expected(name)
        assert f.shape == s.shape == (c["runs"], len(c["weights"])) and L.shape == (c["runs"],)
        assert np.array_equal(f.sum(axis=1), L) and (f >= 0).all() and (s >= 0).all()
        # an honest run of D ms holds about D / 600 s blocks (10 s delays lose under 2 % of them to forks)
        assert abs(L.mean() / (c["duration"] / 599_999.5) - 1) < 0.05 or c["selfish"][0], name

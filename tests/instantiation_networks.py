"""Networks of tests/test_gpu_instantiations.py: one deterministic set per miner count M = 1..15, so that every
per-M instantiation of K2, K3, the per-lane kernel, E1 and E2 (MSIM_FOR_EACH_M) runs on the device. Nothing here
draws from an RNG: a case cannot be skipped by an unlucky seed. tests/test_instantiation_networks.py checks the
set on the CPU (accepted by msim_config_create, on the intended path, the oracle finishes each case).

A case is a dict: percs, props, selfish (lists of M), W (total weight), env (test switches to set), path (the
msim_pipeline_info `uses_pipeline` it must report: 0 per-lane kernel, 1 event-skipping pipeline, 3 entity engine),
key (names the oracle result it shares with other cases)."""

DURATION_MS = 5 * 10**9
N_RUNS = 70  # one wave and a ragged second
HETERO_MS = [0, 1, 100, 1000, 10_000]


def _split(total, parts):
    """`parts` positive integers summing to `total`, descending (triangular weights), the first the largest."""
    w = [parts - i for i in range(parts)]
    rest = total - parts
    out = [1 + rest * x // sum(w) for x in w]
    for i in range(total - sum(out)):
        out[i % parts] += 1
    assert sum(out) == total and all(x > 0 for x in out) and out == sorted(out, reverse=True)
    return out


def percs(m):
    """Positive integer percentages summing to 100. From three miners miner 0 holds 40 and is the largest; with two
    miners it holds 40 (a selfish miner 0 stays a minority) and miner 1 the other 60; alone it holds 100."""
    if m == 1:
        return [100]
    if m == 2:
        return [40, 60]
    return [40] + _split(60, m - 1)


def percs_multi(m, ns):
    """ns selfish miners at the END of the list holding 45 % together (25/20 or 20/15/10), the honest 55 % on the
    first m - ns miners: miner 0 holds 30 and is the largest, the other 25 are split over the rest; where it is the
    only honest miner it holds all 55 (two selfish miners of three, three of four: no split keeps it at 40)."""
    sel = {2: [25, 20], 3: [20, 15, 10]}[ns]
    return ([55] if m - ns == 1 else [30] + _split(25, m - ns - 1)) + sel


def _case(p, q, s, W=100, env=None, path=1, key=None):
    return {"percs": list(p), "props": list(q), "selfish": list(s), "W": W, "env": dict(env or {}), "path": path,
            "key": key}


def hetero(m, lo=0, shift=0):
    """Delays cycling through 0, 1, 100, 1 000, 10 000 ms by miner index (+ shift), raised to at least `lo` ms."""
    return [max(lo, HETERO_MS[(k + shift) % len(HETERO_MS)]) for k in range(m)]


def _one_selfish(m):
    return [k == 0 for k in range(m)]


# name -> (smallest M, builder)
CASES = {
    # path 1: K1, K2 lean<M>, K3<M>
    "honest_100ms": (1, lambda m: _case(percs(m), [100] * m, [False] * m, key="h100")),
    # path 1: K2 mid<M> (rho ~ 1.7 %: episodes really run)
    "honest_10s": (1, lambda m: _case(percs(m), [10_000] * m, [False] * m, key="h10s")),
    "honest_hetero": (1, lambda m: _case(percs(m), hetero(m), [False] * m, key="hhet")),
    # path 0: the per-lane kernel<M> and its retry
    "honest_100ms_no_pipeline": (1, lambda m: _case(percs(m), [100] * m, [False] * m, env={"MSIM_NO_PIPELINE": "1"},
                                                    path=0, key="h100")),
    # path 3: E1<M, 1, UNI>
    "selfish_uniform_1s": (2, lambda m: _case(percs(m), [1000] * m, _one_selfish(m), path=3, key="s1s")),
    # UNI = false (1, 100, ... ms: two miners already differ), the settled form still applies (every delay >= 1 ms)
    "selfish_hetero_1ms": (2, lambda m: _case(percs(m), hetero(m, 1, 1), _one_selfish(m), path=3, key="shet1")),
    # a 0 ms delay: macro = 0, the entity engine alone
    "selfish_zero_delay": (2, lambda m: _case(percs(m), [1000] * (m - 1) + [0], _one_selfish(m), path=3, key="s0")),
    # weights summing to 1 000 (not multiples of 10): every pick is the weighted one
    "selfish_weights_1000": (2, lambda m: _case([10 * percs(m)[0] + 3, 10 * percs(m)[1] - 3] +
                                                [10 * x for x in percs(m)[2:]], [1000] * m, _one_selfish(m), W=1000,
                                                path=3, key="sw")),
    # E2<M>
    "selfish_uniform_1s_forced_retry": (2, lambda m: _case(percs(m), [1000] * m, _one_selfish(m),
                                                            env={"MSIM_SEL_FORCE_RETRY": "1"}, path=3, key="s1s")),
    # selfish classes 2 and 4, E1 and E2
    "two_selfish": (3, lambda m: _case(percs_multi(m, 2), hetero(m), [k >= m - 2 for k in range(m)], path=3, key="s2")),
    "two_selfish_forced_retry": (3, lambda m: _case(percs_multi(m, 2), hetero(m), [k >= m - 2 for k in range(m)],
                                                    env={"MSIM_SEL_FORCE_RETRY": "1"}, path=3, key="s2")),
    "three_selfish": (4, lambda m: _case(percs_multi(m, 3), hetero(m), [k >= m - 3 for k in range(m)], path=3,
                                         key="s3")),
    "three_selfish_forced_retry": (4, lambda m: _case(percs_multi(m, 3), hetero(m), [k >= m - 3 for k in range(m)],
                                                      env={"MSIM_SEL_FORCE_RETRY": "1"}, path=3, key="s3")),
}

MATRIX = [(name, m) for name, (lo, _) in CASES.items() for m in range(lo, 16)]


def case(name, m):
    lo, build = CASES[name]
    assert lo <= m <= 15
    c = build(m)
    assert len(c["percs"]) == m and sum(c["percs"]) == c["W"] and all(x > 0 for x in c["percs"])
    return c


_ORACLE = {}


def oracle_counters(oracle, name, m, run_begin, seed_base):
    """(found, stale) [N_RUNS, M] of the case from the oracle, computed once per network and shared by the cases
    that run it under different switches; the arrays are read-only."""
    c = case(name, m)
    k = (c["key"], m, run_begin, seed_base)
    if k not in _ORACLE:
        f, s, _, _ = oracle.run_batch(c["percs"], c["props"], c["selfish"], DURATION_MS, N_RUNS, run_begin, seed_base,
                                      threads=16, total_weight=c["W"])
        f.setflags(write=False)
        s.setflags(write=False)
        _ORACLE[k] = (f, s)
    return _ORACLE[k]

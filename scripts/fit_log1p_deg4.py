"""Degree-4 minimax polynomial for the draw kernel's fast interval (msim_fastdraw.h, FD4_*).

The fast interval needs  -6e5 * log1p(r)  (milliseconds) for |r| <= 2^-7. This script fits
    P(r) = k0 + k1 r + k2 r^2 + k3 r^3 + k4 r^4  ~  -6e5 * log1p(r)
by the Remez exchange algorithm in 60-digit arithmetic (mpmath), rounds k1..k4 to doubles (k0 is folded into
the A2 table by build_k1_log, in extended precision), and reports the largest |P - (-6e5 log1p)| of the ROUNDED
polynomial on a dense grid, in nanoseconds of 6e11 * E (1 ms = 1e6 ns). Prints the constants as C hex floats.

    python scripts/fit_log1p_deg4.py
"""
import mpmath as mp

mp.mp.dps = 60
A = mp.mpf(2) ** -7
DEG = 4


def f(r):
    return -600000 * mp.log1p(r)


def remez(deg, a, iters=30):
    n = deg + 2
    xs = [-a * mp.cos(mp.pi * i / (n - 1)) for i in range(n)]  # Chebyshev extrema
    coef, e = None, None
    for _ in range(iters):
        m = mp.matrix(n, n)
        b = mp.matrix(n, 1)
        for i, x in enumerate(xs):
            for k in range(deg + 1):
                m[i, k] = x ** k
            m[i, deg + 1] = (-1) ** i
            b[i] = f(x)
        sol = mp.lu_solve(m, b)
        coef, e = [sol[k] for k in range(deg + 1)], sol[deg + 1]

        def err(x):
            return mp.polyval(coef[::-1], x) - f(x)

        # new extrema: the roots of err' between consecutive sign changes, plus the end points
        grid = [-a + 2 * a * i / 4000 for i in range(4001)]
        vals = [err(x) for x in grid]
        ext = [grid[0]]
        for i in range(1, 4000):
            if (vals[i] - vals[i - 1]) * (vals[i + 1] - vals[i]) <= 0:
                x = mp.findroot(lambda t: mp.diff(err, t), grid[i])
                ext.append(x)
        ext.append(grid[-1])
        if len(ext) != n:
            raise SystemExit(f"expected {n} extrema, found {len(ext)}")
        if max(abs(x - y) for x, y in zip(ext, xs)) < mp.mpf(10) ** -30:
            break
        xs = ext
    return coef, abs(e)


coef, lev = remez(DEG, A)
rounded = [mp.mpf(float(c)) for c in coef]
rounded[0] = coef[0]  # k0 joins the table constant before its one rounding
worst = mp.mpf(0)
N = 200000
for i in range(N + 1):
    r = -A + 2 * A * i / N
    worst = max(worst, abs(mp.polyval(rounded[::-1], r) - f(r)))
print(f"levelled error of the exact fit : {float(lev * 1e6):.6f} ns")
print(f"max error, k1..k4 as doubles    : {float(worst * 1e6):.6f} ns  (|r| <= 2^-7, {N + 1} points)")
print(f"FD4_K0 = {mp.nstr(coef[0], 25)}  (long double literal: {mp.nstr(coef[0], 25)}L)")
for k in range(1, DEG + 1):
    print(f"FD4_K{k} = {float(coef[k]).hex()}  ({mp.nstr(coef[k], 20)})")

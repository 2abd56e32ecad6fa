"""Inputs and references shared by tests/test_workload_host.py and tests/test_workload_gpu.py: the knot sets, an exact
rational spline solve, the (seed, id_offset, B) cases of the workload builders and the host workload they are held
against (built once per case)."""
import functools
from fractions import Fraction

import numpy as np

from trajectory_generation_amd.workload import SPLINE_KNOTS_X, make_workload

KINDS = ("spline", "mixed", "parabola")
# (seed, id_offset, B): base case; odd / even tids shifted in `mixed`; two seed words and tid crossing to two words
CASES = ((0, 0, 9), (7, 5, 9), (2 ** 40 + 3, 2 ** 32 - 2, 4))
CASE_IDS = ["base", "shifted", "two-words"]


def exact_spline(xk, yk):
    """The natural cubic spline's (a, b, c, d) rows of float knots in exact rational arithmetic: [n-1][4] Fractions."""
    x = [Fraction(float(v)) for v in xk]
    y = [Fraction(float(v)) for v in yk]
    n = len(x)
    h = [x[i + 1] - x[i] for i in range(n - 1)]
    M = [Fraction(0)] * n
    if n > 2:
        cp, dp = {}, {}
        for i in range(1, n - 1):
            rhs = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
            den = 2 * (h[i - 1] + h[i]) - (h[i - 1] * cp[i - 1] if i > 1 else 0)
            cp[i] = h[i] / den
            dp[i] = (rhs - (h[i - 1] * dp[i - 1] if i > 1 else 0)) / den
        for i in range(n - 2, 0, -1):
            M[i] = dp[i] - cp[i] * M[i + 1]
    return [[y[i], (y[i + 1] - y[i]) / h[i] - h[i] * (2 * M[i] + M[i + 1]) / 6, M[i] / 2,
             (M[i + 1] - M[i]) / (6 * h[i])] for i in range(n - 1)]


def scaled_error(coef, exact):
    """max |coef - exact| over the rows of one trajectory, divided by max(1, max |exact|)."""
    err = max(abs(Fraction(float(coef[i][j])) - exact[i][j]) for i in range(len(exact)) for j in range(4))
    top = max(abs(v) for row in exact for v in row)
    return float(err / max(Fraction(1), top))


@functools.lru_cache(maxsize=None)
def workload_knot_sets():
    """The workload's knots with 64 seeded ordinate sets: list of (xk, yk)."""
    rng = np.random.default_rng(20)
    return [(SPLINE_KNOTS_X.copy(), rng.uniform(-1.0, 1.0, len(SPLINE_KNOTS_X))) for _ in range(64)]


@functools.lru_cache(maxsize=None)
def irregular_knot_sets():
    """200 irregular sets: nk 2..12, spacings U(0.2, 5), ordinates U(-3, 3)."""
    rng = np.random.default_rng(21)
    sets = []
    for i in range(200):
        n = 2 + i % 11
        sets.append((rng.uniform(-10.0, 10.0) + np.cumsum(rng.uniform(0.2, 5.0, n)), rng.uniform(-3.0, 3.0, n)))
    return sets


def pack_knots(sets, kmax):
    """list of (xk, yk) -> kinds [B] (all 2), nk [B], xk / yk [B,kmax] zero-padded."""
    B = len(sets)
    nk = np.array([len(s[0]) for s in sets], dtype=np.int32)
    xk, yk = np.zeros((B, kmax)), np.zeros((B, kmax))
    for b, (x, y) in enumerate(sets):
        xk[b, :len(x)] = x
        yk[b, :len(y)] = y
    return np.full(B, 2, dtype=np.int32), nk, xk, yk


@functools.lru_cache(maxsize=None)
def host_workload(kind, case):
    """make_workload of CASES[case], with the spline kind's ordinates and spline_natural rows stacked: the reference
    every builder test shares (read only)."""
    from trajectory_generation_amd.batch import spline_natural
    seed, off, B = CASES[case]
    w = make_workload(B, 20, 0.05, kind=kind, seed=seed, id_offset=off)
    if kind == "spline":
        w["yk"] = np.array([k[1] for k in w["knots"]])
        w["coef"] = np.array([spline_natural(*k) for k in w["knots"]])
    return w


def ulp_distance(a, b):
    """|a - b| in units of the spacing of b, elementwise."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))

"""Shared by tests/test_mpc_main_host.py and tests/test_closed_stats_gpu.py: exact moments of a sample set, the
forward-error bound of the statistics' accumulation, and seeded synthetic histories.

The bound.  u = 2^-53, V = max |v| over the samples.  A record (n, mean, M2) is built by a chain of operations, each
either Welford's update (Chan's merge with a single sample) or Chan's merge of two records; a merge with an empty side
returns the other side's bits.  L is the longest chain of such operations a sample goes through:
  per trajectory (one wave, lanes stride over t)   ceil(T / 64) Welford updates, then 6 butterfly stages;
  pooled over K kept trajectories (one workgroup)   + ceil(K / 256) merges per thread, 6 butterfly stages, 3 wave merges;
  batch.merge_stats of p parts                      + p - 1.
Mean.  The merged mean ma + (mb - ma) (nb / n) is a convex combination of the inputs, so their errors do not grow:
the result's error is at most the larger input error plus the operation's own roundings -- the difference (2uV), the
weight and the product (relative 2u of a term of size 2V: 4uV), the sum (uV) -- fewer than 8uV.  Hence
    |mean - exact| <= 8 L u V.
M2 / n.  The two M2 terms enter with weights na / n and nb / n (convex again).  The term delta^2 na nb / n^2 has
|delta| <= 2V and weight <= 1/4; delta carries both means' errors, 2 (8 L u V) + 2uV, so delta^2 is off by at most
4V (16 L + 2) u V and the term by (16 L + 2) u V^2; the roundings of the square, the two products and the two sums
(each of a quantity <= V^2) add fewer than 6uV^2.  Per operation (16 L + 8) u V^2, so
    |M2 / n - exact variance| <= (16 L^2 + 8 L) u V^2.
Both are of the form c n u V^k with n the sample count: at T = 130 (L = 9) c = 8 L / n = 0.55 for the mean and
(16 L^2 + 8 L) / n = 10.5 for the variance; pooled over 67 such trajectories (n = 8710, L = 19) 0.017 and 0.68.  L counts
every stage, also those whose other side is empty (T < 64), so it over-counts there; the bound is kept at that L.  With
V <= 1.1 every bound used is below 1e-12 (assert_moments asserts that before using one).
"""
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53


def exact_moments(v):
    """(mean, variance with ddof = 0) of the float samples v in exact rational arithmetic, rounded once at the end."""
    fr = [Fraction(float(x)) for x in np.asarray(v, dtype=np.float64).ravel()]
    n = len(fr)
    mean = sum(fr, Fraction(0)) / n
    var = sum(((x - mean) ** 2 for x in fr), Fraction(0)) / n
    return float(mean), float(var)


def chain_length(T, pooled_over=0, parts=1):
    """L of the module docstring: per trajectory; + the pool over `pooled_over` kept trajectories; + merge_stats of
    `parts` parts."""
    L = -(-int(T) // 64) + 6
    if pooled_over:
        L += -(-int(pooled_over) // 256) + 6 + 3
    return L + (int(parts) - 1)


def mean_bound(L, V):
    return 8.0 * L * U53 * V


def var_bound(L, V):
    return (16.0 * L * L + 8.0 * L) * U53 * V * V


def assert_moments(rec, samples, L, what=""):
    """rec (n, mean, M2, min, max) against the exact moments of `samples` within the bounds for chain length L; n, min
    and max exactly."""
    v = np.asarray(samples, dtype=np.float64).ravel()
    V = float(np.abs(v).max())
    mb, vb = mean_bound(L, V), var_bound(L, V)
    assert mb < 1e-12 and vb < 1e-12, (what, L, V, mb, vb)
    mean, var = exact_moments(v)
    assert rec[0] == v.size, (what, rec[0], v.size)
    assert abs(rec[1] - mean) <= mb, (what, "mean", rec[1], mean, abs(rec[1] - mean), mb)
    assert abs(rec[2] / rec[0] - var) <= vb, (what, "var", rec[2] / rec[0], var, abs(rec[2] / rec[0] - var), vb)
    assert rec[3] == v.min() and rec[4] == v.max(), (what, rec[3], v.min(), rec[4], v.max())
    return abs(rec[1] - mean), abs(rec[2] / rec[0] - var)


def synthetic_history(seed, B, T):
    """Seeded histories of the closed loop's shapes and ranges (no solver behind them): X [B,T+1,6], U [B,T,2],
    u0 [B,2], parabola coefficients pcs [B,4] (kind 0), vref0 [B]."""
    rng = np.random.default_rng(seed)
    X = np.empty((B, T + 1, 6))
    X[:, :, 0] = rng.uniform(-2, 2, (B, 1)) + np.cumsum(rng.uniform(0.01, 0.04, (B, T + 1)), axis=1)
    pcs = np.zeros((B, 4))
    pcs[:, 2] = rng.uniform(0.05, 0.15, B)
    X[:, :, 1] = pcs[:, 2:3] * X[:, :, 0] ** 2 + rng.uniform(-0.3, 0.3, (B, T + 1))
    X[:, :, 2] = np.arctan(2 * pcs[:, 2:3] * X[:, :, 0]) + rng.uniform(-0.2, 0.2, (B, T + 1))
    X[:, :, 3] = rng.uniform(0.4, 1.6, (B, T + 1))
    X[:, :, 4] = rng.uniform(-0.05, 0.05, (B, T + 1))
    X[:, :, 5] = rng.uniform(-1, 1, (B, T + 1))
    U = np.stack([rng.uniform(-0.2, 0.9, (B, T)), rng.uniform(-0.5, 0.5, (B, T))], axis=2)
    u0 = np.stack([rng.uniform(0.1, 0.3, B), np.zeros(B)], axis=1)
    return X, U, u0, pcs, np.full(B, 0.8)


def fsum_record(v):
    """(n, mean, M2, min, max) of the samples with math.fsum sums (the mean's sum is exact; each squared deviation is
    rounded before its exact sum)."""
    v = [float(x) for x in np.asarray(v, dtype=np.float64).ravel()]
    mean = math.fsum(v) / len(v)
    return np.array([len(v), mean, math.fsum((x - mean) ** 2 for x in v), min(v), max(v)])

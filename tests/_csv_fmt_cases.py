"""Values shared by the CSV formatter tests (test_csv_format_host.py, test_csv_format_gpu.py)."""
import math
import sys

import numpy as np


def edge_values():
    """Signed zeros, infinities, NaN, the subnormal / normal / overflow boundaries, the values where repr changes
    notation (1e-4, 1e16), every power of two and the neighbours of 10^k for k = -20 .. 22; each also negated."""
    inf = float("inf")
    v = [0.0, -0.0, inf, -inf, float("nan"),
         5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, sys.float_info.max,
         1e-5, 1e-4, 9.999999999999999e-05, 0.0001, 1e15, 1e16, 9999999999999998.0, 123456789012345.6, 1e22, 1e23,
         5e-324, 0.1, 0.3, 2 / 3]
    v += [math.ldexp(1.0, k) for k in range(-1074, 1024)]
    for k in range(-20, 23):
        p = float(f"1e{k}")
        v += [math.nextafter(p, 0.0), p, math.nextafter(p, inf)]
    v += [-x for x in v]
    return np.array(v, dtype=np.float64)


def py_fields(v):
    """What the CSV holds for each value: repr(float), NaN as the empty field."""
    return [b"" if x != x else repr(x).encode() for x in v.tolist()]

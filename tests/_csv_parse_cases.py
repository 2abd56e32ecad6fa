"""Tokens shared by the CSV parser tests (test_csv_parse_host.py, test_csv_parse_gpu.py).  The reference of every
token is Python's float(): the correctly rounded double."""
import functools
import struct

import numpy as np

from tests._csv_fmt_cases import edge_values


def float_bits(tokens):
    """float(token) of every token as uint64 bit patterns."""
    return np.array([struct.unpack("<Q", struct.pack("<d", float(t)))[0] for t in tokens], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def edge_spellings():
    """repr, %.17e and %.18e (19 digits) of every finite edge value."""
    v = edge_values()
    v = v[np.isfinite(v)].tolist()
    return [s.encode() for x in v for s in (repr(x), "%.17e" % x, "%.18e" % x)]


@functools.lru_cache(maxsize=None)
def random_reprs():
    """repr of the finite values among the 200,000 random bit patterns test_format_f64_batch_equals_repr draws."""
    v = np.random.default_rng(5).integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64)
    return [repr(x).encode() for x in v[np.isfinite(v)].tolist()]


@functools.lru_cache(maxsize=None)
def random_19_digits():
    """%.18e of 50,000 of them."""
    v = np.random.default_rng(5).integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64)
    return [("%.18e" % x).encode() for x in v[np.isfinite(v)][:50_000].tolist()]


@functools.lru_cache(maxsize=None)
def halfway_integers():
    """Exact halfway cases: odd multiples of half an ulp in [2^53, 2^64), at most 19 digits; the first two by hand."""
    rng = np.random.default_rng(53)
    out = [2 ** 53 + 1, 2 ** 53 + 3]
    for k in range(53, 64):
        half = 1 << (k - 53)
        for j in rng.integers(0, 2 ** 52, size=120).tolist():
            v = (1 << k) + (2 * j + 1) * half
            if v < 10 ** 19:
                out.append(v)
    return [str(v).encode() for v in out]


@functools.lru_cache(maxsize=None)
def dataset_magnitudes():
    rng = np.random.default_rng(77)
    v = rng.standard_normal(100_000) * 10.0 ** rng.uniform(-6, 3, 100_000)
    return [repr(x).encode() for x in v.tolist()]


# each gives float()'s bits or is declined, never anything else; the first five must parse
RANGE_EDGES = [b"1e999", b"-1e-999", b"1.7976931348623159e308", b"2.4703282292062327e-324", b"2.4703282292062328e-324",
               b"0." + b"0" * 60 + b"123456789", b"0." + b"0" * 3000 + b"17", b"1e99999999999", b"1e-99999999999"]
# declined, the output left untouched
FALLBACKS = [b"123456789012345678901234567890", b"+1.0", b" 1.0", b"1.0 ", b"1e", b"--1", b"1.2.3", b"0x10",
             b"infinity"]
NAN_BITS = 0x7FF8000000000000      # <cmath>'s NAN, what the host reader stores for an empty field

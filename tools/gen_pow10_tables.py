"""Writes trajectory_generation_amd/csrc/fmt_pow10_tables.h: the 128-bit powers of ten that the shortest-round-trip
double formatter (csrc/fmt_f64.h, Schubfach: R. Giulietti, "The Schubfach way to render doubles", 2020) multiplies by.

  python tools/gen_pow10_tables.py [--check-only] [--out PATH]                 (Python integers only)

For every decimal exponent k the formatter can need (a double's binary exponent q runs over -1074 .. 971, so
-floor(log10 2^q) runs over FMT_POW10_LO = -292 .. FMT_POW10_HI = 324 of fmt_f64.h) the table holds
    g(k) = ceil(10^k * 2^(127 - e(k))),   e(k) = floor(log2 10^k),
so 2^127 <= g(k) < 2^128 and 10^k = g(k) 2^(e(k) - 127) (1 - eps), 0 <= eps < 2^-127; g is exact where 10^k has at
most 128 significant bits (k = 0 .. 55).  Each entry is two 64-bit words, high word first.

The formatter also replaces two logarithms by integer multiplies and shifts.  This script proves them on the whole
range the formatter uses before it writes anything:
    floor(log2 10^k)      == (k * 1741647) >> 19              for |k| <= 350
    floor(log10 2^q)      == (q * 1262611) >> 22              for |q| <= 1100
    floor(log10 (3/4) 2^q) == (q * 1262611 - 524031) >> 22    for |q| <= 1100
"""
import argparse
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "trajectory_generation_amd", "csrc", "fmt_pow10_tables.h")
K_MIN, K_MAX = -292, 324


def floor_log2_pow10(k):
    """floor(log2 10^k), exact."""
    if k >= 0:
        return (10 ** k).bit_length() - 1
    return -(10 ** -k).bit_length()      # 10^-k is no power of two for k < 0


def floor_log10_pow2(q, three_quarters=False):
    """floor(log10 (2^q)) or floor(log10 (3/4 2^q)), exact: the largest d with 10^d <= num / den."""
    num, den = (3 if three_quarters else 1), (4 if three_quarters else 1)
    if q >= 0:
        num <<= q
    else:
        den <<= -q
    d = (len(str(num)) - 1) - (len(str(den)) - 1)     # within one of the answer
    d += 1
    while not (10 ** d * den <= num if d >= 0 else den <= num * 10 ** -d):
        d -= 1
    return d


def g(k):
    e = floor_log2_pow10(k)
    if k >= 0:
        p, s = 10 ** k, e - 127
        v = -((-p) >> s) if s > 0 else p << -s           # ceil(p / 2^s)
    else:
        p = 10 ** -k
        v = -((-(1 << (127 - e))) // p)                   # ceil(2^(127 - e) / p)
    assert 1 << 127 <= v < 1 << 128, k
    return v


def check_logs():
    for k in range(-350, 351):
        assert (k * 1741647) >> 19 == floor_log2_pow10(k), k
    for q in range(-1100, 1101):
        assert (q * 1262611) >> 22 == floor_log10_pow2(q), q
        assert (q * 1262611 - 524031) >> 22 == floor_log10_pow2(q, True), q


def text():
    lines = [
        "// fmt_pow10_tables.h -- written by tools/gen_pow10_tables.py (do not edit): g(k) = ceil(10^k 2^(127 - e)),",
        f"// e = floor(log2 10^k), for k = {K_MIN} .. {K_MAX} (fmt_f64.h FMT_POW10_LO / _HI), as {{high, low}} 64-bit words.  Plain constant",
        "// arrays; the includer sets FMT_POW10_DECL (storage, e.g. `static const`) and FMT_POW10_NAME (the array's name)",
        "// and may include the file once per copy it needs.",
        f"FMT_POW10_DECL unsigned long long FMT_POW10_NAME[{K_MAX - K_MIN + 1}][2] = {{",
    ]
    for k in range(K_MIN, K_MAX + 1):
        v = g(k)
        lines.append(f"    {{0x{v >> 64:016X}ULL, 0x{v & (2 ** 64 - 1):016X}ULL}},  // {k}")
    lines += ["};", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    check_logs()
    t = text()
    if a.check_only:
        same = os.path.exists(a.out) and open(a.out).read() == t
        print("identical" if same else "DIFFERENT", a.out)
        raise SystemExit(0 if same else 1)
    with open(a.out, "w") as f:
        f.write(t)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

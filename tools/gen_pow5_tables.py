"""Writes trajectory_generation_amd/csrc/parse_pow5_tables.h: the 128-bit normalised powers of five that the decimal
parser (csrc/parse_f64.h, Eisel-Lemire: D. Lemire, "Number parsing at a gigabyte per second", 2021) multiplies by.

  python tools/gen_pow5_tables.py [--check-only] [--out PATH]                  (Python integers only)

For every decimal exponent q = PARSE_POW5_LO = -342 .. PARSE_POW5_HI = 308 of parse_f64.h the table holds t(q) with
2^127 <= t(q) < 2^128 and 5^q ~ t(q) 2^b:
    q >= 0          t = floor(5^q 2^s), the top 128 bits of 5^q (exact for q <= 55: 5^55 < 2^128);
    -27 <= q < 0    t = floor(2^(z + 127) / 5^-q) + 1, z = ceil(log2 5^-q)      (the reciprocal, rounded up);
    q < -27         t = the top 128 bits of floor(2^(2 z + 128) / 5^-q) + 1     (truncated: a floor).
Each entry is two 64-bit words, high word first.  fmt_pow10_tables.h (ceilings, -292 .. 324) does not serve here.

The parser replaces floor(log2 5^q) + q by an integer multiply and shift; this script proves it on the whole range
before it writes anything:
    floor(log2 10^q) == (q * 217706) >> 16              for -342 <= q <= 308
"""
import argparse
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "trajectory_generation_amd", "csrc", "parse_pow5_tables.h")
Q_MIN, Q_MAX = -342, 308


def t(q):
    if q >= 0:
        p = 5 ** q
        n = p.bit_length()
        v = p << (128 - n) if n <= 128 else p >> (n - 128)
    else:
        p = 5 ** -q
        z = (p - 1).bit_length()             # the least z with 2^z >= p
        if q >= -27:
            v = (1 << (z + 127)) // p + 1
        else:
            v = (1 << (2 * z + 128)) // p + 1
            v >>= v.bit_length() - 128
    assert 1 << 127 <= v < 1 << 128, q
    return v


def floor_log2_pow10(q):
    if q >= 0:
        return (10 ** q).bit_length() - 1
    return -(10 ** -q).bit_length()          # 10^-q is no power of two for q < 0


def check_logs():
    for q in range(Q_MIN, Q_MAX + 1):
        assert (q * 217706) >> 16 == floor_log2_pow10(q), q


def text():
    lines = [
        "// parse_pow5_tables.h -- written by tools/gen_pow5_tables.py (do not edit): the top 128 bits of 5^q for",
        f"// q = {Q_MIN} .. {Q_MAX} (parse_f64.h PARSE_POW5_LO / _HI), as {{high, low}} 64-bit words: floors for q >= 0 and q < -27,",
        "// the reciprocal rounded up for -27 <= q < 0.  Plain constant arrays; the includer sets PARSE_POW5_DECL (storage,",
        "// e.g. `static const`) and PARSE_POW5_NAME (the array's name) and may include the file once per copy it needs.",
        f"PARSE_POW5_DECL unsigned long long PARSE_POW5_NAME[{Q_MAX - Q_MIN + 1}][2] = {{",
    ]
    for q in range(Q_MIN, Q_MAX + 1):
        v = t(q)
        lines.append(f"    {{0x{v >> 64:016X}ULL, 0x{v & (2 ** 64 - 1):016X}ULL}},  // {q}")
    lines += ["};", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    check_logs()
    txt = text()
    if a.check_only:
        same = os.path.exists(a.out) and open(a.out).read() == txt
        print("identical" if same else "DIFFERENT", a.out)
        raise SystemExit(0 if same else 1)
    with open(a.out, "w") as f:
        f.write(txt)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

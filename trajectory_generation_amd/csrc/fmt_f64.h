// fmt_f64.h -- Python's repr(float) for host and device: the shortest decimal that round-trips (the closest one if
// several are shortest), fixed notation for decimal exponents -4 .. 15 with at least one fractional digit, otherwise
// d[.ddd]e+XX; -0.0, inf, -inf; NaN as the empty field (the CSV spelling of dataset_csv.cpp's py_repr).  At most
// FMT_F64_MAX = 24 characters.  Also int64 in decimal.
//
// Digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020), integer arithmetic only -- one
// 128-bit power of ten from fmt_pow10_tables.h (tools/gen_pow10_tables.py) and three 64 x 128-bit multiplies per
// value; no libm, no floating-point operation.  The digits stay in one 64-bit integer: a value is first decomposed
// (fmt_decompose -> FmtDec: sign, digits, digit count, decimal exponent), its printed length follows from that alone
// (fmt_len), and fmt_emit writes exactly fmt_len characters to their destination, last digit first -- no per-thread
// character buffer, so nothing is indexed at run time in private memory.
//
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#ifndef TGMPC_FMT_F64_H
#define TGMPC_FMT_F64_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FMT_HD __host__ __device__ __forceinline__
#else
#define FMT_HD inline
#endif

#define FMT_F64_MAX 24     /* -1.2345678901234567e-308 */
#define FMT_I64_MAX 20     /* -9223372036854775808 */
#define FMT_POW10_LO (-292)
#define FMT_POW10_HI 324

namespace tgfmt {

typedef const unsigned long long (*Pow10Table)[2];   // [FMT_POW10_HI - FMT_POW10_LO + 1][2], {high, low}

enum { FMT_FINITE = 0, FMT_NAN = 1, FMT_INF = 2 };

struct FmtDec {
    uint64_t d;   // the digits, no trailing zero (0 for +-0.0)
    int nd;       // how many: 1 .. 17
    int e;        // decimal exponent of the first digit: value = d.ddd x 10^e
    int kind;     // FMT_FINITE / FMT_NAN / FMT_INF
    int neg;      // sign bit
};

// floor(g * cp / 2^128) with the discarded bits ORed into bit 0 (round to odd); g = {hi, lo}, cp < 2^60
FMT_HD uint64_t fmt_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    const unsigned __int128 x = (unsigned __int128)glo * cp;
    const unsigned __int128 y = (unsigned __int128)ghi * cp + (uint64_t)(x >> 64);
    const uint64_t y0 = (uint64_t)y, y1 = (uint64_t)(y >> 64);
    return y1 | (uint64_t)(y0 > 1);
}

// Shortest digits of the positive finite double c * 2^q given as its IEEE fields (Schubfach, figures 4 and 6):
// returns s, sets k, value ~ s * 10^k; s may end in zeros.
FMT_HD uint64_t fmt_schubfach(uint64_t frac, int bexp, Pow10Table g, int& k_out) {
    uint64_t c;
    int q;
    if (bexp != 0) {
        c = (1ull << 52) | frac;
        q = bexp - 1075;
    } else {
        c = frac;
        q = -1074;
    }
    const bool even = (c & 1) == 0;
    const bool closer = frac == 0 && bexp > 1;      // the lower neighbour is half as far
    const uint64_t cbl = 4 * c - 2 + (closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    // floor(log10 2^q), or floor(log10 3/4 2^q); an arithmetic shift (tools/gen_pow10_tables.py checks both)
    const int k = (q * 1262611 - (closer ? 524031 : 0)) >> 22;
    const int h = q + ((-k * 1741647) >> 19) + 1;   // 1 .. 4
    const uint64_t ghi = g[-k - FMT_POW10_LO][0], glo = g[-k - FMT_POW10_LO][1];
    const uint64_t vbl = fmt_round_to_odd(ghi, glo, cbl << h);
    const uint64_t vb = fmt_round_to_odd(ghi, glo, cb << h);
    const uint64_t vbr = fmt_round_to_odd(ghi, glo, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb >> 2;
    if (s >= 10) {
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) {
            k_out = k + 1;
            return sp + (wp_in ? 1 : 0);
        }
    }
    k_out = k;
    const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
    if (u_in != w_in) return s + (w_in ? 1 : 0);
    const uint64_t mid = 4 * s + 2;
    const bool up = vb > mid || (vb == mid && (s & 1) != 0);
    return s + (up ? 1 : 0);
}

FMT_HD FmtDec fmt_decompose(double v, Pow10Table g) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    FmtDec r;
    r.neg = (int)(b >> 63);
    const uint64_t frac = b & ((1ull << 52) - 1);
    const int bexp = (int)((b >> 52) & 0x7FF);
    r.d = 0;
    r.nd = 1;
    r.e = 0;
    r.kind = FMT_FINITE;
    if (bexp == 0x7FF) {
        r.kind = frac ? FMT_NAN : FMT_INF;
        return r;
    }
    if ((b << 1) == 0) return r;     // +-0.0: the digit 0
    int k;
    uint64_t d = fmt_schubfach(frac, bexp, g, k);
    // trailing zeros off (d < 10^17: eight at once first, then one at a time in 32 bits where it fits)
    if (d % 100000000u == 0) {
        d /= 100000000u;
        k += 8;
    }
    while (d != 0 && d % 10 == 0) {
        d /= 10;
        ++k;
    }
    int nd = 1;
    for (uint64_t t = 10; d >= t; t *= 10) ++nd;    // t <= 10^17 < 2^64
    r.d = d;
    r.nd = nd;
    r.e = k + nd - 1;
    return r;
}

FMT_HD int fmt_len(const FmtDec& x) {
    if (x.kind == FMT_NAN) return 0;
    if (x.kind == FMT_INF) return 3 + x.neg;
    const int e = x.e, nd = x.nd;
    int n;
    if (e >= -4 && e < 16) {
        if (e < 0) n = 1 - e + nd;                  // 0. + (-e - 1) zeros + digits
        else n = nd > e + 1 ? nd + 1 : e + 3;       // ddd.ddd, or digits + zeros + .0
    } else {
        n = (nd > 1 ? nd + 1 : 1) + 2 + ((e < 0 ? -e : e) >= 100 ? 3 : 2);
    }
    return n + x.neg;
}

// digit i (0 = first) of the nd-digit d < 10^17 to p[i + (i > dot)]: the caller puts '.' at p[dot + 1]
FMT_HD void fmt_put_digits(char* p, uint64_t d, int nd, int dot) {
    uint32_t lo = (uint32_t)(d % 100000000u), hi = (uint32_t)(d / 100000000u);
    int i = nd - 1;
    const int nlo = nd < 8 ? nd : 8;
    for (int j = 0; j < nlo; ++j, --i) {
        p[i + (i > dot ? 1 : 0)] = (char)('0' + lo % 10);
        lo /= 10;
    }
    for (; i >= 0; --i) {
        p[i + (i > dot ? 1 : 0)] = (char)('0' + hi % 10);
        hi /= 10;
    }
}

// writes fmt_len(x) characters at p
FMT_HD void fmt_emit(const FmtDec& x, char* p) {
    if (x.kind == FMT_NAN) return;
    if (x.neg) *p++ = '-';
    if (x.kind == FMT_INF) {
        p[0] = 'i'; p[1] = 'n'; p[2] = 'f';
        return;
    }
    const int e = x.e, nd = x.nd;
    if (e >= -4 && e < 16) {
        if (e < 0) {
            p[0] = '0';
            p[1] = '.';
            for (int i = 0; i < -e - 1; ++i) p[2 + i] = '0';
            fmt_put_digits(p + 1 - e, x.d, nd, nd);
        } else if (nd > e + 1) {
            fmt_put_digits(p, x.d, nd, e);
            p[e + 1] = '.';
        } else {
            fmt_put_digits(p, x.d, nd, nd);
            for (int i = nd; i <= e; ++i) p[i] = '0';
            p[e + 1] = '.';
            p[e + 2] = '0';
        }
    } else {
        fmt_put_digits(p, x.d, nd, 0);
        char* q = p + 1;
        if (nd > 1) {
            p[1] = '.';
            q = p + nd + 1;
        }
        int ae = e < 0 ? -e : e;
        q[0] = 'e';
        q[1] = e < 0 ? '-' : '+';
        q += 2;
        if (ae >= 100) {
            *q++ = (char)('0' + ae / 100);
            ae %= 100;
        }
        q[0] = (char)('0' + ae / 10);
        q[1] = (char)('0' + ae % 10);
    }
}

// one double at p (room for FMT_F64_MAX characters); returns the length
FMT_HD int fmt_f64(double v, Pow10Table g, char* p) {
    const FmtDec x = fmt_decompose(v, g);
    fmt_emit(x, p);
    return fmt_len(x);
}

// ---- int64 in decimal (std::to_chars' spelling) ----
FMT_HD int fmt_i64_len(long long v) {
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    int n = 1;
    while (m >= 10) {
        m /= 10;
        ++n;
    }
    return n + (v < 0 ? 1 : 0);
}

// writes n = fmt_i64_len(v) characters at p
FMT_HD void fmt_i64_emit(long long v, int n, char* p) {
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (v < 0) p[0] = '-';
    for (int i = n - 1; i >= (v < 0 ? 1 : 0); --i) {
        p[i] = (char)('0' + m % 10);
        m /= 10;
    }
}

}  // namespace tgfmt

#endif

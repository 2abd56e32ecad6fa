// parse_f64.h -- one CSV field of decimal text to the nearest double, for host and device: the inverse of fmt_f64.h.
//
// parse_field(s, e, g, out) takes the field [s, e):
//   the empty field                      NaN (the CSV spelling fmt_f64.h writes; the bits of <cmath>'s NAN)
//   -?digits[.digits][(e|E)[+-]digits]   and the .digits / digits. forms std::from_chars takes; any number of leading
//                                        zeros; exponent digits saturate
//   nan  NaN  inf  -inf
// and returns PARSE_OK with *out written, or PARSE_FALLBACK with nothing written for everything else: more than 19
// significant digits (after leading zeros and the digit string's trailing zeros are dropped), a '+' sign, blanks, any
// other byte.  It never guesses: what it declines goes to the host's std::from_chars (csv_token.h).
//
// Value: Eisel-Lemire (D. Lemire, "Number parsing at a gigabyte per second", 2021), integer arithmetic only -- the
// digits in one 64-bit integer w, one or two 64 x 64 -> 128-bit multiplies by the 128-bit power of five of
// parse_pow5_tables.h (tools/gen_pow5_tables.py) for decimal exponents -342 .. 308, round to even on the exact halfway
// products of -4 <= q <= 23, subnormals, underflow to +-0 and overflow to +-inf.  No ambiguous case remains for a
// 64-bit w (J. Mushtak, D. Lemire, "Fast number parsing without fallback", 2023), so there is no check for one.  No
// libm, no floating-point operation, no per-thread character buffer: the field is read once, byte by byte.
//
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#ifndef TGMPC_PARSE_F64_H
#define TGMPC_PARSE_F64_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PARSE_HD __host__ __device__ __forceinline__
#else
#define PARSE_HD inline
#endif

#define PARSE_OK 0
#define PARSE_FALLBACK 1
#define PARSE_POW5_LO (-342)
#define PARSE_POW5_HI 308
#define PARSE_MAX_DIGITS 19          /* 10^19 - 1 < 2^64 */
#define PARSE_EXP_SAT 100000         /* exponent digits stop counting here: far past every finite double */

namespace tgparse {

typedef const unsigned long long (*Pow5Table)[2];   // [PARSE_POW5_HI - PARSE_POW5_LO + 1][2], {high, low}

PARSE_HD int parse_clz64(uint64_t x) {              // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The IEEE bits (sign excluded) of the double nearest to w * 10^q.
PARSE_HD uint64_t parse_eisel_lemire(uint64_t w, long long q, Pow5Table g) {
    const uint64_t inf = 0x7FF0000000000000ull;
    if (w == 0 || q < PARSE_POW5_LO) return 0;      // w < 10^19: w 10^-343 < 2^-1075, half the least subnormal
    if (q > PARSE_POW5_HI) return inf;
    int lz = parse_clz64(w);
    w <<= lz;
    // the top 128 bits of w * 5^q; the low half of the power only when the high half leaves the 55 bits undecided
    const uint64_t phi = g[q - PARSE_POW5_LO][0], plo = g[q - PARSE_POW5_LO][1];
    const unsigned __int128 first = (unsigned __int128)w * phi;
    uint64_t upper = (uint64_t)(first >> 64), lower = (uint64_t)first;
    if ((upper & 0x1FF) == 0x1FF) {
        const uint64_t second_hi = (uint64_t)(((unsigned __int128)w * plo) >> 64);
        lower += second_hi;
        if (second_hi > lower) ++upper;
    }
    const int upperbit = (int)(upper >> 63);
    uint64_t m = upper >> (upperbit + 9);           // 54 bits: the significand and one rounding bit
    // the biased binary exponent; floor(log2 10^q) = (217706 q) >> 16 on this range (tools/gen_pow5_tables.py checks it)
    int p2 = (int)((217706 * q) >> 16) + 63 + upperbit - lz + 1023;
    if (p2 <= 0) {                                  // subnormal, or zero
        if (-p2 + 1 >= 64) return 0;
        m >>= -p2 + 1;
        m += m & 1;
        m >>= 1;
        return m;                                   // m = 2^52 is the least normal: its bits are already right
    }
    // exactly halfway between two doubles: to even.  Only 5^q that fit 64 bits can give it (-4 <= q <= 23).
    if (lower <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << (upperbit + 9)) == upper) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {
        m = 1ull << 52;
        ++p2;
    }
    m &= ~(1ull << 52);
    if (p2 >= 0x7FF) return inf;
    return ((uint64_t)p2 << 52) | m;
}

PARSE_HD void parse_store(double* out, uint64_t bits) { memcpy(out, &bits, sizeof(bits)); }

PARSE_HD int parse_field(const char* s, const char* e, Pow5Table g, double* out) {
    const uint64_t nan_bits = 0x7FF8000000000000ull, inf_bits = 0x7FF0000000000000ull;
    if (s == e) {
        parse_store(out, nan_bits);
        return PARSE_OK;
    }
    const long long n = e - s;
    if (n == 3 && s[0] == 'n' && s[1] == 'a' && s[2] == 'n') { parse_store(out, nan_bits); return PARSE_OK; }
    if (n == 3 && s[0] == 'N' && s[1] == 'a' && s[2] == 'N') { parse_store(out, nan_bits); return PARSE_OK; }
    if (n == 3 && s[0] == 'i' && s[1] == 'n' && s[2] == 'f') { parse_store(out, inf_bits); return PARSE_OK; }
    if (n == 4 && s[0] == '-' && s[1] == 'i' && s[2] == 'n' && s[3] == 'f') {
        parse_store(out, inf_bits | (1ull << 63));
        return PARSE_OK;
    }
    const char* p = s;
    const uint64_t sign = *p == '-' ? 1ull << 63 : 0;
    if (sign) ++p;
    // One pass over the digits.  w holds the significant digits up to the last non-zero one; zeros after it wait in
    // `zeros` until another non-zero digit shows they are inside the number (trailing ones never reach w).
    uint64_t w = 0;
    int nd = 0;                  // digits in w
    long long zeros = 0;         // zeros seen since the last non-zero digit (once w != 0)
    long long pos = 0;           // digits read, leading zeros included
    long long last_sig = 0;      // pos just after the last non-zero digit
    long long dot = -1;          // pos at the '.', -1 if none
    for (; p < e; ++p) {
        const unsigned c = (unsigned char)*p;
        if (c == '.') {
            if (dot >= 0) return PARSE_FALLBACK;
            dot = pos;
            continue;
        }
        const unsigned d = c - '0';
        if (d > 9) break;
        ++pos;
        if (d == 0) {
            if (w != 0) ++zeros;
            continue;
        }
        if (nd + zeros + 1 > PARSE_MAX_DIGITS) return PARSE_FALLBACK;
        for (; zeros > 0; --zeros, ++nd) w *= 10;
        w = w * 10 + d;
        ++nd;
        last_sig = pos;
    }
    if (pos == 0) return PARSE_FALLBACK;              // no digit: "", "-", ".", "e5", ...
    long long ex = 0;
    if (p < e) {
        if (*p != 'e' && *p != 'E') return PARSE_FALLBACK;
        ++p;
        bool eneg = false;
        if (p < e && (*p == '+' || *p == '-')) {
            eneg = *p == '-';
            ++p;
        }
        if (p == e) return PARSE_FALLBACK;
        for (; p < e; ++p) {
            const unsigned d = (unsigned)(unsigned char)*p - '0';
            if (d > 9) return PARSE_FALLBACK;
            if (ex < PARSE_EXP_SAT) ex = ex * 10 + d;
        }
        if (eneg) ex = -ex;
    }
    // value = w * 10^q: the digits between the last significant one and the decimal point (either side) move q
    const long long q = (dot < 0 ? pos : dot) - last_sig + ex;
    parse_store(out, sign | parse_eisel_lemire(w, q, g));
    return PARSE_OK;
}

}  // namespace tgparse

#endif

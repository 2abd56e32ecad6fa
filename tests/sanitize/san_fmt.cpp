// san_fmt.cpp -- csrc/fmt_f64.h on the host under AddressSanitizer / UBSan: every value is formatted into an exactly
// sized heap block (fmt_len bytes, so one byte too many is a report) and compared with std::to_chars laid out as
// Python's repr (the host CSV writer's py_repr).  Edge list, every power of two, the neighbours of the powers of ten,
// 10^6 random bit patterns, 10^5 values of dataset magnitude, and int64.  Prints "san_fmt ok".
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../trajectory_generation_amd/csrc/fmt_f64.h"

#define FMT_POW10_DECL static const
#define FMT_POW10_NAME pow10_host
#include "../../trajectory_generation_amd/csrc/fmt_pow10_tables.h"

static std::string py_repr(double v) {
    if (std::isnan(v)) return "";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char sci[64];
    auto r = std::to_chars(sci, sci + sizeof(sci), v, std::chars_format::scientific);
    *r.ptr = 0;
    std::string s, dig;
    const char* p = sci;
    if (*p == '-') { s += '-'; ++p; }
    for (; *p && *p != 'e'; ++p)
        if (*p != '.') dig += *p;
    const int e = std::atoi(p + 1), nd = (int)dig.size();
    if (e >= -4 && e < 16) {
        if (e < 0) {
            s += "0." + std::string(-e - 1, '0') + dig;
        } else {
            for (int i = 0; i <= e; ++i) s += i < nd ? dig[i] : '0';
            s += '.';
            s += nd > e + 1 ? dig.substr(e + 1) : "0";
        }
    } else {
        s += dig[0];
        if (nd > 1) s += "." + dig.substr(1);
        char eb[16];
        std::snprintf(eb, sizeof(eb), "e%c%02d", e < 0 ? '-' : '+', std::abs(e));
        s += eb;
    }
    return s;
}

static long long checked = 0;

static void check(double v) {
    const tgfmt::FmtDec x = tgfmt::fmt_decompose(v, pow10_host);
    const int n = tgfmt::fmt_len(x);
    std::unique_ptr<char[]> buf(new char[n ? n : 1]);
    tgfmt::fmt_emit(x, buf.get());
    const std::string want = py_repr(v);
    if (n > FMT_F64_MAX || (size_t)n != want.size() || std::memcmp(buf.get(), want.data(), n) != 0) {
        uint64_t b;
        std::memcpy(&b, &v, 8);
        std::printf("MISMATCH bits %016llx: got '%.*s' want '%s'\n", (unsigned long long)b, n, buf.get(), want.c_str());
        std::exit(1);
    }
    ++checked;
}

static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double edge[] = {0.0, -0.0, inf, -inf, std::nan(""), 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308,
                           1.7976931348623157e308, 1e-5, 1e-4, 9.999999999999999e-05, 0.0001, 1e15, 1e16,
                           9999999999999998.0, 123456789012345.6, 1e22, 1e23, 0.1, 0.3, 2.0 / 3.0, 1.0, -1.5, 0.5,
                           1.2345678901234567e-300, -1.2345678901234567e-308};
    for (double v : edge) { check(v); check(-v); }
    for (int k = -1074; k <= 1023; ++k) check(std::ldexp(1.0, k));
    for (int k = -20; k <= 22; ++k) {
        const double p = std::strtod(("1e" + std::to_string(k)).c_str(), nullptr);
        check(p);
        check(std::nextafter(p, 0.0));
        check(std::nextafter(p, inf));
    }
    uint64_t s = 2024;
    for (int i = 0; i < 1000000; ++i) check(from_bits(splitmix(s)));
    for (int i = 0; i < 100000; ++i) {
        // dataset magnitude: a mantissa in [1, 2) scaled by 2^-20 .. 2^10, either sign
        const uint64_t r = splitmix(s);
        const int ex = 1023 - 20 + (int)(splitmix(s) % 31);
        check(from_bits((r & 0x800FFFFFFFFFFFFFull) | ((uint64_t)ex << 52)));
    }
    const long long ints[] = {0, 1, -1, 9, 10, 99, 100, 1099511627777LL, -1099511627777LL,
                              std::numeric_limits<long long>::max(), std::numeric_limits<long long>::min()};
    for (long long v : ints) {
        const int n = tgfmt::fmt_i64_len(v);
        std::unique_ptr<char[]> buf(new char[n]);
        tgfmt::fmt_i64_emit(v, n, buf.get());
        char ref[32];
        const size_t rn = std::to_chars(ref, ref + sizeof(ref), v).ptr - ref;
        if (n > FMT_I64_MAX || (size_t)n != rn || std::memcmp(buf.get(), ref, rn) != 0) {
            std::printf("MISMATCH int %lld\n", v);
            return 1;
        }
    }
    std::printf("san_fmt ok: %lld doubles\n", checked);
    return 0;
}

// san_parse.cpp -- csrc/parse_f64.h and the host token function (csrc/csv_token.h) on the host under AddressSanitizer
// / UBSan.  Every token is copied into an exactly sized heap block, so the field ends at the block's last byte and one
// byte read too many is a report.  What parse_field accepts must have the bits of the host token function (which is
// std::from_chars); what it declines must leave the output untouched.  Spellings: shortest round trip (d.ddde+XX), %.17e and
// %.18e (19 digits) of an edge list, every power of two, the neighbours of the powers of ten, 200,000 random bit
// patterns and 100,000 values of dataset magnitude; exact halfway integers in [2^53, 2^64); range edges; the
// literals; the fallbacks.  Prints "san_parse ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../trajectory_generation_amd/csrc/csv_token.h"
#include "../../trajectory_generation_amd/csrc/parse_f64.h"

#define PARSE_POW5_DECL static const
#define PARSE_POW5_NAME pow5_host
#include "../../trajectory_generation_amd/csrc/parse_pow5_tables.h"

static long long checked = 0, declined = 0;
static const uint64_t UNTOUCHED = 0xA5A5A5A5A5A5A5A5ull;

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// parse_field on an exactly sized copy of tok: the status; *got = the output's bits
static int run(const std::string& tok, uint64_t* got) {
    std::unique_ptr<char[]> buf(new char[tok.size() ? tok.size() : 1]);
    std::memcpy(buf.get(), tok.data(), tok.size());
    double out = from_bits(UNTOUCHED);
    const int st = tgparse::parse_field(buf.get(), buf.get() + tok.size(), pow5_host, &out);
    *got = bits_of(out);
    return st;
}

static void fail(const char* what, const std::string& tok, uint64_t got, uint64_t want) {
    std::printf("MISMATCH (%s) '%s': got %016llx want %016llx\n", what, tok.c_str(), (unsigned long long)got,
                (unsigned long long)want);
    std::exit(1);
}

// tok must parse, to the bits of the host token function
static void must_parse(const std::string& tok) {
    uint64_t got;
    if (run(tok, &got) != PARSE_OK) fail("declined", tok, got, 0);
    std::unique_ptr<char[]> buf(new char[tok.size() ? tok.size() : 1]);
    std::memcpy(buf.get(), tok.data(), tok.size());
    double want = NAN;
    if (!tok.empty() && !tgcsv::csv_token_f64(buf.get(), buf.get() + tok.size(), &want)) fail("host error", tok, got, 0);
    if (got != bits_of(want)) fail("value", tok, got, bits_of(want));
    ++checked;
}

// tok must be declined with the output untouched
static void must_decline(const std::string& tok) {
    uint64_t got;
    if (run(tok, &got) != PARSE_FALLBACK || got != UNTOUCHED) fail("not declined", tok, got, UNTOUCHED);
    ++declined;
}

// either the host's bits or declined, never anything else
static void parse_or_decline(const std::string& tok) {
    uint64_t got;
    if (run(tok, &got) == PARSE_FALLBACK) {
        if (got != UNTOUCHED) fail("declined but written", tok, got, UNTOUCHED);
        ++declined;
        return;
    }
    must_parse(tok);
}

static void spellings(double v, bool long_forms) {
    if (std::isnan(v)) return;
    if (std::isinf(v)) {
        must_parse(v < 0 ? "-inf" : "inf");
        return;
    }
    char b[64];
    auto r = std::to_chars(b, b + sizeof(b), v, std::chars_format::scientific);
    must_parse(std::string(b, r.ptr));
    if (long_forms) {
        std::snprintf(b, sizeof(b), "%.17e", v);
        must_parse(b);
        std::snprintf(b, sizeof(b), "%.18e", v);
        must_parse(b);
    }
}

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double edge[] = {0.0, inf, 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
                           1e-5, 1e-4, 9.999999999999999e-05, 0.0001, 1e15, 1e16, 9999999999999998.0,
                           123456789012345.6, 1e22, 1e23, 0.1, 0.3, 2.0 / 3.0, 1.0, 1.5, 0.5, 1.2345678901234567e-300,
                           1.2345678901234567e-308};
    for (double v : edge) { spellings(v, true); spellings(-v, true); }
    for (int k = -1074; k <= 1023; ++k) { spellings(std::ldexp(1.0, k), true); spellings(-std::ldexp(1.0, k), true); }
    for (int k = -20; k <= 22; ++k) {
        const double p = std::strtod(("1e" + std::to_string(k)).c_str(), nullptr);
        for (double v : {p, std::nextafter(p, 0.0), std::nextafter(p, inf)}) { spellings(v, true); spellings(-v, true); }
    }
    uint64_t s = 2024;
    for (int i = 0; i < 200000; ++i) spellings(from_bits(splitmix(s)), i < 50000);
    for (int i = 0; i < 100000; ++i) {
        // dataset magnitude: a mantissa in [1, 2) scaled by 2^-20 .. 2^10, either sign
        const uint64_t r = splitmix(s);
        const int ex = 1023 - 20 + (int)(splitmix(s) % 31);
        spellings(from_bits((r & 0x800FFFFFFFFFFFFFull) | ((uint64_t)ex << 52)), false);
    }
    // exact halfway integers: odd multiples of half an ulp in [2^53, 2^64), at most 19 digits
    for (int k = 53; k < 64; ++k) {
        const uint64_t half = 1ull << (k - 53);
        for (int i = 0; i < 120; ++i) {
            const uint64_t j = splitmix(s) >> 12;                       // < 2^52
            const uint64_t v = (1ull << k) + (2 * j + 1) * half;        // < 2^(k + 1)
            if (v <= 9999999999999999999ull) must_parse(std::to_string(v));
        }
    }
    must_parse("9007199254740993");      // 2^53 + 1: to even, down
    must_parse("9007199254740995");      // 2^53 + 3: to even, up
    // zeros, range edges
    must_parse("-0.0"); must_parse("0"); must_parse("-0"); must_parse("0e0"); must_parse("000.000e-5");
    must_parse("1e999"); must_parse("-1e-999"); must_parse("1.7976931348623159e308");
    must_parse("2.4703282292062327e-324"); must_parse("2.4703282292062328e-324");
    parse_or_decline("0." + std::string(60, '0') + "123456789");
    parse_or_decline("0." + std::string(3000, '0') + "17");
    parse_or_decline("1e99999999999"); parse_or_decline("1e-99999999999");
    parse_or_decline("1e2147483648"); parse_or_decline("1e-18446744073709551616");
    parse_or_decline(std::string(400, '0') + "1" + std::string(300, '0') + "e-300");
    // forms from_chars takes
    must_parse(".5"); must_parse("5."); must_parse("-.5e1"); must_parse("1E5"); must_parse("1e+05"); must_parse("1e-05");
    must_parse("00012.500"); must_parse("12345678901234567890e-5"); must_parse("1234567890123456789");
    must_parse("9999999999999999999"); must_parse("0.9999999999999999999");
    // literals
    must_parse(""); must_parse("nan"); must_parse("NaN"); must_parse("inf"); must_parse("-inf");
    // declined, output untouched
    for (const char* t : {"123456789012345678901234567890", "12345678901234567891", "+1.0", " 1.0", "1.0 ", "1e", "1e+",
                          "--1", "1.2.3", "0x10", "infinity", "-", ".", "-.", "e5", ".e5", "-nan", "Inf", "INF", "nan ",
                          "1,0", "1e5.0", "1e-", "1d5", "\t1"})
        must_decline(t);
    must_decline(std::string("1\0", 2));
    must_decline(std::string("\xff\xfe", 2));
    std::printf("san_parse ok: %lld parsed, %lld declined\n", checked, declined);
    return 0;
}

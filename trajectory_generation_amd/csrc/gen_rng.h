// gen_rng.h -- numpy's Generator(PCG64) stream, restated for host and device: the same functions draw, bit for bit,
// what np.random.default_rng(seed) draws (numpy/random: pcg64.h, distributions.c), from the state of
// np.random.PCG64(seed): the host hands it over (np.random.PCG64(seed).state) or seed_seq.h computes it from the seed,
// on the host or in the kernel (SeedSequence and PCG64's seeding, restated there).
//
//   Generator call                     here
//   bit_generator.random_raw()         pcg64_next
//   random()                           rng_next_double        (u64 >> 11) * 2^-53
//   uniform(lo, hi)                    rng_uniform            lo + (hi - lo) * next_double, hi - lo formed once
//   choice(a, p=p)                     rng_choice             one next_double through searchsorted(cdf, u, 'right')
//   standard_normal()                  rng_standard_normal    the 256-layer ziggurat, wedge (exp) and tail (log1p)
//   normal(0.0, s)                     rng_normal             0.0 + s * standard_normal
//
// Built with -ffp-contract=off like the rest of the library: no product here may fuse into an fma.  exp and log1p
// come from the platform's libm on the host (what numpy calls) and from the device library on the GPU, which can
// differ in the last bits: the wedge test is a comparison (a flip needs a draw within an ulp of the density, of order
// 2^-52 per wedge draw) and the tail value carries the log1p rounding (|z| > r, about one draw in 4,000).
// A caller that must have the host's bits (dataset_noise.hip) passes a ZigAudit: it gets the two uniforms of an
// accepted tail draw, to recompute the value with the host's libm, and a flag for every comparison against exp or
// log1p whose two sides lie within a relative tie_margin, which it must not trust.  Without one nothing changes.
// The tables are passed in (ZigTables): constant arrays on the host, a copy in LDS in the kernels -- lanes index
// them with a random layer.
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RNG_HD __host__ __device__ __forceinline__
#define RNG_HD_OUTLINE __host__ __device__ inline
#else
#define RNG_HD inline
#define RNG_HD_OUTLINE inline
#endif

#include <cmath>
#include <cstdint>

namespace tgmpc {

struct Pcg64 {
    uint64_t hi, lo;          // the 128-bit LCG state
    uint64_t inc_hi, inc_lo;  // the stream's increment (odd)
};

struct ZigTables {
    const double* wi;
    const uint64_t* ki;
    const double* fi;
};

constexpr uint64_t PCG_MULT_HI = 0x2360ED051FC65DA4ULL, PCG_MULT_LO = 0x4385DF649FCCF645ULL;
constexpr double ZIG_NOR_R = 3.6541528853610087963519472518;
constexpr double ZIG_NOR_INV_R = 0.27366123732975827203338247596;

RNG_HD uint64_t rng_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// state = state * MULT + inc (mod 2^128); output = rotr64(hi ^ lo, hi >> 58) of the new state (XSL-RR)
RNG_HD uint64_t pcg64_next(Pcg64& s) {
    const uint64_t plo = s.lo * PCG_MULT_LO;
    const uint64_t phi = rng_mulhi64(s.lo, PCG_MULT_LO) + s.hi * PCG_MULT_LO + s.lo * PCG_MULT_HI;
    const uint64_t lo = plo + s.inc_lo;
    const uint64_t hi = phi + s.inc_hi + (lo < plo ? 1u : 0u);
    s.lo = lo;
    s.hi = hi;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

RNG_HD double rng_next_double(Pcg64& s) {
    return (double)(pcg64_next(s) >> 11) * (1.0 / 9007199254740992.0);
}

RNG_HD double rng_uniform(Pcg64& s, double lo, double hi) {
    const double range = hi - lo;
    return lo + range * rng_next_double(s);
}

// searchsorted(cdf, u, side='right'): the number of entries <= u; held below n (cdf[n-1] is 1.0 and u < 1)
RNG_HD int rng_choice(Pcg64& s, const double* cdf, int n) {
    const double u = rng_next_double(s);
    int idx = 0;
    for (int i = 0; i < n; ++i) idx += (cdf[i] <= u) ? 1 : 0;
    return idx < n ? idx : n - 1;
}

// What a caller that needs the host's bits asks of rng_standard_normal.  tie_margin is the caller's; near_tie is only
// ever set (the caller clears it), u1 / u2 / negative describe the last accepted tail draw.
struct ZigAudit {
    double tie_margin;   // relative distance below which a comparison against exp / log1p is not trusted
    bool near_tie;       // some wedge test or tail test of this stream had its two sides that close
    double u1, u2;       // the uniforms that went through log1p: xx = -log1p(-u1) / r, yy = -log1p(-u2)
    bool negative;       // the tail draw's sign: z = -(r + xx)
};

RNG_HD bool rng_near(double a, double b, double margin) {
    return fabs(a - b) <= margin * fmax(fabs(a), fabs(b));
}

// The value of a tail draw from its two uniforms, and whether the tail test accepts it (this libm's log1p).
RNG_HD double rng_tail_value(double u1, double u2, bool negative, bool* accepted) {
    const double xx = -ZIG_NOR_INV_R * log1p(-u1);
    const double yy = -log1p(-u2);
    *accepted = yy + yy > xx * xx;
    return negative ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx;
}

// random_standard_normal (distributions.c).  *tail (optional) is set when the draw came from the tail; *audit
// (optional) as described at ZigAudit.  Neither changes a draw.
RNG_HD_OUTLINE double rng_standard_normal(Pcg64& s, const ZigTables& z, bool* tail = nullptr,
                                          ZigAudit* audit = nullptr) {
    for (;;) {
        uint64_t r = pcg64_next(s);
        const int idx = (int)(r & 0xff);
        r >>= 8;
        const int sign = (int)(r & 0x1);
        const uint64_t rabs = (r >> 1) & 0x000fffffffffffffULL;
        double x = (double)rabs * z.wi[idx];
        if (sign) x = -x;
        if (rabs < z.ki[idx]) return x;
        if (idx == 0) {
            for (;;) {
                const double u1 = rng_next_double(s);
                const double xx = -ZIG_NOR_INV_R * log1p(-u1);
                const double u2 = rng_next_double(s);
                const double yy = -log1p(-u2);
                const double lhs = yy + yy, rhs = xx * xx;
                if (audit && rng_near(lhs, rhs, audit->tie_margin)) audit->near_tie = true;
                if (lhs > rhs) {
                    const bool negative = ((rabs >> 8) & 0x1) != 0;
                    if (tail) *tail = true;
                    if (audit) {
                        audit->u1 = u1;
                        audit->u2 = u2;
                        audit->negative = negative;
                    }
                    return negative ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx;
                }
            }
        } else {
            const double lhs = (z.fi[idx - 1] - z.fi[idx]) * rng_next_double(s) + z.fi[idx];
            const double rhs = exp(-0.5 * x * x);
            if (audit && rng_near(lhs, rhs, audit->tie_margin)) audit->near_tie = true;
            if (lhs < rhs) return x;
        }
    }
}

RNG_HD double rng_normal(Pcg64& s, const ZigTables& z, double scale) {
    return 0.0 + scale * rng_standard_normal(s, z);
}

}  // namespace tgmpc

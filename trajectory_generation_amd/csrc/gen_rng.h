// gen_rng.h -- numpy's Generator(PCG64) stream, restated for host and device: the same functions draw, bit for bit,
// what np.random.default_rng(seed) draws (numpy/random: pcg64.h, distributions.c), from a state the host takes from
// np.random.PCG64(seed).state.  SeedSequence stays on the host.
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
// The tables are passed in (ZigTables): constant arrays on the host, a copy in LDS in the kernels -- lanes index
// them with a random layer.
#pragma once
#include <hip/hip_runtime.h>

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

__host__ __device__ __forceinline__ uint64_t rng_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// state = state * MULT + inc (mod 2^128); output = rotr64(hi ^ lo, hi >> 58) of the new state (XSL-RR)
__host__ __device__ __forceinline__ uint64_t pcg64_next(Pcg64& s) {
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

__host__ __device__ __forceinline__ double rng_next_double(Pcg64& s) {
    return (double)(pcg64_next(s) >> 11) * (1.0 / 9007199254740992.0);
}

__host__ __device__ __forceinline__ double rng_uniform(Pcg64& s, double lo, double hi) {
    const double range = hi - lo;
    return lo + range * rng_next_double(s);
}

// searchsorted(cdf, u, side='right'): the number of entries <= u; held below n (cdf[n-1] is 1.0 and u < 1)
__host__ __device__ __forceinline__ int rng_choice(Pcg64& s, const double* cdf, int n) {
    const double u = rng_next_double(s);
    int idx = 0;
    for (int i = 0; i < n; ++i) idx += (cdf[i] <= u) ? 1 : 0;
    return idx < n ? idx : n - 1;
}

// random_standard_normal (distributions.c).  *tail (optional) is set when the draw came from the tail.
__host__ __device__ inline double rng_standard_normal(Pcg64& s, const ZigTables& z, bool* tail = nullptr) {
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
                const double xx = -ZIG_NOR_INV_R * log1p(-rng_next_double(s));
                const double yy = -log1p(-rng_next_double(s));
                if (yy + yy > xx * xx) {
                    if (tail) *tail = true;
                    return ((rabs >> 8) & 0x1) ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx;
                }
            }
        } else {
            if ((z.fi[idx - 1] - z.fi[idx]) * rng_next_double(s) + z.fi[idx] < exp(-0.5 * x * x)) return x;
        }
    }
}

__host__ __device__ __forceinline__ double rng_normal(Pcg64& s, const ZigTables& z, double scale) {
    return 0.0 + scale * rng_standard_normal(s, z);
}

}  // namespace tgmpc

// seed_seq.h -- numpy's SeedSequence and PCG64's seeding from it, restated for host and device: from the entropy words
// to the generator state of np.random.PCG64(entropy), i.e. of np.random.default_rng(entropy), bit for bit
// (numpy/random/bit_generator.pyx: SeedSequence.mix_entropy / generate_state; _pcg64.pyx and pcg64.h:
// pcg64_set_seed, pcg_setseq_128_srandom_r).
//
//   SeedSequence(entropy)                  seed_seq_mix       the pool of 4 uint32: hashmix of the first 4 words (0 where
//                                                             there are fewer) with the evolving hash constant, every
//                                                             pair mixed, then one more pass for words 5, 6, ...
//   .generate_state(4, uint64)             seed_seq_state64   8 uint32 from the pool taken in a cycle, paired little-endian
//   PCG64 seeding                          pcg64_seed_words   state = 0, inc = (initseq << 1) | 1, step,
//                                                             state += initstate, step
//
// The input is the entropy as numpy coerces it: uint32 words, little-endian, at least one word per int, the words of a
// sequence of ints concatenated.  That coercion is the caller's (Python's).  Zero words after the last one change
// nothing while the count stays within the pool (hashmix(0) is what a missing word contributes), so an int below 2^64
// may always be given as two words; past 4 words every word counts.
//
// 32- and 64-bit integer arithmetic only, no table, no libm: equality with numpy is exact or the code is wrong.
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#ifndef TGMPC_SEED_SEQ_H
#define TGMPC_SEED_SEQ_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SEED_HD __host__ __device__ __forceinline__
#else
#define SEED_HD inline
#endif

#define SEED_SEQ_POOL 4
#define SEED_SEQ_MAX_WORDS 8      /* the entry points' limit, not numpy's */

namespace tgseed {

constexpr uint32_t SS_INIT_A = 0x43b0d7e5u, SS_MULT_A = 0x931e8875u;
constexpr uint32_t SS_INIT_B = 0x8b51f9ddu, SS_MULT_B = 0x58f38dedu;
constexpr uint32_t SS_MIX_L = 0xca01f9ddu, SS_MIX_R = 0x4973f715u;
constexpr int SS_XSHIFT = 16;
constexpr uint64_t SS_PCG_MULT_HI = 0x2360ED051FC65DA4ULL, SS_PCG_MULT_LO = 0x4385DF649FCCF645ULL;

SEED_HD uint32_t ss_hashmix(uint32_t value, uint32_t& hash_const) {
    value ^= hash_const;
    hash_const *= SS_MULT_A;
    value *= hash_const;
    value ^= value >> SS_XSHIFT;
    return value;
}

SEED_HD uint32_t ss_mix(uint32_t x, uint32_t y) {
    uint32_t r = SS_MIX_L * x - SS_MIX_R * y;
    r ^= r >> SS_XSHIFT;
    return r;
}

// SeedSequence.mix_entropy: entropy[0 .. n), n >= 1 -> pool[4]
SEED_HD void seed_seq_mix(const uint32_t* entropy, int n, uint32_t pool[SEED_SEQ_POOL]) {
    uint32_t hc = SS_INIT_A;
    for (int i = 0; i < SEED_SEQ_POOL; ++i) pool[i] = ss_hashmix(i < n ? entropy[i] : 0u, hc);
    for (int s = 0; s < SEED_SEQ_POOL; ++s)
        for (int d = 0; d < SEED_SEQ_POOL; ++d)
            if (s != d) pool[d] = ss_mix(pool[d], ss_hashmix(pool[s], hc));
    for (int s = SEED_SEQ_POOL; s < n; ++s)
        for (int d = 0; d < SEED_SEQ_POOL; ++d) pool[d] = ss_mix(pool[d], ss_hashmix(entropy[s], hc));
}

// SeedSequence.generate_state(4, uint64): word k = (uint32[2k + 1] << 32) | uint32[2k]
SEED_HD void seed_seq_state64(const uint32_t pool[SEED_SEQ_POOL], uint64_t out[4]) {
    uint32_t hc = SS_INIT_B;
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & (SEED_SEQ_POOL - 1)];
        v ^= hc;
        hc *= SS_MULT_B;
        v *= hc;
        v ^= v >> SS_XSHIFT;
        w[i] = v;
    }
    for (int k = 0; k < 4; ++k) out[k] = ((uint64_t)w[2 * k + 1] << 32) | (uint64_t)w[2 * k];
}

SEED_HD uint64_t ss_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// state = state * MULT + inc (mod 2^128)
SEED_HD void ss_pcg_step(uint64_t& hi, uint64_t& lo, uint64_t inc_hi, uint64_t inc_lo) {
    const uint64_t plo = lo * SS_PCG_MULT_LO;
    const uint64_t phi = ss_mulhi64(lo, SS_PCG_MULT_LO) + hi * SS_PCG_MULT_LO + lo * SS_PCG_MULT_HI;
    const uint64_t nlo = plo + inc_lo;
    hi = phi + inc_hi + (nlo < plo ? 1u : 0u);
    lo = nlo;
}

// PCG64's seeding from generate_state's four words v: initstate = v[0] : v[1], initseq = v[2] : v[3] (high : low).
// st = (state >> 64, state & M, inc >> 64, inc & M), the layout of traj_gen_piecewise_batch's rng_state.
SEED_HD void pcg64_seed_words(const uint64_t v[4], unsigned long long st[4]) {
    const uint64_t inc_hi = (v[2] << 1) | (v[3] >> 63), inc_lo = (v[3] << 1) | 1u;
    uint64_t hi = 0, lo = 0;
    ss_pcg_step(hi, lo, inc_hi, inc_lo);
    const uint64_t slo = lo + v[1];
    hi = hi + v[0] + (slo < lo ? 1u : 0u);
    lo = slo;
    ss_pcg_step(hi, lo, inc_hi, inc_lo);
    st[0] = hi; st[1] = lo; st[2] = inc_hi; st[3] = inc_lo;
}

// np.random.PCG64(entropy).state from the entropy's n words, 1 <= n
SEED_HD void pcg64_seed(const uint32_t* entropy, int n, unsigned long long st[4]) {
    uint32_t pool[SEED_SEQ_POOL];
    uint64_t v[4];
    seed_seq_mix(entropy, n, pool);
    seed_seq_state64(pool, v);
    pcg64_seed_words(v, st);
}

}  // namespace tgseed

#endif

// noise_draw.h -- the measurement noise of one trajectory (dataset/schema.py measurement_noise, the reference's
// generation_type1.py:312-320), for host and device:
//
//   rng = np.random.default_rng(seed)                                   seed_seq.h
//   np.column_stack([rng.normal(0, sigma[ch], n_rows) for ch in 0..5])  gen_rng.h, channel by channel
//
// into out[r * 6 + ch] = 0.0 + sigma[ch] * z, the [n_rows, 6] block the CSV writers read.  The draw is audited
// (gen_rng.h ZigAudit): every accepted tail draw is handed to `tails` as (index r * 6 + ch, u1, u2, negative), and
// the return value tells whether some comparison against exp / log1p came within tie_margin of a tie -- the
// trajectory is then not to be trusted on a libm that is not numpy's.
//
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#ifndef TGMPC_NOISE_DRAW_H
#define TGMPC_NOISE_DRAW_H

#include "gen_rng.h"
#include "seed_seq.h"

namespace tgmpc {

constexpr int NOISE_CH = 6;

struct NoTails {
    RNG_HD void operator()(long long, double, double, bool) const {}
};

// seed: the non-negative int given to default_rng, as its two little-endian uint32 words (a zero high word is what
// numpy's one-word coercion amounts to, seed_seq.h).
template <typename Tails>
RNG_HD bool noise_draw_trajectory(unsigned long long seed, int n_rows, const double* sigma, const ZigTables& z,
                                  double tie_margin, double* out, Tails tails) {
    const uint32_t words[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
    unsigned long long st[4];
    tgseed::pcg64_seed(words, 2, st);
    Pcg64 s{st[0], st[1], st[2], st[3]};
    ZigAudit audit;
    audit.tie_margin = tie_margin;
    audit.near_tie = false;
    audit.u1 = audit.u2 = 0.0;
    audit.negative = false;
    for (int ch = 0; ch < NOISE_CH; ++ch) {
        const double sg = sigma[ch];
        for (int r = 0; r < n_rows; ++r) {
            bool tail = false;
            const double v = rng_standard_normal(s, z, &tail, &audit);
            const long long i = (long long)r * NOISE_CH + ch;
            out[i] = 0.0 + sg * v;
            if (tail) tails(i, audit.u1, audit.u2, audit.negative);
        }
    }
    return audit.near_tie;
}

}  // namespace tgmpc

#endif

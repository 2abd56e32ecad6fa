// san_noise.cpp -- csrc/seed_seq.h, csrc/gen_rng.h and the draw loop of csrc/noise_draw.h on the host under
// AddressSanitizer / UBSan.  Every buffer is an exactly sized heap block, so one element read or written too many is a
// report.  Seeding: 1 to 8 entropy words, each from a block of exactly that many words, against the states numpy gives
// for [1], [1, 2], ... (np.random.PCG64(list).state, recorded below).  Draw loop: 0 rows, 1 row, 129 rows;
// seeds on both sides of the one-word / two-word boundary; the tail records collected by the audit are recomputed with
// rng_tail_value and must give the stored value back; a margin of 0 declines nothing, a margin of 1 everything that
// met a wedge.  Prints "san_noise ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../trajectory_generation_amd/csrc/noise_draw.h"

#define GEN_ZIG_DECL static const
#define GEN_ZIG_NAME(x) zig_##x
#include "../../trajectory_generation_amd/csrc/gen_zig_tables.h"

using namespace tgmpc;

// np.random.PCG64(list(range(1, n + 1))).state for n = 1 .. 8: state >> 64, state & M, inc >> 64, inc & M
static const unsigned long long NUMPY_STATE[8][4] = {
    {0x9c5b484bfedb756cull, 0x2a6e7d6f320fbc7eull, 0x922af2da2645f895ull, 0xa19857b95740937bull},
    {0xcfde2256a71fcea6ull, 0xb4f9ad1e87555637ull, 0xae870aae63496ea4ull, 0x98b6579724095b27ull},
    {0xb5f7801c017411beull, 0xf4f61d010361d979ull, 0x21efe6ce1468888bull, 0x311a8c35e9261f19ull},
    {0x7e6e13c17fad88bdull, 0x1af5a42dbcfd8816ull, 0xe93b9112d91c0430ull, 0x031b67c38c8ea157ull},
    {0x76fe718e9683762bull, 0x30155c68a59b80bfull, 0x5406d36f034cecceull, 0x86e8e4390e5af5e3ull},
    {0x27705aa33bb35021ull, 0x7f413aa6045c0bc1ull, 0x3643bb03c9f9eb6cull, 0x36bba14611c4ce17ull},
    {0xfa5ca3d78233b774ull, 0x652b80f8484db5a8ull, 0x8bf2af09960ff29eull, 0x99abc2042335abc1ull},
    {0x0c114341c13e057eull, 0x649f8fdb559520ccull, 0x330f834ef712a4fdull, 0x8e1d1f847aa0ddb9ull},
};

struct Rec {
    long long i;
    double u1, u2;
    bool negative;
};

struct Collect {
    std::vector<Rec>* v;
    void operator()(long long i, double u1, double u2, bool negative) const { v->push_back(Rec{i, u1, u2, negative}); }
};

static void die(const char* what, long long a, long long b) {
    std::printf("MISMATCH (%s) %lld %lld\n", what, a, b);
    std::exit(1);
}

int main() {
    // seeding, 1 .. 8 words
    for (int n = 1; n <= SEED_SEQ_MAX_WORDS; ++n) {
        std::unique_ptr<uint32_t[]> e(new uint32_t[n]);
        for (int i = 0; i < n; ++i) e[i] = (uint32_t)(i + 1);
        std::unique_ptr<unsigned long long[]> st(new unsigned long long[4]);
        tgseed::pcg64_seed(e.get(), n, st.get());
        for (int j = 0; j < 4; ++j)
            if (st[j] != NUMPY_STATE[n - 1][j]) die("seed", n, j);
    }
    // extreme words: every multiply and shift of the mixers on all-ones input
    {
        std::unique_ptr<uint32_t[]> e(new uint32_t[8]);
        for (int i = 0; i < 8; ++i) e[i] = 0xffffffffu;
        unsigned long long st[4];
        tgseed::pcg64_seed(e.get(), 8, st);
        if (!(st[3] & 1ull)) die("inc is odd", 0, 0);
    }
    const ZigTables z{zig_wi, (const uint64_t*)zig_ki, zig_fi};
    const double sigma[NOISE_CH] = {0.05, 0.05, 0.003, 0.010, 0.003, 0.030};
    long long tails = 0, declined0 = 0, declined1 = 0, draws = 0;
    const unsigned long long seeds[] = {0ull, 12345ull, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull};
    {   // no rows: the stream is seeded and a zero-length block is not touched
        std::unique_ptr<double[]> none(new double[0]);
        if (noise_draw_trajectory(12345ull, 0, sigma, z, 1.0, none.get(), NoTails{})) die("empty draw declined", 0, 0);
    }
    const int rows[] = {1, 129};
    for (int n_rows : rows) {
        for (unsigned long long base : seeds) {
            for (unsigned long long k = 0; k < 24; ++k) {
                const unsigned long long seed = base > 0x7fffffffffffff00ull ? base - k : base + k;
                std::unique_ptr<double[]> out(new double[(size_t)n_rows * NOISE_CH]);
                for (int i = 0; i < n_rows * NOISE_CH; ++i) out[i] = NAN;
                std::vector<Rec> recs;
                const bool d0 = noise_draw_trajectory(seed, n_rows, sigma, z, 0.0, out.get(), Collect{&recs});
                for (int i = 0; i < n_rows * NOISE_CH; ++i)
                    if (!std::isfinite(out[i])) die("not written", (long long)seed, i);
                for (const Rec& r : recs) {
                    if (r.i < 0 || r.i >= (long long)n_rows * NOISE_CH) die("tail index", (long long)seed, r.i);
                    bool ok = false;
                    const double v = 0.0 + sigma[r.i % NOISE_CH] * rng_tail_value(r.u1, r.u2, r.negative, &ok);
                    if (!ok || std::memcmp(&v, &out[r.i], 8) != 0) die("tail value", (long long)seed, r.i);
                    if (!(std::fabs(out[r.i]) > sigma[r.i % NOISE_CH] * 3.65)) die("tail size", (long long)seed, r.i);
                }
                tails += (long long)recs.size();
                draws += (long long)n_rows * NOISE_CH;
                // the margin changes no value
                std::unique_ptr<double[]> out1(new double[(size_t)n_rows * NOISE_CH]);
                const bool d1 = noise_draw_trajectory(seed, n_rows, sigma, z, 1.0, out1.get(), NoTails{});
                if (std::memcmp(out.get(), out1.get(), sizeof(double) * n_rows * NOISE_CH) != 0)
                    die("margin moved a value", (long long)seed, n_rows);
                declined0 += d0;
                declined1 += d1;
            }
        }
    }
    if (declined0 != 0) die("margin 0 declined", declined0, 0);
    if (declined1 < 100) die("margin 1 declined too few", declined1, 0);
    if (tails < 10) die("tail draws", tails, draws);
    // the plain call (no audit) draws the same values
    {
        unsigned long long st[4];
        const uint32_t w[2] = {12345u, 0u};
        tgseed::pcg64_seed(w, 2, st);
        Pcg64 s{st[0], st[1], st[2], st[3]};
        std::unique_ptr<double[]> out(new double[129 * NOISE_CH]);
        noise_draw_trajectory(12345ull, 129, sigma, z, 0.0, out.get(), NoTails{});
        for (int ch = 0; ch < NOISE_CH; ++ch)
            for (int r = 0; r < 129; ++r) {
                const double v = rng_normal(s, z, sigma[ch]);
                if (std::memcmp(&v, &out[r * NOISE_CH + ch], 8) != 0) die("audit moved a draw", ch, r);
            }
    }
    std::printf("san_noise ok: %lld draws, %lld tails, %lld declined at margin 1\n", draws, tails, declined1);
    return 0;
}

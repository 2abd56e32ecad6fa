// dataset_noise.hip -- the noisy CSV's measurement noise drawn on the GPU with numpy's bits, and the seeding it rests
// on (seed_seq.h: SeedSequence -> PCG64 state) as entry points of its own.
//
// measurement_noise(id, n_rows) seeds np.random.default_rng(seed_base + id) and draws six normal(0, sigma, n_rows)
// vectors.  A stream is sequential, so one lane draws one trajectory (noise_draw.h), 64 trajectories per workgroup,
// the ziggurat tables in LDS.  A lane stores 8 bytes at a time into its own [n_rows, 6] block, 48 bytes apart within a
// channel: direct stores, as in the generators' kernels (the L2 gathers a block's lines, which the lane revisits once
// per channel).
//
// What the device library's exp / log1p could do differently from the host libm's (numpy's) never reaches the result:
//   - an accepted tail draw (|z| > r, one draw in about 3,900) also goes to the tail list -- index, the two uniforms
//     that fed log1p, the sign -- and traj_dataset_noise_tails_host recomputes its value with the host libm;
//   - a wedge or tail test whose two sides lie within tie_margin of each other marks the trajectory as declined: the
//     caller draws that one on the host.
// So the block the caller ends up with is the host's, bit for bit, whatever the device library rounds.
//
// Built with the library's FLAGS: -ffp-contract=off, no product may fuse into an fma.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/trajgen.h"
#include "gen_zig_lds.h"
#include "noise_draw.h"
#include "seed_seq.h"

namespace tgmpc {

constexpr int NOISE_WAVE = 64;
constexpr int SEED_BLOCK = 256;

// seed_base + id without signed overflow; a negative result is refused by every caller
__host__ __device__ __forceinline__ long long noise_seed(long long seed_base, long long id) {
    return (long long)((unsigned long long)seed_base + (unsigned long long)id);
}

struct NoiseSigma {
    double s[NOISE_CH];
};

// appends to the tail list through the device counter, which goes on counting past the capacity
struct DeviceTails {
    unsigned long long* count;
    unsigned long long* rec;
    long long capacity, base;

    __device__ __forceinline__ void operator()(long long i, double u1, double u2, bool negative) const {
        const unsigned long long k = atomicAdd(count, 1ull);
        if (k < (unsigned long long)capacity) {
            unsigned long long* e = rec + 4 * k;
            e[0] = (unsigned long long)(base + i);
            e[1] = (unsigned long long)__double_as_longlong(u1);
            e[2] = (unsigned long long)__double_as_longlong(u2);
            e[3] = negative ? 1ull : 0ull;
        }
    }
};

__global__ __launch_bounds__(NOISE_WAVE) void noise_kernel(int B, int n_rows, long long seed_base,
                                                           const long long* noise_ids, NoiseSigma sigma,
                                                           double tie_margin, double* noise, int* declined,
                                                           unsigned long long* tail_count, unsigned long long* tail_rec,
                                                           long long tail_capacity) {
    __shared__ ZigLds lds;
    __shared__ double sg[NOISE_CH];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NOISE_CH; ++j) sg[j] = sigma.s[j];
    }
    zig_load(lds);
    const long long b = (long long)blockIdx.x * NOISE_WAVE + threadIdx.x;
    if (b >= B) return;
    const long long seed = noise_seed(seed_base, noise_ids[b]);
    if (seed < 0) {            // numpy refuses it; so does the caller, before the launch
        declined[b] = 1;
        return;
    }
    const ZigTables z{lds.wi, lds.ki, lds.fi};
    const long long base = b * (long long)n_rows * NOISE_CH;
    const DeviceTails tails{tail_count, tail_rec, tail_capacity, base};
    const bool near_tie = noise_draw_trajectory((unsigned long long)seed, n_rows, sg, z, tie_margin, noise + base, tails);
    declined[b] = near_tie ? 1 : 0;
}

__global__ __launch_bounds__(SEED_BLOCK) void seed_kernel(const uint32_t* entropy, int B, int nwords,
                                                          unsigned long long* states) {
    const long long b = (long long)blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (b >= B) return;
    unsigned long long st[4];
    tgseed::pcg64_seed(entropy + b * nwords, nwords, st);
#pragma unroll
    for (int j = 0; j < 4; ++j) states[4 * b + j] = st[j];
}

static bool seed_args_ok(const void* entropy, int B, int nwords, const void* states) {
    return B >= 0 && nwords >= 1 && nwords <= SEED_SEQ_MAX_WORDS && (B == 0 || (entropy && states));
}

}  // namespace tgmpc

extern "C" {

int traj_gen_seed_pcg64_host(const uint32_t* entropy, int B, int nwords, unsigned long long* states) {
    if (!tgmpc::seed_args_ok(entropy, B, nwords, states)) return TRAJ_E_ARG;
    for (long long b = 0; b < B; ++b) tgseed::pcg64_seed(entropy + b * nwords, nwords, states + 4 * b);
    return TRAJ_OK;
}

int traj_gen_seed_pcg64_batch(const uint32_t* entropy, int B, int nwords, unsigned long long* states, void* stream) {
    using namespace tgmpc;
    if (!seed_args_ok(entropy, B, nwords, states)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    const dim3 grid((unsigned)((B + SEED_BLOCK - 1) / SEED_BLOCK)), block(SEED_BLOCK);
    hipLaunchKernelGGL(seed_kernel, grid, block, 0, (hipStream_t)stream, entropy, B, nwords, states);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_noise_host(int B, int n_rows, long long seed_base, const long long* noise_ids, const double* sigma,
                            double tie_margin, double* noise, int* declined) {
    using namespace tgmpc;
    if (B < 0 || n_rows < 1 || !sigma || !(tie_margin >= 0.0)) return TRAJ_E_ARG;
    if (B > 0 && (!noise_ids || !noise)) return TRAJ_E_ARG;
    for (int b = 0; b < B; ++b)
        if (noise_seed(seed_base, noise_ids[b]) < 0) return TRAJ_E_ARG;
    const ZigTables z = zig_host_tables();
    for (long long b = 0; b < B; ++b) {
        const bool near_tie = noise_draw_trajectory((unsigned long long)noise_seed(seed_base, noise_ids[b]), n_rows, sigma, z,
                                                    tie_margin, noise + b * (long long)n_rows * NOISE_CH, NoTails{});
        if (declined) declined[b] = near_tie ? 1 : 0;
    }
    return TRAJ_OK;
}

int traj_dataset_noise_batch(int B, int n_rows, long long seed_base, const long long* noise_ids, const double* sigma,
                             double tie_margin, double* noise, int* declined, unsigned long long* tail_count,
                             unsigned long long* tail_rec, long long tail_capacity, void* stream) {
    using namespace tgmpc;
    if (B < 0 || n_rows < 1 || !sigma || !(tie_margin >= 0.0) || tail_capacity < 0) return TRAJ_E_ARG;
    if (B > 0 && (!noise_ids || !noise || !declined || !tail_count || (tail_capacity > 0 && !tail_rec)))
        return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    NoiseSigma sg;
    std::memcpy(sg.s, sigma, sizeof(sg.s));
    const dim3 grid((unsigned)((B + NOISE_WAVE - 1) / NOISE_WAVE)), block(NOISE_WAVE);
    hipLaunchKernelGGL(noise_kernel, grid, block, 0, (hipStream_t)stream, B, n_rows, seed_base, noise_ids, sg, tie_margin,
                       noise, declined, tail_count, tail_rec, tail_capacity);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_noise_tails_host(long long n, const unsigned long long* tail_rec, const double* sigma, double* value,
                                  int* accepted) {
    using namespace tgmpc;
    if (n < 0 || !sigma || (n > 0 && (!tail_rec || !value || !accepted))) return TRAJ_E_ARG;
    for (long long k = 0; k < n; ++k) {
        const unsigned long long* e = tail_rec + 4 * k;
        double u1, u2;
        std::memcpy(&u1, e + 1, 8);
        std::memcpy(&u2, e + 2, 8);
        bool ok;
        const double zv = rng_tail_value(u1, u2, e[3] != 0, &ok);
        value[k] = 0.0 + sigma[e[0] % NOISE_CH] * zv;
        accepted[k] = ok ? 1 : 0;
    }
    return TRAJ_OK;
}

}  // extern "C"

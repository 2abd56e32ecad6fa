// workload.hip -- the closed loop's synthetic workload (workload.make_workload) and its spline paths (batch.PathSet)
// built on the GPU, one lane per trajectory: no per-trajectory Python in front of the closed-loop kernel.
//
//   traj_gen_spline_coef_batch / _host   PathSet.build's loop: spline.h on every kind-2 row of given knots
//   traj_gen_workload_batch / _host      make_workload's loop body for tid = id_offset + b:
//       np.random.default_rng([seed, tid])   seed_seq.h on the seed's words followed by tid's (numpy's coercion)
//       rng.uniform(...)                     gen_rng.h rng_uniform, in make_workload's order
//       spline_natural                       spline.h
//       y(X), y'(X)                          path_eval (mpc_common.h) on the row just written -- the rule the closed
//                                            loop applies to it later; the host entry restates it with the host libm
//       atan, d_steady_state                 the library's atan; batch.d_steady_state's expression with v * v
//
// workload_row below is one text for the kernel and for traj_gen_workload_host.  What the two can round differently
// is what goes through libm: atan(y') in phi, and sincos in the sinusoid rows' Y and phi.  Everything else -- the
// draws, kinds, pcs, knots, coefficients, X, vx, vy, omega, u0 -- is integer arithmetic or float64 +, -, *, / in one
// written order: the same bits.
//
// Built with the library's FLAGS: -ffp-contract=off, no product may fuse into an fma.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/trajgen.h"
#include "gen_rng.h"
#include "mpc_common.h"
#include "seed_seq.h"
#include "spline.h"

namespace tgmpc {

constexpr int WL_BLOCK = 64;
constexpr int WL_MAX_SEED_WORDS = TRAJ_WORKLOAD_MAX_SEED_WORDS;

struct WlSeed {
    uint32_t w[WL_MAX_SEED_WORDS];
    int n;
};

struct WlOut {
    int kmax;
    int* kind;       // [B]
    double* pc;      // [B,4]
    int* nk;         // [B]
    double* xk;      // [B,kmax]
    double* yk;      // [B,kmax]
    double* coef;    // [B,kmax-1,4]
    double* x0;      // [B,6]
    double* u0;      // [B,2]
};

// y(x), y'(x) of row b: the kernels' own path_eval on the device, the same expressions with the host libm's sin and
// cos on the host (what make_workload's lambdas and spline_eval compute there)
__host__ __device__ inline void wl_path_eval(const PathArgs& pa, long long b, double x, double& y, double& dy) {
#if defined(__HIP_DEVICE_COMPILE__)
    path_eval(pa, (int)b, x, y, dy);
#else
    const int kind = pa.kind[b];
    const double* c = pa.pc + 4 * b;
    if (kind == 0) {
        y = c[0] + x * (c[1] + x * (c[2] + x * c[3]));
        dy = c[1] + x * (2.0 * c[2] + x * 3.0 * c[3]);
    } else if (kind == 1) {
        const double a = c[1] * x + c[2];
        y = c[0] * std::sin(a) + c[3];
        dy = c[0] * c[1] * std::cos(a);
    } else {
        const int nk = pa.nk[b];
        const double* xk = pa.xk + (size_t)pa.kmax * b;
        const double* cf = pa.coef + (size_t)(pa.kmax - 1) * 4 * b;
        if (x <= xk[0]) {
            y = cf[0] + cf[1] * (x - xk[0]);
            dy = cf[1];
        } else if (x >= xk[nk - 1]) {
            const double* q = cf + 4 * (nk - 2);
            const double h = xk[nk - 1] - xk[nk - 2];
            const double ye = q[0] + h * (q[1] + h * (q[2] + h * q[3]));
            const double se = q[1] + h * (2.0 * q[2] + h * 3.0 * q[3]);
            y = ye + se * (x - xk[nk - 1]);
            dy = se;
        } else {
            int j = 0;
            while (j < nk - 2 && x >= xk[j + 1]) ++j;
            const double* q = cf + 4 * j;
            const double tt = x - xk[j];
            y = q[0] + tt * (q[1] + tt * (q[2] + tt * q[3]));
            dy = q[1] + tt * (2.0 * q[2] + tt * 3.0 * q[3]);
        }
    }
#endif
}

__host__ __device__ inline double wl_atan(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return pm_atan(v);
#else
    return std::atan(v);
#endif
}

// make_workload's loop body for trajectory b of the call, tid = id_offset + b
__host__ __device__ inline void workload_row(const traj_vehicle_params& p, int workload, const WlSeed& seed,
                                             long long id_offset, long long b, const WlOut& o) {
    const int kmax = o.kmax;
    const unsigned long long tid = (unsigned long long)(id_offset + b);
    int* kind = o.kind + b;
    double* pc = o.pc + 4 * b;
    double* xk = o.xk + (size_t)kmax * b;
    double* yk = o.yk + (size_t)kmax * b;
    double* coef = o.coef + (size_t)(kmax - 1) * 4 * b;
    double* x0 = o.x0 + 6 * b;
    double* u0 = o.u0 + 2 * b;

    // numpy's coercion of [seed, tid]: the seed's words, then tid's (one below 2^32, else two)
    uint32_t ent[SEED_SEQ_MAX_WORDS];
    int n = 0;
    for (int i = 0; i < WL_MAX_SEED_WORDS; ++i)
        if (i < seed.n) ent[n++] = seed.w[i];
    ent[n++] = (uint32_t)(tid & 0xffffffffull);
    if (tid >> 32) ent[n++] = (uint32_t)(tid >> 32);
    unsigned long long st[4];
    tgseed::pcg64_seed(ent, n, st);
    Pcg64 s{st[0], st[1], st[2], st[3]};

    for (int i = 0; i < 4; ++i) pc[i] = 0.0;
    for (int i = 0; i < kmax; ++i) xk[i] = yk[i] = 0.0;
    int nk = 0;
    if (workload == TRAJ_WORKLOAD_SPLINE) {
        *kind = 2;
        nk = TRAJ_WORKLOAD_SPLINE_KNOTS;
        for (int i = 0; i < nk; ++i) {
            xk[i] = TRAJ_WORKLOAD_SPLINE_X0 + TRAJ_WORKLOAD_SPLINE_DX * (double)i;
            yk[i] = rng_uniform(s, -1.0, 1.0);
        }
    } else if (workload == TRAJ_WORKLOAD_MIXED && (tid & 1ull) == 0) {
        *kind = 1;
        pc[0] = 0.5 * rng_uniform(s, 0.8, 1.2);
        pc[1] = 0.5 * rng_uniform(s, 0.8, 1.2);
        pc[2] = rng_uniform(s, 0.0, 2.0 * 3.141592653589793);
    } else if (workload == TRAJ_WORKLOAD_MIXED) {
        *kind = 0;
        pc[2] = rng_uniform(s, 0.05, 0.15);
    } else {
        *kind = 0;
        pc[2] = 0.1;
    }
    o.nk[b] = nk;
    tgspline::spline_coef_row(*kind, nk, kmax, xk, yk, coef);

    if (workload == TRAJ_WORKLOAD_PARABOLA) {       // MPC/main.py:77
        x0[0] = 0.0; x0[1] = 0.5; x0[2] = 0.0; x0[3] = 1.0; x0[4] = 0.0; x0[5] = 0.0;
    } else {
        const PathArgs pa{kmax, o.kind, o.pc, o.nk, o.xk, o.coef};
        const double X = rng_uniform(s, -2.0, 2.0);
        double y, dy;
        wl_path_eval(pa, b, X, y, dy);
        x0[0] = X;
        x0[1] = y + rng_uniform(s, -0.5, 0.5);
        x0[2] = wl_atan(dy) + rng_uniform(s, -0.2, 0.2);
        x0[3] = rng_uniform(s, 0.4, 1.5);
        x0[4] = rng_uniform(s, -0.05, 0.05);
        x0[5] = rng_uniform(s, -1.0, 1.0);
    }
    const double v = x0[3];
    u0[0] = (p.Cr0 + p.Cr2 * (v * v)) / (p.Cm1 - p.Cm2 * v);
    u0[1] = 0.0;
}

__global__ __launch_bounds__(WL_BLOCK) void workload_kernel(traj_vehicle_params p, int workload, WlSeed seed,
                                                            long long id_offset, int B, WlOut o) {
    const long long b = (long long)blockIdx.x * WL_BLOCK + threadIdx.x;
    if (b >= B) return;
    workload_row(p, workload, seed, id_offset, b, o);
}

__global__ __launch_bounds__(WL_BLOCK) void spline_coef_kernel(int B, int kmax, const int* kind, const int* nk,
                                                               const double* xk, const double* yk, double* coef,
                                                               int* flag) {
    const long long b = (long long)blockIdx.x * WL_BLOCK + threadIdx.x;
    if (b >= B) return;
    flag[b] = tgspline::spline_coef_row(kind[b], nk[b], kmax, xk + (size_t)kmax * b, yk + (size_t)kmax * b,
                                        coef + (size_t)(kmax - 1) * 4 * b);
}

static bool coef_args_ok(int B, int kmax, const void* kind, const void* nk, const void* xk, const void* yk,
                         const void* coef, const void* flag) {
    return B >= 1 && kmax >= 2 && kind && nk && xk && yk && coef && flag;
}

static bool workload_args_ok(const traj_vehicle_params* p, int workload, const uint32_t* seed_words, int ns,
                             long long id_offset, int B, const WlOut& o, WlSeed* seed) {
    if (!p || !seed_words || ns < 1 || ns > WL_MAX_SEED_WORDS || B < 1 || id_offset < 0) return false;
    if (id_offset > 0x7fffffffffffffffLL - B) return false;
    if (workload != TRAJ_WORKLOAD_SPLINE && workload != TRAJ_WORKLOAD_MIXED && workload != TRAJ_WORKLOAD_PARABOLA)
        return false;
    if (o.kmax < (workload == TRAJ_WORKLOAD_SPLINE ? TRAJ_WORKLOAD_SPLINE_KNOTS : 2)) return false;
    if (!o.kind || !o.pc || !o.nk || !o.xk || !o.yk || !o.coef || !o.x0 || !o.u0) return false;
    seed->n = ns;
    for (int i = 0; i < WL_MAX_SEED_WORDS; ++i) seed->w[i] = i < ns ? seed_words[i] : 0u;
    return true;
}

}  // namespace tgmpc

extern "C" {

int traj_gen_spline_coef_host(int B, int kmax, const int* kind, const int* nk, const double* xk, const double* yk,
                              double* coef, int* flag) {
    using namespace tgmpc;
    if (!coef_args_ok(B, kmax, kind, nk, xk, yk, coef, flag)) return TRAJ_E_ARG;
    for (long long b = 0; b < B; ++b)
        flag[b] = tgspline::spline_coef_row(kind[b], nk[b], kmax, xk + (size_t)kmax * b, yk + (size_t)kmax * b,
                                            coef + (size_t)(kmax - 1) * 4 * b);
    return TRAJ_OK;
}

int traj_gen_spline_coef_batch(int B, int kmax, const int* kind, const int* nk, const double* xk, const double* yk,
                               double* coef, int* flag, void* stream) {
    using namespace tgmpc;
    if (!coef_args_ok(B, kmax, kind, nk, xk, yk, coef, flag)) return TRAJ_E_ARG;
    const dim3 grid((unsigned)((B + WL_BLOCK - 1) / WL_BLOCK)), block(WL_BLOCK);
    hipLaunchKernelGGL(spline_coef_kernel, grid, block, 0, (hipStream_t)stream, B, kmax, kind, nk, xk, yk, coef, flag);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_gen_workload_host(const traj_vehicle_params* p, int workload, const uint32_t* seed_words, int ns,
                           long long id_offset, int B, int kmax, int* kind, double* pc, int* nk, double* xk,
                           double* yk, double* coef, double* x0, double* u0) {
    using namespace tgmpc;
    const WlOut o{kmax, kind, pc, nk, xk, yk, coef, x0, u0};
    WlSeed seed;
    if (!workload_args_ok(p, workload, seed_words, ns, id_offset, B, o, &seed)) return TRAJ_E_ARG;
    for (long long b = 0; b < B; ++b) workload_row(*p, workload, seed, id_offset, b, o);
    return TRAJ_OK;
}

int traj_gen_workload_batch(const traj_vehicle_params* p, int workload, const uint32_t* seed_words, int ns,
                            long long id_offset, int B, int kmax, int* kind, double* pc, int* nk, double* xk,
                            double* yk, double* coef, double* x0, double* u0, void* stream) {
    using namespace tgmpc;
    const WlOut o{kmax, kind, pc, nk, xk, yk, coef, x0, u0};
    WlSeed seed;
    if (!workload_args_ok(p, workload, seed_words, ns, id_offset, B, o, &seed)) return TRAJ_E_ARG;
    const dim3 grid((unsigned)((B + WL_BLOCK - 1) / WL_BLOCK)), block(WL_BLOCK);
    hipLaunchKernelGGL(workload_kernel, grid, block, 0, (hipStream_t)stream, *p, workload, seed, id_offset, B, o);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

}  // extern "C"

// openloop.hip -- the open-loop dataset generators (include/trajgen.h): slew limiter, output clip and
// explicit-Euler simulation of B trajectories in one launch, one lane per trajectory.
//
// The steps of a trajectory are a serial chain, so a lane keeps its state in registers and walks its own
// trajectory.  Per step a lane reads 16 B of u_raw and writes 16 B of U and 48 B of X, at strides of 16 T and
// 48 (T + 1) bytes between lanes.  The staged form moves K = TRAJ_GEN_STAGE_STEPS steps of all 64 trajectories
// through LDS: per trajectory the K steps are one contiguous run in memory (2 K doubles of u_raw / U, 6 K of
// X), which the whole wave loads and stores with consecutive lanes on consecutive addresses.  The direct form
// lets every lane load and store its own rows.  Both run the same step function and are bit-identical.
//
// Built with the library's FLAGS: -ffp-contract=off keeps every expression in the reference's order.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>

#include "../../include/trajgen.h"
#include "gen_model.h"
#include "physics.h"

namespace tgmpc {

template <int MODEL>
__device__ __forceinline__ void gen_model_f(const VP& p, const double* x, const double* u, double* xd) {
    if (MODEL == TRAJ_GEN_MODEL_MPC) f_cont(p, x, u, xd);
    else gen_f_cont<MODEL == TRAJ_GEN_MODEL_TYPE2>(p, x, u[0], u[1], xd);
}

// The limits of one launch, by value in the kernel arguments.
struct GenLimits {
    double Ts;
    double u_lo[2], u_hi[2], du_lo[2], du_hi[2];
    int slew[2];        // 0: the channel has no limiter (du_lo = -inf and du_hi = +inf)
    int clip_state;
    double vx_min, omega_max;
};

// One step of one trajectory: generation_type1.py:131-137 (the limiter, on the unclipped sequence s),
// :287-288 (the output clip, never fed back into s), :76-82 (Euler step, then the clip of the stored state).
template <int MODEL>
__device__ __forceinline__ void gen_step(const VP& p, const GenLimits& g, bool first, const double* ur, double* s,
                                         double* u, double* x) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (first || !g.slew[c]) s[c] = ur[c];
        else s[c] = s[c] + clampd(ur[c] - s[c], g.du_lo[c], g.du_hi[c]);
        u[c] = clampd(s[c], g.u_lo[c], g.u_hi[c]);
    }
    double f[6];
    gen_model_f<MODEL>(p, x, u, f);
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = x[j] + g.Ts * f[j];
    if (g.clip_state) {
        x[3] = (x[3] < g.vx_min) ? g.vx_min : x[3];            // python max(vx, vx_min)
        x[5] = clampd(x[5], -g.omega_max, g.omega_max);        // np.clip
    }
}

constexpr int GEN_WAVE = 64;

// Staged form.  LDS per wave: 64 rows (one per trajectory) of 2 K doubles of u_raw, overwritten in place by U,
// and 64 rows of 6 K doubles of X; each row padded by 2 doubles so that the lanes' own reads and writes (one row
// per lane) spread over the banks.  The next chunk's u_raw is fetched into registers before the current chunk is
// computed and lands in LDS after it, so its latency overlaps the serial steps.
template <int MODEL, int K>
__global__ __launch_bounds__(GEN_WAVE) void gen_staged_kernel(VP p, GenLimits g, int B, int T, const double* x0,
                                                              const double* u_raw, double* X, double* U) {
    constexpr int NU = 2 * K, NX = 6 * K, SU = NU + 2, SX = NX + 2;
    __shared__ double sU[GEN_WAVE * SU];
    __shared__ double sX[GEN_WAVE * SX];
    const int lane = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * GEN_WAVE;
    const long long b = b0 + lane;
    const bool active = b < B;

    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s[2] = {0.0, 0.0};
    if (active) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            x[j] = x0[b * 6 + j];
            X[b * (long long)(T + 1) * 6 + j] = x[j];
        }
    }

    // element i of the wave's chunk: row r (trajectory b0 + r), column c of that row's run
    double pre[NU];
    auto fetch = [&](int k0) {
        const int kc = (T - k0 < K) ? (T - k0) : K;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int flat = i * GEN_WAVE + lane, r = flat / NU, c = flat % NU;
            pre[i] = (b0 + r < B && c < 2 * kc) ? u_raw[((b0 + r) * (long long)T + k0) * 2 + c] : 0.0;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += K) {
        const int kc = (T - k0 < K) ? (T - k0) : K;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int flat = i * GEN_WAVE + lane, r = flat / NU, c = flat % NU;
            sU[r * SU + c] = pre[i];
        }
        __syncthreads();
        if (k0 + K < T) fetch(k0 + K);
        if (active) {
            for (int k = 0; k < kc; ++k) {
                double ur[2] = {sU[lane * SU + 2 * k], sU[lane * SU + 2 * k + 1]}, u[2];
                gen_step<MODEL>(p, g, k0 + k == 0, ur, s, u, x);
                sU[lane * SU + 2 * k] = u[0];
                sU[lane * SU + 2 * k + 1] = u[1];
#pragma unroll
                for (int j = 0; j < 6; ++j) sX[lane * SX + 6 * k + j] = x[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int flat = i * GEN_WAVE + lane, r = flat / NU, c = flat % NU;
            if (b0 + r < B && c < 2 * kc) U[((b0 + r) * (long long)T + k0) * 2 + c] = sU[r * SU + c];
        }
#pragma unroll 8
        for (int i = 0; i < NX; ++i) {
            const int flat = i * GEN_WAVE + lane, r = flat / NX, c = flat % NX;
            if (b0 + r < B && c < 6 * kc) X[((b0 + r) * (long long)(T + 1) + k0 + 1) * 6 + c] = sX[r * SX + c];
        }
        __syncthreads();
    }
}

// Direct form: every lane loads its own u_raw row (the next step's before the current step is computed) and
// stores its own U and X rows.
template <int MODEL>
__global__ __launch_bounds__(GEN_WAVE) void gen_direct_kernel(VP p, GenLimits g, int B, int T, const double* x0,
                                                              const double* u_raw, double* X, double* U) {
    const long long b = (long long)blockIdx.x * GEN_WAVE + threadIdx.x;
    if (b >= B) return;
    const double* ub = u_raw + b * (long long)T * 2;
    double* Ub = U + b * (long long)T * 2;
    double* Xb = X + b * (long long)(T + 1) * 6;
    double x[6], s[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        x[j] = x0[b * 6 + j];
        Xb[j] = x[j];
    }
    double nxt[2] = {ub[0], ub[1]};
    for (int k = 0; k < T; ++k) {
        double ur[2] = {nxt[0], nxt[1]}, u[2];
        if (k + 1 < T) {
            nxt[0] = ub[2 * (k + 1)];
            nxt[1] = ub[2 * (k + 1) + 1];
        }
        gen_step<MODEL>(p, g, k == 0, ur, s, u, x);
        Ub[2 * k] = u[0];
        Ub[2 * k + 1] = u[1];
#pragma unroll
        for (int j = 0; j < 6; ++j) Xb[6 * (k + 1) + j] = x[j];
    }
}

static std::atomic<int> g_gen_form{0};

template <int MODEL>
static void gen_launch(int form, const VP& p, const GenLimits& g, int B, int T, const double* x0,
                       const double* u_raw, double* X, double* U, hipStream_t st) {
    const dim3 grid((unsigned)((B + GEN_WAVE - 1) / GEN_WAVE)), block(GEN_WAVE);
    if (form == 2)
        hipLaunchKernelGGL(gen_direct_kernel<MODEL>, grid, block, 0, st, p, g, B, T, x0, u_raw, X, U);
    else
        hipLaunchKernelGGL((gen_staged_kernel<MODEL, TRAJ_GEN_STAGE_STEPS>), grid, block, 0, st, p, g, B, T, x0,
                           u_raw, X, U);
}

}  // namespace tgmpc

extern "C" {

int traj_gen_abi_version(void) { return TRAJGEN_ABI_VERSION; }

int traj_gen_default_config(traj_gen_config* c, int model, double Ts) {
    if (!c || model < TRAJ_GEN_MODEL_MPC || model > TRAJ_GEN_MODEL_TYPE2) return TRAJ_E_ARG;
    std::memset(c, 0, sizeof(*c));
    c->model = model;
    c->Ts = Ts;
    for (int i = 0; i < 2; ++i) {
        c->u_lo[i] = c->du_lo[i] = -INFINITY;
        c->u_hi[i] = c->du_hi[i] = INFINITY;
    }
    c->clip_state = (model != TRAJ_GEN_MODEL_MPC);
    c->vx_min = 0.0;
    c->omega_max = 6.0;
    if (model == TRAJ_GEN_MODEL_TYPE1) {
        c->u_lo[0] = -1.0; c->u_hi[0] = 1.0; c->u_lo[1] = -0.6; c->u_hi[1] = 0.6;
        c->du_lo[0] = -0.1; c->du_hi[0] = 0.1; c->du_lo[1] = -0.04; c->du_hi[1] = 0.04;
    }
    return TRAJ_OK;
}

int traj_gen_debug_store_form(int form) {
    if (form < 0 || form > 2) return TRAJ_E_ARG;
    tgmpc::g_gen_form.store(form);
    return TRAJ_OK;
}

int traj_gen_simulate_batch(const traj_vehicle_params* p, const traj_gen_config* c, int B, int T, const double* x0,
                            const double* u_raw, double* X, double* U, void* stream) {
    using namespace tgmpc;
    if (!p || !c || B < 0 || T < 1) return TRAJ_E_ARG;
    if (c->model < TRAJ_GEN_MODEL_MPC || c->model > TRAJ_GEN_MODEL_TYPE2 || !std::isfinite(c->Ts)) return TRAJ_E_ARG;
    if (B > 0 && (!x0 || !u_raw || !X || !U)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    GenLimits g;
    g.Ts = c->Ts;
    for (int i = 0; i < 2; ++i) {
        g.u_lo[i] = c->u_lo[i]; g.u_hi[i] = c->u_hi[i];
        g.du_lo[i] = c->du_lo[i]; g.du_hi[i] = c->du_hi[i];
        g.slew[i] = !(std::isinf(c->du_lo[i]) && c->du_lo[i] < 0 && std::isinf(c->du_hi[i]) && c->du_hi[i] > 0);
    }
    g.clip_state = c->clip_state != 0;
    g.vx_min = c->vx_min;
    g.omega_max = c->omega_max;
    int form = g_gen_form.load();
    if (form == 0) form = TRAJ_GEN_DEFAULT_FORM;
    hipStream_t st = (hipStream_t)stream;
    switch (c->model) {
        case TRAJ_GEN_MODEL_MPC: gen_launch<TRAJ_GEN_MODEL_MPC>(form, *p, g, B, T, x0, u_raw, X, U, st); break;
        case TRAJ_GEN_MODEL_TYPE1: gen_launch<TRAJ_GEN_MODEL_TYPE1>(form, *p, g, B, T, x0, u_raw, X, U, st); break;
        default: gen_launch<TRAJ_GEN_MODEL_TYPE2>(form, *p, g, B, T, x0, u_raw, X, U, st); break;
    }
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

}  // extern "C"

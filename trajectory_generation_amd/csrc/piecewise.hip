// piecewise.hip -- the type-2 dataset generator (generation_type2.py:95-157, :180-187) whole on the GPU: the
// piecewise state-machine controller, its random stream (gen_rng.h: numpy's Generator(PCG64)) and the Euler
// integration, one lane per trajectory, the whole T-step walk in one launch.
//
// The controller reads the speed of a shadow simulation at every segment start and every step, so its controls
// cannot be drawn ahead of the simulation.  The shadow state (:152-154) and the ground truth (:182-187) are the
// same arithmetic on the same inputs: the lane integrates once.  A lane keeps in registers its PCG64 state, the
// vehicle state, prev_mode, prev_delta_cmd and the running segment's mode, d, delta and remaining length.
// Per step it stores 16 B of U, 48 B of X and one byte of mode with direct per-lane stores (the form that measured
// faster for the open-loop kernel, profiles/openloop_probe.json).  A segment starts about once in 95 steps; the
// lanes of a wave start theirs at different steps, so that branch runs for few lanes at a time.
// The ziggurat tables (6 KB) are copied into LDS at launch: lanes index them with a random layer.
//
// Built with the library's FLAGS: -ffp-contract=off keeps every expression in the reference's order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/trajgen.h"
#include "gen_model.h"
#include "gen_rng.h"
#include "gen_zig_lds.h"

namespace tgmpc {

constexpr int PW_WAVE = 64;

__host__ __device__ __forceinline__ void pcg_load(Pcg64& s, const unsigned long long* p) {
    s.hi = p[0]; s.lo = p[1]; s.inc_hi = p[2]; s.inc_lo = p[3];
}
__host__ __device__ __forceinline__ void pcg_store(const Pcg64& s, unsigned long long* p) {
    p[0] = s.hi; p[1] = s.lo; p[2] = s.inc_hi; p[3] = s.inc_lo;
}

template <typename OUT>
__host__ __device__ __forceinline__ void rng_draw(Pcg64& s, const ZigTables& z, int kind, long long n, OUT* out) {
    if (kind == TRAJ_RNG_RAW) {
        unsigned long long* o = (unsigned long long*)out;
        for (long long i = 0; i < n; ++i) o[i] = pcg64_next(s);
    } else if (kind == TRAJ_RNG_DOUBLE) {
        double* o = (double*)out;
        for (long long i = 0; i < n; ++i) o[i] = rng_next_double(s);
    } else {
        double* o = (double*)out;
        for (long long i = 0; i < n; ++i) o[i] = rng_standard_normal(s, z);
    }
}

__global__ __launch_bounds__(PW_WAVE) void rng_draw_kernel(int B, int n, int kind, const unsigned long long* states,
                                                           void* out, unsigned long long* states_out) {
    __shared__ ZigLds lds;
    zig_load(lds);
    const long long b = (long long)blockIdx.x * PW_WAVE + threadIdx.x;
    if (b >= B) return;
    const ZigTables z{lds.wi, lds.ki, lds.fi};
    Pcg64 s;
    pcg_load(s, states + 4 * b);
    rng_draw(s, z, kind, n, (unsigned long long*)out + b * (long long)n);   // 8 bytes per draw of either type
    if (states_out) pcg_store(s, states_out + 4 * b);
}

// The per-launch constants of the controller, by value in the kernel arguments.
struct FsmArgs {
    traj_gen_fsm_rules r;
    double Ts, max_step;     // max_step = delta_rate_max * Ts
    int stall_len;           // int(round(0.3 / Ts))
    int clip_state;
    double vx_min, omega_max;
};

// python max(a, b) / min(a, b): the first argument unless the second is strictly greater / smaller
__device__ __forceinline__ double py_max(double a, double b) { return (b > a) ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return (b < a) ? b : a; }

__global__ __launch_bounds__(PW_WAVE) void piecewise_kernel(VP p, FsmArgs g, int B, int T, const double* x0,
                                                            const unsigned long long* rng_state, double* X, double* U,
                                                            unsigned char* mode_out, unsigned long long* rng_state_out) {
    __shared__ ZigLds lds;
    zig_load(lds);
    const long long b = (long long)blockIdx.x * PW_WAVE + threadIdx.x;
    if (b >= B) return;
    const ZigTables z{lds.wi, lds.ki, lds.fi};
    double* Ub = U + b * (long long)T * 2;
    double* Xb = X + b * (long long)(T + 1) * 6;
    unsigned char* Mb = mode_out + b * (long long)T;

    Pcg64 s;
    pcg_load(s, rng_state + 4 * b);
    double x[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        x[j] = x0[b * 6 + j];
        Xb[j] = x[j];
    }
    double prev_delta_cmd = 0.0, d = 0.0, delta = 0.0;
    bool prev_turn = false;          // prev_mode in (turn_left, turn_right); "init" is not
    int mode = TRAJ_FSM_ACCELERATE, left = 0;

    for (int k = 0; k < T; ++k) {
        if (left == 0) {
            // ---- segment start, generation_type2.py:107-133, the draws in the reference's order
            if (prev_turn) mode = rng_choice(s, g.r.cdf_after_turn, 2);
            else mode = rng_choice(s, g.r.cdf_any, 4);
            const double len = rint(rng_uniform(s, TRAJ_FSM_SEG_LO, TRAJ_FSM_SEG_HI) / g.Ts);   // half to even
            left = (len < 1.0) ? 1 : ((len > 2147483647.0) ? 2147483647 : (int)len);
            const double v = hypot(x[3], x[4]);
            if (mode == TRAJ_FSM_ACCELERATE) {
                if (v >= g.r.v_high) mode = TRAJ_FSM_CRUISE;      // the label only
                d = rng_uniform(s, TRAJ_FSM_ACCEL_D_LO, g.r.d_range[1]);
                delta = rng_normal(s, z, g.r.delta_straight_noise);
            } else if (mode == TRAJ_FSM_CRUISE) {
                d = rng_uniform(s, TRAJ_FSM_CRUISE_D_LO, TRAJ_FSM_CRUISE_D_HI);
                delta = rng_normal(s, z, g.r.delta_straight_noise);
            } else {
                d = (v > g.r.v_turn_max) ? rng_uniform(s, TRAJ_FSM_TURN_FAST_D_LO, TRAJ_FSM_TURN_FAST_D_HI)
                                         : rng_uniform(s, TRAJ_FSM_TURN_D_LO, TRAJ_FSM_TURN_D_HI);
                const double mag = rng_uniform(s, g.r.delta_turn_range[0], g.r.delta_turn_range[1]);
                const double scale = py_min(1.0, g.r.v_turn_max / py_max(v, 1e-3));
                delta = ((mode == TRAJ_FSM_TURN_LEFT) ? mag : -mag) * scale;
            }
            if (v < TRAJ_FSM_V_STALL) {
                mode = TRAJ_FSM_ACCELERATE;
                d = rng_uniform(s, TRAJ_FSM_STALL_D_LO, TRAJ_FSM_STALL_D_HI);
                delta = rng_normal(s, z, g.r.delta_straight_noise);
                left = left > g.stall_len ? left : g.stall_len;
            }
            prev_turn = mode >= TRAJ_FSM_TURN_LEFT;       // prev_mode of the next start: the label after relabelling
        }
        // ---- one step, :138-155
        const double v = hypot(x[3], x[4]);
        if (v < TRAJ_FSM_V_FLOOR) d = py_max(d, TRAJ_FSM_D_BOOST_MIN);
        const double d_k = clampd(d, g.r.d_range[0], g.r.d_range[1]);
        double delta_k = clampd(delta, -TRAJ_FSM_DELTA_CLIP, TRAJ_FSM_DELTA_CLIP);
        delta_k = clampd(delta_k, prev_delta_cmd - g.max_step, prev_delta_cmd + g.max_step);
        prev_delta_cmd = delta_k;
        Ub[2 * k] = d_k;
        Ub[2 * k + 1] = delta_k;
        Mb[k] = (unsigned char)mode;

        double f[6];
        gen_f_cont<true>(p, x, d_k, delta_k, f);
#pragma unroll
        for (int j = 0; j < 6; ++j) x[j] = x[j] + g.Ts * f[j];
        if (g.clip_state) {
            x[3] = (x[3] < g.vx_min) ? g.vx_min : x[3];            // python max(vx, vx_min)
            x[5] = clampd(x[5], -g.omega_max, g.omega_max);        // np.clip
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) Xb[6 * (k + 1) + j] = x[j];
        --left;
    }
    if (rng_state_out) pcg_store(s, rng_state_out + 4 * b);
}

}  // namespace tgmpc

extern "C" {

int traj_gen_fsm_default_rules(traj_gen_fsm_rules* r) {
    if (!r) return TRAJ_E_ARG;
    std::memset(r, 0, sizeof(*r));
    r->v_turn_max = 1.2;
    r->v_high = 4.0;
    r->d_range[0] = 0.0; r->d_range[1] = 0.33;
    r->delta_turn_range[0] = 0.015; r->delta_turn_range[1] = 0.04;
    r->delta_straight_noise = 0.004;
    // p.cumsum() / p.cumsum()[-1], term by term as numpy adds them
    const double p2[2] = {0.5, 0.5}, p4[4] = {0.35, 0.35, 0.15, 0.15};
    double acc = 0.0;
    for (int i = 0; i < 2; ++i) { acc = acc + p2[i]; r->cdf_after_turn[i] = acc; }
    for (int i = 0; i < 2; ++i) r->cdf_after_turn[i] = r->cdf_after_turn[i] / acc;
    acc = 0.0;
    for (int i = 0; i < 4; ++i) { acc = acc + p4[i]; r->cdf_any[i] = acc; }
    for (int i = 0; i < 4; ++i) r->cdf_any[i] = r->cdf_any[i] / acc;
    return TRAJ_OK;
}

int traj_gen_piecewise_batch(const traj_vehicle_params* p, const traj_gen_config* c, const traj_gen_fsm_rules* r, int B,
                             int T, const double* x0, const unsigned long long* rng_state, double* X, double* U,
                             unsigned char* mode, unsigned long long* rng_state_out, void* stream) {
    using namespace tgmpc;
    if (!p || !c || !r || B < 0 || T < 1) return TRAJ_E_ARG;
    if (c->model != TRAJ_GEN_MODEL_TYPE2 || !std::isfinite(c->Ts) || !(c->Ts > 0.0)) return TRAJ_E_ARG;
    if (r->cdf_after_turn[1] != 1.0 || r->cdf_any[3] != 1.0) return TRAJ_E_ARG;
    if (B > 0 && (!x0 || !rng_state || !X || !U || !mode)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    FsmArgs g;
    g.r = *r;
    g.Ts = c->Ts;
    g.max_step = TRAJ_FSM_DELTA_RATE_MAX * c->Ts;
    const double sl = std::rint(TRAJ_FSM_STALL_SEG / c->Ts);
    g.stall_len = sl > 2147483647.0 ? 2147483647 : (int)sl;
    g.clip_state = c->clip_state != 0;
    g.vx_min = c->vx_min;
    g.omega_max = c->omega_max;
    const dim3 grid((unsigned)((B + PW_WAVE - 1) / PW_WAVE)), block(PW_WAVE);
    hipLaunchKernelGGL(piecewise_kernel, grid, block, 0, (hipStream_t)stream, *p, g, B, T, x0, rng_state, X, U, mode,
                       rng_state_out);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_gen_rng_draw_host(const unsigned long long* state, int kind, long long n, void* out,
                           unsigned long long* state_out) {
    using namespace tgmpc;
    if (!state || n < 0 || kind < TRAJ_RNG_RAW || kind > TRAJ_RNG_NORMAL || (n > 0 && !out)) return TRAJ_E_ARG;
    const ZigTables z{zig_host_wi, (const uint64_t*)zig_host_ki, zig_host_fi};
    Pcg64 s;
    pcg_load(s, state);
    rng_draw(s, z, kind, n, (unsigned long long*)out);
    if (state_out) pcg_store(s, state_out);
    return TRAJ_OK;
}

int traj_gen_rng_draw_batch(int B, int n, int kind, const unsigned long long* states, void* out,
                            unsigned long long* states_out, void* stream) {
    using namespace tgmpc;
    if (B < 0 || n < 0 || kind < TRAJ_RNG_RAW || kind > TRAJ_RNG_NORMAL) return TRAJ_E_ARG;
    if (B > 0 && (!states || (n > 0 && !out))) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    const dim3 grid((unsigned)((B + PW_WAVE - 1) / PW_WAVE)), block(PW_WAVE);
    hipLaunchKernelGGL(rng_draw_kernel, grid, block, 0, (hipStream_t)stream, B, n, kind, states, out, states_out);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

}  // extern "C"

// mpc_frame.h -- the frame the condensed solve kernels share: what surrounds a tier's linear algebra and is not tuned
// per tier.  mpc_solve.h and mpc_long.h call all of it, closed_sb_plant_kernel (trajmpc.hip) the plant update, and
// mpc_split.h the open-loop outputs (its closed-loop frame is its own: see there).
// Every helper takes the kernel's argument block `a` and thread index `t` from its caller: the fused instances read
// `a` through an opaque kernarg pointer and `t` through an opaque move so that nothing is hoisted out of the item loop,
// and a helper that re-read threadIdx.x or the by-value argument would undo that.  FUSED selects the coherent (sc1)
// loads and stores of state handed between workgroups (st_coh / ld_coh); the values are the same either way.
#pragma once
#include "mpc_common.h"

namespace tgmpc {

// ---- inputs ----
// x (6) and u_prev (2) of instance b into LDS: the closed loop's state (fused: what the previous step published), or the
// step entry point's x0 / u_prev
template <bool CLOSED, bool FUSED>
__device__ __forceinline__ void load_state(const KArgs& a, int b, int t, double* s_x, double* s_u) {
    if (FUSED) {
        if (t < 6) s_x[t] = ld_coh(a.x_state + 6 * b + t);
        if (t < 2) s_u[t] = ld_coh(a.u_state + 2 * b + t);
    } else if (CLOSED) {
        if (t < 6) s_x[t] = a.x_state[6 * b + t];
        if (t < 2) s_u[t] = a.u_state[2 * b + t];
    } else {
        if (t < 6) s_x[t] = a.x0[6 * b + t];
        if (t < 2) s_u[t] = a.u_prev[2 * b + t];
    }
}

// The window of instance b (main.py:51-68) from x00 = X (LDS, loaded and synchronized by the caller) into pref [N + 1][3]
// (LDS): xs_0 = X, xs_{k+1} = xs_k + vref_k Ts (serial on thread 0: a running sum), then per stage path(xs) and
// phi* = atan(path'(xs)).  Called by the whole block; the caller synchronizes before other threads read pref.
__device__ __forceinline__ void build_window(const KArgs& a, int b, int N, double Ts, const double* x00,
                                             const double* vref, double* pref, int t, int NT) {
    if (t == 0) {
        double xs = x00[0];
        pref[0] = xs;
        for (int k = 0; k < N; ++k) {
            xs = xs + vref[k] * Ts;
            pref[3 * (k + 1)] = xs;
        }
    }
    __syncthreads();
    for (int k = t; k <= N; k += NT) {
        double y, dy;
        path_eval(a.path, b, pref[3 * k], y, dy);
        pref[3 * k + 1] = y;
        pref[3 * k + 2] = pm_atan(dy);
    }
}

// ---- warm record (wsWarm: rho, valid, iterations, mean iterations) ----
// thread 0, a.wsWarm set: the record the instance's next step starts from
template <bool FUSED>
__device__ __forceinline__ void store_warm(const KArgs& a, int b, double rho, bool ok, int iter) {
    double* wv = a.wsWarm + 4 * (size_t)b;
    const double w[3] = {rho, ok ? 1.0 : 0.0, (double)iter};
    for (int i = 0; i < 3; ++i) {
        if (FUSED) st_coh(wv + i, w[i]);
        else wv[i] = w[i];
    }
}
// ... after an early exit (no solve): not valid, no iterations; rho stays
template <bool FUSED>
__device__ __forceinline__ void store_warm_early(const KArgs& a, int b) {
    if (FUSED) {
        st_coh(a.wsWarm + 4 * (size_t)b + 1, 0.0);
        st_coh(a.wsWarm + 4 * (size_t)b + 2, 0.0);
    } else {
        a.wsWarm[4 * (size_t)b + 1] = 0.0;
        a.wsWarm[4 * (size_t)b + 2] = 0.0;
    }
}

// ---- plant update and step outcome ----
// one thread: plant x <- x + Ts f(x, u_cmd) (main.py:97), u_prev <- u_cmd (:101), and the history rows of step tstep
// (plant_publish: the stores, given f = f(x, u_cmd))
template <bool FUSED>
__device__ __forceinline__ void plant_publish(const KArgs& a, int b, int tstep, const double* xs, const double* f,
                                              double uc0, double uc1) {
    for (int i = 0; i < 6; ++i) {
        const double xn = xs[i] + a.c.Ts * f[i];
        if (FUSED) st_coh(a.x_state + 6 * (size_t)b + i, xn);
        else a.x_state[6 * (size_t)b + i] = xn;
        if (a.hist_x) a.hist_x[((size_t)b * (a.hist_T + 1) + tstep + 1) * 6 + i] = xn;
    }
    if (FUSED) {
        st_coh(a.u_state + 2 * (size_t)b, uc0);
        st_coh(a.u_state + 2 * (size_t)b + 1, uc1);
    } else {
        a.u_state[2 * (size_t)b] = uc0;
        a.u_state[2 * (size_t)b + 1] = uc1;
    }
    if (a.hist_u) {
        a.hist_u[((size_t)b * a.hist_T + tstep) * 2] = uc0;
        a.hist_u[((size_t)b * a.hist_T + tstep) * 2 + 1] = uc1;
    }
}
template <bool FUSED>
__device__ __forceinline__ void plant_update(const KArgs& a, int b, int tstep, const double* x0, double uc0, double uc1) {
    double xs[6], f[6], u[2] = {uc0, uc1};
    for (int i = 0; i < 6; ++i) xs[i] = x0[i];
    f_cont(a.p, xs, u, f);
    plant_publish<FUSED>(a, b, tstep, xs, f, uc0, uc1);
}
// The same update where the item linearized in the workgroup (block_linearize's park): f(x_0, u_cmd) from what stage 0
// of the rollout already evaluated at x_0.  park[0] = atan2(omega lf + vy, vx_eff) and park[1] = the rear Pacejka sine
// sin(Cr atan(Br alpha_r)) do not depend on u; park[2], park[3] = sin / cos(phi_0).  They are the values tire_forces /
// f_cont_sc form from the same x_0 (mpc_linearize.h, the rollout lanes' exact identities), so what is left is the front
// slip at delta_cmd, Frx at d_cmd and sin / cos(delta_cmd).  The slip is tire_forces' "-atan2(...) + delta": the unary
// minus of the parked atan2 (exact), then one add; every other expression is f_cont_sc's, term by term.
template <bool FUSED>
__device__ __forceinline__ void plant_update_parked(const KArgs& a, int b, int tstep, const double* x0, double uc0,
                                                    double uc1, const double* park) {
    const VP& p = a.p;
    double xs[6], f[6];
    for (int i = 0; i < 6; ++i) xs[i] = x0[i];
    const double vx = xs[3], vy = xs[4], omega = xs[5];
    const double at = park[0], sphi = park[2], cphi = park[3];
    const double alpha_f = clampd(-at + uc1, -p.maxAlpha, p.maxAlpha);
    const double Fy_f = p.Df * pm_tire_sin(p.Cf * pm_atan(p.Bf * alpha_f));
    const double Fy_r = p.Dr * park[1];
    const double Frx = (p.Cm1 - p.Cm2 * vx) * uc0 - p.Cr0 - p.Cr2 * (vx * vx);
    double sd, cd;
    pm_sincos(uc1, &sd, &cd);
    f[0] = vx * cphi - vy * sphi;
    f[1] = vx * sphi + vy * cphi;
    f[2] = omega;
    f[3] = (1.0 / p.m) * (Frx - Fy_f * sd + p.m * vy * omega);
    f[4] = (1.0 / p.m) * (Fy_r + Fy_f * cd - p.m * vx * omega);
    f[5] = (1.0 / p.Iz) * (Fy_f * p.lf * cd - Fy_r * p.lr);
    plant_publish<FUSED>(a, b, tstep, xs, f, uc0, uc1);
}
// one thread: this step's status and iterations (row `step` of the launch), and, fused, the mean iterations per step of
// this launch (the next launch's order), accumulated in the warm record
template <bool FUSED>
__device__ __forceinline__ void step_outcome(const KArgs& a, int b, int step, int status, int iter) {
    if (a.status) a.status[(size_t)step * a.B + b] = status;
    if (a.iters) a.iters[(size_t)step * a.B + b] = iter;
    if (FUSED) {
        if (a.wsWarm) {
            double* m = a.wsWarm + 4 * (size_t)b + 3;
            const double acc = (step == 0 ? 0.0 : ld_coh(m)) + iter;
            st_coh(m, (step == a.nsteps - 1) ? acc / a.nsteps : acc);
        }
    }
}
// thread 0 at the end of a closed-loop step (fused: the caller's diagnostics stamps and the hand-off follow); park: the
// item's parked stage-0 values (PARK: plant_update_parked)
template <bool FUSED, bool PARK = false>
__device__ __forceinline__ void plant_step(const KArgs& a, int b, int step, int tstep, const double* x0, double uc0,
                                           double uc1, int status, int iter, const double* park = nullptr) {
    if (PARK) plant_update_parked<FUSED>(a, b, tstep, x0, uc0, uc1, park);
    else plant_update<FUSED>(a, b, tstep, x0, uc0, uc1);
    step_outcome<FUSED>(a, b, step, status, iter);
}

// ---- open-loop outputs (mpc_6stati.py:217-275) ----
// X_opt by the linear model X_{k+1} = A_k X_k + B_k U_k + g_k into Xs [N + 1][6] (LDS), stage by stage (thread i < 6:
// state i), with its barriers; U (stage-major) in Ub, stage k's A, B, g at gA + RA k, gB + RB k, gg + RG k
__device__ __forceinline__ void rollout_xopt(const double* gA, const double* gB, const double* gg, int RA, int RB, int RG,
                                             int N, const double* Ub, const double* x0, double* Xs, int t) {
    if (t < 6) Xs[t] = x0[t];
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        if (t < 6) {
            double v = 0.0;
            for (int cc = 0; cc < 6; ++cc) v += gA[RA * k + t * 6 + cc] * Xs[6 * k + cc];
            v += gB[RB * k + t * 2] * Ub[2 * k] + gB[RB * k + t * 2 + 1] * Ub[2 * k + 1] + gg[RG * k + t];
            Xs[6 * (k + 1) + t] = v;
        }
        __syncthreads();
    }
}
// the cost of :217-250 of stage k at (X_opt, U_opt), added to the thread's partial op (threads take k = t, t + NT, ...;
// the kernel's own block sum follows); s, co = sin / cos(phi*_k) from wherever the kernel keeps them
__device__ __forceinline__ void stage_cost(const traj_mpc_config& c, int k, int N, const double* Xs, const double* pref,
                                           double vref_k, double s, double co, const double* Ub, const double* up,
                                           double& op) {
    const double* X = Xs + 6 * k;
    const double ec = s * (X[0] - pref[3 * k]) - co * (X[1] - pref[3 * k + 1]);
    const double ep = X[2] - pref[3 * k + 2];
    const double ev = X[3] - vref_k;
    op += c.q_c * ec * ec + c.q_phi * ep * ep + c.q_vx * ev * ev;
    if (k < N) {
        const double u0 = Ub[2 * k], u1 = Ub[2 * k + 1];
        const double d0 = u0 - (k == 0 ? up[0] : Ub[2 * k - 2]);
        const double d1 = u1 - (k == 0 ? up[1] : Ub[2 * k - 1]);
        op += u0 * (c.R[0] * u0 + c.R[1] * u1) + u1 * (c.R[2] * u0 + c.R[3] * u1);
        op += d0 * (c.Rd[0] * d0 + c.Rd[1] * d1) + d1 * (c.Rd[2] * d0 + c.Rd[3] * d1);
    }
}
// u_cmd / status / objective / iters / polished (thread 0), and U_opt [2][N] (the thread that holds variable 2 kk + ch:
// uown) and X_opt [6][N + 1], NaN unless the solve is good
__device__ __forceinline__ void store_outputs(const KArgs& a, int b, int N, int t, int NT, bool good, double uc0,
                                              double uc1, int status, double obj, int iter, int pol, bool uown, int ch,
                                              int kk, double xsol, const double* Xs) {
    const double nan = __builtin_nan("");
    if (t == 0) {
        a.u_cmd[2 * b] = uc0;
        a.u_cmd[2 * b + 1] = uc1;
        a.status[b] = status;
        if (a.objective) a.objective[b] = good ? obj : nan;
        if (a.iters) a.iters[b] = iter;
        if (a.polished) a.polished[b] = pol;
    }
    if (a.U_opt && uown) a.U_opt[(size_t)b * 2 * N + ch * N + kk] = good ? xsol : nan;
    if (a.X_opt) {
        for (int i = t; i < 6 * (N + 1); i += NT) {
            const int r = i / (N + 1), k = i % (N + 1);
            a.X_opt[(size_t)b * 6 * (N + 1) + i] = good ? Xs[6 * k + r] : nan;
        }
    }
}

}  // namespace tgmpc

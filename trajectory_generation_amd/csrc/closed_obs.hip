// closed_obs.hip -- the closed loop on a state estimate (include/trajobs.h): per step a device copy x_ctl <- x_hat,
// traj_closed_loop_step_sched on the copy (every solver tier, the warm start and the speed schedule are that entry
// point's, untouched), and the observe kernel below: the plant update on the true state, the measurement, the estimator
// and the history rows.
//
// The EKF step has two forms that give the same bits (-ffp-contract=off: the same expressions, the same roundings):
//   scalar      ekf_step of knet_ekf_step.h, one thread per trajectory -- ekf_kernel's loop body, the anchor;
//   lane group  ekf_step_group below, 16 lanes per trajectory and 4 trajectories per wave: the 13 model evaluations of
//               the central-difference Jacobian on lanes 0..12 side by side, the 36-element products three elements
//               per lane, the gain's six columns on lanes 0..5, operands exchanged through LDS; every element's sum
//               runs in ekf_step's order.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/trajobs.h"
#include "mpc_host.h"   // launched, nblk
#include "physics.h"

namespace {

#include "knet_ekf_step.h"   // KPd, veh_f, ekf_step

using tgmpc::VP, tgmpc::launched, tgmpc::nblk;

struct ObsArgs {
    VP p;      // the plant's parameters (f_cont)
    KPd k;     // the EKF's model: the same parameters and the clamp limits
    double Ts;
    double Q[6], R[5];
    int B, est, t, hist_T;
    double* x_true;
    double* x_hat;
    double* P;
    const double* u;       // u_prev after the step: u_cmd
    const double* noise;
    double* hist_x;
    double* hist_xhat;
    double* hist_u;
    double* hist_y;
};

// one thread: the plant update of the closed loop (plant_update / plant_publish of mpc_frame.h: f_cont on the state,
// xs[i] + Ts * f[i]), the measurement y = rows 0,1,3,4,5 (+ noise), and the history rows of x, u and y
__device__ __forceinline__ void plant_measure(const ObsArgs& a, int b, double u0, double u1, double* xn, double* yv) {
    const int hr[5] = {0, 1, 3, 4, 5};
    double xs[6], f[6], u[2] = {u0, u1};
    for (int i = 0; i < 6; ++i) xs[i] = a.x_true[6 * (size_t)b + i];
    tgmpc::f_cont(a.p, xs, u, f);
    for (int i = 0; i < 6; ++i) {
        xn[i] = xs[i] + a.Ts * f[i];
        a.x_true[6 * (size_t)b + i] = xn[i];
        if (a.hist_x) a.hist_x[((size_t)b * (a.hist_T + 1) + a.t + 1) * 6 + i] = xn[i];
    }
    const size_t row = (size_t)b * a.hist_T + a.t;
    for (int c = 0; c < 5; ++c) {
        yv[c] = a.noise ? xn[hr[c]] + a.noise[row * 5 + c] : xn[hr[c]];
        if (a.hist_y) a.hist_y[row * 5 + c] = yv[c];
    }
    if (a.hist_u) {
        a.hist_u[row * 2] = u0;
        a.hist_u[row * 2 + 1] = u1;
    }
}

// the observe kernel, one thread per trajectory (every estimator; the EKF in its scalar form)
__global__ __launch_bounds__(64) void observe_kernel(const ObsArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const double u0 = a.u[2 * (size_t)b], u1 = a.u[2 * (size_t)b + 1];
    double xn[6], yv[5];
    plant_measure(a, b, u0, u1, xn, yv);
    if (a.est == TRAJ_OBS_EXTERNAL) return;
    double xh[6];
    if (a.est == TRAJ_OBS_EKF) {
        double P[6][6];
        for (int i = 0; i < 6; ++i) {
            xh[i] = a.x_hat[6 * (size_t)b + i];
            for (int j = 0; j < 6; ++j) P[i][j] = a.P[36 * (size_t)b + 6 * i + j];
        }
        ekf_step(a.k, a.Ts, xh, P, u0, u1, yv, a.Q, a.R);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) a.P[36 * (size_t)b + 6 * i + j] = P[i][j];
    } else {
        for (int i = 0; i < 6; ++i) xh[i] = xn[i];
    }
    for (int i = 0; i < 6; ++i) {
        a.x_hat[6 * (size_t)b + i] = xh[i];
        if (a.hist_xhat) a.hist_xhat[((size_t)b * (a.hist_T + 1) + a.t + 1) * 6 + i] = xh[i];
    }
}

// ---- the lane-group form ----
// One group's LDS record (doubles): the state, the measurement, the 13 model evaluations (row 0 the centre = the
// predicted state, rows 1..6 the + side, 7..12 the - side), F, P, F P / A Pm, Pm, K' [5][6], A, Q and R.
constexpr int G_X = 0, G_Y = 6, G_FE = 12, G_F = 90, G_P = 126, G_FP = 162, G_PM = 198, G_KT = 234, G_A = 264,
              G_Q = 300, G_R = 306, GROUP_DOUBLES = 312;
constexpr int GROUP_LANES = 16, GROUPS = 4;   // one wave per workgroup: __syncthreads is the wave's own barrier

// One EKF step of the group's record S, lane g of 16: X, P (and Y, Q, R) in, X and P out.  Every lane of the workgroup
// calls it (the barriers); each expression is ekf_step's, term by term and in its order.
__device__ __forceinline__ void ekf_step_group(const KPd& p, double Ts, int g, double* S, double d, double de) {
    const int hr[5] = {0, 1, 3, 4, 5};
    double *X = S + G_X, *Yv = S + G_Y, *FE = S + G_FE, *F = S + G_F, *P = S + G_P, *FP = S + G_FP, *Pm = S + G_PM,
           *Kt = S + G_KT, *A = S + G_A;
    const double *Q = S + G_Q, *R = S + G_R;
    // predict: the centre and the +- h evaluations, one per lane
    if (g < 13) {
        const int j = g == 0 ? -1 : (g - 1) % 6;
        const double h = 1e-6 * fmax(1.0, fabs(X[j < 0 ? 0 : j]));
        double xe[6], fe[6];
        for (int i = 0; i < 6; ++i) {
            const double x = X[i], hh = (i == j) ? h : 0.0;
            xe[i] = g == 0 ? x : (g <= 6 ? x + hh : x - hh);
        }
        veh_f(p, Ts, xe, d, de, fe);
        for (int i = 0; i < 6; ++i) FE[6 * g + i] = fe[i];
    }
    __syncthreads();
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        const double h = 1e-6 * fmax(1.0, fabs(X[j]));
        F[e] = (FE[6 * (1 + j) + i] - FE[6 * (7 + j) + i]) / (2.0 * h);
    }
    __syncthreads();
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += F[6 * i + k] * P[6 * k + j];
        FP[e] = s;
    }
    __syncthreads();
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += FP[6 * i + k] * F[6 * j + k];
        Pm[e] = s + (i == j ? Q[i] : 0.0);
    }
    __syncthreads();
    // update: S = H Pm H' + R and its Cholesky factor on every lane (25 registers, the same bits on each); the gain's
    // column j on lane j
    {
        double Sm[5][5], L[5][5] = {};
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = 0; c < 5; ++c) Sm[a][c] = Pm[6 * hr[a] + hr[c]] + (a == c ? R[a] : 0.0);
#pragma unroll
        for (int a = 0; a < 5; ++a) {
#pragma unroll
            for (int c = 0; c <= a; ++c) {
                double s = Sm[a][c];
#pragma unroll
                for (int k = 0; k < c; ++k) s -= L[a][k] * L[c][k];
                L[a][c] = (a == c) ? sqrt(s) : s / L[c][c];
            }
        }
        if (g < 6) {
            const int j = g;
            double z[5], kt[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                double s = Pm[6 * hr[a] + j];
#pragma unroll
                for (int k = 0; k < a; ++k) s -= L[a][k] * z[k];
                z[a] = s / L[a][a];
            }
#pragma unroll
            for (int a = 4; a >= 0; --a) {
                double s = z[a];
#pragma unroll
                for (int k = a + 1; k < 5; ++k) s -= L[k][a] * kt[k];
                kt[a] = s / L[a][a];
            }
#pragma unroll
            for (int a = 0; a < 5; ++a) Kt[6 * a + j] = kt[a];
        }
    }
    __syncthreads();
    if (g < 6) {
        const int i = g;
        double s = 0.0;
        for (int a = 0; a < 5; ++a) s += Kt[6 * a + i] * (Yv[a] - FE[hr[a]]);
        X[i] = FE[i] + s;
    }
    // Joseph form: P = A Pm A' + K R K', A = I - K H
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        double kh = 0.0;
        for (int a = 0; a < 5; ++a) kh += (hr[a] == j) ? Kt[6 * a + i] : 0.0;
        A[e] = (i == j ? 1.0 : 0.0) - kh;
    }
    __syncthreads();
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += A[6 * i + k] * Pm[6 * k + j];
        FP[e] = s;
    }
    __syncthreads();
    for (int e = g; e < 36; e += GROUP_LANES) {
        const int i = e / 6, j = e % 6;
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += FP[6 * i + k] * A[6 * j + k];
        double kr = 0.0;
        for (int a = 0; a < 5; ++a) kr += Kt[6 * a + i] * R[a] * Kt[6 * a + j];
        P[e] = s + kr;
    }
    __syncthreads();
}

// the group's record filled: x [6], P [36] (NULL: a group past the batch, all zeros -- it runs the step for the
// barriers' sake and stores nothing), Q, R
__device__ __forceinline__ void group_load(int g, double* S, const double* x, const double* P, const double* Q,
                                           const double* R) {
    if (g < 6) S[G_X + g] = x ? x[g] : 0.0;
    if (g < 6) S[G_Q + g] = Q[g];
    if (g < 5) S[G_R + g] = R[g];
    if (g < 5 && !x) S[G_Y + g] = 0.0;
    for (int e = g; e < 36; e += GROUP_LANES) S[G_P + e] = P ? P[e] : 0.0;
}

// the observe kernel with the EKF in its lane-group form: lane 15 of a group runs the plant and the measurement
__global__ __launch_bounds__(GROUP_LANES * GROUPS) void observe_group_kernel(const ObsArgs a) {
    __shared__ double lds[GROUPS * GROUP_DOUBLES];
    const int g = threadIdx.x % GROUP_LANES, grp = threadIdx.x / GROUP_LANES;
    const int b = blockIdx.x * GROUPS + grp;
    const bool live = b < a.B;
    double* S = lds + grp * GROUP_DOUBLES;
    const double u0 = live ? a.u[2 * (size_t)b] : 0.0, u1 = live ? a.u[2 * (size_t)b + 1] : 0.0;
    group_load(g, S, live ? a.x_hat + 6 * (size_t)b : nullptr, live ? a.P + 36 * (size_t)b : nullptr, a.Q, a.R);
    if (live && g == GROUP_LANES - 1) {
        double xn[6], yv[5];
        plant_measure(a, b, u0, u1, xn, yv);
        for (int c = 0; c < 5; ++c) S[G_Y + c] = yv[c];
    }
    __syncthreads();
    ekf_step_group(a.k, a.Ts, g, S, u0, u1);
    if (!live) return;
    if (g < 6) {
        a.x_hat[6 * (size_t)b + g] = S[G_X + g];
        if (a.hist_xhat) a.hist_xhat[((size_t)b * (a.hist_T + 1) + a.t + 1) * 6 + g] = S[G_X + g];
    }
    for (int e = g; e < 36; e += GROUP_LANES) a.P[36 * (size_t)b + e] = S[G_P + e];
}

// the estimator alone (traj_ekf_step_f64), in the two forms
__global__ __launch_bounds__(64) void ekf_step_kernel(KPd p, double Ts, int B, double* x, double* Pg, const double* u,
                                                      const double* y, const double* Q, const double* R) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double xh[6], P[6][6], yv[5];
    for (int i = 0; i < 6; ++i) {
        xh[i] = x[6 * (size_t)b + i];
        for (int j = 0; j < 6; ++j) P[i][j] = Pg[36 * (size_t)b + 6 * i + j];
    }
    for (int c = 0; c < 5; ++c) yv[c] = y[5 * (size_t)b + c];
    ekf_step(p, Ts, xh, P, u[2 * (size_t)b], u[2 * (size_t)b + 1], yv, Q, R);
    for (int i = 0; i < 6; ++i) {
        x[6 * (size_t)b + i] = xh[i];
        for (int j = 0; j < 6; ++j) Pg[36 * (size_t)b + 6 * i + j] = P[i][j];
    }
}

__global__ __launch_bounds__(GROUP_LANES * GROUPS) void ekf_step_group_kernel(KPd p, double Ts, int B, double* x,
                                                                              double* Pg, const double* u,
                                                                              const double* y, const double* Q,
                                                                              const double* R) {
    __shared__ double lds[GROUPS * GROUP_DOUBLES];
    const int g = threadIdx.x % GROUP_LANES, grp = threadIdx.x / GROUP_LANES;
    const int b = blockIdx.x * GROUPS + grp;
    const bool live = b < B;
    double* S = lds + grp * GROUP_DOUBLES;
    const double u0 = live ? u[2 * (size_t)b] : 0.0, u1 = live ? u[2 * (size_t)b + 1] : 0.0;
    group_load(g, S, live ? x + 6 * (size_t)b : nullptr, live ? Pg + 36 * (size_t)b : nullptr, Q, R);
    if (live && g < 5) S[G_Y + g] = y[5 * (size_t)b + g];
    __syncthreads();
    ekf_step_group(p, Ts, g, S, u0, u1);
    if (!live) return;
    if (g < 6) x[6 * (size_t)b + g] = S[G_X + g];
    for (int e = g; e < 36; e += GROUP_LANES) Pg[36 * (size_t)b + e] = S[G_P + e];
}


KPd kpd_of(const traj_vehicle_params* p, const traj_knet_limits* lim) {
    return KPd{p->Cm1, p->Cm2, p->Cr0, p->Cr2, p->Br, p->Cr, p->Dr, p->Bf, p->Cf, p->Df, p->m, p->Iz, p->lf, p->lr,
               p->maxAlpha, p->vx_zero,
               {lim->x_min, lim->y_min, lim->phi_min, lim->vx_min, lim->vy_min, lim->omega_min},
               {lim->x_max, lim->y_max, lim->phi_max, lim->vx_max, lim->vy_max, lim->omega_max}};
}

std::atomic<int> g_obs_lanes{TRAJ_OBS_DEFAULT_LANES};

inline size_t closed_bytes8(const traj_mpc_config* c, int B) {
    return (traj_closed_loop_workspace_bytes(c, B) + 7) & ~(size_t)7;
}

// the estimator's part of the checks: the parameters, the batch, the estimator's code and, for the EKF, the limits and
// the covariances (NaN fails every comparison)
int est_check(const traj_vehicle_params* p, const traj_knet_limits* lim, const traj_obs_config* o, int B) {
    if (!p || !o || B < 0) return TRAJ_E_ARG;
    if (o->estimator < TRAJ_OBS_TRUTH || o->estimator > TRAJ_OBS_EXTERNAL) return TRAJ_E_ARG;
    if (o->estimator == TRAJ_OBS_EKF) {
        if (!lim) return TRAJ_E_ARG;
        for (int i = 0; i < 5; ++i)
            if (!(o->R[i] > 0.0)) return TRAJ_E_ARG;
        for (int i = 0; i < 6; ++i)
            if (!(o->Q[i] >= 0.0)) return TRAJ_E_ARG;
    }
    return TRAJ_OK;
}

// the observe kernel's launch in the form traj_debug_obs_lanes selects (a: this step's arguments)
int launch_observe(const ObsArgs& a, hipStream_t st) {
    if (a.est == TRAJ_OBS_EKF && g_obs_lanes.load(std::memory_order_relaxed) == GROUP_LANES)
        hipLaunchKernelGGL(observe_group_kernel, dim3(nblk(a.B, GROUPS)), dim3(GROUP_LANES * GROUPS), 0, st, a);
    else
        hipLaunchKernelGGL(observe_kernel, dim3(nblk(a.B, 64)), dim3(64), 0, st, a);
    return launched();
}

// what both entry points refuse before any launch, for the steps t0 .. t0 + steps - 1 (steps >= 1)
int obs_check(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths,
              const traj_knet_limits* lim, const traj_obs_config* o, int B, const double* x_true, const double* x_hat,
              const double* P, const double* u_prev, const double* vref, long long vref_row, int vref_len,
              int vref_step, const double* noise, int t0, int steps, int hist_T, bool hist, const void* workspace,
              size_t workspace_bytes) {
    if (!c || !paths) return TRAJ_E_ARG;
    if (const int e = est_check(p, lim, o, B)) return e;
    // the configuration, the paths and the schedule by traj_closed_loop_step_sched's own rules: its B = 0 call checks
    // them and launches nothing (the last step's window reaches furthest)
    const int e = traj_closed_loop_step_sched(p, c, paths, 0, nullptr, nullptr, nullptr, vref_row, vref_len, vref_step,
                                              t0 + steps - 1, hist_T, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              nullptr);
    if (e) return e;
    if (B == 0) return TRAJ_OK;
    if (!x_true || !x_hat || !u_prev || !vref) return TRAJ_E_ARG;
    if (o->estimator == TRAJ_OBS_EKF && !P) return TRAJ_E_ARG;
    if (!workspace || workspace_bytes < traj_closed_loop_obs_workspace_bytes(c, B)) return TRAJ_E_ARG;
    if ((hist || noise) && (t0 < 0 || t0 + steps > hist_T)) return TRAJ_E_ARG;
    if (vref_step && t0 < 0) return TRAJ_E_ARG;
    return TRAJ_OK;
}

// one step's launches (arguments checked)
int obs_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths, const ObsArgs& a0, int t,
             const double* vref, long long vref_row, int vref_len, int vref_step, int* status, int* iters,
             void* workspace, hipStream_t st) {
    const int B = a0.B;
    const size_t closed = closed_bytes8(c, B);
    double* x_ctl = (double*)((char*)workspace + closed);
    if (hipMemcpyAsync(x_ctl, a0.x_hat, (size_t)B * 6 * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return TRAJ_E_LAUNCH;
    const int e = traj_closed_loop_step_sched(p, c, paths, B, x_ctl, const_cast<double*>(a0.u), vref, vref_row,
                                              vref_len, vref_step, t, a0.hist_T, nullptr, nullptr, status, iters,
                                              workspace, closed, st);
    if (e) return e;
    ObsArgs a = a0;
    a.t = t;
    return launch_observe(a, st);
}

ObsArgs obs_args(const traj_vehicle_params* p, double Ts, const traj_knet_limits* lim,
                 const traj_obs_config* o, int B, double* x_true, double* x_hat, double* P, double* u_prev,
                 const double* noise, int hist_T, double* hist_x, double* hist_xhat, double* hist_u, double* hist_y) {
    ObsArgs a{};
    a.p = *p;
    if (o->estimator == TRAJ_OBS_EKF) a.k = kpd_of(p, lim);
    a.Ts = Ts;
    for (int i = 0; i < 6; ++i) a.Q[i] = o->Q[i];
    for (int i = 0; i < 5; ++i) a.R[i] = o->R[i];
    a.B = B;
    a.est = o->estimator;
    a.hist_T = hist_T;
    a.x_true = x_true;
    a.x_hat = x_hat;
    a.P = P;
    a.u = u_prev;
    a.noise = noise;
    a.hist_x = hist_x;
    a.hist_xhat = hist_xhat;
    a.hist_u = hist_u;
    a.hist_y = hist_y;
    return a;
}

}  // namespace

extern "C" {

size_t traj_closed_loop_obs_workspace_bytes(const traj_mpc_config* c, int B) {
    const size_t closed = traj_closed_loop_workspace_bytes(c, B);
    if (closed == 0 || B < 0) return 0;
    return ((closed + 7) & ~(size_t)7) + (size_t)B * 6 * sizeof(double);
}

int traj_closed_loop_obs_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths,
                              const traj_knet_limits* lim, const traj_obs_config* o, int B, double* x_true,
                              double* x_hat, double* P, double* u_prev, const double* vref, long long vref_row,
                              int vref_len, int vref_step, const double* noise, int t, int hist_T, double* hist_x,
                              double* hist_xhat, double* hist_u, double* hist_y, int* status, int* iters,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const bool hist = hist_x || hist_xhat || hist_u || hist_y;
    const int e = obs_check(p, c, paths, lim, o, B, x_true, x_hat, P, u_prev, vref, vref_row, vref_len, vref_step,
                            noise, t, 1, hist_T, hist, workspace, workspace_bytes);
    if (e || B == 0) return e;
    const ObsArgs a = obs_args(p, c->Ts, lim, o, B, x_true, x_hat, P, u_prev, noise, hist_T, hist_x, hist_xhat, hist_u,
                               hist_y);
    return obs_step(p, c, paths, a, t, vref, vref_row, vref_len, vref_step, status, iters, workspace,
                    (hipStream_t)stream);
}

int traj_closed_loop_obs_run(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths,
                             const traj_knet_limits* lim, const traj_obs_config* o, int B, double* x_true,
                             double* x_hat, double* P, double* u_prev, const double* vref, long long vref_row,
                             int vref_len, int vref_step, const double* noise, int t0, int steps, int hist_T,
                             double* hist_x, double* hist_xhat, double* hist_u, double* hist_y, int* status, int* iters,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (steps < 0) return TRAJ_E_ARG;
    const bool hist = hist_x || hist_xhat || hist_u || hist_y;
    // (steps == 0: the checks of a one-step call that reads nothing of the schedule or the histories)
    const int e = steps > 0 ? obs_check(p, c, paths, lim, o, B, x_true, x_hat, P, u_prev, vref, vref_row, vref_len,
                                        vref_step, noise, t0, steps, hist_T, hist, workspace, workspace_bytes)
                            : obs_check(p, c, paths, lim, o, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vref_row,
                                        vref_len, vref_step, nullptr, 0, 1, 1, false, nullptr, 0);
    if (e || B == 0 || steps == 0) return e;
    if (t0 < 0) return TRAJ_E_ARG;
    const ObsArgs a = obs_args(p, c->Ts, lim, o, B, x_true, x_hat, P, u_prev, noise, hist_T, hist_x, hist_xhat, hist_u,
                               hist_y);
    for (int s = 0; s < steps; ++s) {
        const int es = obs_step(p, c, paths, a, t0 + s, vref, vref_row, vref_len, vref_step,
                                status ? status + (size_t)s * B : nullptr, iters ? iters + (size_t)s * B : nullptr,
                                workspace, (hipStream_t)stream);
        if (es) return es;
    }
    return TRAJ_OK;
}

int traj_closed_loop_observe(const traj_vehicle_params* p, double Ts, const traj_knet_limits* lim,
                             const traj_obs_config* o, int B, double* x_true, double* x_hat, double* P,
                             const double* u_cmd, const double* noise, int t, int hist_T, double* hist_x,
                             double* hist_xhat, double* hist_u, double* hist_y, void* stream) {
    if (const int e = est_check(p, lim, o, B)) return e;
    if (!(Ts > 0.0)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x_true || !x_hat || !u_cmd || (o->estimator == TRAJ_OBS_EKF && !P)) return TRAJ_E_ARG;
    if ((hist_x || hist_xhat || hist_u || hist_y || noise) && (t < 0 || t >= hist_T)) return TRAJ_E_ARG;
    ObsArgs a = obs_args(p, Ts, lim, o, B, x_true, x_hat, P, const_cast<double*>(u_cmd), noise, hist_T, hist_x,
                         hist_xhat, hist_u, hist_y);
    a.t = t;
    return launch_observe(a, (hipStream_t)stream);
}

int traj_ekf_step_f64(const traj_vehicle_params* p, const traj_knet_limits* lim, double Ts, int B, double* x,
                      double* P, const double* u, const double* y, const double* Q, const double* R, void* stream) {
    if (!p || !lim || B < 0 || !(Ts > 0.0)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x || !P || !u || !y || !Q || !R) return TRAJ_E_ARG;
    const KPd k = kpd_of(p, lim);
    if (g_obs_lanes.load(std::memory_order_relaxed) == GROUP_LANES)
        hipLaunchKernelGGL(ekf_step_group_kernel, dim3(nblk(B, GROUPS)), dim3(GROUP_LANES * GROUPS), 0,
                           (hipStream_t)stream, k, Ts, B, x, P, u, y, Q, R);
    else
        hipLaunchKernelGGL(ekf_step_kernel, dim3(nblk(B, 64)), dim3(64), 0, (hipStream_t)stream, k, Ts, B, x, P, u, y,
                           Q, R);
    return launched();
}

int traj_debug_obs_lanes(int lanes) {
    if (lanes != 1 && lanes != GROUP_LANES) return TRAJ_E_ARG;
    g_obs_lanes.store(lanes, std::memory_order_relaxed);
    return TRAJ_OK;
}

}  // extern "C"

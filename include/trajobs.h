/*
 * trajobs.h -- C ABI of the closed loop on a state estimate in libtrajmpc.so (gfx950): the MPC closed loop of
 * trajmpc.h fed by an estimator instead of the plant's true state (output feedback).  Additive: the ABI version of
 * trajmpc.h stays 4.
 *
 * One step t, as a launch sequence on the caller's stream (no synchronisation, no allocation: a whole run can be
 * captured in a HIP graph):
 *   1. x_ctl <- x_hat                       (an asynchronous device copy into the workspace)
 *   2. traj_closed_loop_step_sched on (x_ctl, u_prev), unchanged, without history: the window from the estimate, the
 *      warm-started rho, every solver tier and the speed schedule are that entry point's; it leaves u_prev = u_cmd.
 *      The model prediction it writes into x_ctl is discarded.
 *   3. the observe kernel, per trajectory b:
 *        plant        x_true <- x_true + Ts f_cont(x_true, u_cmd)      (the closed loop's plant update, bit for bit)
 *        measurement  y[a] = x_true[hr[a]] + noise[b, t, a], hr = {0, 1, 3, 4, 5} (X, Y, vx, vy, omega; phi is not
 *                     measured); one IEEE addition, none with noise == NULL
 *        estimator    TRUTH: x_hat <- x_true.  EKF: one predict / update of traj_ekf_run_f64's filter on (x_hat, P)
 *                     with u_cmd and y.  EXTERNAL: x_hat is left as it is, for the caller to overwrite before the
 *                     next step.
 *        history      hist_x[b, t+1, :] = x_true, hist_xhat[b, t+1, :] = x_hat (not in EXTERNAL mode: the caller's
 *                     estimate is the caller's to record), hist_u[b, t, :] = u_cmd, hist_y[b, t, :] = y; each optional
 *
 * Conventions as trajmpc.h: device pointers, row-major, asynchronous on `stream`, 0 / TRAJ_E_*.
 */
#ifndef TRAJOBS_H
#define TRAJOBS_H

#include "trajknet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAJ_OBS_TRUTH 0
#define TRAJ_OBS_EKF 1
#define TRAJ_OBS_EXTERNAL 2

typedef struct {
    int estimator;   /* TRAJ_OBS_TRUTH, TRAJ_OBS_EKF, TRAJ_OBS_EXTERNAL */
    double Q[6];     /* EKF: process noise (diagonal), every entry >= 0 */
    double R[5];     /* EKF: measurement noise (diagonal), every entry > 0 */
} traj_obs_config;

/* traj_closed_loop_workspace_bytes(c, B) rounded up to 8, plus the control copy x_ctl [B,6]; 0 where that is 0. */
size_t traj_closed_loop_obs_workspace_bytes(const traj_mpc_config* c, int B);

/* One step (above).  x_true, x_hat [B,6] and u_prev [B,2] are updated in place; P [B,6,6] (EKF only) too.  lim: the
 * clamp limits of the EKF's vehicle model (EKF only).  vref, vref_row, vref_len, vref_step: the speed schedule of
 * traj_closed_loop_step_sched ((N + 1, N + 1, 0): the same vref [B,N+1] at every step).  noise [B,hist_T,5] or NULL.
 * hist_x, hist_xhat [B,hist_T+1,6], hist_u [B,hist_T,2], hist_y [B,hist_T,5], each or NULL.  status / iters [B]
 * (optional): this step's solver outcome.  Pass the same workspace to every step of one run (it holds the closed
 * loop's warm-start records).
 * TRAJ_E_ARG, before any launch: a null p, c, paths or o; B < 0; an estimator outside 0..2; EKF without lim or P, or
 * with an entry of R that is not > 0 or an entry of Q that is not >= 0 (NaN included); an invalid configuration or
 * schedule (traj_closed_loop_step_sched's rules); and with B > 0: a null x_true, x_hat, u_prev, vref or workspace, a
 * workspace below traj_closed_loop_obs_workspace_bytes, t outside 0 .. hist_T - 1 with a history or noise, t < 0 with
 * vref_step = 1.  B == 0: TRAJ_OK, no launch. */
int traj_closed_loop_obs_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths,
                              const traj_knet_limits* lim, const traj_obs_config* o, int B, double* x_true,
                              double* x_hat, double* P, double* u_prev, const double* vref, long long vref_row,
                              int vref_len, int vref_step, const double* noise, int t, int hist_T, double* hist_x,
                              double* hist_xhat, double* hist_u, double* hist_y, int* status, int* iters,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Steps t0 .. t0 + steps - 1, in order on the stream: exactly that many traj_closed_loop_obs_step calls.  status /
 * iters (optional) are [steps, B].  TRAJ_E_ARG as above, for every step of the call and before the first launch
 * (steps < 0, t0 < 0, t0 + steps > hist_T with a history or noise, the last step's window past the schedule);
 * steps == 0: TRAJ_OK, no launch. */
int traj_closed_loop_obs_run(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_paths* paths,
                             const traj_knet_limits* lim, const traj_obs_config* o, int B, double* x_true,
                             double* x_hat, double* P, double* u_prev, const double* vref, long long vref_row,
                             int vref_len, int vref_step, const double* noise, int t0, int steps, int hist_T,
                             double* hist_x, double* hist_xhat, double* hist_u, double* hist_y, int* status, int* iters,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Launch 3 alone -- plant, measurement, estimator and history rows for the commands u_cmd [B,2] -- for a caller with a
 * controller of its own; traj_closed_loop_obs_step ends with exactly this launch (Ts = c->Ts, u_cmd = u_prev after the
 * solve).  TRAJ_E_ARG: the estimator's rules above; Ts not > 0; with B > 0 a null x_true, x_hat or u_cmd, t outside
 * 0 .. hist_T - 1 with a history or noise.  B == 0: TRAJ_OK, no launch. */
int traj_closed_loop_observe(const traj_vehicle_params* p, double Ts, const traj_knet_limits* lim,
                             const traj_obs_config* o, int B, double* x_true, double* x_hat, double* P,
                             const double* u_cmd, const double* noise, int t, int hist_T, double* hist_x,
                             double* hist_xhat, double* hist_u, double* hist_y, void* stream);

/* The estimator alone: one EKF predict / update for B filters, in place on x [B,6] and P [B,6,6], with the commands
 * u [B,2] and the measurements y [B,5]; Q [6], R [5] device pointers, as traj_ekf_run_f64 takes them.  T calls on the
 * columns of a sequence give traj_ekf_run_f64's estimates bit for bit.  TRAJ_E_ARG: a null pointer, B < 0, Ts not
 * > 0; B == 0: TRAJ_OK, no launch. */
int traj_ekf_step_f64(const traj_vehicle_params* p, const traj_knet_limits* lim, double Ts, int B, double* x,
                      double* P, const double* u, const double* y, const double* Q, const double* R, void* stream);

/* The EKF step's form in the observe kernel and in traj_ekf_step_f64: 1 = one thread per filter (ekf_kernel's loop
 * body); 16 = sixteen lanes per filter, four filters per wave (the thirteen model evaluations of the Jacobian side by
 * side, the matrix products spread over the lanes, every sum in the scalar form's order: the same bits).  Returns
 * TRAJ_E_ARG for any other value.  For tests and measurements; the default is TRAJ_OBS_DEFAULT_LANES, the form that
 * measured faster (tools/closed_obs_bench.py). */
#define TRAJ_OBS_DEFAULT_LANES 16
int traj_debug_obs_lanes(int lanes);

#ifdef __cplusplus
}
#endif

#endif /* TRAJOBS_H */

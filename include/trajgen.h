/*
 * trajgen.h -- C ABI of the open-loop dataset generators (libtrajmpc.so, MI355X / gfx950).
 *
 * Drop-in boundary for DorianaG01/trajectory_generation generation_traj/: the slew-rate limiter, the
 * output clip and the explicit-Euler simulation of one trajectory, batched over B trajectories in
 * one launch.
 *
 *   reference (file:line)                              entry point here
 *   generation_type1.py:131-137 apply_du_bounds        traj_gen_simulate_batch (slew limiter)
 *   generation_type1.py:287-288 np.clip(..., lo, hi)   traj_gen_simulate_batch (output clip)
 *   generation_type1.py:70-84   simulate_trajectory    traj_gen_simulate_batch (Euler + state clip)
 *   generation_type1.py:38-68   tire_forces / f_cont   TRAJ_GEN_MODEL_TYPE1
 *   generation_type2.py:52-86   tire_forces / f_cont   TRAJ_GEN_MODEL_TYPE2
 *   generation_type2.py:180-187 integration loop       TRAJ_GEN_MODEL_TYPE2 with given controls
 *
 * Conventions are trajmpc.h's: device pointers, row-major float64, asynchronous on `stream`
 * (a hipStream_t, NULL = default stream), no allocation and no host synchronization (capturable in
 * a hipGraph), 0 on success and a negative TRAJ_E_* otherwise.  The version of this surface is
 * TRAJGEN_ABI_VERSION; trajmpc.h's TRAJMPC_ABI_VERSION does not change with it.
 */
#ifndef TRAJGEN_H
#define TRAJGEN_H

#include "trajmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAJGEN_ABI_VERSION 1

/* The three copies of the bicycle model the reference carries.  Against MODEL_MPC, types 1 and 2 use
 * vx_eff = max(|vx|, vx_zero) without the sign of vx, form Frx with vx_eff, and divide by m and Iz
 * (the MPC copy multiplies by 1/m and 1/Iz); type 1 clamps only the front slip angle, type 2 both. */
#define TRAJ_GEN_MODEL_MPC   0   /* mpc_6stati.py:25-71  (the model of traj_f_cont_batch)          */
#define TRAJ_GEN_MODEL_TYPE1 1   /* generation_type1.py:38-68                                  */
#define TRAJ_GEN_MODEL_TYPE2 2   /* generation_type2.py:52-86                                  */

typedef struct {
    int model; double Ts;
    double u_lo[2], u_hi[2];     /* output clip of d, delta (type 1: +-1, +-0.6)               */
    double du_lo[2], du_hi[2];   /* per-step slew limits (type 1: +-0.1, +-0.04); +-inf = none */
    int clip_state;              /* 1: vx <- max(vx, vx_min), omega <- clip(+-omega_max)       */
    double vx_min, omega_max;    /* 0.0, 6.0                                                   */
} traj_gen_config;

int traj_gen_abi_version(void);

/* Defaults per model.  TYPE1: the limits of generation_type1.py:251, :287-288 and the state clip of
 * :81-82.  TYPE2: no slew limit and no output clip (the controls of generation_type2.py:95-157 are
 * replayed as given), the state clip of :186-187.  MPC: no limits and no state clip (the plant update
 * of MPC/main.py:97).  TRAJ_E_ARG for a null pointer or an unknown model. */
int traj_gen_default_config(traj_gen_config* c, int model, double Ts);

/* B trajectories of T steps, one lane per trajectory:
 *   s[0] = u_raw[0];  s[k] = s[k-1] + clip(u_raw[k] - s[k-1], du_lo, du_hi)   (never fed the clipped U)
 *   U[k] = clip(s[k], u_lo, u_hi)
 *   X[0] = x0;  X[k+1] = X[k] + Ts * f(X[k], U[k]);  with clip_state, vx then omega of X[k+1] are
 *   clipped as stored, and the clipped state feeds the next step.
 * A channel whose du_lo is -inf and du_hi is +inf has no limiter: s[k] = u_raw[k] exactly.  NaN passes
 * every clip, as np.clip and Python's max pass it.
 * TRAJ_E_ARG: null pointer (data pointers only when B > 0), B < 0, T < 1, unknown model, Ts not finite.
 * B == 0: TRAJ_OK, no launch.  Nothing outside X[B,T+1,6] and U[B,T,2] is written. */
int traj_gen_simulate_batch(const traj_vehicle_params* p, const traj_gen_config* c, int B, int T,
                            const double* x0 /*[B,6]*/, const double* u_raw /*[B,T,2]*/,
                            double* X /*[B,T+1,6]*/, double* U /*[B,T,2]*/, void* stream);

/* The kernel form of the following traj_gen_simulate_batch calls: 0 the default, 1 the LDS-staged form
 * (TRAJ_GEN_STAGE_STEPS steps per wave staged in LDS, whole-wave coalesced loads and stores), 2 the
 * direct form (every lane loads and stores its own trajectory's rows).  The two are bit-identical.
 * The default is TRAJ_GEN_DEFAULT_FORM, the faster of the two at the reference's size (B = 5,000,
 * T = 1,200: profiles/openloop_probe.json).  For the measurement and the tests that compare them.
 * TRAJ_E_ARG for any other value. */
#define TRAJ_GEN_STAGE_STEPS 8
#define TRAJ_GEN_DEFAULT_FORM 2
int traj_gen_debug_store_form(int form);

#ifdef __cplusplus
}
#endif
#endif

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
 *   generation_type2.py:95-157  sample_controls_piecewise   traj_gen_piecewise_batch (controller, its
 *                               + :180-187                  numpy random stream and the integration)
 *
 * Conventions are trajmpc.h's: device pointers, row-major float64, asynchronous on `stream`
 * (a hipStream_t, NULL = default stream), no allocation and no host synchronization (capturable in
 * a hipGraph), 0 on success and a negative TRAJ_E_* otherwise.  The version of this surface is
 * TRAJGEN_ABI_VERSION; trajmpc.h's TRAJMPC_ABI_VERSION does not change with it.
 */
#ifndef TRAJGEN_H
#define TRAJGEN_H

#include <stdint.h>

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

/* ---- generation_type2.py:95-157, :180-187: the piecewise (state-machine) generator, whole on the GPU ----
 *
 * sample_controls_piecewise is a feedback controller: it draws a driving mode, a segment length and the
 * segment's controls from np.random.default_rng(seed + i), and reads the speed of a shadow simulation at
 * every segment start and every step.  The shadow simulation and the ground-truth integration of :180-187
 * are the same arithmetic on the same inputs, so one integration per lane serves both.  The random stream
 * is numpy's Generator(PCG64), reproduced in the kernel (csrc/gen_rng.h); the caller supplies each
 * trajectory's generator state, np.random.PCG64(seed + i).state, as four uint64
 * (state >> 64, state & (2^64 - 1), inc >> 64, inc & (2^64 - 1)) -- taken from numpy, or computed from the seed by
 * traj_gen_seed_pcg64_host / _batch below. */

/* The rules of generation_type2.py:22-30 that the controller reads, and the two mode distributions of
 * :109-112 as cumulative sums, cdf = p.cumsum() / p.cumsum()[-1] (what Generator.choice searches). */
typedef struct {
    double v_turn_max, v_high;          /* 1.2, 4.0                                                     */
    double d_range[2];                  /* (0.0, 0.33)                                                  */
    double delta_turn_range[2];         /* (0.015, 0.04)                                                */
    double delta_straight_noise;        /* 0.004                                                        */
    double cdf_after_turn[2];           /* accelerate, cruise:                         p = .5 .5        */
    double cdf_any[4];                  /* accelerate, cruise, turn_left, turn_right:  p = .35 .35 .15 .15 */
} traj_gen_fsm_rules;

/* The controller's constants (generation_type2.py:97, :101, :114, :120-124, :131-133, :142). */
#define TRAJ_FSM_DELTA_RATE_MAX 0.30   /* steering rate limit, rad/s                                    */
#define TRAJ_FSM_V_FLOOR        0.35   /* below it d is raised to TRAJ_FSM_D_BOOST_MIN, for good        */
#define TRAJ_FSM_D_BOOST_MIN    0.15
#define TRAJ_FSM_V_STALL        0.5    /* below it at a segment start: the stall override               */
#define TRAJ_FSM_STALL_D_LO     0.5
#define TRAJ_FSM_STALL_D_HI     1.0
#define TRAJ_FSM_STALL_SEG      0.3    /* the overridden segment lasts at least rint(0.3 / Ts) steps    */
#define TRAJ_FSM_SEG_LO         0.4    /* segment length, seconds: uniform(0.4, 1.5)                    */
#define TRAJ_FSM_SEG_HI         1.5
#define TRAJ_FSM_ACCEL_D_LO     0.3    /* accelerate: d = uniform(0.3, d_range[1])                      */
#define TRAJ_FSM_CRUISE_D_LO    (-0.05)
#define TRAJ_FSM_CRUISE_D_HI    0.2
#define TRAJ_FSM_TURN_FAST_D_LO 0.0    /* turn entered with v > v_turn_max                              */
#define TRAJ_FSM_TURN_FAST_D_HI 0.15
#define TRAJ_FSM_TURN_D_LO      0.05
#define TRAJ_FSM_TURN_D_HI      0.25
#define TRAJ_FSM_DELTA_CLIP     0.6

/* Mode codes of the mode[B,T] output. */
#define TRAJ_FSM_ACCELERATE 0
#define TRAJ_FSM_CRUISE     1
#define TRAJ_FSM_TURN_LEFT  2
#define TRAJ_FSM_TURN_RIGHT 3

/* ControlRules() of generation_type2.py:22-30 and the cdfs of its two choice calls.  TRAJ_E_ARG: null. */
int traj_gen_fsm_default_rules(traj_gen_fsm_rules* r);

/* B trajectories of T steps, one lane per trajectory, the whole walk in one launch.  Per trajectory:
 * sample_controls_piecewise(T, cfg->Ts, x0, params, rules) on the stream rng_state[b], its shadow state
 * being the trajectory itself: U[k] is the command of step k, X[k+1] = X[k] + Ts f2(X[k], U[k]) with the
 * state clip of cfg (vx_min, omega_max, as traj_gen_simulate_batch applies it), mode[k] the segment's
 * label after relabelling.  cfg->model must be TRAJ_GEN_MODEL_TYPE2; the limits of cfg (u_lo .. du_hi) are
 * not read: the controller has its own (d_range, TRAJ_FSM_DELTA_CLIP, TRAJ_FSM_DELTA_RATE_MAX).
 * rng_state_out (may be NULL): each stream's state after its last draw, in the layout of rng_state.
 * TRAJ_E_ARG: null pointer (data pointers only when B > 0), B < 0, T < 1, another model, Ts not finite or
 * not positive, a cdf that does not end at 1.0.  B == 0: TRAJ_OK, no launch.  Nothing outside X[B,T+1,6],
 * U[B,T,2], mode[B,T] and rng_state_out[B,4] is written. */
int traj_gen_piecewise_batch(const traj_vehicle_params* p, const traj_gen_config* cfg,
                             const traj_gen_fsm_rules* rules, int B, int T, const double* x0 /*[B,6]*/,
                             const unsigned long long* rng_state /*[B,4]*/, double* X /*[B,T+1,6]*/,
                             double* U /*[B,T,2]*/, unsigned char* mode /*[B,T]*/,
                             unsigned long long* rng_state_out /*[B,4] or NULL*/, void* stream);

/* For the tests of csrc/gen_rng.h and for nothing else: n draws of one kind from a stream.
 * kind: 0 raw 64-bit words (out is uint64), 1 doubles in [0, 1), 2 standard normals (out is double).
 * _host runs the header on the CPU (host pointers, synchronous); _batch runs it on the GPU, lane b drawing
 * out[b, 0..n) from states[b] (device pointers, asynchronous).  states_out may be NULL.
 * TRAJ_E_ARG: null state / out, n < 0, B < 0, unknown kind. */
#define TRAJ_RNG_RAW    0
#define TRAJ_RNG_DOUBLE 1
#define TRAJ_RNG_NORMAL 2
int traj_gen_rng_draw_host(const unsigned long long* state /*[4]*/, int kind, long long n, void* out /*[n]*/,
                           unsigned long long* state_out /*[4] or NULL*/);
int traj_gen_rng_draw_batch(int B, int n, int kind, const unsigned long long* states /*[B,4]*/,
                            void* out /*[B,n]*/, unsigned long long* states_out /*[B,4] or NULL*/,
                            void* stream);

/* ---- np.random.PCG64(entropy).state from the entropy (csrc/seed_seq.h: numpy's SeedSequence.generate_state(4, uint64)
 * and PCG64's seeding from those four words, in integer arithmetic: equal to numpy's or wrong) ----
 * entropy [B,nwords]: per stream the entropy as numpy coerces an int or a sequence of ints -- uint32 words,
 * little-endian, at least one word per int, a sequence's words concatenated (the caller's, i.e. Python's, job; numpy
 * refuses a negative int and so must the caller).  Every stream of a call has nwords words, 1 <= nwords <= 8; zero
 * words appended to a shorter entropy change nothing as long as nwords <= 4 (SeedSequence's pool size).
 * states [B,4]: the layout of traj_gen_piecewise_batch's rng_state.
 * _host: host pointers, synchronous.  _batch: device pointers, asynchronous on `stream`, one thread per stream.
 * TRAJ_E_ARG: null pointer (when B > 0), B < 0, nwords outside 1 .. 8.  B == 0: TRAJ_OK, no launch. */
int traj_gen_seed_pcg64_host(const uint32_t* entropy /*[B,nwords]*/, int B, int nwords,
                             unsigned long long* states /*[B,4]*/);
int traj_gen_seed_pcg64_batch(const uint32_t* entropy /*[B,nwords]*/, int B, int nwords,
                              unsigned long long* states /*[B,4]*/, void* stream);

/* ---- the closed loop's workload and its spline paths built on the device (csrc/workload.hip, csrc/spline.h) ----
 *
 * Natural cubic spline piece coefficients (batch.spline_natural's columns) of B trajectories, one lane per trajectory:
 * what PathSet.build computes in a Python loop.  kind [B] (traj_paths' codes: 2 = spline), nk [B] knots per trajectory,
 * xk / yk [B,kmax] knot abscissae / ordinates -> coef [B,kmax-1,4], flag [B].
 * A kind-2 row gets its nk - 1 pieces (second derivatives by the Thomas algorithm; nk = 2: the chord) and zeros after
 * them; a row of another kind is all zeros.  A kind-2 row with nk < 2, nk > kmax, knots that do not strictly increase
 * or a knot or ordinate that is not finite gets flag[b] = 1 and zeros; every other row flag[b] = 0.
 * _host: host pointers, synchronous, the same text on the CPU -- the same bits.  _batch: device pointers, asynchronous.
 * TRAJ_E_ARG: B < 1, kmax < 2, a null pointer. */
int traj_gen_spline_coef_host(int B, int kmax, const int* kind /*[B]*/, const int* nk /*[B]*/,
                              const double* xk /*[B,kmax]*/, const double* yk /*[B,kmax]*/,
                              double* coef /*[B,kmax-1,4]*/, int* flag /*[B]*/);
int traj_gen_spline_coef_batch(int B, int kmax, const int* kind /*[B]*/, const int* nk /*[B]*/,
                               const double* xk /*[B,kmax]*/, const double* yk /*[B,kmax]*/,
                               double* coef /*[B,kmax-1,4]*/, int* flag /*[B]*/, void* stream);

/* workload.make_workload's three kinds, and the spline kind's knot abscissae xk[i] = X0 + DX i (SPLINE_KNOTS_X). */
#define TRAJ_WORKLOAD_SPLINE   0
#define TRAJ_WORKLOAD_MIXED    1
#define TRAJ_WORKLOAD_PARABOLA 2
#define TRAJ_WORKLOAD_SPLINE_KNOTS 11
#define TRAJ_WORKLOAD_SPLINE_X0 (-6.0)
#define TRAJ_WORKLOAD_SPLINE_DX 4.0
#define TRAJ_WORKLOAD_MAX_SEED_WORDS 6   /* + tid's two = csrc/seed_seq.h's SEED_SEQ_MAX_WORDS */

/* make_workload's loop body for the trajectories tid = id_offset + b, b < B, one lane per trajectory: the stream
 * np.random.default_rng([seed, tid]) (entropy: seed_words[0 .. ns), the seed's uint32 words as numpy coerces it, little
 * end first and at least one -- a HOST pointer, read before the call returns -- followed by tid's one word, or two from
 * 2^32 on), its uniform draws in make_workload's order, the path they describe and the initial state on it:
 *   spline    11 knot ordinates in (-1, 1), kind 2, nk = 11, the coefficients as traj_gen_spline_coef_batch forms them
 *   mixed     even tid: A, w, phase -> kind 1, pc = (A, w, phase, 0);  odd tid: a -> kind 0, pc = (0, 0, a, 0)
 *   parabola  no draw: kind 0, pc = (0, 0, 0.1, 0), x0 = (0, 0.5, 0, 1, 0, 0) (MPC/main.py:77)
 *   x0        draws X, dY, dphi, vx, vy, omega: (X, y(X) + dY, atan(y'(X)) + dphi, vx, vy, omega), y and y' by the rule
 *             the closed loop applies to the row (path_eval)
 *   u0        ((Cr0 + Cr2 vx vx) / (Cm1 - Cm2 vx), 0)  (MPC/main.py:9-22)
 * Outputs: kind [B], pc [B,4], nk [B] (0 off the spline kind), xk / yk [B,kmax] and coef [B,kmax-1,4] (zeros past the
 * knots and off the spline kind), x0 [B,6], u0 [B,2]: traj_paths' arrays plus the closed loop's initial state.
 * _host: host pointers, synchronous, the same text on the CPU: the same bits except where libm enters (atan in phi;
 * sin / cos in a sinusoid row's Y and phi).  _batch: device pointers (but seed_words), asynchronous on `stream`.
 * TRAJ_E_ARG: a null pointer, an unknown workload, ns outside 1 .. TRAJ_WORKLOAD_MAX_SEED_WORDS, B < 1, id_offset < 0
 * or id_offset + B past 2^63 - 1, kmax < 2 (spline: < TRAJ_WORKLOAD_SPLINE_KNOTS). */
int traj_gen_workload_host(const traj_vehicle_params* p, int workload, const uint32_t* seed_words /*[ns]*/, int ns,
                           long long id_offset, int B, int kmax, int* kind /*[B]*/, double* pc /*[B,4]*/,
                           int* nk /*[B]*/, double* xk /*[B,kmax]*/, double* yk /*[B,kmax]*/,
                           double* coef /*[B,kmax-1,4]*/, double* x0 /*[B,6]*/, double* u0 /*[B,2]*/);
int traj_gen_workload_batch(const traj_vehicle_params* p, int workload, const uint32_t* seed_words /*[ns]*/, int ns,
                            long long id_offset, int B, int kmax, int* kind /*[B]*/, double* pc /*[B,4]*/,
                            int* nk /*[B]*/, double* xk /*[B,kmax]*/, double* yk /*[B,kmax]*/,
                            double* coef /*[B,kmax-1,4]*/, double* x0 /*[B,6]*/, double* u0 /*[B,2]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif

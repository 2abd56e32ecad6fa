/*
 * trajtrack.h -- C ABI of the MPC closed loop on closed tracks in libtrajmpc.so (gfx950).  Additive: the ABI version
 * of trajmpc.h stays 4.
 *
 * The reference paths of trajmpc.h are function graphs y(x): a vehicle always drives towards +x.  A track is a closed
 * parametric curve: a periodic C2 cubic spline P(s) = (X(s), Y(s)) through M knots, parametrised by cumulative chord
 * length s in [0, L).  The vehicle's place on it is found by projection, the MPC's window advances along it in s, and
 * the reference heading is unwound onto the vehicle's own branch, so a run may go round the track any number of times.
 * The rules (csrc/track.h holds them, one text for host and device):
 *
 *   wrap      wrap(s) = s - L floor(s / L); a result that rounds to L, or below 0, becomes 0
 *   project   candidates c(i, j) = sig[i] + (sig[i+1] - sig[i]) j / samples, i = 0 .. M-1, j = 0 .. samples-1.
 *             Local search (s_prev not NaN): the candidates whose signed cyclic offset wrap(c - s_prev + L/2) - L/2
 *             lies in [-back, fwd]; global search (all candidates) with a NaN s_prev and when no local candidate wins.
 *             The smallest (Px - X)^2 + (Py - Y)^2 wins, the lowest (i, j) on a tie; a distance that is not finite
 *             never wins, and with no winner the choice is (0, 0).  Then `newton` iterations (a fixed count) on
 *             g = (P - p) . P' with g' = P' . P' + (P - p) . P'': while g' > 0, s <- wrap(s - clamp(g / g', +-h)), h the
 *             chosen piece's candidate spacing; otherwise stop (a step that is NaN stops too: a point that is not
 *             finite still gets a place in [0, L)).
 *   window    s_0 = the projection, s_{k+1} = s_k + vref_k Ts / |P'(s_k)|; (X*_k, Y*_k) = P(wrap(s_k));
 *             a_k = atan2(Y', X');  n_0 = rint((phi - a_0) / 2 pi) (0 without a heading),
 *             n_k = n_{k-1} - rint((a_k - a_{k-1}) / 2 pi),  phi*_k = a_k + 2 pi n_k.
 *
 * One closed-loop step t, as a launch sequence on the caller's stream (no synchronisation, no allocation: a whole run
 * can be captured in a HIP graph, as a linear chain):
 *   1. the track kernel: s[b] <- project((X, Y) of x[b], s[b]); the window path_ref [B,N+1,3] and this step's
 *      contiguous slice vref [B,N+1] of the speed schedule into the workspace
 *   2. traj_mpc_step_batch on (x, u_prev, path_ref, vref), unchanged: every solver tier, state bounds and every
 *      setting are that entry point's; rho starts cold at each step.  It leaves u_cmd = u_prev and its status for an
 *      instance that did not solve.
 *   3. the plant kernel: x <- x + Ts f_cont(x, u_cmd) (the closed loop's plant update, the same expressions),
 *      u_prev <- u_cmd, and the rows hist_x[b,t+1,:] = x, hist_u[b,t,:] = u_cmd, hist_s[b,t] = s[b], each optional
 *
 * Conventions as trajmpc.h: device pointers (except the two _host functions'), row-major float64, asynchronous on
 * `stream`, 0 / TRAJ_E_*, TRAJ_E_ARG before any launch, B == 0: TRAJ_OK and no launch.
 */
#ifndef TRAJTRACK_H
#define TRAJTRACK_H

#include "trajmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tracks are shared: a few circuits, thousands of cars.  Track i has nk[i] knots (3 <= nk[i] <= kmax; the device
 * cannot refuse a bad count, so it reads nk clamped to 1 .. kmax and track_of clamped to 0 .. n_tracks - 1, and the
 * builder, TrackSet.build, refuses M < 3), parameters sig[i, 0 .. nk[i]] (sig[i,0] = 0, sig[i,nk[i]] = L_i) and piece
 * coefficients coef[i, j, c, 0..3], c = 0 for X and 1 for Y: c0 + t (c1 + t (c2 + t c3)), t = s - sig[i,j]. */
typedef struct {
    int n_tracks;             /* >= 1 */
    int kmax;                 /* knot capacity per track, >= 3 */
    const int* nk;            /* [n_tracks] */
    const double* sig;        /* [n_tracks, kmax + 1] */
    const double* coef;       /* [n_tracks, kmax, 2, 4] */
    const int* track_of;      /* [B]: trajectory b's track, or NULL: track 0 for all */
} traj_tracks;

/* The projection's search.  Accepted: 1 <= samples <= TRAJ_TRACK_MAX_SAMPLES, newton >= 0, back >= 0, fwd >= 0 (NaN
 * is refused); anything else is TRAJ_E_ARG. */
#define TRAJ_TRACK_MAX_SAMPLES 4096
typedef struct {
    int samples;              /* candidates per piece (default 8) */
    double back, fwd;         /* the local search's reach behind / ahead of s_prev, metres (defaults 0.5, 1.0) */
    int newton;               /* refinement iterations (default 8) */
} traj_track_search;
int traj_track_default_search(traj_track_search* search);

/* project: point b is (xy[xy_stride b], xy[xy_stride b + 1]) (xy_stride in doubles, >= 2: 6 for state rows); s_prev
 * [B] or NULL (NaN entries, or NULL: global search).  Outputs s [B] and, if non-NULL, dist2 [B], the squared distance
 * to P(s).  s may alias s_prev.
 * TRAJ_E_ARG: a null tracks / search, their rules above, B < 0, xy_stride < 2; with B > 0 a null xy or s. */
int traj_track_project_batch(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                             long long xy_stride, const double* s_prev, double* s, double* dist2, void* stream);

/* window: path_ref [B,N+1,3] from s0 [B] (each in [0, L)) and the vehicle headings phi [B] (NULL: n_0 = 0), with the
 * speeds vref_k = vref[vref_row b + vref_off + k], k = 0 .. N (vref_row in doubles; 0 = one row shared by all).
 * TRAJ_E_ARG: a null tracks, its rules, B < 0, N < 1, Ts not > 0, vref_len < N + 1, vref_row neither 0 nor >=
 * vref_len, vref_off < 0 or vref_off + N >= vref_len; with B > 0 a null s0, vref or path_ref. */
int traj_track_window_batch(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* phi,
                            const double* vref, long long vref_row, int vref_len, long long vref_off,
                            double* path_ref, void* stream);

/* The same two functions on HOST pointers (the tracks' arrays too), synchronous: csrc/track.h compiled for the host,
 * so the rules can be tested without a GPU.  They differ from the device's by atan2 alone (the host libm's against
 * the device library's).  On the host a knot count outside 3 .. kmax or a track_of entry outside 0 .. n_tracks - 1 is
 * TRAJ_E_ARG. */
int traj_track_project_host(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                            long long xy_stride, const double* s_prev, double* s, double* dist2);
int traj_track_window_host(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* phi,
                           const double* vref, long long vref_row, int vref_len, long long vref_off, double* path_ref);

/* Workspace of the closed loop on tracks: traj_mpc_step_workspace_bytes(c, B) rounded up to 8, plus the window
 * [B,N+1,3], the vref slice [B,N+1], u_cmd [B,2] and a status row [B]; 0 for a null or invalid configuration or
 * B < 0. */
size_t traj_closed_loop_track_workspace_bytes(const traj_mpc_config* c, int B);

/* One step (above), in place on x [B,6], u_prev [B,2] and s [B] (in: the previous step's parameter, NaN = global
 * search; out: this step's).  vref, vref_row, vref_len, vref_step: the speed schedule of traj_closed_loop_step_sched
 * ((N + 1, N + 1, 0): the same vref [B,N+1] at every step).  hist_x [B,hist_T+1,6], hist_u [B,hist_T,2], hist_s
 * [B,hist_T], each or NULL.  status / iters [B] (optional): this step's solver outcome.
 * TRAJ_E_ARG, before any launch: a null p, c, tracks or search; their rules; B < 0; an invalid configuration or
 * schedule (traj_closed_loop_step_sched's rules); and with B > 0: a null x, u_prev, s, vref or workspace, a workspace
 * below traj_closed_loop_track_workspace_bytes, t outside 0 .. hist_T - 1 with a history, t < 0 with vref_step = 1. */
int traj_closed_loop_track_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
                                const traj_track_search* search, int B, double* x, double* u_prev, double* s,
                                const double* vref, long long vref_row, int vref_len, int vref_step, int t, int hist_T,
                                double* hist_x, double* hist_u, double* hist_s, int* status, int* iters,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Steps t0 .. t0 + steps - 1, in order on the stream: exactly that many traj_closed_loop_track_step calls.  status /
 * iters (optional) are [steps, B].  TRAJ_E_ARG as above, for every step of the call and before the first launch
 * (steps < 0, t0 < 0, t0 + steps > hist_T with a history, the last step's window past the schedule); steps == 0:
 * TRAJ_OK, no launch. */
int traj_closed_loop_track_run(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
                               const traj_track_search* search, int B, double* x, double* u_prev, double* s,
                               const double* vref, long long vref_row, int vref_len, int vref_step, int t0, int steps,
                               int hist_T, double* hist_x, double* hist_u, double* hist_s, int* status, int* iters,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Launch 1 alone -- the track kernel as the step launches it: s [B] in / out, path_ref [B,N+1,3] and vref_out [B,N+1]
 * (the N + 1 speeds from vref[vref_row b + vref_off]) from the states x [B,6] (X, Y and the heading phi).  TRAJ_E_ARG:
 * traj_track_project_batch's and traj_track_window_batch's rules; with B > 0 a null x, s, vref, path_ref or vref_out. */
int traj_closed_loop_track_window(const traj_tracks* tracks, const traj_track_search* search, int B, int N, double Ts,
                                  const double* x, double* s, const double* vref, long long vref_row, int vref_len,
                                  long long vref_off, double* path_ref, double* vref_out, void* stream);

/* Launch 3 alone -- the plant update and the history rows for the commands u_cmd [B,2] (s [B] is read for hist_s
 * only, NULL without it).  traj_closed_loop_track_step ends with exactly this launch.  TRAJ_E_ARG: a null p, Ts not
 * > 0, B < 0; with B > 0 a null x, u_prev or u_cmd, hist_s without s, t outside 0 .. hist_T - 1 with a history. */
int traj_closed_loop_track_plant(const traj_vehicle_params* p, double Ts, int B, double* x, double* u_prev,
                                 const double* u_cmd, const double* s, int t, int hist_T, double* hist_x,
                                 double* hist_u, double* hist_s, void* stream);

/* Tracking errors of finished histories, one thread per (b, t): with the track point and raw heading a at
 * hist_s[b,t], err[b,t,0] = e_c = sin(a)(X - X*) - cos(a)(Y - Y*) (lateral_error's formula, mpc_6stati.py:111-117) and
 * err[b,t,1] = e_phi = atan2(sin(phi - a), cos(phi - a)).  hist_x [B,T1,6], hist_s [B,T1] (wrapped on the way in),
 * err [B,T1,2].  TRAJ_E_ARG: a null tracks, its rules, B < 0, T1 < 1; with B > 0 a null hist_x, hist_s or err. */
int traj_track_errors_batch(const traj_tracks* tracks, int B, int T1, const double* hist_x, const double* hist_s,
                            double* err, void* stream);

/* The track kernel's form: 1 = one thread per trajectory; 16 = sixteen lanes per trajectory, four trajectories per
 * wave (the candidates spread over the lanes and joined by a shuffle argmin with the tie rule; the serial s chain
 * redundant on all lanes; the N + 1 evaluations, atan2s and output rows spread over the lanes; the windings an integer
 * scan).  The same bits either way.  Returns TRAJ_E_ARG for any other value.  For tests and measurements. */
#define TRAJ_TRACK_DEFAULT_LANES 16
int traj_debug_track_lanes(int lanes);

#ifdef __cplusplus
}
#endif

#endif /* TRAJTRACK_H */

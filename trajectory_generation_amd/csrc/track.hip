// track.hip -- the MPC closed loop on closed tracks (include/trajtrack.h): per step the track kernel (projection, window
// and the step's vref slice into the workspace), traj_mpc_step_batch on them (every solver tier is that entry point's,
// untouched) and the plant kernel (plant update, u_prev, the history rows).  The geometry is csrc/track.h, one text for
// the kernels here and the _host entry points.
//
// The track kernel has two forms that give the same bits (-ffp-contract=off: the same expressions, the same roundings;
// every choice in track.h is made on exact quantities):
//   scalar      one thread per trajectory: trk_project and trk_window as the host runs them -- the anchor;
//   lane group  16 lanes per trajectory and 4 trajectories per wave: candidate e on lane e % 16, the winner by a
//               shuffle butterfly over trk_better (a total order: the tie rule holds in any partition); the Newton
//               chain and the s chain redundant on all 16 lanes; stage k's evaluation, atan2 and output row on lane
//               k % 16; the windings by an integer scan over the lanes.  No LDS, no barrier: a group past the batch
//               simply leaves.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/trajtrack.h"
#include "mpc_host.h"   // launched, nblk
#include "physics.h"

#define TRK_DEVICE_ATAN2(y, x) tgmpc::pm_atan2(y, x)
#include "track.h"

namespace {

using namespace tgtrack;
using tgmpc::VP, tgmpc::launched, tgmpc::nblk;

struct TrackArgs {
    // the tracks
    int n_tracks, kmax;
    const int* nk;
    const double* sig;
    const double* coef;
    const int* track_of;
    Search se;
    int B, N;
    double Ts;
    // projection (xy != NULL): point b at xy[xy_stride b], s_prev [B] or NULL -> s_out [B], d2 [B] or NULL
    const double* xy;
    long long xy_stride;
    const double* s_prev;
    double* s_out;
    double* d2;
    // window (pref != NULL): from the projection, or from s0 [B] without one; phi[phi_stride b] or NULL; vref row b at
    // vref + vrow b + voff; vr_out [B,N+1] or NULL: the row's N + 1 entries copied
    const double* s0;
    const double* phi;
    long long phi_stride;
    const double* vref;
    long long vrow, voff;
    double* pref;
    double* vr_out;
};

__host__ __device__ inline Track track_of(const TrackArgs& a, int b) {
    int i = a.track_of ? a.track_of[b] : 0;
    i = i < 0 ? 0 : (i >= a.n_tracks ? a.n_tracks - 1 : i);
    int M = a.nk[i];
    M = M < 1 ? 1 : (M > a.kmax ? a.kmax : M);
    Track tr;
    tr.M = M;
    tr.sig = a.sig + (size_t)i * (a.kmax + 1);
    tr.coef = a.coef + (size_t)i * a.kmax * 8;
    tr.L = tr.sig[M];
    return tr;
}

// one trajectory, serially: the scalar kernel's thread and the host entry points' loop body
__host__ __device__ inline void track_one(const TrackArgs& a, int b) {
    const Track tr = track_of(a, b);
    double s;
    if (a.xy) {
        const double* p = a.xy + (size_t)a.xy_stride * b;
        s = trk_project(tr, a.se, p[0], p[1], a.s_prev ? a.s_prev[b] : trk_nan());
        a.s_out[b] = s;
        if (a.d2) a.d2[b] = trk_dist2(tr, s, p[0], p[1]);
    } else {
        s = a.s0[b];
    }
    if (!a.pref) return;
    const double* vr = a.vref + (size_t)a.vrow * b + (size_t)a.voff;
    trk_window(tr, s, a.phi != nullptr, a.phi ? a.phi[(size_t)a.phi_stride * b] : 0.0, vr, a.N, a.Ts,
               a.pref + (size_t)b * (a.N + 1) * 3);
    if (a.vr_out)
        for (int k = 0; k <= a.N; ++k) a.vr_out[(size_t)b * (a.N + 1) + k] = vr[k];
}

__global__ __launch_bounds__(64) void track_kernel(const TrackArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    track_one(a, b);
}

// ---- the lane-group form ----
constexpr int GROUP_LANES = 16, GROUPS = 4;   // one wave per workgroup

__device__ __forceinline__ int group_scan_incl(int v, int g) {   // inclusive sum over the 16 lanes of a group
#pragma unroll
    for (int o = 1; o < GROUP_LANES; o <<= 1) {
        const int up = __shfl_up(v, o, GROUP_LANES);
        if (g >= o) v += up;
    }
    return v;
}

__global__ __launch_bounds__(GROUP_LANES * GROUPS) void track_group_kernel(const TrackArgs a) {
    const int g = threadIdx.x % GROUP_LANES, grp = threadIdx.x / GROUP_LANES;
    const int b = blockIdx.x * GROUPS + grp;
    if (b >= a.B) return;   // (the whole group: its shuffles stay among its own 16 lanes)
    const Track tr = track_of(a, b);
    double s;
    if (a.xy) {
        const double* p = a.xy + (size_t)a.xy_stride * b;
        const double px = p[0], py = p[1];
        const double s_prev = a.s_prev ? a.s_prev[b] : trk_nan();
        const bool local = s_prev == s_prev;
        double dl = HUGE_VAL, dg = HUGE_VAL;
        int el = TRK_NONE, eg = TRK_NONE;
        const int n = tr.M * a.se.samples;
        for (int e = g; e < n; e += GROUP_LANES) trk_score(tr, a.se, px, py, s_prev, local, e, dl, el, dg, eg);
#pragma unroll
        for (int o = GROUP_LANES / 2; o >= 1; o >>= 1) {
            const double odl = __shfl_xor(dl, o, GROUP_LANES), odg = __shfl_xor(dg, o, GROUP_LANES);
            const int oel = __shfl_xor(el, o, GROUP_LANES), oeg = __shfl_xor(eg, o, GROUP_LANES);
            if (trk_better(odl, oel, dl, el)) {
                dl = odl;
                el = oel;
            }
            if (trk_better(odg, oeg, dg, eg)) {
                dg = odg;
                eg = oeg;
            }
        }
        s = trk_refine(tr, a.se, px, py, trk_choice(el, eg));
        if (g == 0) {
            a.s_out[b] = s;
            if (a.d2) a.d2[b] = trk_dist2(tr, s, px, py);
        }
    } else {
        s = a.s0[b];
    }
    if (!a.pref) return;
    const int N = a.N;
    const double* vr = a.vref + (size_t)a.vrow * b + (size_t)a.voff;
    double* pref = a.pref + (size_t)b * (N + 1) * 3;
    const bool has_phi = a.phi != nullptr;
    const double phi = has_phi ? a.phi[(size_t)a.phi_stride * b] : 0.0;
    // stages k0 .. k0 + 15 per pass: the chain walked by every lane, lane g keeping stage k0 + g's s
    double a_carry = 0.0;   // a of stage k0 - 1
    int n_carry = 0;        // n of stage k0 - 1 (pass 0: n_0 itself, set below)
    for (int k0 = 0; k0 <= N; k0 += GROUP_LANES) {
        double mine = s;
        for (int j = 0; j < GROUP_LANES; ++j) {
            if (j == g) mine = s;
            if (k0 + j < N) s = trk_advance(tr, s, vr[k0 + j] * a.Ts);   // (uniform over the group)
        }
        const int k = k0 + g;
        const bool live = k <= N;
        double X = 0.0, Y = 0.0, ak = 0.0, sn;
        if (live) trk_stage(tr, mine, 0.0, X, Y, ak, sn);
        double a_prev = __shfl_up(ak, 1, GROUP_LANES);
        if (g == 0) a_prev = a_carry;
        // this stage's turn; stage 0 carries -n_0, so that n_k = -(the inclusive sum) + carry throughout
        int turn = live ? (k == 0 ? -trk_wind0(has_phi, phi, ak) : trk_turn(ak, a_prev)) : 0;
        const int n = n_carry - group_scan_incl(turn, g);
        if (live) {
            pref[3 * k] = X;
            pref[3 * k + 1] = Y;
            pref[3 * k + 2] = trk_heading(ak, n);
            if (a.vr_out) a.vr_out[(size_t)b * (N + 1) + k] = vr[k];
        }
        a_carry = __shfl(ak, GROUP_LANES - 1, GROUP_LANES);
        n_carry = __shfl(n, GROUP_LANES - 1, GROUP_LANES);
    }
}

// ---- the plant kernel: plant_update / plant_publish of mpc_frame.h (f_cont on the state, xs[i] + Ts * f[i]) ----
struct PlantArgs {
    VP p;
    double Ts;
    int B, t, hist_T;
    double* x;
    double* u_prev;
    const double* u_cmd;
    const double* s;
    double* hist_x;
    double* hist_u;
    double* hist_s;
};

__global__ __launch_bounds__(64) void track_plant_kernel(const PlantArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    double xs[6], f[6], u[2] = {a.u_cmd[2 * (size_t)b], a.u_cmd[2 * (size_t)b + 1]};
    for (int i = 0; i < 6; ++i) xs[i] = a.x[6 * (size_t)b + i];
    tgmpc::f_cont(a.p, xs, u, f);
    for (int i = 0; i < 6; ++i) {
        const double xn = xs[i] + a.Ts * f[i];
        a.x[6 * (size_t)b + i] = xn;
        if (a.hist_x) a.hist_x[((size_t)b * (a.hist_T + 1) + a.t + 1) * 6 + i] = xn;
    }
    a.u_prev[2 * (size_t)b] = u[0];
    a.u_prev[2 * (size_t)b + 1] = u[1];
    const size_t row = (size_t)b * a.hist_T + a.t;
    if (a.hist_u) {
        a.hist_u[row * 2] = u[0];
        a.hist_u[row * 2 + 1] = u[1];
    }
    if (a.hist_s) a.hist_s[row] = a.s[b];
}

// ---- tracking errors, one thread per (b, t) ----
__global__ __launch_bounds__(256) void track_errors_kernel(const TrackArgs a, int T1, const double* hist_x,
                                                           const double* hist_s, double* err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.B * T1) return;
    const int b = (int)(i / T1);
    const Track tr = track_of(a, b);
    const double* x = hist_x + 6 * (size_t)i;
    const Point q = trk_eval(tr, trk_wrap(hist_s[i], tr.L));
    const double ang = tgmpc::pm_atan2(q.dY, q.dX);
    err[2 * (size_t)i] = tgmpc::lateral_error(x[0], x[1], q.X, q.Y, ang);
    double se, ce;
    tgmpc::pm_sincos(x[2] - ang, &se, &ce);
    err[2 * (size_t)i + 1] = tgmpc::pm_atan2(se, ce);
}

std::atomic<int> g_track_lanes{TRAJ_TRACK_DEFAULT_LANES};

bool tracks_ok(const traj_tracks* t) {
    return t && t->n_tracks >= 1 && t->kmax >= 3 && t->nk && t->sig && t->coef;
}
bool search_ok(const traj_track_search* s) {
    return s && s->samples >= 1 && s->samples <= TRAJ_TRACK_MAX_SAMPLES && s->newton >= 0 && s->back >= 0.0 &&
           s->fwd >= 0.0;   // (NaN fails the comparisons)
}
// a speed row read at vref_off .. vref_off + N
bool vrow_ok(int N, long long vref_row, int vref_len, long long vref_off) {
    if (vref_len < N + 1) return false;
    if (vref_row != 0 && vref_row < vref_len) return false;
    return vref_off >= 0 && vref_off + N < (long long)vref_len;
}
// the _sched entry points' schedule rules; `last` = the step whose window reaches furthest
bool sched_ok(int N, long long vref_row, int vref_len, int vref_step, long long last) {
    if (vref_step != 0 && vref_step != 1) return false;
    if (vref_len < N + 1) return false;
    if (vref_row != 0 && vref_row < vref_len) return false;
    return last < 0 || last * vref_step + N < (long long)vref_len;
}

TrackArgs track_args(const traj_tracks* t, const traj_track_search* s, int B) {
    TrackArgs a{};
    a.n_tracks = t->n_tracks;
    a.kmax = t->kmax;
    a.nk = t->nk;
    a.sig = t->sig;
    a.coef = t->coef;
    a.track_of = t->track_of;
    if (s) a.se = Search{s->samples, s->back, s->fwd, s->newton};
    a.B = B;
    return a;
}

int launch_track(const TrackArgs& a, hipStream_t st) {
    if (g_track_lanes.load(std::memory_order_relaxed) == GROUP_LANES)
        hipLaunchKernelGGL(track_group_kernel, dim3(nblk(a.B, GROUPS)), dim3(GROUP_LANES * GROUPS), 0, st, a);
    else
        hipLaunchKernelGGL(track_kernel, dim3(nblk(a.B, 64)), dim3(64), 0, st, a);
    return launched();
}

// host: the tracks' arrays can be read, so a bad count or index is refused
bool tracks_host_ok(const traj_tracks* t, int B) {
    for (int i = 0; i < t->n_tracks; ++i)
        if (t->nk[i] < 3 || t->nk[i] > t->kmax) return false;
    if (t->track_of)
        for (int b = 0; b < B; ++b)
            if (t->track_of[b] < 0 || t->track_of[b] >= t->n_tracks) return false;
    return true;
}

inline size_t step_bytes8(const traj_mpc_config* c, int B) {
    return (traj_mpc_step_workspace_bytes(c, B) + 7) & ~(size_t)7;
}

// what the loop's entry points refuse before any launch, for the steps t0 .. t0 + steps - 1 (steps >= 1)
int loop_check(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
               const traj_track_search* search, int B, const double* x, const double* u_prev, const double* s,
               const double* vref, long long vref_row, int vref_len, int vref_step, int t0, int steps, int hist_T,
               bool hist, const void* workspace, size_t workspace_bytes) {
    if (!p || !c || B < 0 || !tracks_ok(tracks) || !search_ok(search)) return TRAJ_E_ARG;
    // the configuration by the step entry point's own rules: its B = 0 call checks it and launches nothing
    const int e = traj_mpc_step_batch(p, c, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    if (e) return e;
    if (!sched_ok(c->N, vref_row, vref_len, vref_step, (long long)t0 + steps - 1)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x || !u_prev || !s || !vref) return TRAJ_E_ARG;
    if (!workspace || workspace_bytes < traj_closed_loop_track_workspace_bytes(c, B)) return TRAJ_E_ARG;
    if (hist && (t0 < 0 || t0 + steps > hist_T)) return TRAJ_E_ARG;
    if (vref_step && t0 < 0) return TRAJ_E_ARG;
    return TRAJ_OK;
}

int launch_plant(const PlantArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(track_plant_kernel, dim3(nblk(a.B, 64)), dim3(64), 0, st, a);
    return launched();
}

// launch 1's arguments: projection from the states' (X, Y) and s, window from their phi, the vref slice
TrackArgs step_track_args(const traj_tracks* tracks, const traj_track_search* search, int B, int N, double Ts,
                          const double* x, double* s, const double* vref, long long vref_row, long long vref_off,
                          double* pref, double* vr_out) {
    TrackArgs a = track_args(tracks, search, B);
    a.N = N;
    a.Ts = Ts;
    a.xy = x;
    a.xy_stride = 6;
    a.s_prev = s;
    a.s_out = s;
    a.phi = x + 2;
    a.phi_stride = 6;
    a.vref = vref;
    a.vrow = vref_row;
    a.voff = vref_off;
    a.pref = pref;
    a.vr_out = vr_out;
    return a;
}

// one step's launches (arguments checked)
int loop_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
              const traj_track_search* search, int B, double* x, double* u_prev, double* s, const double* vref,
              long long vref_row, int vref_step, int t, int hist_T, double* hist_x, double* hist_u, double* hist_s,
              int* status, int* iters, void* workspace, hipStream_t st) {
    const int N = c->N;
    const size_t step = step_bytes8(c, B);
    double* const pref = (double*)((char*)workspace + step);
    double* const vr = pref + (size_t)B * (N + 1) * 3;
    double* const uc = vr + (size_t)B * (N + 1);
    int* const sbuf = (int*)(uc + (size_t)B * 2);
    if (const int e = launch_track(step_track_args(tracks, search, B, N, c->Ts, x, s, vref, vref_row,
                                                   (long long)vref_step * t, pref, vr), st))
        return e;
    const int e = traj_mpc_step_batch(p, c, B, x, u_prev, pref, vr, uc, status ? status : sbuf, nullptr, nullptr,
                                      nullptr, iters, nullptr, workspace, step, st);
    if (e) return e;
    PlantArgs q{*p, c->Ts, B, t, hist_T, x, u_prev, uc, s, hist_x, hist_u, hist_s};
    return launch_plant(q, st);
}

}  // namespace

extern "C" {

int traj_track_default_search(traj_track_search* search) {
    if (!search) return TRAJ_E_ARG;
    *search = traj_track_search{8, 0.5, 1.0, 8};
    return TRAJ_OK;
}

static int project_check(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                         long long xy_stride, const double* s) {
    if (!tracks_ok(tracks) || !search_ok(search) || B < 0 || xy_stride < 2) return TRAJ_E_ARG;
    if (B > 0 && (!xy || !s)) return TRAJ_E_ARG;
    return TRAJ_OK;
}
static TrackArgs project_args(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                              long long xy_stride, const double* s_prev, double* s, double* dist2) {
    TrackArgs a = track_args(tracks, search, B);
    a.xy = xy;
    a.xy_stride = xy_stride;
    a.s_prev = s_prev;
    a.s_out = s;
    a.d2 = dist2;
    return a;
}

static int window_check(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* vref,
                        long long vref_row, int vref_len, long long vref_off, const double* path_ref) {
    if (!tracks_ok(tracks) || B < 0 || N < 1 || !(Ts > 0.0) || !vrow_ok(N, vref_row, vref_len, vref_off))
        return TRAJ_E_ARG;
    if (B > 0 && (!s0 || !vref || !path_ref)) return TRAJ_E_ARG;
    return TRAJ_OK;
}
static TrackArgs window_args(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* phi,
                             const double* vref, long long vref_row, long long vref_off, double* path_ref) {
    TrackArgs a = track_args(tracks, nullptr, B);
    a.N = N;
    a.Ts = Ts;
    a.s0 = s0;
    a.phi = phi;
    a.phi_stride = 1;
    a.vref = vref;
    a.vrow = vref_row;
    a.voff = vref_off;
    a.pref = path_ref;
    return a;
}

int traj_track_project_batch(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                             long long xy_stride, const double* s_prev, double* s, double* dist2, void* stream) {
    const int e = project_check(tracks, search, B, xy, xy_stride, s);
    if (e || B == 0) return e;
    return launch_track(project_args(tracks, search, B, xy, xy_stride, s_prev, s, dist2), (hipStream_t)stream);
}

int traj_track_window_batch(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* phi,
                            const double* vref, long long vref_row, int vref_len, long long vref_off,
                            double* path_ref, void* stream) {
    const int e = window_check(tracks, B, N, Ts, s0, vref, vref_row, vref_len, vref_off, path_ref);
    if (e || B == 0) return e;
    return launch_track(window_args(tracks, B, N, Ts, s0, phi, vref, vref_row, vref_off, path_ref),
                        (hipStream_t)stream);
}

int traj_track_project_host(const traj_tracks* tracks, const traj_track_search* search, int B, const double* xy,
                            long long xy_stride, const double* s_prev, double* s, double* dist2) {
    const int e = project_check(tracks, search, B, xy, xy_stride, s);
    if (e) return e;
    if (!tracks_host_ok(tracks, B)) return TRAJ_E_ARG;
    const TrackArgs a = project_args(tracks, search, B, xy, xy_stride, s_prev, s, dist2);
    for (int b = 0; b < B; ++b) track_one(a, b);
    return TRAJ_OK;
}

int traj_track_window_host(const traj_tracks* tracks, int B, int N, double Ts, const double* s0, const double* phi,
                           const double* vref, long long vref_row, int vref_len, long long vref_off,
                           double* path_ref) {
    const int e = window_check(tracks, B, N, Ts, s0, vref, vref_row, vref_len, vref_off, path_ref);
    if (e) return e;
    if (!tracks_host_ok(tracks, B)) return TRAJ_E_ARG;
    const TrackArgs a = window_args(tracks, B, N, Ts, s0, phi, vref, vref_row, vref_off, path_ref);
    for (int b = 0; b < B; ++b) track_one(a, b);
    return TRAJ_OK;
}

size_t traj_closed_loop_track_workspace_bytes(const traj_mpc_config* c, int B) {
    if (!c || B < 0) return 0;
    const size_t step = traj_mpc_step_workspace_bytes(c, B);
    if (step == 0) return 0;
    return ((step + 7) & ~(size_t)7) + ((size_t)B * (c->N + 1) * 4 + (size_t)B * 2) * sizeof(double) +
           (((size_t)B * sizeof(int) + 7) & ~(size_t)7);
}

int traj_closed_loop_track_step(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
                                const traj_track_search* search, int B, double* x, double* u_prev, double* s,
                                const double* vref, long long vref_row, int vref_len, int vref_step, int t, int hist_T,
                                double* hist_x, double* hist_u, double* hist_s, int* status, int* iters,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const bool hist = hist_x || hist_u || hist_s;
    const int e = loop_check(p, c, tracks, search, B, x, u_prev, s, vref, vref_row, vref_len, vref_step, t, 1, hist_T,
                             hist, workspace, workspace_bytes);
    if (e || B == 0) return e;
    return loop_step(p, c, tracks, search, B, x, u_prev, s, vref, vref_row, vref_step, t, hist_T, hist_x, hist_u,
                     hist_s, status, iters, workspace, (hipStream_t)stream);
}

int traj_closed_loop_track_run(const traj_vehicle_params* p, const traj_mpc_config* c, const traj_tracks* tracks,
                               const traj_track_search* search, int B, double* x, double* u_prev, double* s,
                               const double* vref, long long vref_row, int vref_len, int vref_step, int t0, int steps,
                               int hist_T, double* hist_x, double* hist_u, double* hist_s, int* status, int* iters,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (steps < 0) return TRAJ_E_ARG;
    const bool hist = hist_x || hist_u || hist_s;
    // (steps == 0: the checks of a one-step call that reads nothing of the schedule or the histories)
    const int e = steps > 0 ? loop_check(p, c, tracks, search, B, x, u_prev, s, vref, vref_row, vref_len, vref_step, t0,
                                         steps, hist_T, hist, workspace, workspace_bytes)
                            : loop_check(p, c, tracks, search, 0, nullptr, nullptr, nullptr, nullptr, vref_row, vref_len,
                                         vref_step, 0, 1, 1, false, nullptr, 0);
    if (e || B == 0 || steps == 0) return e;
    if (t0 < 0) return TRAJ_E_ARG;
    for (int k = 0; k < steps; ++k) {
        const int es = loop_step(p, c, tracks, search, B, x, u_prev, s, vref, vref_row, vref_step, t0 + k, hist_T,
                                 hist_x, hist_u, hist_s, status ? status + (size_t)k * B : nullptr,
                                 iters ? iters + (size_t)k * B : nullptr, workspace, (hipStream_t)stream);
        if (es) return es;
    }
    return TRAJ_OK;
}

int traj_closed_loop_track_window(const traj_tracks* tracks, const traj_track_search* search, int B, int N, double Ts,
                                  const double* x, double* s, const double* vref, long long vref_row, int vref_len,
                                  long long vref_off, double* path_ref, double* vref_out, void* stream) {
    if (const int e = project_check(tracks, search, B, x, 6, s)) return e;
    if (const int e = window_check(tracks, B, N, Ts, s, vref, vref_row, vref_len, vref_off, path_ref)) return e;
    if (B == 0) return TRAJ_OK;
    if (!vref_out) return TRAJ_E_ARG;
    return launch_track(step_track_args(tracks, search, B, N, Ts, x, s, vref, vref_row, vref_off, path_ref, vref_out),
                        (hipStream_t)stream);
}

int traj_closed_loop_track_plant(const traj_vehicle_params* p, double Ts, int B, double* x, double* u_prev,
                                 const double* u_cmd, const double* s, int t, int hist_T, double* hist_x,
                                 double* hist_u, double* hist_s, void* stream) {
    if (!p || !(Ts > 0.0) || B < 0) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x || !u_prev || !u_cmd || (hist_s && !s)) return TRAJ_E_ARG;
    if ((hist_x || hist_u || hist_s) && (t < 0 || t >= hist_T)) return TRAJ_E_ARG;
    PlantArgs q{*p, Ts, B, t, hist_T, x, u_prev, u_cmd, s, hist_x, hist_u, hist_s};
    return launch_plant(q, (hipStream_t)stream);
}

int traj_track_errors_batch(const traj_tracks* tracks, int B, int T1, const double* hist_x, const double* hist_s,
                            double* err, void* stream) {
    if (!tracks_ok(tracks) || B < 0 || T1 < 1) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!hist_x || !hist_s || !err) return TRAJ_E_ARG;
    const TrackArgs a = track_args(tracks, nullptr, B);
    hipLaunchKernelGGL(track_errors_kernel, dim3((unsigned)(((long long)B * T1 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a, T1, hist_x, hist_s, err);
    return launched();
}

int traj_debug_track_lanes(int lanes) {
    if (lanes != 1 && lanes != GROUP_LANES) return TRAJ_E_ARG;
    g_track_lanes.store(lanes, std::memory_order_relaxed);
    return TRAJ_OK;
}

}  // extern "C"

// closed_stats.hip -- the evaluation that follows the closed loop (MPC/main.py:107-121), on finished histories.
//
//   traj_closed_loop_stats        per trajectory, seven series over steps t = 0 .. T-1, each as the record
//                                 (n, mean, M2 = sum of squared deviations, min, max):
//       d, delta      hist_u[b,t,:]                                   what main.py:110-111 takes
//       dd, ddelta    hist_u[b,t,:] - hist_u[b,t-1,:], u0[b] for t-1 = -1   the rates the QP bounds
//       e_c, e_phi, e_v   the stage-0 terms of the controller's cost at the post-step state x = hist_x[b,t+1,:]
//                     (main.py's traj_X): the window's first point X* = X, Y* = y(X), phi* = atan(y'(X)) by
//                     path_eval / pm_atan as build_window (mpc_frame.h) forms it; e_c = lateral_error
//                     (mpc_6stati.py:111-117), e_phi = atan2(sin(phi - phi*), cos(phi - phi*)), e_v = vx - vref[b,0];
//                     with a speed schedule (traj_closed_loop_stats_sched, vref_step = 1) e_v = vx - S[b, t+1]: stage 0 of
//                     the window the NEXT step starts from, as the other two errors are taken at that window's first point
//   traj_closed_loop_stats_pool   the B records (those the mask keeps) merged into one
//
// One wave per trajectory, four per workgroup; lanes stride over t, each with Welford's update on its own samples;
// the 64 partial records are joined by Chan's pairwise merge over a __shfl_xor butterfly, offsets 1, 2, .. 32, the
// lower lane's record always the merge's left operand -- every lane ends with the same bits, lane 0 stores them.  No
// atomics, no LDS, no scratch.  The pool is one workgroup: the kept trajectory of rank r (its place among the kept
// ones, so what the mask leaves out has no part in the order) goes to thread r mod 256, ranks ascending; then the same
// butterfly per wave and the four wave records merged 0, 1, 2, 3 through LDS.  Both are deterministic.
//
// A series with a non-finite sample has NaN in mean, M2, min and max (n stays the count); the merges carry that on.
//
// Built with the library's FLAGS: -ffp-contract=off, the accumulation is the written order.
#include <hip/hip_runtime.h>

#include "mpc_common.h"
#include "mpc_host.h"

namespace tgmpc {

constexpr int ST_S = TRAJ_STATS_SERIES;
constexpr int ST_F = TRAJ_STATS_FIELDS;
constexpr int ST_BLOCK = 256;
constexpr int ST_WAVES = ST_BLOCK / 64;

struct StatRec {
    double n, mean, m2, lo, hi;
};

__device__ __forceinline__ double st_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// min / max that keep a NaN (fmin / fmax drop it)
__device__ __forceinline__ double st_min(double a, double b) { return (a != a || b != b) ? st_nan() : fmin(a, b); }
__device__ __forceinline__ double st_max(double a, double b) { return (a != a || b != b) ? st_nan() : fmax(a, b); }

// Chan's merge, a on the left; an empty side returns the other unchanged
__device__ __forceinline__ StatRec st_merge(const StatRec& a, const StatRec& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    StatRec r;
    r.n = a.n + b.n;
    const double delta = b.mean - a.mean;
    r.mean = a.mean + delta * (b.n / r.n);
    r.m2 = (a.m2 + b.m2) + (delta * delta) * (a.n * (b.n / r.n));
    r.lo = st_min(a.lo, b.lo);
    r.hi = st_max(a.hi, b.hi);
    return r;
}

__device__ __forceinline__ StatRec st_shfl_xor(const StatRec& v, int off) {
    StatRec o;
    o.n = __shfl_xor(v.n, off, 64);
    o.mean = __shfl_xor(v.mean, off, 64);
    o.m2 = __shfl_xor(v.m2, off, 64);
    o.lo = __shfl_xor(v.lo, off, 64);
    o.hi = __shfl_xor(v.hi, off, 64);
    return o;
}

// the wave's 64 records joined in a fixed order; every lane returns the whole
__device__ __forceinline__ StatRec st_wave_merge(StatRec v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const StatRec o = st_shfl_xor(v, off);
        const bool upper = (lane & off) != 0;
        v = st_merge(upper ? o : v, upper ? v : o);
    }
    return v;
}

__device__ __forceinline__ int st_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(ST_BLOCK) void closed_stats_kernel(PathArgs pa, int B, int T, int hist_T,
                                                                const double* hist_x, const double* hist_u,
                                                                const double* u0, const double* vref,
                                                                long long vref_row, int vref_step,
                                                                const int* status, double* rec, int* fails) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;   // (the whole wave: nothing below synchronizes across waves)
    const double* hx = hist_x + (size_t)b * (hist_T + 1) * 6;
    const double* hu = hist_u + (size_t)b * hist_T * 2;
    const double* vr = vref + (size_t)vref_row * b;

    double mean[ST_S], m2[ST_S], lo[ST_S], hi[ST_S];
    bool bad[ST_S];
#pragma unroll
    for (int s = 0; s < ST_S; ++s) {
        mean[s] = 0.0;
        m2[s] = 0.0;
        lo[s] = __longlong_as_double(0x7ff0000000000000LL);
        hi[s] = -lo[s];
        bad[s] = false;
    }
    int n = 0, nfail = 0;
    for (int t = lane; t < T; t += 64) {
        const double* up = t > 0 ? hu + 2 * (size_t)(t - 1) : u0 + 2 * (size_t)b;
        const double* x = hx + 6 * (size_t)(t + 1);
        double v[ST_S];
        v[0] = hu[2 * (size_t)t];
        v[1] = hu[2 * (size_t)t + 1];
        v[2] = v[0] - up[0];
        v[3] = v[1] - up[1];
        double ys, dy;
        path_eval(pa, b, x[0], ys, dy);
        const double phis = pm_atan(dy);
        v[4] = lateral_error(x[0], x[1], x[0], ys, phis);
        double se, ce;
        pm_sincos(x[2] - phis, &se, &ce);
        v[5] = pm_atan2(se, ce);
        v[6] = x[3] - vr[(size_t)(t + 1) * vref_step];
        ++n;
        const double rn = 1.0 / (double)n;
#pragma unroll
        for (int s = 0; s < ST_S; ++s) {
            const double d = v[s] - mean[s];
            mean[s] = mean[s] + d * rn;
            m2[s] = m2[s] + d * (v[s] - mean[s]);
            lo[s] = fmin(lo[s], v[s]);
            hi[s] = fmax(hi[s], v[s]);
            bad[s] = bad[s] || !(fabs(v[s]) < __longlong_as_double(0x7ff0000000000000LL));
        }
        if (status) {
            const int st = status[(size_t)t * B + b];
            nfail += (st != TRAJ_STATUS_OPTIMAL && st != TRAJ_STATUS_OPTIMAL_INACCURATE) ? 1 : 0;
        }
    }
#pragma unroll
    for (int s = 0; s < ST_S; ++s) {
        StatRec r;
        r.n = (double)n;
        r.mean = bad[s] ? st_nan() : mean[s];
        r.m2 = bad[s] ? st_nan() : m2[s];
        r.lo = bad[s] ? st_nan() : lo[s];
        r.hi = bad[s] ? st_nan() : hi[s];
        r = st_wave_merge(r, lane);
        if (lane == 0) {
            double* o = rec + ((size_t)b * ST_S + s) * ST_F;
            o[0] = r.n;
            o[1] = r.mean;
            o[2] = r.m2;
            o[3] = r.lo;
            o[4] = r.hi;
        }
    }
    if (fails) {
        nfail = st_wave_sum(nfail);
        if (lane == 0) fails[b] = nfail;
    }
}

__global__ __launch_bounds__(ST_BLOCK) void closed_stats_pool_kernel(int B, const double* rec, const int* fails,
                                                                     const unsigned char* mask, double* pooled,
                                                                     long long* fails_total) {
    __shared__ int s_idx[ST_BLOCK];
    __shared__ int s_cnt[ST_WAVES];
    __shared__ double s_rec[ST_WAVES][ST_S][ST_F];
    __shared__ long long s_fail[ST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    StatRec acc[ST_S];
#pragma unroll
    for (int s = 0; s < ST_S; ++s) acc[s] = StatRec{0.0, 0.0, 0.0, 0.0, 0.0};
    long long nfail = 0;
    int base = 0;   // kept trajectories before this chunk, mod ST_BLOCK
    for (int c0 = 0; c0 < B; c0 += ST_BLOCK) {
        const int b = c0 + tid;   // (c0 <= B - 1 and tid < 256: no overflow for B <= INT_MAX - 255, checked on the host)
        const bool keep = b < B && (!mask || mask[b] != 0);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull));
        int total = 0;
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            total += s_cnt[w];
        }
        if (keep) s_idx[(base + before) & (ST_BLOCK - 1)] = b;
        __syncthreads();
        // this thread's slot holds the kept trajectory of rank base + k, k = (tid - base) mod 256, if k < total
        if (((tid - base) & (ST_BLOCK - 1)) < total) {
            const int bb = s_idx[tid];
            const double* r = rec + (size_t)bb * ST_S * ST_F;
#pragma unroll
            for (int s = 0; s < ST_S; ++s)
                acc[s] = st_merge(acc[s], StatRec{r[ST_F * s], r[ST_F * s + 1], r[ST_F * s + 2], r[ST_F * s + 3],
                                                  r[ST_F * s + 4]});
            if (fails) nfail += fails[bb];
        }
        base = (base + total) & (ST_BLOCK - 1);
        __syncthreads();   // s_idx, s_cnt are rewritten by the next chunk
    }
#pragma unroll
    for (int s = 0; s < ST_S; ++s) {
        const StatRec r = st_wave_merge(acc[s], lane);
        if (lane == 0) {
            s_rec[wave][s][0] = r.n;
            s_rec[wave][s][1] = r.mean;
            s_rec[wave][s][2] = r.m2;
            s_rec[wave][s][3] = r.lo;
            s_rec[wave][s][4] = r.hi;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nfail += __shfl_xor(nfail, off, 64);
    if (lane == 0) s_fail[wave] = nfail;
    __syncthreads();
    if (tid < ST_S) {
        StatRec r{s_rec[0][tid][0], s_rec[0][tid][1], s_rec[0][tid][2], s_rec[0][tid][3], s_rec[0][tid][4]};
        for (int w = 1; w < ST_WAVES; ++w)
            r = st_merge(r, StatRec{s_rec[w][tid][0], s_rec[w][tid][1], s_rec[w][tid][2], s_rec[w][tid][3],
                                    s_rec[w][tid][4]});
        double* o = pooled + ST_F * tid;
        o[0] = r.n;
        // nothing kept: n = 0 and no value to report
        o[1] = r.n == 0.0 ? st_nan() : r.mean;
        o[2] = r.n == 0.0 ? st_nan() : r.m2;
        o[3] = r.n == 0.0 ? st_nan() : r.lo;
        o[4] = r.n == 0.0 ? st_nan() : r.hi;
    }
    if (tid == 0 && fails_total) {
        long long f = 0;
        for (int w = 0; w < ST_WAVES; ++w) f += s_fail[w];
        *fails_total = f;
    }
}

}  // namespace tgmpc

// both statistics entry points: vref row b at vref + vref_row b, e_v at step t against its entry (t + 1) vref_step
static int stats_launch(const traj_paths* paths, int B, int N, int T, int hist_T, const double* hist_x,
                        const double* hist_u, const double* u0, const double* vref, long long vref_row, int vref_step,
                        const int* status, double* rec, int* fails, void* stream) {
    using namespace tgmpc;
    if (B < 0 || N < 1 || T < 1 || T > hist_T || !paths_ok(paths)) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!hist_x || !hist_u || !u0 || !vref || !rec) return TRAJ_E_ARG;
    hipLaunchKernelGGL(closed_stats_kernel, dim3(nblk(B, ST_WAVES)), dim3(ST_BLOCK), 0, (hipStream_t)stream,
                       path_args(paths), B, T, hist_T, hist_x, hist_u, u0, vref, vref_row, vref_step, status, rec, fails);
    return launched();
}

extern "C" {

int traj_closed_loop_stats_sched(const traj_paths* paths, int B, int N, int T, int hist_T, const double* hist_x,
                                 const double* hist_u, const double* u0, const double* vref, long long vref_row,
                                 int vref_len, int vref_step, const int* status, double* rec, int* fails,
                                 void* stream) {
    if ((vref_step != 0 && vref_step != 1) || (long long)vref_len < (long long)N + 1 ||
        (vref_row != 0 && vref_row < vref_len) || (long long)T * vref_step >= (long long)vref_len)
        return TRAJ_E_ARG;
    return stats_launch(paths, B, N, T, hist_T, hist_x, hist_u, u0, vref, vref_row, vref_step, status, rec, fails,
                        stream);
}

// (the plain [B,N+1] reference: the schedule entry point's (N + 1, N + 1, 0))
int traj_closed_loop_stats(const traj_paths* paths, int B, int N, int T, int hist_T, const double* hist_x,
                           const double* hist_u, const double* u0, const double* vref, const int* status, double* rec,
                           int* fails, void* stream) {
    return stats_launch(paths, B, N, T, hist_T, hist_x, hist_u, u0, vref, (long long)N + 1, 0, status, rec, fails,
                        stream);
}

int traj_closed_loop_stats_pool(int B, const double* rec, const int* fails, const unsigned char* mask, double* pooled,
                                long long* fails_total, void* stream) {
    using namespace tgmpc;
    if (B < 0 || B > 0x7fffffff - ST_BLOCK) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!rec || !pooled) return TRAJ_E_ARG;
    hipLaunchKernelGGL(closed_stats_pool_kernel, dim3(1), dim3(ST_BLOCK), 0, (hipStream_t)stream, B, rec, fails, mask,
                       pooled, fails_total);
    return launched();
}

}  // extern "C"

// knet.hip -- the KalmanNet ops for gfx950 (include/trajknet.h; float32, as the reference runs): the entry points,
// their argument checks and launches.  The kernels live in the knet_*.h headers, one per stage, all included below
// inside one anonymous namespace, each after what its first comment names.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/trajknet.h"

namespace {

#include "knet_vehicle.h"   // the vehicle physics, the prior and the posterior of one sequence
#include "knet_ops.h"       // the per-op kernels: prior, GRU gates, update
#include "knet_rollout.h"   // the open-loop rollout and the prediction loss
#include "knet_bwd.h"       // the backward kernels and the chunk loss of truncated-BPTT training
#include "knet_opt.h"       // the batch gather and clipping + AdamW of chunk-and-shuffle training
#include "knet_dense.h"     // the fused step's packed weights, dense layers and GRU cells
#include "knet_fc2.h"       // FC2 in its three product modes
#include "knet_step.h"      // the fused step's front, back and back-front kernels
#include "knet_ekf_step.h"  // one float64 EKF step (shared with closed_obs.hip)
#include "knet_ekf.h"       // the float64 EKF baseline

inline int nblk(long long n, int t) { return (int)((n + t - 1) / t); }

// the launch just queued: TRAJ_OK, or TRAJ_E_LAUNCH when the runtime refused it
inline int launched() { return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH; }

KP kp_of(const traj_vehicle_params* p) {   // the vehicle parameters rounded to float32
    return KP{(float)p->Cm1, (float)p->Cm2, (float)p->Cr0, (float)p->Cr2, (float)p->Br, (float)p->Cr, (float)p->Dr,
              (float)p->Bf,  (float)p->Cf,  (float)p->Df,  (float)p->m,   (float)p->Iz, (float)p->lf, (float)p->lr,
              (float)p->maxAlpha, (float)p->vx_zero};
}

// FC2's slabs of hidden units = the workspace's partials per sequence
int fc2_nslab(const traj_knet_net* net) { return net->d_fc2h / fc2_slab(net->d_fc2h); }

}  // namespace

// traj_knet_set_fc2_mode: 2 = knet_fc2y_kernel (three-term bf16 operands, the tile split once per workgroup; the
// default), 1 = knet_fc2x_kernel (the same terms and sums, every wave splitting the tile), 0 = knet_fc2_kernel (f32).
static std::atomic<int> g_fc2_mode{2};

// FC2 launch in the mode of traj_knet_set_fc2_mode
static int fc2_launch(const traj_knet_net* net, int B, const float* x2, float* ws, void* stream) {
    const int hs = fc2_slab(net->d_fc2h), nslab = fc2_nslab(net), nbb = nblk(B, F2_BT);
    const int mode = g_fc2_mode.load(std::memory_order_relaxed);
    auto kern = mode == 2 ? (hs == 320 ? knet_fc2y_kernel<5> : knet_fc2y_kernel<4>)
              : mode == 1 ? (hs == 320 ? knet_fc2x_kernel<5> : knet_fc2x_kernel<4>)
                          : (hs == 320 ? knet_fc2_kernel<5> : knet_fc2_kernel<4>);
    hipLaunchKernelGGL(kern, dim3(nslab * nbb), dim3(256), 0, (hipStream_t)stream, B, net->d_fc2h, x2, net->fc2a_w,
                       net->fc2a_b, net->fc2b_w, net->n * net->m, ws);
    return launched();
}

extern "C" {

int traj_knet_prior_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts, int B,
                        const float* x_post, const float* u, const float* y, const float* x_mean,
                        const float* x_std, const float* y_mean, const float* y_std, const float* u_mean,
                        const float* u_std, float* m1x_prior, float* m1y, float* dy, void* stream) {
    if (!p || !lim || B < 0) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x_post || !u || !x_mean || !x_std || !y_mean || !y_std || !m1x_prior || !m1y) return TRAJ_E_ARG;
    if (dy && !y) return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_prior_kernel, dim3(nblk(B, 256)), dim3(256), 0, (hipStream_t)stream, k, *lim, Ts, B,
                       x_post, u, y, x_mean, x_std, y_mean, y_std, u_mean, u_std, m1x_prior, m1y, dy);
    return launched();
}

int traj_knet_gru_gates_f32(int B, int H, const float* gi, const float* gh, const float* h, float* h_out,
                            void* stream) {
    if (B < 0 || H < 1) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!gi || !gh || !h || !h_out) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_gru_kernel, dim3(nblk((long long)B * H, 256)), dim3(256), 0, (hipStream_t)stream, B, H,
                       gi, gh, h, h_out);
    return launched();
}

int traj_knet_update_f32(int B, const float* x_prior, const float* KG, const float* dy, const float* innov_logit,
                         float* x_post, void* stream) {
    if (B < 0) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x_prior || !KG || !dy || !innov_logit || !x_post) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_update_kernel, dim3(nblk(B, 256)), dim3(256), 0, (hipStream_t)stream, B, x_prior, KG, dy,
                       innov_logit, x_post);
    return launched();
}

int traj_knet_rollout_windows(int T, int H, int t0, int step) {
    if (T < 0 || H < 1 || t0 < 0 || step < 1) return -1;
    const int end = T - H;   // range(t0, T - H, step)
    return end > t0 ? (end - t0 + step - 1) / step : 0;
}

int traj_knet_rollout_eval_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts, int B, int T,
                               int H, int t0, int step, int nwin, const float* x_est, int e_sb, int e_sc, int e_st,
                               const float* x_mean, const float* x_std, const float* u, const float* x_gt, float* ade,
                               float* fde, float* err_profile, float* pred, void* stream) {
    if (!p || !lim || B < 0 || T < 0 || H < 1 || t0 < 0 || step < 1 || nwin < 0) return TRAJ_E_ARG;
    // every window's inputs u[:, :, t .. t + H - 1] (and, when scored, its ground truth x_gt[:, :, t + 1 .. t + H])
    // lie inside the sequence
    if (nwin > 0 && (long long)t0 + (long long)(nwin - 1) * step + H > (long long)T - (x_gt ? 1 : 0))
        return TRAJ_E_ARG;
    if ((long long)B * nwin > 0x7fffffffLL || e_sb < 0 || e_sc < 0 || e_st < 0) return TRAJ_E_ARG;
    if (B == 0 || nwin == 0) return TRAJ_OK;
    if (!x_est || !u || (!x_mean) != (!x_std)) return TRAJ_E_ARG;
    if (x_gt ? (!ade || !fde) : !pred) return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_rollout_kernel, dim3(nblk((long long)B * nwin, 64)), dim3(64), 0, (hipStream_t)stream, k,
                       *lim, Ts, B, T, H, t0, step, nwin, x_est, e_sb, e_sc, e_st, x_mean, x_std, u, x_gt, ade, fde,
                       x_gt ? err_profile : nullptr, pred);
    return launched();
}

int traj_knet_pred_loss_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts, int B, int T, int H,
                            int t0, int step, int nwin, const float* x_est, int e_sb, int e_sc, int e_sw,
                            const float* x_mean, const float* x_std, const float* u_mean, const float* u_std,
                            const float* u, const float* x_gt_norm, float* part, float* grad, void* stream) {
    if (!p || !lim || B < 0 || T < 1 || H < 1 || t0 < 0 || step < 1 || nwin < 0) return TRAJ_E_ARG;
    // every window starts inside the sequence (a window at t = T - 1 has no step and scores 0)
    if (nwin > 0 && (long long)t0 + (long long)(nwin - 1) * step > (long long)T - 1) return TRAJ_E_ARG;
    if ((long long)B * nwin > 0x7fffffffLL || e_sb < 0 || e_sc < 0 || e_sw < 0) return TRAJ_E_ARG;
    if (B == 0 || nwin == 0) return TRAJ_OK;
    if (!x_est || !x_mean || !x_std || !u || !x_gt_norm || !part || (!u_mean) != (!u_std)) return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_pred_loss_kernel, dim3(nblk((long long)B * nwin, 64)), dim3(64), 0, (hipStream_t)stream,
                       k, *lim, Ts, B, T, H, t0, step, nwin, x_est, e_sb, e_sc, e_sw, x_mean, x_std, u_mean, u_std, u,
                       x_gt_norm, part, grad);
    return launched();
}

int traj_knet_prior_bwd_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts, int B,
                            const float* x_post, const float* u, const float* x_mean, const float* x_std,
                            const float* y_mean, const float* y_std, const float* u_mean, const float* u_std,
                            const float* g_prior, const float* g_dy, float* g_x_post, void* stream) {
    if (!p || !lim || B < 0) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x_post || !u || !x_mean || !x_std || !y_mean || !y_std || !g_prior || !g_x_post) return TRAJ_E_ARG;
    if ((!u_mean) != (!u_std)) return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_prior_bwd_kernel, dim3(nblk(B, 256)), dim3(256), 0, (hipStream_t)stream, k, *lim, Ts, B,
                       x_post, u, x_mean, x_std, y_std, u_mean, u_std, g_prior, g_dy, g_x_post);
    return launched();
}

int traj_knet_gru_gates_bwd_f32(int B, int H, const float* gi, const float* gh, const float* h, const float* g_out,
                                int g_out_ld, const float* g_out2, int g_out2_ld, float* g_gi, float* g_gh, float* g_h,
                                void* stream) {
    if (B < 0 || H < 1 || (long long)B * H > 0x7fffffffLL / 3) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!gi || !gh || !h || !g_out || !g_gi || !g_gh || !g_h) return TRAJ_E_ARG;
    if (g_out_ld < H || (g_out2 && g_out2_ld < H)) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_gru_bwd_kernel, dim3(nblk((long long)B * H, 256)), dim3(256), 0, (hipStream_t)stream, B, H,
                       gi, gh, h, g_out, g_out_ld, g_out2, g_out2_ld, g_gi, g_gh, g_h);
    return launched();
}

int traj_knet_update_bwd_f32(int B, const float* KG, const float* dy, const float* innov_logit, const float* g_post,
                             const float* g_post2, float* g_prior, float* g_KG, float* g_dy, float* g_logit,
                             void* stream) {
    if (B < 0) return TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!KG || !dy || !innov_logit || !g_post || !g_prior || !g_KG || !g_dy || !g_logit) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_update_bwd_kernel, dim3(nblk(B, 256)), dim3(256), 0, (hipStream_t)stream, B, KG, dy,
                       innov_logit, g_post, g_post2, g_prior, g_KG, g_dy, g_logit);
    return launched();
}

int traj_knet_dense_bwd_f32(int rows, int cols, const float* g_a, int ld_a, const float* g_b, int ld_b,
                            const float* act, const float* mask, float* g_pre, void* stream) {
    if (rows < 0 || cols < 1) return TRAJ_E_ARG;
    if (rows == 0) return TRAJ_OK;
    if (!g_a || !g_pre || ld_a < cols || (g_b && ld_b < cols)) return TRAJ_E_ARG;
    const long long n = (long long)rows * cols;
    if (nblk(n, 256) <= 0 || n > 0x7fffffffLL * 256) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_dense_bwd_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, n, cols, g_a,
                       ld_a, g_b, ld_b, act, mask, g_pre);
    return launched();
}

int traj_knet_train_loss_f32(int B, int K, const float* x_out, int sb, int sc, int sk, const float* x_tgt,
                             const float* y_tgt, const float* x_mean, const float* x_std, float alpha,
                             const float* g_extra, float* loss, float* grad, void* stream) {
    if (B < 1 || K < 1 || sb < 0 || sc < 0 || sk < 0 || !(alpha >= 0.0f && alpha <= 1.0f)) return TRAJ_E_ARG;
    if ((long long)B * K > 0x7fffffffLL / 6) return TRAJ_E_ARG;
    if (!x_out || !x_tgt || !x_mean || !x_std || !loss || !grad || (alpha < 1.0f && !y_tgt)) return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_train_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, K, x_out, sb, sc, sk,
                       x_tgt, y_tgt, x_mean, x_std, alpha, g_extra, loss, grad);
    return launched();
}

int traj_knet_chunk_gather_f32(int n_traj, int T_full, int Tc, int B, const float* y, const float* u, const float* x,
                               const int* chunk_ids, const float* x_mean, const float* x_std, const float* y_mean,
                               const float* y_std, const float* noise, float noise_std, float* Y, float* U,
                               float* x_tgt, float* y_tgt, float* m1x0, void* stream) {
    if (B < 1 || n_traj < 1 || Tc < 1 || Tc > T_full) return TRAJ_E_ARG;
    if ((long long)B * Tc > 0x7fffffffLL / 6 || (long long)n_traj * T_full > 0x7fffffffLL / 6) return TRAJ_E_ARG;
    if (!y || !u || !x || !chunk_ids || !x_mean || !x_std || !y_mean || !y_std || !Y || !U || !x_tgt || !m1x0)
        return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_chunk_gather_kernel, dim3(nblk((long long)B * Tc, 256)), dim3(256), 0, (hipStream_t)stream,
                       n_traj, T_full, Tc, B, y, u, x, chunk_ids, x_mean, x_std, y_mean, y_std, noise, noise_std, Y, U,
                       x_tgt, y_tgt, m1x0);
    return launched();
}

size_t traj_knet_clip_adamw_workspace_bytes(void) { return (size_t)OPT_NORM_BLOCKS * sizeof(double); }

int traj_knet_clip_adamw_f32(const traj_knet_opt_entry* table, int n_tensors, long long n_total, const float* lr,
                             double beta1, double beta2, double eps, double weight_decay, double max_norm, int* step,
                             float* total_norm, void* ws, size_t ws_bytes, void* stream) {
    if (n_tensors < 1 || n_total < n_tensors) return TRAJ_E_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) ||
        max_norm != max_norm)
        return TRAJ_E_ARG;
    if (!table || !lr || !step || !ws || ((size_t)ws & 7u) || ws_bytes < traj_knet_clip_adamw_workspace_bytes())
        return TRAJ_E_ARG;
    // a float4 per thread and sweep: the norm pass in at most OPT_NORM_BLOCKS workgroups (one partial each), the update
    // pass in at most OPT_MAX_BLOCKS, both grid-striding over the rest
    const long long want = (n_total + 1023) / 1024;
    const int nb_norm = (int)(want < OPT_NORM_BLOCKS ? want : OPT_NORM_BLOCKS);
    const int nb_upd = (int)(want < OPT_MAX_BLOCKS ? want : OPT_MAX_BLOCKS);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(knet_opt_norm_kernel, dim3(nb_norm), dim3(256), 0, (hipStream_t)stream, table, n_tensors, step,
                       partial);
    if (hipGetLastError() != hipSuccess) return TRAJ_E_LAUNCH;
    hipLaunchKernelGGL(knet_opt_update_kernel, dim3(nb_upd), dim3(256), 0, (hipStream_t)stream, table, n_tensors, lr,
                       beta1, beta2, eps, weight_decay, max_norm, (const int*)step, (const double*)partial, nb_norm,
                       total_norm);
    return launched();
}

static bool knet_ok(const traj_knet_net* w) {
    // FC5 / [FC1 | FC7] outputs live in 64-wide zero-padded LDS rows: in_mult 5 and 10 (d_fc5 30 / 60)
    return w && w->m == 6 && w->n == 5 && w->hidden == KH && w->d_fc5 > 0 && w->d_fc5 <= 64 && w->d_fc1 > 0 &&
           w->d_fc7 > 0 && w->d_fc1 + w->d_fc7 <= 64 && w->d_fc3 > 0 && w->d_fc3 <= 64 && w->fc5_w && w->fc5_b &&
           w->gru_q_wih && w->gru_q_bih && w->gru_q_whh && w->gru_q_bhh && w->gru_sigma_wih && w->gru_sigma_bih &&
           w->gru_sigma_whh && w->gru_sigma_bhh && w->fc1_w && w->fc1_b && w->fc7_w && w->fc7_b && w->gru_s_wih &&
           w->gru_s_bih && w->gru_s_whh && w->gru_s_bhh && w->fc3_w && w->fc3_b && w->fc4_w && w->fc4_b && w->innov_logit &&
           w->d_fc2h > 0 && w->d_fc2h % 256 == 0 && w->fc2a_w && w->fc2a_b && w->fc2b_w && w->fc2b_b;
}
static KNet knet_args(const traj_knet_net* w, const float* packed) {
    const PackPlan pl = pack_plan(w);
    auto P = [&](int i) { return reinterpret_cast<const float4*>(packed + pl.off[i]); };
    return KNet{w->m,     w->n,     w->d_fc5, w->d_fc1, w->d_fc7, w->d_fc3, w->fc5_b,  w->gru_q_bih, w->gru_q_bhh,
                w->gru_sigma_bih, w->gru_sigma_bhh, w->fc1_b, w->fc7_b, w->gru_s_bih, w->gru_s_bhh, w->fc3_b,
                w->fc4_b, w->innov_logit, w->fc2b_b, P(0), P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10)};
}

size_t traj_knet_packed_bytes(const traj_knet_net* net) {
    if (!knet_ok(net)) return 0;
    return pack_plan(net).off[11] * sizeof(float);
}

int traj_knet_pack_f32(const traj_knet_net* net, float* packed, size_t bytes, void* stream) {
    if (!net || !packed) return TRAJ_E_ARG;
    if (!knet_ok(net)) return TRAJ_E_UNSUPPORTED;
    const PackPlan pl = pack_plan(net);
    if (bytes < pl.off[11] * sizeof(float) || ((uintptr_t)packed & 15)) return TRAJ_E_ARG;
    const float* W[11] = {net->fc5_w, net->gru_q_wih, net->gru_q_whh, net->gru_sigma_wih, net->gru_sigma_whh,
                          net->fc1_w, net->fc7_w,     net->gru_s_wih, net->gru_s_whh,     net->fc3_w,
                          net->fc4_w};
    for (int i = 0; i < 11; ++i) {
        const long long n = (long long)(pl.off[i + 1] - pl.off[i]);
        hipLaunchKernelGGL(knet_pack_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, W[i], pl.N[i],
                           pl.K[i], packed + pl.off[i]);
    }
    return launched();
}

int traj_knet_front_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts, const traj_knet_net* net,
                        const float* packed, int B, const float* x_post, const float* u, int u_stride_b,
                        int u_stride_c, const float* y, int y_stride_b, int y_stride_c, const float* x_mean,
                        const float* x_std, const float* y_mean, const float* y_std, const float* u_mean,
                        const float* u_std, float* h_q, const float* h_sigma, float* h_s, float* m1x_prior, float* dy,
                        float* x2, void* stream) {
    if (!p || !lim || B < 0) return TRAJ_E_ARG;
    if (!knet_ok(net)) return net ? TRAJ_E_UNSUPPORTED : TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!packed || ((uintptr_t)packed & 15) || !x_post || !u || !y || !x_mean || !x_std || !y_mean || !y_std || !h_q ||
        !h_sigma || !h_s || !m1x_prior || !dy || !x2)
        return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_front_kernel, dim3(nblk(B, KS)), dim3(KT), 0, (hipStream_t)stream, k, *lim, Ts,
                       knet_args(net, packed), B, x_post, u, u_stride_b, u_stride_c, y, y_stride_b, y_stride_c, x_mean,
                       x_std, y_mean, y_std, u_mean, u_std, h_q, h_sigma, h_s, m1x_prior, dy, x2);
    return launched();
}

size_t traj_knet_fc2_workspace_bytes(const traj_knet_net* net, int B) {
    if (!knet_ok(net) || B < 0) return 0;
    return (size_t)fc2_nslab(net) * (size_t)B * 32 * sizeof(float);
}

int traj_knet_fc2_f32(const traj_knet_net* net, int B, const float* x2, float* ws, size_t ws_bytes, void* stream) {
    if (B < 0) return TRAJ_E_ARG;
    if (!knet_ok(net)) return net ? TRAJ_E_UNSUPPORTED : TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!x2 || !ws || ws_bytes < traj_knet_fc2_workspace_bytes(net, B) || ((uintptr_t)x2 & 15) ||
        ((uintptr_t)net->fc2a_w & 15) || ((uintptr_t)net->fc2a_b & 15) || ((uintptr_t)net->fc2b_w & 15))
        return TRAJ_E_ARG;
    return fc2_launch(net, B, x2, ws, stream);
}

int traj_knet_set_fc2_mode(int mode) {
    if (mode < 0 || mode > 2) return -1;
    return g_fc2_mode.exchange(mode);
}

int traj_knet_back_f32(const traj_knet_net* net, const float* packed, int B, const float* x2, const float* ws,
                       const float* m1x_prior, const float* dy, float* h_sigma, float* x_post, float* out,
                       int out_stride_b, int out_stride_c, float* KG_out, void* stream) {
    if (B < 0) return TRAJ_E_ARG;
    if (!knet_ok(net)) return net ? TRAJ_E_UNSUPPORTED : TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!packed || ((uintptr_t)packed & 15) || !x2 || !ws || !m1x_prior || !dy || !h_sigma || !x_post)
        return TRAJ_E_ARG;
    hipLaunchKernelGGL(knet_back_kernel, dim3(nblk(B, KS)), dim3(KT), 0, (hipStream_t)stream, knet_args(net, packed),
                       B, x2, ws, fc2_nslab(net), m1x_prior, dy, h_sigma, x_post, out, out_stride_b, out_stride_c,
                       KG_out);
    return launched();
}

int traj_knet_back_front_f32(const traj_vehicle_params* p, const traj_knet_limits* lim, float Ts,
                             const traj_knet_net* net, const float* packed, int B, const float* ws, float* out,
                             int out_stride_b, int out_stride_c, const float* u, int u_stride_b, int u_stride_c,
                             const float* y, int y_stride_b, int y_stride_c, const float* x_mean, const float* x_std,
                             const float* y_mean, const float* y_std, const float* u_mean, const float* u_std,
                             float* h_q, float* h_sigma, float* h_s, float* x_post, float* m1x_prior, float* dy,
                             float* x2, void* stream) {
    if (!p || !lim || B < 0) return TRAJ_E_ARG;
    if (!knet_ok(net)) return net ? TRAJ_E_UNSUPPORTED : TRAJ_E_ARG;
    if (B == 0) return TRAJ_OK;
    if (!packed || ((uintptr_t)packed & 15) || !ws || !u || !y || !x_mean || !x_std || !y_mean || !y_std || !h_q ||
        !h_sigma || !h_s || !x_post || !m1x_prior || !dy || !x2)
        return TRAJ_E_ARG;
    if (!out) return TRAJ_E_ARG;
    const KP k = kp_of(p);
    hipLaunchKernelGGL(knet_back_front_kernel, dim3(nblk(B, KS)), dim3(KT), 0, (hipStream_t)stream,
                       knet_args(net, packed), B, ws, fc2_nslab(net), out, out_stride_b, out_stride_c, k, *lim, Ts, u,
                       u_stride_b, u_stride_c, y, y_stride_b, y_stride_c, x_mean, x_std, y_mean, y_std, u_mean, u_std,
                       h_q, h_sigma, h_s, x_post, m1x_prior, dy, x2);
    return launched();
}

int traj_ekf_run_f64(const traj_vehicle_params* p, const traj_knet_limits* lim, double Ts, int B, int T,
                     const double* y, const double* u, const double* x0, const double* P0, const double* Q,
                     const double* R, double* x_est, void* stream) {
    if (!p || !lim || B < 0 || T < 0) return TRAJ_E_ARG;
    if (B == 0 || T == 0) return TRAJ_OK;
    if (!y || !u || !x0 || !P0 || !Q || !R || !x_est) return TRAJ_E_ARG;
    KPd k{p->Cm1, p->Cm2, p->Cr0, p->Cr2, p->Br, p->Cr, p->Dr, p->Bf, p->Cf, p->Df, p->m, p->Iz, p->lf, p->lr,
          p->maxAlpha, p->vx_zero,
          {lim->x_min, lim->y_min, lim->phi_min, lim->vx_min, lim->vy_min, lim->omega_min},
          {lim->x_max, lim->y_max, lim->phi_max, lim->vx_max, lim->vy_max, lim->omega_max}};
    hipLaunchKernelGGL(ekf_kernel, dim3(nblk(B, 64)), dim3(64), 0, (hipStream_t)stream, k, Ts, B, T, y, u, x0, P0, Q,
                       R, x_est);
    return launched();
}

}  // extern "C"

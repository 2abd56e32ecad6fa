// knet_rollout.h -- the open-loop rollouts over windows of a sequence: the evaluation metrics
// (traj_knet_rollout_eval_f32) and the training loss with its gradient (traj_knet_pred_loss_f32).  Included by knet.hip
// inside its anonymous namespace, after knet_vehicle.h.

// test_prediction.py:198-221 for every (sequence b, window w) at once: the window starts at
// t = t0 + w * step from the filter's estimate x_est[b, :, t] (normalized -> real, :202-203), runs
// rollout_open_loop (:67-87: H clamped Euler steps of f with u[b, :, t + k]) and scores the XY error
// against x_gt[b, :, t + 1 + k] (compute_metrics / get_error_profile, :89-112).  One thread per window;
// the serial chain is H steps of the same physics as the filter's prior (veh_step).
__global__ __launch_bounds__(64) void knet_rollout_kernel(KP p, traj_knet_limits L, float Ts, int B, int T, int H,
                                                          int t0, int step, int nwin, const float* __restrict__ xe,
                                                          int e_sb, int e_sc, int e_st,
                                                          const float* __restrict__ xm, const float* __restrict__ xs,
                                                          const float* __restrict__ u, const float* __restrict__ xg,
                                                          float* __restrict__ ade, float* __restrict__ fde,
                                                          float* __restrict__ prof, float* __restrict__ pred) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * nwin) return;
    const int b = i / nwin, t = t0 + (i % nwin) * step;
    const float* eb = xe + (size_t)b * e_sb + (size_t)t * e_st;
    const float* ub = u + (size_t)b * 2 * T;
    const float* gb = xg ? xg + (size_t)b * 6 * T : nullptr;
    float x[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const float v = eb[(size_t)c * e_sc];
        x[c] = xm ? __fadd_rn(__fmul_rn(v, xs[c]), xm[c]) : v;   // x_start_norm * x_std + x_mean
    }
    double sum = 0.0;
    float e = 0.0f;
    // each step's inputs are loaded one step ahead: a launch holds about one wave per SIMD (B * nwin
    // threads), so no other wave hides the load latency of the serial chain
    float ud = ub[t], ue = ub[T + t], gx = gb ? gb[t + 1] : 0.0f, gy = gb ? gb[T + t + 1] : 0.0f;
    for (int k = 0; k < H; ++k) {
        const float cd = ud, ce = ue, cgx = gx, cgy = gy;
        if (k + 1 < H) {
            ud = ub[t + k + 1];
            ue = ub[T + t + k + 1];
            if (gb) {
                gx = gb[t + k + 2];
                gy = gb[T + t + k + 2];
            }
        }
        float xn[6];
        veh_step(p, L, Ts, x, cd, ce, xn);
        if (gb) {
            const float dx = __fsub_rn(xn[0], cgx), dyv = __fsub_rn(xn[1], cgy);
            e = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dyv, dyv)));   // sqrt(sum(diff**2)) over X, Y
            sum += (double)e;
            if (prof) prof[(size_t)i * H + k] = e;
        }
        if (pred) {
#pragma unroll
            for (int c = 0; c < 6; ++c) pred[((size_t)i * 6 + c) * H + k] = xn[c];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) x[c] = xn[c];
    }
    if (gb) {
        ade[i] = (float)(sum / (double)H);   // err_dist.mean()
        fde[i] = e;                          // err_dist[0, -1]
    }
}

// pipeline_prediction.py:61-99 (compute_prediction_loss, with _compute_step_loss_real :45-59) for every (sequence b,
// window w) at once, with the derivative its autograd gives.  Window w starts at t = t0 + w * step from
// x_est[b, :, w] (indexed by window), rolls the physics valid = max(0, min(H, T - 1 - t)) steps and sums the squared
// error against the denormalized ground truth, phi as the wrapped difference (derivative 1):
//   part[b, w] = sum_k sum_c e^2 / (6 valid),   grad[b, :, w] = d part[b, w] / d x_est[b, :, w].
// The gradient rides forward with the rollout as the sensitivity S = d x_k / d x_0 (no stored states): X and Y enter
// no derivative, so S is the two scalars d X_k / d X_0, d Y_k / d Y_0 and the 6 x 4 block of columns phi .. omega.
// One thread per window; every sum runs in a fixed order (k, then c).
__global__ __launch_bounds__(64) void knet_pred_loss_kernel(KP p, traj_knet_limits L, float Ts, int B, int T, int H,
                                                            int t0, int step, int nwin, const float* __restrict__ xe,
                                                            int e_sb, int e_sc, int e_sw,
                                                            const float* __restrict__ xm, const float* __restrict__ xs,
                                                            const float* __restrict__ um, const float* __restrict__ us,
                                                            const float* __restrict__ u, const float* __restrict__ xg,
                                                            float* __restrict__ part, float* __restrict__ grad) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * nwin) return;
    const int b = i / nwin, w = i - b * nwin, t = t0 + w * step;
    const int valid = max(0, min(H, T - 1 - t));
    const float* eb = xe + (size_t)b * e_sb + (size_t)w * e_sw;
    const float* ub = u + (size_t)b * 2 * T;
    const float* gb = xg + (size_t)b * 6 * T;
    float mean[6], sd[6], x[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        mean[c] = xm[c];
        sd[c] = xs[c];
        x[c] = __fadd_rn(__fmul_rn(eb[(size_t)c * e_sc], sd[c]), mean[c]);   // _denorm_x
    }
    const bool un = um && us;
    const float us0 = un ? us[0] : 1.0f, us1 = un ? us[1] : 1.0f, um0 = un ? um[0] : 0.0f, um1 = un ? um[1] : 0.0f;
    float sxx = 1.0f, syy = 1.0f, S[6][4], g[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) S[r][c] = (r == c + 2) ? 1.0f : 0.0f;
    double sum = 0.0;
    // step k's control and target are loaded one step ahead (as knet_rollout_kernel: about one wave per SIMD, so no
    // other wave hides the load latency of the serial chain)
    float ud = 0.0f, ue = 0.0f, tg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid > 0) {
        ud = ub[t];
        ue = ub[T + t];
#pragma unroll
        for (int c = 0; c < 6; ++c) tg[c] = gb[(size_t)c * T + t + 1];
    }
    for (int k = 1; k <= valid; ++k) {
        float cd = ud, ce = ue, ct[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) ct[c] = tg[c];
        if (k < valid) {
            ud = ub[t + k];
            ue = ub[T + t + k];
#pragma unroll
            for (int c = 0; c < 6; ++c) tg[c] = gb[(size_t)c * T + t + k + 1];
        }
        if (un) {   // _denorm_u
            cd = __fadd_rn(__fmul_rn(cd, us0), um0);
            ce = __fadd_rn(__fmul_rn(ce, us1), um1);
        }
        float xn[6];
        VehJac J;
        veh_step_t<true>(p, L, Ts, x, cd, ce, xn, &J);
        // S <- d xn / d x . S
        float Sn[6][4];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) a = fmaf(J.A[r][q], S[2 + q][c], a);
                Sn[r][c] = J.post[r] * fmaf(Ts, a, S[r][c]);
            }
        sxx *= J.post[0];
        syy *= J.post[1];
        // _compute_step_loss_real against x_gt_norm * x_std + x_mean
        float e[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) e[c] = __fsub_rn(xn[c], __fadd_rn(__fmul_rn(ct[c], sd[c]), mean[c]));
        e[2] = atan2f(sinf(e[2]), cosf(e[2]));
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) s = __fadd_rn(s, __fmul_rn(e[c], e[c]));
        sum += (double)s;
        g[0] = fmaf(e[0], sxx, g[0]);
        g[1] = fmaf(e[1], syy, g[1]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) g[2 + c] = fmaf(e[r], Sn[r][c], g[2 + c]);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            x[r] = xn[r];
#pragma unroll
            for (int c = 0; c < 4; ++c) S[r][c] = Sn[r][c];
        }
    }
    const float inv = valid > 0 ? 1.0f / (6.0f * (float)valid) : 0.0f;
    part[i] = valid > 0 ? (float)(sum / (6.0 * (double)valid)) : 0.0f;
    if (grad) {
#pragma unroll
        for (int c = 0; c < 6; ++c)   // d e^2 = 2 e de; the x_std of the denormalization
            grad[((size_t)b * 6 + c) * nwin + w] = valid > 0 ? __fmul_rn(__fmul_rn(2.0f * g[c], sd[c]), inv) : 0.0f;
    }
}

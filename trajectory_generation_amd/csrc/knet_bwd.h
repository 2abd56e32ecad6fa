// knet_bwd.h -- the non-GEMM parts of one KalmanNet step's backward and the chunk loss of truncated-BPTT training
// (include/trajknet.h: traj_knet_*_bwd_f32, traj_knet_train_loss_f32).  Included by knet.hip inside its anonymous
// namespace, after veh_step_t / KP / sigmoidf_, so the backward differentiates the very expressions the forward runs.
//
// All float32, no atomics, every sum in a fixed order, plain vector stores.  The derivatives are the ones torch's
// autograd gives for kalman_net.py:145-216 and pipeline.py:16-60: clamp passes the gradient on the closed interval,
// relu's mask is (output > 0), the wrapped angle difference atan2(sin, cos) has derivative 1.

// Transposed chain of knet_prior_kernel for one sequence per thread:
//   g_x_post = x_std * J' (g_prior / x_std - scatter_h(g_dy / y_std)),  J = d xn / d x of veh_step_t<true>
// (dy = y - m1y, m1y = rows 0, 1, 3, 4, 5 of xn renormalized by the y statistics; u is not differentiated).
__global__ __launch_bounds__(256) void knet_prior_bwd_kernel(KP p, traj_knet_limits L, float Ts, int B,
                                                             const float* __restrict__ x_post,
                                                             const float* __restrict__ u, const float* __restrict__ xm,
                                                             const float* __restrict__ xs, const float* __restrict__ ys,
                                                             const float* __restrict__ um, const float* __restrict__ us,
                                                             const float* __restrict__ g_prior,
                                                             const float* __restrict__ g_dy,
                                                             float* __restrict__ g_x_post) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float x[6], sd[6], gx[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        sd[i] = xs[i];
        x[i] = __fadd_rn(__fmul_rn(x_post[6 * b + i], sd[i]), xm[i]);   // _denorm_x, as prior_one
        gx[i] = g_prior[6 * b + i] / sd[i];                             // through _renorm_x
    }
    float d = u[2 * b], delta = u[2 * b + 1];
    if (um && us) {
        d = __fadd_rn(__fmul_rn(d, us[0]), um[0]);
        delta = __fadd_rn(__fmul_rn(delta, us[1]), um[1]);
    }
    if (g_dy) {   // dy = y - m1y, m1y_j = (xn[hr[j]] - y_mean_j) / y_std_j
        const int hr[5] = {0, 1, 3, 4, 5};
#pragma unroll
        for (int j = 0; j < 5; ++j) gx[hr[j]] -= g_dy[5 * b + j] / ys[j];
    }
    float xn[6];
    VehJac J;
    veh_step_t<true>(p, L, Ts, x, d, delta, xn, &J);
    float gr[6];   // gradient at the Euler step's raw output: the six clamps after the step
#pragma unroll
    for (int i = 0; i < 6; ++i) gr[i] = gx[i] * J.post[i];
    // xn_raw = x + Ts xdot(phi, vx, vy, omega): X and Y pass through the identity only
    g_x_post[6 * b + 0] = gr[0] * sd[0];
    g_x_post[6 * b + 1] = gr[1] * sd[1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 6; ++i) a = fmaf(gr[i], J.A[i][c], a);
        g_x_post[6 * b + 2 + c] = fmaf(Ts, a, gr[2 + c]) * sd[2 + c];
    }
}

// Backward of knet_gru_kernel: one thread per (row, hidden unit); r, z, n recomputed from gi / gh with the forward's
// expressions.  g = g_out (+ g_out2 when given; both with a row stride, so a slice of a wider matrix is read in place).
__global__ __launch_bounds__(256) void knet_gru_bwd_kernel(int B, int H, const float* __restrict__ gi,
                                                           const float* __restrict__ gh, const float* __restrict__ h,
                                                           const float* __restrict__ g_out, int ld1,
                                                           const float* __restrict__ g_out2, int ld2,
                                                           float* __restrict__ g_gi, float* __restrict__ g_gh,
                                                           float* __restrict__ g_h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, k = i - b * H;
    const size_t o = (size_t)b * 3 * H;
    const float* gib = gi + o;
    const float* ghb = gh + o;
    const float r = sigmoidf_(__fadd_rn(ghb[k], gib[k]));
    const float z = sigmoidf_(__fadd_rn(ghb[H + k], gib[H + k]));
    const float ghn = ghb[2 * H + k];
    const float nn = tanhf(__fadd_rn(gib[2 * H + k], __fmul_rn(ghn, r)));
    float g = g_out[(size_t)b * ld1 + k];
    if (g_out2) g += g_out2[(size_t)b * ld2 + k];
    // h' = (h - n) z + n
    const float gz = g * (h[i] - nn), gn = g * (1.0f - z);
    const float dan = gn * (1.0f - nn * nn);          // through tanh
    const float dar = dan * ghn * (r * (1.0f - r));   // through sigmoid of the r gate
    const float daz = gz * (z * (1.0f - z));
    g_gi[o + k] = dar;
    g_gh[o + k] = dar;
    g_gi[o + H + k] = daz;
    g_gh[o + H + k] = daz;
    g_gi[o + 2 * H + k] = dan;
    g_gh[o + 2 * H + k] = dan * r;
    g_h[i] = g * z;
}

// Backward of knet_update_kernel, one thread per sequence: g = g_post (+ g_post2 when given);
//   g_prior = g, g_KG[i][j] = gamma g_i dy_j, g_dy[j] = gamma sum_i g_i KG[i][j],
//   g_logit[b] = gamma (1 - gamma) sum_i g_i (sum_j KG[i][j] dy_j)   (the caller sums over b)
__global__ __launch_bounds__(256) void knet_update_bwd_kernel(int B, const float* __restrict__ KG,
                                                              const float* __restrict__ dy,
                                                              const float* __restrict__ logit,
                                                              const float* __restrict__ g_post,
                                                              const float* __restrict__ g_post2,
                                                              float* __restrict__ g_prior, float* __restrict__ g_KG,
                                                              float* __restrict__ g_dy, float* __restrict__ g_logit) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float gamma = sigmoidf_(logit[0]);
    const float* K = KG + (size_t)b * 30;
    float e[5], g[6], gd[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 5; ++j) e[j] = dy[5 * b + j];
    float gl = 0.0f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        g[i] = g_post[6 * b + i];
        if (g_post2) g[i] += g_post2[6 * b + i];
        g_prior[6 * b + i] = g[i];
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const float kij = K[5 * i + j];
            s = fmaf(kij, e[j], s);
            gd[j] = fmaf(g[i], kij, gd[j]);
            g_KG[(size_t)b * 30 + 5 * i + j] = gamma * (g[i] * e[j]);
        }
        gl = fmaf(g[i], s, gl);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) g_dy[5 * b + j] = gamma * gd[j];
    g_logit[b] = gamma * (1.0f - gamma) * gl;
}

// Dense-layer epilogue on the way back: g_pre = (g_a + g_b) * dropout mask * (post-activation > 0), every factor
// optional (g_b, mask, act may be NULL); g_a / g_b are read with a row stride, act / mask / g_pre are [rows, cols].
// g_pre may alias g_a when ld_a == cols.
__global__ __launch_bounds__(256) void knet_dense_bwd_kernel(long long n, int cols, const float* g_a, int ld_a,
                                                             const float* __restrict__ g_b, int ld_b,
                                                             const float* __restrict__ act,
                                                             const float* __restrict__ mask, float* g_pre) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    float g = g_a[r * ld_a + c];
    if (g_b) g += g_b[r * ld_b + c];
    if (mask) g *= mask[i];
    if (act) g = act[i] > 0.0f ? g : 0.0f;
    g_pre[i] = g;
}

// Chunk loss of training (pipeline.py:22-60) over the stacked posteriors x_out[b, c, k] = xo[b sb + c sc + k sk] against
// x_tgt [B,6,K] (and y_tgt [B,5,K] when alpha < 1), with its gradient written at the same strides:
//   loss_x = 5/6 mean_{c != phi} (xo - xt)^2 + 1/6 mean wrap(phi_o - phi_t)^2 (phi denormalized),
//   loss   = alpha loss_x + (1 - alpha) mean (xo[c != phi] - y)^2;   grad += g_extra [B,6,K] when given.
// One workgroup: thread t sums elements t, t + 256, ... in float64, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void knet_train_loss_kernel(int B, int K, const float* __restrict__ xo, int sb, int sc,
                                                              int sk, const float* __restrict__ xt,
                                                              const float* __restrict__ yt,
                                                              const float* __restrict__ xm, const float* __restrict__ xs,
                                                              float alpha, const float* __restrict__ g_extra,
                                                              float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ double red[256];
    const long long n = (long long)B * K;
    const double inv_n = 1.0 / (double)n;
    const float m2 = xm[2], s2 = xs[2];
    // d loss / d xo: alpha 5/6 2 d / (5 n) = alpha d / (3 n); phi: alpha 1/6 2 w s2 / n; y term (1 - alpha) 2 e / (5 n)
    const float cx = (float)((double)alpha * inv_n / 3.0), cp = (float)((double)alpha * inv_n / 3.0) * s2;
    const float cy = (float)((1.0 - (double)alpha) * 2.0 * inv_n / 5.0);
    const bool comp = yt != nullptr && alpha < 1.0f;
    double sx = 0.0, sp = 0.0, sy = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const int b = (int)(i / K), k = (int)(i - (long long)b * K);
        const size_t eo = (size_t)b * sb + (size_t)k * sk;
        int j = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const size_t ti = ((size_t)b * 6 + c) * K + k;
            const float o = xo[eo + (size_t)c * sc], t = xt[ti];
            float g;
            if (c == 2) {
                const float df = __fsub_rn(__fadd_rn(__fmul_rn(o, s2), m2), __fadd_rn(__fmul_rn(t, s2), m2));
                const float w = atan2f(sinf(df), cosf(df));
                sp += (double)w * (double)w;
                g = cp * w;
            } else {
                const float df = __fsub_rn(o, t);
                sx += (double)df * (double)df;
                g = cx * df;
                if (comp) {
                    const float e = __fsub_rn(o, yt[((size_t)b * 5 + j) * K + k]);
                    sy += (double)e * (double)e;
                    g = fmaf(cy, e, g);
                }
                ++j;
            }
            if (g_extra) g += g_extra[ti];
            grad[eo + (size_t)c * sc] = g;
        }
    }
    double tot = (double)alpha * ((5.0 / 6.0) * (sx / 5.0) + (1.0 / 6.0) * sp) * inv_n;
    if (comp) tot += (1.0 - (double)alpha) * (sy / 5.0) * inv_n;
    red[threadIdx.x] = tot;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
}

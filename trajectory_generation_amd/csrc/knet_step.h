// knet_step.h -- the fused step's kernels around FC2 (traj_knet_front_f32, traj_knet_back_f32,
// traj_knet_back_front_f32): front, back, and back(t) + front(t + 1) in one launch.  Included by knet.hip inside its
// anonymous namespace, after knet_vehicle.h (prior_one, posterior_one) and knet_dense.h (the layers).

// The pieces the back-front kernel shares with the back kernel (staging, slab sum, h_Sigma store) and with the front
// kernel (the last store).  b0: the workgroup's first sequence, nb: how many of its KS are below B, t: the thread.

// back's staging: x2 = [out_Sigma | h_S] k-major into s_b[0, KH) and s_a[0, KH) (sequences past B: zero), and the zero
// rows behind them that pad FC4's input (s_b rows KH .. KH + 63) and FC3's (s_a rows KH + 32 .. KH + 63)
__device__ __forceinline__ void back_stage_x2(const float* __restrict__ x2, int b0, int nb, float* s_a, float* s_b,
                                              int t) {
    for (int i = t; i < KS * 2 * KH; i += KT) {
        const int s = i / (2 * KH), k = i - s * 2 * KH;
        const float v = (s < nb) ? x2[(size_t)(b0 + s) * 2 * KH + k] : 0.0f;
        if (k < KH) s_b[k * KS + s] = v;
        else s_a[(k - KH) * KS + s] = v;
    }
    for (int i = t; i < 64 * KS; i += KT) s_b[KH * KS + i] = 0.0f;
    for (int i = t; i < 32 * KS; i += KT) s_a[(KH + 32) * KS + i] = 0.0f;
}

// KG = b2b + sum over FC2's slabs into s_a rows KH .. KH + 31 (rows >= n m and sequences past B: zero), and to KG_out
// when given.  Two stages, a barrier after each: thread (s, j, q) sums the slabs sl = q mod 4 into s_red[s][j][q],
// then thread (s, j) adds the four.
__device__ __forceinline__ void back_slab_sum(const float* __restrict__ b2b, int nm, int B,
                                              const float* __restrict__ part, int nslab, int b0, int nb,
                                              float (&s_red)[KS][32][4], float* s_a, float* KG_out, int t) {
    {
        const int s = t >> 7, j = (t >> 2) & 31, q = t & 3;
        float a = 0.0f;
        if (s < nb) {
            const float* pp = part + ((size_t)b0 + s) * 32 + j;
#pragma unroll 8
            for (int sl = q; sl < nslab; sl += 4) a = __fadd_rn(a, pp[(size_t)sl * B * 32]);
        }
        s_red[s][j][q] = a;
    }
    __syncthreads();
    if (t < KS * 32) {
        const int s = t >> 5, j = t & 31;
        float v = 0.0f;
        if (j < nm && s < nb) {
            v = __fadd_rn(b2b[j], __fadd_rn(__fadd_rn(s_red[s][j][0], s_red[s][j][1]),
                                            __fadd_rn(s_red[s][j][2], s_red[s][j][3])));
            if (KG_out) KG_out[(size_t)(b0 + s) * nm + j] = v;
        }
        s_a[(KH + j) * KS + s] = v;
    }
    __syncthreads();
}

// the new h_Sigma (FC4's output, k-major in s_o) to its rows
__device__ __forceinline__ void store_hsig(float* hSig, const float* s_o, int b0, int nb, int t) {
    for (int i = t; i < nb * KH; i += KT) {
        const int s = i / KH, k = i - s * KH;
        hSig[(size_t)(b0 + s) * KH + k] = s_o[k * KS + s];
    }
}

// front's results to their rows: the new h_Q and h_S, and x2 = [out_Sigma | h_S] for FC2
__device__ __forceinline__ void store_front(float* hQ, float* hS, float* x2, const float* s_q, const float* s_g,
                                            const float* s_hs, int b0, int nb, int t) {
    for (int i = t; i < nb * KH; i += KT) {
        const int s = i / KH, k = i - s * KH;
        const size_t b = (size_t)(b0 + s);
        hQ[b * KH + k] = s_q[k * KS + s];
        hS[b * KH + k] = s_hs[k * KS + s];
        x2[b * 2 * KH + k] = s_g[k * KS + s];
        x2[b * 2 * KH + KH + k] = s_hs[k * KS + s];
    }
}

__device__ __forceinline__ void front_body(KP p, traj_knet_limits L, float Ts, KNet net, int B,
                                           const float* __restrict__ x_post, const float* __restrict__ u, int u_sb,
                                           int u_sc, const float* __restrict__ y, int y_sb, int y_sc,
                                           const float* __restrict__ xm, const float* __restrict__ xs,
                                           const float* __restrict__ ym, const float* __restrict__ ys,
                                           const float* __restrict__ um, const float* __restrict__ us, float* hQ,
                                           const float* hSig, float* hS, float* prior, float* dy, float* x2) {
    __shared__ __attribute__((aligned(16))) float s_h[3][KH * KS];   // h_Q, h_Sigma, h_S (inputs), k-major
    __shared__ __attribute__((aligned(16))) float s_q[KH * KS];      // new h_Q
    __shared__ __attribute__((aligned(16))) float s_g[KH * KS];      // out_Sigma
    __shared__ __attribute__((aligned(16))) float s_hs[KH * KS];     // new h_S
    __shared__ __attribute__((aligned(16))) float s_pr[64 * KS];     // prior, zero-padded to k4_
    __shared__ __attribute__((aligned(16))) float s_dy[64 * KS];     // innovation, zero-padded
    __shared__ __attribute__((aligned(16))) float s_o5[64 * KS];     // FC5 output, zero-padded
    __shared__ __attribute__((aligned(16))) float s_c1[64 * KS];     // [FC1 | FC7], zero-padded
    __shared__ __attribute__((aligned(16))) float s_x[KQ * KH * 6 * KS];   // K-quarter partial sums
    const int t = threadIdx.x, b0 = blockIdx.x * KS;
    const int nb = min(KS, B - b0);
    for (int i = t; i < 3 * KS * KH; i += KT) {   // coalesced row reads -> k-major LDS
        const int w = i / (KS * KH), r = i - w * KS * KH, s = r / KH, k = r - s * KH;
        const float* src = (w == 0) ? hQ : (w == 1 ? hSig : hS);
        s_h[w][k * KS + s] = (s < nb) ? src[(size_t)(b0 + s) * KH + k] : 0.0f;
    }
    if (t < 64 * KS) s_o5[t] = s_c1[t] = s_pr[t] = s_dy[t] = 0.0f;
    __syncthreads();
    if (t < KS) {
        float pr[6] = {0, 0, 0, 0, 0, 0}, e[5] = {0, 0, 0, 0, 0};
        if (t < nb) {
            const int b = b0 + t;
            prior_one(p, L, Ts, x_post + 6 * b, u[(size_t)b * u_sb], u[(size_t)b * u_sb + u_sc], y + (size_t)b * y_sb,
                      y_sc, xm, xs, ym, ys, um, us, pr, nullptr, e);
            for (int i = 0; i < 6; ++i) prior[6 * b + i] = pr[i];
            for (int j = 0; j < 5; ++j) dy[5 * b + j] = e[j];
        }
        for (int i = 0; i < 6; ++i) s_pr[i * KS + t] = pr[i];
        for (int j = 0; j < 5; ++j) s_dy[j * KS + t] = e[j];
    }
    __syncthreads();
    dense_ks(s_pr, k4_(net.m), net.W5, net.b5, net.dFC5, s_o5, true, s_x, t);                    // FC5 + ReLU
    gru_ks(s_o5, k4_(net.dFC5), s_h[0], net.WiQ, net.biQ, net.WhQ, net.bhQ, s_q, s_x, t);        // GRU_Q
    gru_ks(s_q, KH / 4, s_h[1], net.WiG, net.biG, net.WhG, net.bhG, s_g, s_x, t);               // GRU_Sigma
    dense_ks(s_g, KH / 4, net.W1, net.b1, net.dFC1, s_c1, true, s_x, t);                         // FC1 + ReLU
    dense_ks(s_dy, k4_(net.n), net.W7, net.b7, net.dFC7, s_c1 + KS * net.dFC1, true, s_x, t);    // FC7 + ReLU
    gru_ks(s_c1, k4_(net.dFC1 + net.dFC7), s_h[2], net.WiS, net.biS, net.WhS, net.bhS, s_hs, s_x, t);   // GRU_S
    store_front(hQ, hS, x2, s_q, s_g, s_hs, b0, nb, t);
}

__device__ __forceinline__ void back_body(KNet net, int B, const float* __restrict__ x2,
                                          const float* __restrict__ part, int nslab, const float* __restrict__ prior,
                                          const float* __restrict__ dy, float* hSig, float* x_post, float* out,
                                          int o_sb, int o_sc, float* KG_out) {
    __shared__ __attribute__((aligned(16))) float s_a[(KH + 64) * KS];    // [h_S | KG | 0]: FC3's input
    __shared__ __attribute__((aligned(16))) float s_b[(KH + 64) * KS];    // [out_Sigma | FC3 | 0]: FC4's input
    __shared__ __attribute__((aligned(16))) float s_o[KH * KS];           // FC4 output (new h_Sigma)
    __shared__ __attribute__((aligned(16))) float s_x[(KQ - 1) * KH * KS];   // K-quarter partial sums
    __shared__ float s_red[KS][32][4];
    const int t = threadIdx.x, b0 = blockIdx.x * KS;
    const int nb = min(KS, B - b0);
    const int nm = net.n * net.m;
    back_stage_x2(x2, b0, nb, s_a, s_b, t);
    back_slab_sum(net.b2b, nm, B, part, nslab, b0, nb, s_red, s_a, KG_out, t);
    // FC3 + ReLU on cat(h_S, out_FC2); FC4 + ReLU on cat(out_Sigma, out_FC3) = the new h_Sigma
    dense_ks(s_a, k4_(KH + nm), net.W3, net.b3, net.dFC3, s_b + KH * KS, true, s_x, t);
    dense_ks(s_b, k4_(KH + net.dFC3), net.W4, net.b4, KH, s_o, true, s_x, t);
    store_hsig(hSig, s_o, b0, nb, t);
    if (t < nb) {   // posterior (kalman_net.py:169-178), as knet_update_kernel
        // (posterior_one's sum written out: with the net's m / n as bounds the shared form allocates one SGPR fewer)
        const int b = b0 + t;
        const float gamma = sigmoidf_(net.logit[0]);
        for (int i = 0; i < net.m; ++i) {
            float sacc = 0.0f;
            for (int j = 0; j < net.n; ++j)
                sacc = __fadd_rn(sacc, __fmul_rn(s_a[(KH + net.n * i + j) * KS + t], dy[5 * b + j]));
            const float v = __fadd_rn(prior[6 * b + i], __fmul_rn(gamma, sacc));
            x_post[6 * b + i] = v;
            if (out) out[(size_t)b * o_sb + (size_t)i * o_sc] = v;
        }
    }
}

__global__ __launch_bounds__(KT) void knet_front_kernel(KP p, traj_knet_limits L, float Ts, KNet net, int B,
                                                        const float* x_post, const float* u, int u_sb, int u_sc,
                                                        const float* y, int y_sb, int y_sc, const float* xm,
                                                        const float* xs, const float* ym, const float* ys,
                                                        const float* um, const float* us, float* hQ, const float* hSig,
                                                        float* hS, float* prior, float* dy, float* x2) {
    front_body(p, L, Ts, net, B, x_post, u, u_sb, u_sc, y, y_sb, y_sc, xm, xs, ym, ys, um, us, hQ, hSig, hS, prior, dy,
               x2);
}

__global__ __launch_bounds__(KT) void knet_back_kernel(KNet net, int B, const float* x2, const float* part, int nslab,
                                                       const float* prior, const float* dy, float* hSig, float* x_post,
                                                       float* out, int o_sb, int o_sc, float* KG_out) {
    back_body(net, B, x2, part, nslab, prior, dy, hSig, x_post, out, o_sb, o_sc, KG_out);
}

// back(t) and front(t + 1) in one launch: a workgroup finishes step t of its four sequences and goes
// straight on to step t + 1 -- one launch and one workgroup start per step fewer, h_Sigma(t) handed
// over in LDS, and the posterior x_post(t) (it needs FC2's output, not FC3/FC4) plus step t + 1's prior
// computed by four threads that FC3 leaves idle (units >= d_fc3) while the others run FC3.  Each
// workgroup reads and writes only its own sequences' rows.  Bit-identical to back(t) + front(t + 1).
__global__ __launch_bounds__(KT) void knet_back_front_kernel(KNet net, int B, const float* __restrict__ part,
                                                             int nslab, float* __restrict__ out, int o_sb, int o_sc,
                                                             KP p, traj_knet_limits L, float Ts,
                                                             const float* __restrict__ u, int u_sb, int u_sc,
                                                             const float* __restrict__ y, int y_sb, int y_sc,
                                                             const float* __restrict__ xm, const float* __restrict__ xs,
                                                             const float* __restrict__ ym, const float* __restrict__ ys,
                                                             const float* __restrict__ um, const float* __restrict__ us,
                                                             float* __restrict__ hQ, float* __restrict__ hSig,
                                                             float* __restrict__ hS, float* __restrict__ x_post,
                                                             float* __restrict__ prior, float* __restrict__ dy,
                                                             float* __restrict__ x2) {
    __shared__ __attribute__((aligned(16))) float s_a[(KH + 64) * KS];    // [h_S(t) | KG | 0]: FC3's input
    __shared__ __attribute__((aligned(16))) float s_b[(KH + 64) * KS];    // [out_Sigma(t) | FC3 | 0]: FC4's input
    __shared__ __attribute__((aligned(16))) float s_o[KH * KS];           // FC4 output = h_Sigma(t)
    __shared__ __attribute__((aligned(16))) float s_hq[KH * KS];          // h_Q(t)
    __shared__ __attribute__((aligned(16))) float s_q[KH * KS];           // h_Q(t + 1)
    __shared__ __attribute__((aligned(16))) float s_g[KH * KS];           // out_Sigma(t + 1)
    __shared__ __attribute__((aligned(16))) float s_hs[KH * KS];          // h_S(t + 1)
    __shared__ __attribute__((aligned(16))) float s_pr[64 * KS];          // prior(t + 1), zero-padded
    __shared__ __attribute__((aligned(16))) float s_dy[64 * KS];          // innovation(t + 1), zero-padded
    __shared__ __attribute__((aligned(16))) float s_o5[64 * KS];          // FC5 output, zero-padded
    __shared__ __attribute__((aligned(16))) float s_c1[64 * KS];          // [FC1 | FC7], zero-padded
    __shared__ __attribute__((aligned(16))) float s_x[KQ * KH * 6 * KS];  // K-quarter partial sums
    __shared__ float s_red[KS][32][4];
    __shared__ __attribute__((aligned(16))) float s_x4[(KQ - 1) * KH * KS];  // FC4's partials (beside GRU_Q's)
    const int t = threadIdx.x, b0 = blockIdx.x * KS;
    const int nb = min(KS, B - b0);
    const int nm = net.n * net.m;
    // ---- staging: x2(t) = [out_Sigma | h_S] and h_Q(t), k-major
    back_stage_x2(x2, b0, nb, s_a, s_b, t);
    for (int i = t; i < KS * KH; i += KT) {
        const int s = i / KH, k = i - s * KH;
        s_hq[k * KS + s] = (s < nb) ? hQ[(size_t)(b0 + s) * KH + k] : 0.0f;
    }
    if (t < 64 * KS) s_o5[t] = s_c1[t] = s_pr[t] = s_dy[t] = 0.0f;
    back_slab_sum(net.b2b, nm, B, part, nslab, b0, nb, s_red, s_a, nullptr, t);
    // ---- posterior x_post(t) (kalman_net.py:169-178) and step t + 1's prior (:145-162): threads
    // KT - KS .. KT - 1 (K quarter 3, units 124..127: idle in FC3), overlapping FC3
    if (t >= KT - KS) {
        const int s = t - (KT - KS);
        float pr[6] = {0, 0, 0, 0, 0, 0}, e[5] = {0, 0, 0, 0, 0};
        if (s < nb) {
            const int b = b0 + s;
            const float gamma = sigmoidf_(net.logit[0]);
            float xp[6];
            for (int i = 0; i < 6; ++i) {
                xp[i] = posterior_one(s_a + (KH + 5 * i) * KS + s, KS, 5, dy + 5 * b, prior[6 * b + i], gamma);
                x_post[6 * b + i] = xp[i];
                out[(size_t)b * o_sb + (size_t)i * o_sc] = xp[i];
            }
            prior_one(p, L, Ts, xp, u[(size_t)b * u_sb], u[(size_t)b * u_sb + u_sc], y + (size_t)b * y_sb, y_sc, xm,
                      xs, ym, ys, um, us, pr, nullptr, e);
            for (int i = 0; i < 6; ++i) prior[6 * b + i] = pr[i];
            for (int j = 0; j < 5; ++j) dy[5 * b + j] = e[j];
        }
        for (int i = 0; i < 6; ++i) s_pr[i * KS + s] = pr[i];
        for (int j = 0; j < 5; ++j) s_dy[j * KS + s] = e[j];
    }
    // ---- back(t): FC3 + ReLU on cat(h_S, out_FC2); FC4 + ReLU on cat(out_Sigma, out_FC3) = h_Sigma(t).
    // FC3 has at most 64 units, so units 64..127 are idle once its partials are published: there they
    // run step t + 1's FC5 (on the prior) and FC7 (on the innovation), one output per thread, instead of
    // two more layer stages after FC4.
    // (fc57's loop strides over any number of FC5 / FC7 outputs: in_mult 10's 60 + 5 units included)
    const bool side = net.dFC3 <= 64 && net.m <= 16 && net.n <= 16;
    auto fc57 = [&]() {
        if (!side || (t & (KH - 1)) < 64) return;
        const int i = (t >> 7) * 64 + (t & 63);
        for (int o = i; o < (net.dFC5 + net.dFC7) * KS; o += KT / 2) {
            const int s = o & (KS - 1), unit = o / KS;
            if (unit < net.dFC5) s_o5[unit * KS + s] = dense_one(s_pr, net.m, net.W5, net.b5, net.dFC5, unit, s);
            else {
                const int v = unit - net.dFC5;
                s_c1[(net.dFC1 + v) * KS + s] = dense_one(s_dy, net.n, net.W7, net.b7, net.dFC7, v, s);
            }
        }
    };
    dense_ks(s_a, k4_(KH + nm), net.W3, net.b3, net.dFC3, s_b + KH * KS, true, s_x, t, fc57);
    // ---- front(t + 1): FC5, GRU_Q, GRU_Sigma (on h_Sigma(t) in LDS), FC1, FC7, GRU_S (on h_S(t) = s_a[0, KH)).
    // With FC5 done above, GRU_Q(t + 1) does not wait for FC4(t): the two share one stage (both
    // publish their quarter partials, one barrier, both finish).
    if (side) {
        const float4 r4 = dense_publish(s_b, k4_(KH + net.dFC3), net.W4, net.b4, KH, s_x4, t);
        gru_publish(s_o5, k4_(net.dFC5), s_hq, net.WiQ, net.biQ, net.WhQ, net.bhQ, s_x, t);
        __syncthreads();
        dense_finish(r4, KH, s_o, true, s_x4, t);
        gru_finish(s_hq, s_q, s_x, t);
        __syncthreads();
    } else {
        dense_ks(s_b, k4_(KH + net.dFC3), net.W4, net.b4, KH, s_o, true, s_x, t);
        dense_ks(s_pr, k4_(net.m), net.W5, net.b5, net.dFC5, s_o5, true, s_x, t);                // FC5 + ReLU
        gru_ks(s_o5, k4_(net.dFC5), s_hq, net.WiQ, net.biQ, net.WhQ, net.bhQ, s_q, s_x, t);      // GRU_Q
    }
    store_hsig(hSig, s_o, b0, nb, t);
    gru_ks(s_q, KH / 4, s_o, net.WiG, net.biG, net.WhG, net.bhG, s_g, s_x, t);     // GRU_Sigma
    dense_ks(s_g, KH / 4, net.W1, net.b1, net.dFC1, s_c1, true, s_x, t);           // FC1 + ReLU
    if (!side) dense_ks(s_dy, k4_(net.n), net.W7, net.b7, net.dFC7, s_c1 + KS * net.dFC1, true, s_x, t);   // FC7
    gru_ks(s_c1, k4_(net.dFC1 + net.dFC7), s_a, net.WiS, net.biS, net.WhS, net.bhS, s_hs, s_x, t);   // GRU_S
    store_front(hQ, hS, x2, s_q, s_g, s_hs, b0, nb, t);
}

// knet_ops.h -- one KalmanNet step op by op (traj_knet_prior_f32, traj_knet_gru_gates_f32, traj_knet_update_f32), the
// element-wise parts around the library GEMMs: one thread per sequence for the prior and the posterior, one per hidden
// unit for the GRU gates.  Included by knet.hip inside its anonymous namespace, after knet_vehicle.h.

__global__ __launch_bounds__(256) void knet_prior_kernel(KP p, traj_knet_limits L, float Ts, int B,
                                                         const float* __restrict__ x_post, const float* __restrict__ u,
                                                         const float* __restrict__ y, const float* __restrict__ xm,
                                                         const float* __restrict__ xs, const float* __restrict__ ym,
                                                         const float* __restrict__ ys, const float* __restrict__ um,
                                                         const float* __restrict__ us, float* __restrict__ m1x_prior,
                                                         float* __restrict__ m1y, float* __restrict__ dy) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    prior_one(p, L, Ts, x_post + 6 * b, u[2 * b], u[2 * b + 1], y ? y + 5 * b : nullptr, 1, xm, xs, ym, ys, um, us,
              m1x_prior + 6 * b, m1y + 5 * b, dy ? dy + 5 * b : nullptr);
}

__global__ __launch_bounds__(256) void knet_gru_kernel(int B, int H, const float* __restrict__ gi,
                                                       const float* __restrict__ gh, const float* h,
                                                       float* h_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, k = i - b * H;
    const float* gib = gi + (size_t)b * 3 * H;
    const float* ghb = gh + (size_t)b * 3 * H;
    // ATen GRUCell: r = sigmoid(h_r + i_r), z = sigmoid(h_z + i_z), n = tanh(i_n + h_n * r),
    // h' = (h - n) * z + n
    const float r = sigmoidf_(__fadd_rn(ghb[k], gib[k]));
    const float z = sigmoidf_(__fadd_rn(ghb[H + k], gib[H + k]));
    const float nn = tanhf(__fadd_rn(gib[2 * H + k], __fmul_rn(ghb[2 * H + k], r)));
    const float hv = h[i];
    h_out[i] = __fadd_rn(__fmul_rn(__fsub_rn(hv, nn), z), nn);
}

__global__ __launch_bounds__(256) void knet_update_kernel(int B, const float* __restrict__ xp,
                                                          const float* __restrict__ KG, const float* __restrict__ dy,
                                                          const float* __restrict__ logit, float* __restrict__ xo) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float gamma = sigmoidf_(logit[0]);
    const float* K = KG + (size_t)b * 30;
    const float* e = dy + (size_t)b * 5;
#pragma unroll
    for (int i = 0; i < 6; ++i) xo[6 * b + i] = posterior_one(K + 5 * i, 1, 5, e, xp[6 * b + i], gamma);
}

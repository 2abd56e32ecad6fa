// knet_dense.h -- the fused step's (throughput path's) building blocks: the packed weight layout and its pack kernel,
// the split dot product, the dense layers and the GRU cells of one workgroup.  Included by knet.hip inside its
// anonymous namespace, after knet_vehicle.h (sigmoidf_); knet_step.h puts the pieces together.
//
// One KalmanNet step in two kernels around FC2 (kalman_net.py:145-216, eval mode):
//   front: prior -> FC5 -> GRU_Q -> GRU_Sigma -> FC1, FC7 -> GRU_S, writing x2 = [out_Sigma | h_S]
//          (FC2's input) and the hidden states;
//   back:  FC3 -> FC4 (the new h_Sigma) -> posterior update, from FC2's output KG.
// A workgroup owns KS sequences through every layer (no cross-workgroup dependency); activations stay
// in LDS, weights stream from L2 in the packed layout P[k4][j][4] = W[j][4 k4 + c] (zero past K), so
// the lanes of a wave (consecutive outputs j) read one contiguous 1 KiB run per float4 load.  GRU
// cells: a thread per hidden unit and K quarter forms the six gate dot products over its quarter; the
// thread (unit, quarter q) then adds the four quarters' partials of sequence q and applies torch's GRU
// gate math (as knet_gru_kernel).  Every dot product is a k-ordered fmaf chain
// started at the bias: float32 results within rounding of the library GEMM path.
constexpr int KS = 4;        // sequences per workgroup
constexpr int KH = 128;      // hidden size (hidden_dim_gru)
constexpr int KQ = 4;        // K parts of every dot product (thread t: unit t & 127, part t >> 7)
constexpr int KT = KH * KQ;  // threads per workgroup: 8 waves, two per SIMD

struct KNet {
    int m, n, dFC5, dFC1, dFC7, dFC3;
    const float *b5, *biQ, *bhQ, *biG, *bhG, *b1, *b7, *biS, *bhS, *b3, *b4, *logit, *b2b;
    const float4 *W5, *WiQ, *WhQ, *WiG, *WhG, *W1, *W7, *WiS, *WhS, *W3, *W4;   // packed
};

// packed rows of 4 k per matrix: K rounded up to a multiple of 64 (zero weights past K), so that each
// quarter of a split dot product runs a whole number of KD-row prefetch groups
__host__ __device__ inline int k4_(int K) { return ((K + 63) / 64) * 16; }

// Packed-buffer offsets (in floats) of the eleven matrices, in the order of traj_knet_net.
struct PackPlan {
    int N[11], K[11];
    size_t off[12];
};
static PackPlan pack_plan(const traj_knet_net* w) {
    PackPlan pl{};
    const int H = w->hidden;
    const int N[11] = {w->d_fc5, 3 * H, 3 * H, 3 * H, 3 * H, w->d_fc1, w->d_fc7, 3 * H, 3 * H, w->d_fc3, H};
    const int K[11] = {w->m, w->d_fc5, H, H, H, H, w->n, w->d_fc1 + w->d_fc7, H, H + w->n * w->m, H + w->d_fc3};
    pl.off[0] = 0;
    for (int i = 0; i < 11; ++i) {
        pl.N[i] = N[i];
        pl.K[i] = K[i];
        pl.off[i + 1] = pl.off[i] + (size_t)4 * k4_(K[i]) * N[i];
    }
    return pl;
}

__global__ void knet_pack_kernel(const float* __restrict__ W, int N, int K, float* __restrict__ P) {
    const int K4 = k4_(K);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)K4 * N * 4) return;
    const int c = (int)(i & 3), j = (int)((i >> 2) % N), k4 = (int)((i >> 2) / N);
    const int k = 4 * k4 + c;
    P[i] = k < K ? W[(size_t)j * K + k] : 0.0f;
}

// Activations live in LDS k-major, xT[k][KS] (one float4 = the KS sequences' k-th input), rows
// zero-padded to a multiple of 4.  Dot products are split over K between the four quarters of the
// workgroup (thread t: output / hidden unit t & 127, K quarter t >> 7) and the quarters' partial sums
// are added through LDS in quarter order; weight loads run KD float4 rows ahead of the FMAs, and the
// two waves of each SIMD cover each other's L2 latency.
constexpr int KD = 4;   // (8 rows in flight for the GRU cells' 8-row quarters measured 71 vs 63 us per step, round 5)

// acc[g][s] += sum_{k4 in [k4b, k4e)} xT[4 k4 + c][s] * P[k4][j + g * KH][c]  (P rows: NR per k4).
// Measured on MI355X (front launch, B = 1024): this compact runtime loop 24.7 us; the same loop with
// compile-time trip counts 27.5 us; fully unrolled straight-line code 29.4 us (register spills); a
// cross-layer chained prefetch gave nothing -- the chain is bound by per-layer barrier / LDS / load
// latency, not by one stalled group.
typedef float f2v __attribute__((ext_vector_type(2)));

template <int G>
__device__ __forceinline__ void dot_ks(const float* xT, int k4b, int k4e, const float4* __restrict__ P, int NR, int j,
                                       float (&acc)[G][KS]) {
    // sequence pairs as packed f32 operands: v_pk_fma_f32 with the weight broadcast to both halves, the pairs straight
    // from the LDS float4s and the accumulators -- no register moves to assemble operand pairs.  Per accumulator it is
    // the scalar chain fmaf(x3, w.w, fmaf(x2, w.z, fmaf(x1, w.y, fmaf(x0, w.x, acc)))), same k order, bit for bit.
    f2v a2[G][2];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        a2[g][0] = f2v{acc[g][0], acc[g][1]};
        a2[g][1] = f2v{acc[g][2], acc[g][3]};
    }
    float4 wb[KD][G];
#pragma unroll
    for (int d = 0; d < KD; ++d)
#pragma unroll
        for (int g = 0; g < G; ++g) wb[d][g] = P[(size_t)(k4b + d) * NR + j + g * KH];
    for (int k4 = k4b; k4 < k4e; k4 += KD) {
#pragma unroll
        for (int d = 0; d < KD; ++d) {
            const int kk = k4 + d;
            const float4* xr = reinterpret_cast<const float4*>(xT + 4 * KS * kk);
            const float4 x0 = xr[0], x1 = xr[1], x2 = xr[2], x3 = xr[3];   // k = 4kk .. 4kk+3, KS seqs each
            float4 w[G];
#pragma unroll
            for (int g = 0; g < G; ++g) w[g] = wb[d][g];
            const int kn = min(kk + KD, k4e - 1);   // past the range: a harmless reload of the last row
#pragma unroll
            for (int g = 0; g < G; ++g) wb[d][g] = P[(size_t)kn * NR + j + g * KH];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const f2v xs[4][2] = {{f2v{x0.x, x0.y}, f2v{x0.z, x0.w}}, {f2v{x1.x, x1.y}, f2v{x1.z, x1.w}},
                                      {f2v{x2.x, x2.y}, f2v{x2.z, x2.w}}, {f2v{x3.x, x3.y}, f2v{x3.z, x3.w}}};
                const float wc[4] = {w[g].x, w[g].y, w[g].z, w[g].w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        a2[g][h] = __builtin_elementwise_fma(xs[c][h], f2v{wc[c], wc[c]}, a2[g][h]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        acc[g][0] = a2[g][0].x;
        acc[g][1] = a2[g][0].y;
        acc[g][2] = a2[g][1].x;
        acc[g][3] = a2[g][1].y;
    }
}

constexpr int K4_H = KH / 4;   // rows of 4 of every W_hh

struct NoSide {
    __device__ void operator()() const {}
};

// One output of a small dense layer (K <= 16: the whole row in quarter 0 of dense_ks) by a single
// thread, bit-identical to dense_ks: the fmaf chain in k order from the bias, then the three zero
// partials of the other quarters (which turn a -0 into +0), then ReLU.  P: packed as dense_ks reads it.
__device__ __forceinline__ float dense_one(const float* xT, int K, const float4* __restrict__ P,
                                           const float* __restrict__ bias, int N, int j, int s) {
    float acc = bias[j];
    for (int k4 = 0; 4 * k4 < K; ++k4) {
        const float4 w = P[(size_t)k4 * N + j];
        const float* x = xT + 4 * KS * k4 + s;
        acc = fmaf(x[0], w.x, acc);
        if (4 * k4 + 1 < K) acc = fmaf(x[KS], w.y, acc);
        if (4 * k4 + 2 < K) acc = fmaf(x[2 * KS], w.z, acc);
        if (4 * k4 + 3 < K) acc = fmaf(x[3 * KS], w.w, acc);
    }
    return fmaxf(__fadd_rn(acc, 0.0f), 0.0f);
}

// First half of dense_ks: quarter `part` of unit j's dot product; quarters 1..3 publish their partial
// to xch, quarter 0 keeps it (returned) for dense_finish after the barrier.
__device__ __forceinline__ float4 dense_publish(const float* xT, int K4, const float4* __restrict__ P,
                                                const float* __restrict__ bias, int N, float* xch, int t) {
    const int j = t & (KH - 1), part = t >> 7, h4 = K4 / KQ;
    float acc[1][KS] = {{0.0f, 0.0f, 0.0f, 0.0f}};
    if (j < N) {
        if (part == 0) acc[0][0] = acc[0][1] = acc[0][2] = acc[0][3] = bias[j];
        dot_ks<1>(xT, part * h4, (part + 1) * h4, P, N, j, acc);
        if (part)
            *reinterpret_cast<float4*>(xch + ((part - 1) * KH + j) * KS) =
                make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
    }
    return make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
}

// Second half (after a barrier that follows dense_publish): quarter 0 adds the other quarters' partials in quarter
// order, applies the activation and writes outT.
__device__ __forceinline__ void dense_finish(float4 r, int N, float* outT, bool relu, const float* xch, int t) {
    const int j = t & (KH - 1), part = t >> 7;
    if (j < N && part == 0) {
#pragma unroll
        for (int q = 1; q < KQ; ++q) {
            const float4 o = *reinterpret_cast<const float4*>(xch + ((q - 1) * KH + j) * KS);
            r = make_float4(__fadd_rn(r.x, o.x), __fadd_rn(r.y, o.y), __fadd_rn(r.z, o.z), __fadd_rn(r.w, o.w));
        }
        if (relu) r = make_float4(fmaxf(r.x, 0.0f), fmaxf(r.y, 0.0f), fmaxf(r.z, 0.0f), fmaxf(r.w, 0.0f));
        *reinterpret_cast<float4*>(outT + KS * j) = r;
    }
}

// Dense layer: outT[j][s] = act(b[j] + sum_k xT[k][s] W[j][k]) for j < N <= KH (outT: LDS, k-major).
// xch: LDS scratch of (KQ - 1) * KH * KS floats.  Called by every thread of the workgroup.  `side` runs
// on every thread between the two barriers (after the partial sums are published, while quarter 0
// finishes): work for the threads the layer leaves idle there (units >= N).
template <class Side = NoSide>
__device__ __forceinline__ void dense_ks(const float* xT, int K4, const float4* __restrict__ P,
                                         const float* __restrict__ bias, int N, float* outT, bool relu, float* xch,
                                         int t, Side side = {}) {
    const float4 r = dense_publish(xT, K4, P, bias, N, xch, t);
    __syncthreads();
    side();
    dense_finish(r, N, outT, relu, xch, t);
    __syncthreads();
}

// GRU cell (torch.nn.GRU, one layer, one step) for the KS sequences: xT [K][KS], hT [KH][KS] -> houtT.
// Thread (unit u, quarter q) forms its quarter's partial gates for all KS sequences, then finishes
// sequence q from the four quarters' partials (added in quarter order).  xch: LDS scratch of
// KQ * KH * 6 * KS floats.
__device__ __forceinline__ void gru_publish(const float* xT, int K4, const float* hT, const float4* __restrict__ Wi,
                                            const float* __restrict__ bi, const float4* __restrict__ Wh,
                                            const float* __restrict__ bh, float* xch, int t) {
    static_assert(KQ == KS, "one finished sequence per K quarter");
    const int u = t & (KH - 1), part = t >> 7;
    float gi[3][KS], gh[3][KS];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            gi[g][q] = part ? 0.0f : bi[g * KH + u];
            gh[g][q] = part ? 0.0f : bh[g * KH + u];
        }
    const int hi = K4 / KQ, hh = K4_H / KQ;
    dot_ks<3>(xT, part * hi, (part + 1) * hi, Wi, 3 * KH, u, gi);
    dot_ks<3>(hT, part * hh, (part + 1) * hh, Wh, 3 * KH, u, gh);
    // publish: xch[part][u][sequence][gi r z n | gh r z n]
    float* mine = xch + (size_t)(part * KH + u) * 6 * KS;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
        *reinterpret_cast<float2*>(mine + 6 * q) = make_float2(gi[0][q], gi[1][q]);
        *reinterpret_cast<float2*>(mine + 6 * q + 2) = make_float2(gi[2][q], gh[0][q]);
        *reinterpret_cast<float2*>(mine + 6 * q + 4) = make_float2(gh[1][q], gh[2][q]);
    }
}

// Second half of the GRU cell (after a barrier that follows gru_publish): thread (unit u, quarter q)
// adds the four quarters' partials of sequence q in quarter order and applies the gates.
__device__ __forceinline__ void gru_finish(const float* hT, float* houtT, const float* xch, int t) {
    const int u = t & (KH - 1), part = t >> 7;
    const int sq = part;   // the sequence this thread finishes
    float ir[3] = {0.0f, 0.0f, 0.0f}, hr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const float* o = xch + (size_t)(q * KH + u) * 6 * KS + 6 * sq;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            ir[g] = q ? __fadd_rn(ir[g], o[g]) : o[g];
            hr[g] = q ? __fadd_rn(hr[g], o[3 + g]) : o[3 + g];
        }
    }
    // ATen GRUCell: r = sigmoid(h_r + i_r), z = sigmoid(h_z + i_z), n = tanh(i_n + h_n * r), h' = (h - n) z + n
    const float r = sigmoidf_(__fadd_rn(hr[0], ir[0]));
    const float z = sigmoidf_(__fadd_rn(hr[1], ir[1]));
    const float nn = tanhf(__fadd_rn(ir[2], __fmul_rn(hr[2], r)));
    const float hv = hT[u * KS + sq];
    houtT[u * KS + sq] = __fadd_rn(__fmul_rn(__fsub_rn(hv, nn), z), nn);
}

__device__ __forceinline__ void gru_ks(const float* xT, int K4, const float* hT, const float4* __restrict__ Wi,
                                       const float* __restrict__ bi, const float4* __restrict__ Wh,
                                       const float* __restrict__ bh, float* houtT, float* xch, int t) {
    gru_publish(xT, K4, hT, Wi, bi, Wh, bh, xch, t);
    __syncthreads();
    gru_finish(hT, houtT, xch, t);
    __syncthreads();
}

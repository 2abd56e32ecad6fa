// knet_opt.h -- what surrounds the fused training chunk when a whole optimizer update is one graph replay
// (include/trajknet.h: traj_knet_chunk_gather_f32, traj_knet_clip_adamw_f32; pipeline_indipendent_chunking.py).
// Included by knet.hip inside its anonymous namespace, as knet_bwd.h.
//
// All float32 in memory, no atomics, every sum in a fixed order, plain vector stores.  No fused multiply-add is formed
// (-ffp-contract=off), so the gather's normalisation is the two IEEE operations torch performs.

// Batch gather of the chunk-and-shuffle pipeline (training_indipendent_chunking.py:14-34 create_chunks and
// pipeline_indipendent_chunking.py:93-106): one thread per (row b, step k) of the batch.  Chunk id c is trajectory
// c / cpt, steps [(c % cpt) Tc, + Tc); consecutive threads read consecutive steps of one channel.  A row whose id is
// outside [0, n_traj cpt) reads nothing and writes zeros.
__global__ __launch_bounds__(256) void knet_chunk_gather_kernel(
    int n_traj, int T_full, int Tc, int B, const float* __restrict__ y, const float* __restrict__ u,
    const float* __restrict__ x, const int* __restrict__ ids, const float* __restrict__ xm, const float* __restrict__ xs,
    const float* __restrict__ ym, const float* __restrict__ ys, const float* __restrict__ noise, float noise_std,
    float* __restrict__ Y, float* __restrict__ U, float* __restrict__ xt, float* __restrict__ yt,
    float* __restrict__ m1x0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Tc) return;
    const int b = i / Tc, k = i - b * Tc;
    const int cpt = T_full / Tc;
    const int c = ids[b];
    const bool ok = c >= 0 && c < (long long)n_traj * cpt;
    const int traj = ok ? c / cpt : 0;
    const size_t t = ok ? (size_t)(c - traj * cpt) * Tc + k : 0;
    const size_t row = (size_t)k * B + b;   // the tape's [Tc, B, .] layout
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float v = ok ? (y[((size_t)traj * 5 + j) * T_full + t] - ym[j]) / ys[j] : 0.0f;
        Y[row * 5 + j] = v;
        if (yt) yt[((size_t)b * 5 + j) * Tc + k] = v;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) U[row * 2 + j] = ok ? u[((size_t)traj * 2 + j) * T_full + t] : 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float v = ok ? (x[((size_t)traj * 6 + j) * T_full + t] - xm[j]) / xs[j] : 0.0f;
        xt[((size_t)b * 6 + j) * Tc + k] = v;
        if (k == 0) m1x0[b * 6 + j] = ok ? (noise ? v + noise_std * noise[b * 6 + j] : v) : 0.0f;
    }
}

// ---------------------------------------------------------------- global-norm clipping + AdamW
// Two launches over the device-resident table: the norm pass leaves one float64 partial sum of g^2 per workgroup and
// advances the step counter; the update pass sums the partials in a fixed order (every workgroup the same bits),
// forms the clip coefficient and the bias corrections once per workgroup and streams p, g, m, v.
//
// Table pointers are only 4-byte aligned: a tensor is processed as a scalar head up to the first 16-byte boundary, a
// float4 body and a scalar tail.  The update pass takes that form when p, g, m and v share their offset within 16
// bytes (what an allocator gives); otherwise the whole tensor goes element by element.

constexpr int OPT_NORM_BLOCKS = 256;   // norm-pass workgroups at most = partials in the workspace
constexpr int OPT_MAX_BLOCKS = 2048;   // update-pass workgroups at most (256 CUs x 8), grid-stride beyond

__device__ inline long long opt_head(const void* p, long long n) {
    const long long h = (long long)((16u - (unsigned)((size_t)p & 15u)) & 15u) >> 2;
    return h < n ? h : n;
}

__global__ __launch_bounds__(256) void knet_opt_norm_kernel(const traj_knet_opt_entry* __restrict__ table,
                                                            int n_tensors, int* __restrict__ step,
                                                            double* __restrict__ partial) {
    __shared__ double red[256];
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x, gsz = (long long)gridDim.x * 256;
    double s = 0.0;
    for (int e = 0; e < n_tensors; ++e) {
        const float* g = table[e].g;
        const long long n = table[e].n;
        const long long head = opt_head(g, n), nvec = (n - head) >> 2, tail = (n - head) & 3;
        for (long long i = gtid; i < head; i += gsz) s += (double)g[i] * (double)g[i];
        const float4* g4 = reinterpret_cast<const float4*>(g + head);
        for (long long q = gtid; q < nvec; q += gsz) {
            const float4 a = g4[q];
            s += (double)a.x * (double)a.x;
            s += (double)a.y * (double)a.y;
            s += (double)a.z * (double)a.z;
            s += (double)a.w * (double)a.w;
        }
        const float* gt = g + head + 4 * nvec;
        for (long long i = gtid; i < tail; i += gsz) s += (double)gt[i] * (double)gt[i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = red[0];
        if (blockIdx.x == 0) step[0] = step[0] + 1;   // read by the update pass, the next launch on the stream
    }
}

struct OptScalars {
    float coef, decay, omb1, b2, omb2, step_size, bc2_sqrt, eps;
};

__device__ inline void adamw_one(const OptScalars& c, float& p, float g, float& m, float& v) {
    g = c.coef * g;
    p = p * c.decay;
    m = m + c.omb1 * (g - m);
    v = c.b2 * v + c.omb2 * g * g;
    p = p - c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.eps));
}

__device__ inline void adamw_at(const OptScalars& c, float* p, const float* g, float* m, float* v, long long i) {
    float pp = p[i], mm = m[i], vv = v[i];
    adamw_one(c, pp, g[i], mm, vv);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
}

__global__ __launch_bounds__(256) void knet_opt_update_kernel(const traj_knet_opt_entry* __restrict__ table,
                                                              int n_tensors, const float* __restrict__ lr, double beta1,
                                                              double beta2, double eps, double weight_decay,
                                                              double max_norm_d,
                                                              const int* __restrict__ step,
                                                              const double* __restrict__ partial, int n_partial,
                                                              float* __restrict__ total_norm) {
    __shared__ double red[256];
    __shared__ OptScalars sc;
    red[threadIdx.x] = (int)threadIdx.x < n_partial ? partial[threadIdx.x] : 0.0;   // n_partial <= 256
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(red[0]), max_norm = (float)max_norm_d;
        const float cc = max_norm / (total + 1e-6f);
        const double t = (double)step[0], l = (double)lr[0];
        sc.coef = (max_norm > 0.0f && cc < 1.0f) ? cc : 1.0f;
        sc.decay = (float)(1.0 - l * weight_decay);
        sc.omb1 = (float)(1.0 - beta1);
        sc.b2 = (float)beta2;
        sc.omb2 = (float)(1.0 - beta2);
        sc.step_size = (float)(l / (1.0 - pow(beta1, t)));
        sc.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
        sc.eps = (float)eps;
        if (blockIdx.x == 0 && total_norm) total_norm[0] = total;
    }
    __syncthreads();
    const OptScalars c = sc;
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x, gsz = (long long)gridDim.x * 256;
    for (int e = 0; e < n_tensors; ++e) {
        float* p = table[e].p;
        const float* g = table[e].g;
        float* m = table[e].m;
        float* v = table[e].v;
        const long long n = table[e].n;
        const unsigned off = (unsigned)((size_t)p & 15u);
        const bool same = ((size_t)g & 15u) == off && ((size_t)m & 15u) == off && ((size_t)v & 15u) == off;
        const long long head = same ? opt_head(p, n) : n, nvec = (n - head) >> 2, tail = (n - head) & 3;
        for (long long i = gtid; i < head; i += gsz) adamw_at(c, p, g, m, v, i);
        float4* p4 = reinterpret_cast<float4*>(p + head);
        const float4* g4 = reinterpret_cast<const float4*>(g + head);
        float4* m4 = reinterpret_cast<float4*>(m + head);
        float4* v4 = reinterpret_cast<float4*>(v + head);
        for (long long q = gtid; q < nvec; q += gsz) {
            float4 pp = p4[q], mm = m4[q], vv = v4[q];
            const float4 gg = g4[q];
            adamw_one(c, pp.x, gg.x, mm.x, vv.x);
            adamw_one(c, pp.y, gg.y, mm.y, vv.y);
            adamw_one(c, pp.z, gg.z, mm.z, vv.z);
            adamw_one(c, pp.w, gg.w, mm.w, vv.w);
            p4[q] = pp;
            m4[q] = mm;
            v4[q] = vv;
        }
        const long long o = head + 4 * nvec;
        for (long long i = gtid; i < tail; i += gsz) adamw_at(c, p, g, m, v, o + i);
    }
}

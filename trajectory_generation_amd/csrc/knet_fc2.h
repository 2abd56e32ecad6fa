// knet_fc2.h -- FC2 of the fused step in its three product modes (traj_knet_fc2_f32, traj_knet_set_fc2_mode): exact f32
// MFMAs, and three-term bf16 operands with the x2 tile split per wave or once per workgroup.  Included by knet.hip
// inside its anonymous namespace, after knet_dense.h (KH).
//
// FC2 = Linear(2H, dH) -> ReLU -> Linear(dH, n m) (kalman_net.py:88-95) without the [B, dH] hidden
// activation ever reaching memory.  Workgroup (slab, bblk) owns 64 sequences x HS = 64 NT hidden units
// (NT = 5: 32 slabs x 16 b-blocks = 512 workgroups at B = 1024, two per CU, every SIMD the same work):
//   1. the x2 tile [64][2H] is staged in LDS (rows padded to 260 floats);
//   2. wave w forms the TRANSPOSED hidden tile hidT[h][b] = W2a[h,:] . x2[b,:] for its 16 NT hidden units
//      and all 64 sequences on v_mfma_f32_16x16x4_f32 (exact f32): A = W2a rows streamed from L2 PD chunks
//      ahead, B = the x2 tile from LDS; NT x 4 independent 16 x 16 accumulators;
//   3. relu(hidT + b2a) stays in the accumulators and IS the B operand of the second product:
//      lane (g = l >> 4, r = l & 15) holds hidT[4g + q][r] in register q, so MFMA step q contracts over
//      h = 4g + q -- outT[j][b] = sum_h W2b[j][h] hidT[h][b] with no LDS round trip (rows j >= n m are
//      zero weights);
//   4. the four waves' outT partials are added through LDS in wave order and the workgroup writes
//      part[slab][b][0:32].
// The back kernel adds b2b and the slabs in slab order (deterministic, no atomics).  K order inside the
// MFMAs: in chunk c (16 k), lane group g takes k = 16c + 4g + e at step e, so one float4 per operand
// feeds four steps.
constexpr int F2_BT = 64, F2_LD = 2 * KH + 4, F2_RS = 68;
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float f4c(const float4& v, int e) {   // component e (constant after unrolling)
    return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
}

// hidden units per workgroup: 320 when dH allows (512 equal workgroups at B = 1024), else 256
__host__ __device__ inline int fc2_slab(int dH) { return (dH % 320 == 0) ? 320 : 256; }

// Workgroup blockIdx.x of the dH / HS slabs x ceil(B / F2_BT) b-blocks -> its (slab, bblk).  With a multiple of 8 slabs
// the blocks are spread so the b-blocks of a slab share an XCD (its W2a slab stays in that XCD's L2).
__device__ __forceinline__ void fc2_work_item(int B, int dH, int HS, int* slab, int* bblk) {
    const int nslab = dH / HS, nbb = (B + F2_BT - 1) / F2_BT;
    const int i = blockIdx.x;
    if ((nslab & 7) == 0) {
        const int xcd = i & 7, local = i >> 3;
        *slab = (local / nbb) * 8 + xcd;
        *bblk = local % nbb;
    } else {
        *slab = i / nbb;
        *bblk = i % nbb;
    }
}

// The x2 tile [F2_BT][2 KH] of sequences b0 .. as floats into LDS rows of F2_LD.
__device__ __forceinline__ void fc2_stage_x2_f32(const float* __restrict__ x2, int B, int b0, float* s_t) {
    constexpr int K = 2 * KH;   // FC2 input width
    const int t = threadIdx.x;
#pragma unroll
    for (int it = 0; it < F2_BT * (K / 4) / 256; ++it) {   // coalesced: a row is 64 consecutive float4s
        const int q = t + 256 * it, row = q / (K / 4), c4 = q - row * (K / 4);
        const int bsrc = min(b0 + row, B - 1);           // rows past B: duplicates, never stored
        *reinterpret_cast<float4*>(s_t + row * F2_LD + 4 * c4) =
            reinterpret_cast<const float4*>(x2 + (size_t)bsrc * K)[c4];
    }
}

// relu(hidT + b2a) in place: register q of lane (g, r) in tile (ht, bt) is hidden unit hw0 + 16 ht + 4 g + q of
// sequence b0 + 16 bt + r
template <int NT, int BT>
__device__ __forceinline__ void fc2_relu_bias(f32x4 (&acc)[NT][BT], const float* __restrict__ b2a, int hw0) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int ht = 0; ht < NT; ++ht) {
        const float4 bias = *reinterpret_cast<const float4*>(b2a + hw0 + 16 * ht + 4 * g);
#pragma unroll
        for (int bt = 0; bt < BT; ++bt)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[ht][bt][q] = fmaxf(__fadd_rn(acc[ht][bt][q], f4c(bias, q)), 0.0f);
    }
}

template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void knet_fc2_kernel(
    int B, int dH, const float* __restrict__ x2, const float* __restrict__ W2a, const float* __restrict__ b2a,
    const float* __restrict__ W2b, int nout, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float s_t[F2_BT * F2_LD];   // x2 tile, then the wave partials
    static_assert(4 * 32 * F2_RS <= F2_BT * F2_LD, "partials fit the x2 tile");
    constexpr int HS = 64 * NT;
    int slab, bblk;
    fc2_work_item(B, dH, HS, &slab, &bblk);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r = l & 15;
    const int b0 = bblk * F2_BT, hw0 = slab * HS + 16 * NT * w;
    constexpr int K = 2 * KH;   // FC2 input width
    fc2_stage_x2_f32(x2, B, b0, s_t);
    const float* pa = W2a + (size_t)(hw0 + r) * K + 4 * g;   // h-tile ht: + 16 ht K; chunk c: + 16 c
    constexpr int NC = K / 16;   // chunks of 16 k
    constexpr int PD = 2;        // chunks of W2a loads in flight ahead of the MFMAs (the depth every build shipped)
    float4 wa[PD][NT];
#pragma unroll
    for (int d = 0; d < PD; ++d)
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) wa[d][ht] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 16 * d);
    __syncthreads();
    f32x4 acc[NT][4];
#pragma unroll
    for (int ht = 0; ht < NT; ++ht)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) acc[ht][bt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* xr = s_t + r * F2_LD + 4 * g;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int d = c % PD;
        float4 a[NT];
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) a[ht] = wa[d][ht];
        if (c + PD < NC) {
#pragma unroll
            for (int ht = 0; ht < NT; ++ht)
                wa[d][ht] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 16 * (c + PD));
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the W2a prefetch ahead of this chunk's MFMAs
        float4 xb[4];
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) xb[bt] = *reinterpret_cast<const float4*>(xr + 16 * bt * F2_LD + 16 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int ht = 0; ht < NT; ++ht)
#pragma unroll
                for (int bt = 0; bt < 4; ++bt)
                    acc[ht][bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ht], e), f4c(xb[bt], e), acc[ht][bt], 0, 0, 0);
    }
    fc2_relu_bias(acc, b2a, hw0);
    // outT[j][b] over this wave's hidden units: A = W2b[j][h] (rows j = 16 jt + r), B = hidT from registers (exact
    // f32 MFMAs: its own loop, not the three-term one of fc2x_epilogue)
    const float m0 = r < nout ? 1.0f : 0.0f, m1 = 16 + r < nout ? 1.0f : 0.0f;
    const float* pb0 = W2b + (size_t)min(r, nout - 1) * dH + hw0 + 4 * g;
    const float* pb1 = W2b + (size_t)min(16 + r, nout - 1) * dH + hw0 + 4 * g;
    f32x4 o[2][4];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) o[jt][bt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ht = 0; ht < NT; ++ht) {
        float4 u0 = *reinterpret_cast<const float4*>(pb0 + 16 * ht);
        float4 u1 = *reinterpret_cast<const float4*>(pb1 + 16 * ht);
        u0.x *= m0; u0.y *= m0; u0.z *= m0; u0.w *= m0;
        u1.x *= m1; u1.y *= m1; u1.z *= m1; u1.w *= m1;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int bt = 0; bt < 4; ++bt) {
                o[0][bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(u0, q), acc[ht][bt][q], o[0][bt], 0, 0, 0);
                o[1][bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(u1, q), acc[ht][bt][q], o[1][bt], 0, 0, 0);
            }
    }
    // (the wave partials below are fc2x_epilogue's at BT = 4, kept as a copy: shared as one helper, the NT = 5
    // instance of this kernel allocates 186 instead of 190 VGPRs, and its registers are held as they are)
    __syncthreads();   // every wave is done with the x2 tile
    // wave partials: register q of o[jt][bt] is outT[16 jt + 4g + q][16 bt + r]
    float* red = s_t + w * 32 * F2_RS;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(16 * jt + 4 * g + q) * F2_RS + 16 * bt + r] = o[jt][bt][q];
    __syncthreads();
    {   // thread t: sequence t >> 2, outputs 8 (t & 3) .. + 7; waves added in order
        const int bb = t >> 2, j0 = 8 * (t & 3);
        float v[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const float* p0 = s_t + (j0 + jj) * F2_RS + bb;
            v[jj] = __fadd_rn(__fadd_rn(__fadd_rn(p0[0], p0[32 * F2_RS]), p0[64 * F2_RS]), p0[96 * F2_RS]);
        }
        if (b0 + bb < B) {
            float4* dst = reinterpret_cast<float4*>(part + ((size_t)slab * B + b0 + bb) * 32 + j0);
            dst[0] = make_float4(v[0], v[1], v[2], v[3]);
            dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}

// FC2 on the bf16 matrix cores with every f32 operand carried as three bf16 terms (the default FC2;
// traj_knet_set_fc2_mode(0) selects knet_fc2_kernel above).  x = h + m + l exactly: h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m), each residual exact in f32 (24 significand bits = 3 x 8).  A product a b is formed from the
// six bf16 products h_a h_b, h_a m_b, m_a h_b, h_a l_b, l_a h_b, m_a m_b -- each exact in the f32 accumulator --
// and the three dropped ones (m_a l_b, l_a m_b, l_a l_b) are below 2^-23 |a b|, the size of one f32 rounding
// of the product.  So the sums carry f32 accuracy (f32 accumulation, different summation order), at six
// v_mfma_f32_16x16x32_bf16 (16 cycles, 16,384 FLOP each) per 16 x 16 x 32 block where the f32 form needs eight
// v_mfma_f32_16x16x4_f32 (32 cycles, 2,048 FLOP each): 96 against 256 matrix-core cycles.
// Same tiling as knet_fc2_kernel (64 sequences x 64 NT hidden units per workgroup, the x2 tile in LDS, wave w's
// transposed hidden tile in registers as the second product's B operand), K steps of 32:
//   A = W2a rows: lane (r, g) of h-tile ht, K step c holds W2a[h0 + 16 ht + r][32 c + 8 g .. + 7] (two float4
//       loads, one K step ahead), split in registers;
//   B = x2 from the LDS tile: lane (r, g) holds x2[b0 + 16 bt + r][32 c + 8 g .. + 7], split in registers;
//   second product, K step s over the tile pair (2s, 2s + 1): B element e of lane (r, g) = hidT[16 (2s + e / 4)
//       + 4 g + e % 4][16 bt + r] = register e % 4 of accumulator (2s + e / 4, bt), so A element e = W2b[j][that
//       same h] (two float4 runs of W2b's row); an odd NT's last step has a zero upper half.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// (the subtractions may pair into v_pk_add_f32: measured 35.0 us for the FC2 launch against 37.4 us with single
// v_sub_f32 forced by inline asm)
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r1 = __fsub_rn(x, (float)h);
    m = (__bf16)r1;
    l = (__bf16)__fsub_rn(r1, (float)m);
}

__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 vh, vm, vl;
        split3(v[e], vh, vm, vl);
        h[e] = vh;
        m[e] = vm;
        l[e] = vl;
    }
}

__device__ __forceinline__ void split3(const float4& a, const float4& b, bf16x8& h, bf16x8& m, bf16x8& l) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split3(v, h, m, l);
}

// acc += a b over one K step of 32, the six kept products, smallest first
__device__ __forceinline__ f32x4 mfma6(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                       const bf16x8& bm, const bf16x8& bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

// The three-term kernels' second half: relu(hidT + b2a) in the accumulators (fc2_relu_bias), the second product on the
// bf16 matrix cores (B = the accumulators, A = W2b split in registers), the four waves' partials added in wave order
// through LDS (s_red: 4 x 32 x (16 BT + 4) floats, free once every wave is past its reads of the tile),
// part[slab][b][0:32] written.  BT: 16-sequence tiles per workgroup.
template <int NT, int BT = 4>
__device__ __forceinline__ void fc2x_epilogue(f32x4 (&acc)[NT][BT], const float* __restrict__ b2a,
                                              const float* __restrict__ W2b, int dH, int nout, int hw0, int B, int b0,
                                              int slab, float* s_red, float* __restrict__ part) {
    constexpr int RS = 16 * BT + 4;   // (F2_RS at BT = 4)
    const int t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r = l & 15;
    fc2_relu_bias(acc, b2a, hw0);
    // outT[j][b] = sum over this wave's units of W2b[j][h] hidT[h][b] (rows j = 16 jt + r; rows >= nout: zero)
    const float m0 = r < nout ? 1.0f : 0.0f, m1 = 16 + r < nout ? 1.0f : 0.0f;
    const float* pb[2] = {W2b + (size_t)min(r, nout - 1) * dH + hw0 + 4 * g,
                          W2b + (size_t)min(16 + r, nout - 1) * dH + hw0 + 4 * g};
    const float mk[2] = {m0, m1};
    f32x4 o[2][BT];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) o[jt][bt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < (NT + 1) / 2; ++s) {
        constexpr float z = 0.0f;
        const bool hi2 = 2 * s + 1 < NT;   // the step's upper tile exists
        bf16x8 wh[2], wm[2], wl[2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            float4 u0 = *reinterpret_cast<const float4*>(pb[jt] + 32 * s);
            float4 u1 = hi2 ? *reinterpret_cast<const float4*>(pb[jt] + 32 * s + 16) : make_float4(z, z, z, z);
            const float v[8] = {u0.x * mk[jt], u0.y * mk[jt], u0.z * mk[jt], u0.w * mk[jt],
                                u1.x * mk[jt], u1.y * mk[jt], u1.z * mk[jt], u1.w * mk[jt]};
            split3(v, wh[jt], wm[jt], wl[jt]);
        }
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = acc[2 * s][bt][e];
                v[4 + e] = hi2 ? acc[hi2 ? 2 * s + 1 : 2 * s][bt][e] : 0.0f;
            }
            bf16x8 bh, bm, bl;
            split3(v, bh, bm, bl);
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) o[jt][bt] = mfma6(wh[jt], wm[jt], wl[jt], bh, bm, bl, o[jt][bt]);
        }
    }
    __syncthreads();   // every wave is done with the tile in LDS
    float* red = s_red + w * 32 * RS;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int bt = 0; bt < BT; ++bt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(16 * jt + 4 * g + q) * RS + 16 * bt + r] = o[jt][bt][q];
    __syncthreads();
    {   // thread t: sequence t / TPS, outputs JW (t % TPS) .. + JW - 1; waves added in order
        constexpr int SEQ = 16 * BT, TPS = 256 / SEQ, JW = 32 / TPS;
        const int bb = t / TPS, j0 = JW * (t % TPS);
        float v[JW];
#pragma unroll
        for (int jj = 0; jj < JW; ++jj) {
            const float* p0 = s_red + (j0 + jj) * RS + bb;
            v[jj] = __fadd_rn(__fadd_rn(__fadd_rn(p0[0], p0[32 * RS]), p0[64 * RS]), p0[96 * RS]);
        }
        if (b0 + bb < B) {
            float4* dst = reinterpret_cast<float4*>(part + ((size_t)slab * B + b0 + bb) * 32 + j0);
#pragma unroll
            for (int k = 0; k < JW / 4; ++k) dst[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void knet_fc2x_kernel(
    int B, int dH, const float* __restrict__ x2, const float* __restrict__ W2a, const float* __restrict__ b2a,
    const float* __restrict__ W2b, int nout, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float s_t[F2_BT * F2_LD];   // x2 tile, then the wave partials
    constexpr int HS = 64 * NT;
    int slab, bblk;
    fc2_work_item(B, dH, HS, &slab, &bblk);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r = l & 15;
    const int b0 = bblk * F2_BT, hw0 = slab * HS + 16 * NT * w;
    constexpr int K = 2 * KH;
    fc2_stage_x2_f32(x2, B, b0, s_t);
    const float* pa = W2a + (size_t)(hw0 + r) * K + 8 * g;   // h-tile ht: + 16 ht K; K step c: + 32 c
    constexpr int NC = K / 32;
    float4 an[NT][2];
    auto load_a = [&](int c) {
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) {
            an[ht][0] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 32 * c);
            an[ht][1] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 32 * c + 4);
        }
    };
    load_a(0);
    __syncthreads();
    f32x4 acc[NT][4];
#pragma unroll
    for (int ht = 0; ht < NT; ++ht)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) acc[ht][bt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* xr = s_t + r * F2_LD + 8 * g;
    for (int c = 0; c < NC; ++c) {
        bf16x8 ah[NT], am[NT], al[NT];
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) split3(an[ht][0], an[ht][1], ah[ht], am[ht], al[ht]);
        if (c + 1 < NC) load_a(c + 1);
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
            const float4* xp = reinterpret_cast<const float4*>(xr + 16 * bt * F2_LD + 32 * c);
            bf16x8 bh, bm, bl;
            split3(xp[0], xp[1], bh, bm, bl);
#pragma unroll
            for (int ht = 0; ht < NT; ++ht) acc[ht][bt] = mfma6(ah[ht], am[ht], al[ht], bh, bm, bl, acc[ht][bt]);
        }
    }
    fc2x_epilogue<NT>(acc, b2a, W2b, dH, nout, hw0, B, b0, slab, s_t, part);
}

// The three-term FC2 with the x2 tile split ONCE per workgroup (knet_fc2x_kernel has every wave split all 64 sequences'
// values at every K step): the tile's three bf16 planes in LDS, one K half at a time (52 KB, so two workgroups still
// share a CU), W2a split in registers as in knet_fc2x_kernel.  Same terms, same summation order, bit for bit.
constexpr int F2_HK = KH;            // K columns per half
constexpr int F2_BLD = F2_HK + 8;    // bf16 per LDS plane row (272 B: rows 4 banks apart)

template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void knet_fc2y_kernel(
    int B, int dH, const float* __restrict__ x2, const float* __restrict__ W2a, const float* __restrict__ b2a,
    const float* __restrict__ W2b, int nout, float* __restrict__ part) {
    constexpr int PL = F2_BT * F2_BLD;
    __shared__ __attribute__((aligned(16))) __bf16 s_b[3 * PL];   // one K half of the tile: hi, mid, lo planes
    static_assert(4 * 32 * F2_RS * sizeof(float) <= sizeof(s_b), "partials fit the planes");
    constexpr int HS = 64 * NT;
    int slab, bblk;
    fc2_work_item(B, dH, HS, &slab, &bblk);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r = l & 15;
    const int b0 = bblk * F2_BT, hw0 = slab * HS + 16 * NT * w;
    constexpr int K = 2 * KH, NC = K / 32;
    const float* pa = W2a + (size_t)(hw0 + r) * K + 8 * g;
    float4 an[NT][2];
    auto load_a = [&](int c) {
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) {
            an[ht][0] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 32 * c);
            an[ht][1] = *reinterpret_cast<const float4*>(pa + (size_t)16 * ht * K + 32 * c + 4);
        }
    };
    // half hf of the tile, split: thread t takes float4 q = t + 256 it (row q / 32, columns hf 128 + 4 (q % 32) .. + 3)
    auto stage = [&](int hf) {
#pragma unroll 4
        for (int it = 0; it < F2_BT * (F2_HK / 4) / 256; ++it) {
            const int q = t + 256 * it, row = q / (F2_HK / 4), c4 = q - row * (F2_HK / 4);
            const int bsrc = min(b0 + row, B - 1);   // rows past B: duplicates, never stored
            const float4 v = reinterpret_cast<const float4*>(x2 + (size_t)bsrc * K + hf * F2_HK)[c4];
            const float vv[4] = {v.x, v.y, v.z, v.w};
            typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
            bf16x4 h, m, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                __bf16 a0, a1, a2;
                split3(vv[e], a0, a1, a2);
                h[e] = a0;
                m[e] = a1;
                lo[e] = a2;
            }
            const int o = row * F2_BLD + 4 * c4;
            *reinterpret_cast<bf16x4*>(s_b + o) = h;
            *reinterpret_cast<bf16x4*>(s_b + PL + o) = m;
            *reinterpret_cast<bf16x4*>(s_b + 2 * PL + o) = lo;
        }
    };
    load_a(0);
    stage(0);
    __syncthreads();
    f32x4 acc[NT][4];
#pragma unroll
    for (int ht = 0; ht < NT; ++ht)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) acc[ht][bt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const __bf16* xr = s_b + r * F2_BLD + 8 * g;
    for (int c = 0; c < NC; ++c) {
        if (c == NC / 2) {   // second K half
            __syncthreads();
            stage(1);
            __syncthreads();
        }
        bf16x8 ah[NT], am[NT], al[NT];
#pragma unroll
        for (int ht = 0; ht < NT; ++ht) split3(an[ht][0], an[ht][1], ah[ht], am[ht], al[ht]);
        if (c + 1 < NC) load_a(c + 1);
        const int cc = c & (NC / 2 - 1);
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
            const __bf16* bp = xr + 16 * bt * F2_BLD + 32 * cc;
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(bp);
            const bf16x8 bm = *reinterpret_cast<const bf16x8*>(bp + PL);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(bp + 2 * PL);
#pragma unroll
            for (int ht = 0; ht < NT; ++ht) acc[ht][bt] = mfma6(ah[ht], am[ht], al[ht], bh, bm, bl, acc[ht][bt]);
        }
    }
    fc2x_epilogue<NT>(acc, b2a, W2b, dH, nout, hw0, B, b0, slab, reinterpret_cast<float*>(s_b), part);
}

// knet_vehicle.h -- the vehicle physics of the KalmanNet ops on one sequence: one clamped Euler step with its Jacobian,
// the filter's prior around it, and the posterior.  Included by knet.hip inside its anonymous namespace, first (it
// needs only include/trajknet.h's traj_knet_limits).
//
// Reference: KalmanNet/kalman_net.py:145-178 (step_prior, KNet_step) and KalmanNet/vehicle_model.py
// :19-79 (pt_tire_forces / pt_f_cont: the KNet physics variant -- vx_eff = max(|vx|, vx_zero) without
// sign, only alpha_f clamped, Frx on vx_eff, phi / vx / vy / omega pre-clamped), :109-134 (Euler step
// + clamp of all six states), :136-153 (h = rows 0,1,3,4,5).  Constants are rounded to
// float32 as PyTorch rounds Python scalars against float32 tensors; transcendentals are the ROCm
// single-precision ones (last-ulp differences to the CPU reference).

__device__ __forceinline__ float clampf_(float x, float lo, float hi) {   // torch.clamp (NaN propagates)
    float t = (x < lo) ? lo : x;
    return (t > hi) ? hi : t;
}

struct KP {   // vehicle parameters rounded to float32
    float Cm1, Cm2, Cr0, Cr2, Br, Cr, Dr, Bf, Cf, Df, m, Iz, lf, lr, maxAlpha, vx_zero;
};

// torch.clamp's backward mask: the gradient passes on the closed interval [lo, hi]
__device__ __forceinline__ float inside_(float x, float lo, float hi) { return (x >= lo && x <= hi) ? 1.0f : 0.0f; }

// d xn / d x of one veh_step, as torch's autograd differentiates vehicle_model.py:19-79,109-134 (clamp passes the
// gradient on the closed interval, abs'(0) = 0, max(|vx|, vx_zero) splits a tie in half):
//   d xn_i / d x_j = post[i] * ((i == j) + Ts * A[i][j - 2])   (A = 0 for j < 2: X and Y enter no derivative)
struct VehJac {
    float A[6][4];   // d xdot_i / d (phi, vx, vy, omega), the masks of the four pre-clamps included
    float post[6];   // masks of the six clamps after the Euler step
};

// VehicleModel.f (vehicle_model.py:109-134) on one real state: xn = clamp(x + Ts f_cont(x, u)); JAC: also its
// Jacobian (the forward value is the same expressions either way, bit for bit)
template <bool JAC>
__device__ __forceinline__ void veh_step_t(const KP& p, const traj_knet_limits& L, float Ts, const float* x, float d,
                                           float delta, float* xn, VehJac* J) {
    // pt_f_cont (vehicle_model.py:45-79)
    const float phi = clampf_(x[2], L.phi_min, L.phi_max);
    const float vx = clampf_(x[3], L.vx_min, L.vx_max);
    const float vy = clampf_(x[4], L.vy_min, L.vy_max);
    const float om = clampf_(x[5], L.omega_min, L.omega_max);
    // pt_tire_forces (:19-42)
    const float avx = fabsf(vx);
    const float vx_eff = (avx > p.vx_zero || avx != avx) ? avx : p.vx_zero;   // torch.max(|vx|, 0.3)
    float alpha_f = __fadd_rn(-atan2f(__fadd_rn(__fmul_rn(om, p.lf), vy), vx_eff), delta);
    const float alpha_r = atan2f(__fsub_rn(__fmul_rn(om, p.lr), vy), vx_eff);
    alpha_f = clampf_(alpha_f, -p.maxAlpha, p.maxAlpha);
    const float Fy_f = __fmul_rn(p.Df, sinf(__fmul_rn(p.Cf, atanf(__fmul_rn(p.Bf, alpha_f)))));
    const float Fy_r = __fmul_rn(p.Dr, sinf(__fmul_rn(p.Cr, atanf(__fmul_rn(p.Br, alpha_r)))));
    const float Frx = __fsub_rn(__fsub_rn(__fmul_rn(__fsub_rn(p.Cm1, __fmul_rn(p.Cm2, vx_eff)), d), p.Cr0),
                                __fmul_rn(p.Cr2, __fmul_rn(vx_eff, vx_eff)));
    const float cphi = cosf(phi), sphi = sinf(phi), cdl = cosf(delta), sdl = sinf(delta);
    float xd[6];
    xd[0] = __fsub_rn(__fmul_rn(vx, cphi), __fmul_rn(vy, sphi));
    xd[1] = __fadd_rn(__fmul_rn(vx, sphi), __fmul_rn(vy, cphi));
    xd[2] = om;
    xd[3] = __fdiv_rn(__fadd_rn(__fsub_rn(Frx, __fmul_rn(Fy_f, sdl)), __fmul_rn(__fmul_rn(p.m, vy), om)), p.m);
    xd[4] = __fdiv_rn(__fsub_rn(__fadd_rn(Fy_r, __fmul_rn(Fy_f, cdl)), __fmul_rn(__fmul_rn(p.m, vx), om)), p.m);
    xd[5] = __fdiv_rn(__fsub_rn(__fmul_rn(__fmul_rn(Fy_f, p.lf), cdl), __fmul_rn(Fy_r, p.lr)), p.Iz);
    // f: Euler step + clamp of all states (:109-134)
    const float lo[6] = {L.x_min, L.y_min, L.phi_min, L.vx_min, L.vy_min, L.omega_min};
    const float hi[6] = {L.x_max, L.y_max, L.phi_max, L.vx_max, L.vy_max, L.omega_max};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float raw = __fadd_rn(x[i], __fmul_rn(Ts, xd[i]));
        xn[i] = clampf_(raw, lo[i], hi[i]);
        if constexpr (JAC) J->post[i] = inside_(raw, lo[i], hi[i]);
    }
    if constexpr (JAC) {
        const float m_phi = inside_(x[2], L.phi_min, L.phi_max), m_vx = inside_(x[3], L.vx_min, L.vx_max);
        const float m_vy = inside_(x[4], L.vy_min, L.vy_max), m_om = inside_(x[5], L.omega_min, L.omega_max);
        // vx_eff = max(|vx|, vx_zero) w.r.t. the clamped vx
        const float sg = vx > 0.0f ? 1.0f : (vx < 0.0f ? -1.0f : 0.0f);
        const float ve_vx = (avx > p.vx_zero ? 1.0f : (avx == p.vx_zero ? 0.5f : 0.0f)) * sg;
        // alpha_f (before its clamp) = -atan2(a1, vx_eff) + delta, alpha_r = atan2(a2, vx_eff)
        const float a1 = __fadd_rn(__fmul_rn(om, p.lf), vy), a2 = __fsub_rn(__fmul_rn(om, p.lr), vy);
        const float af_raw = __fadd_rn(-atan2f(a1, vx_eff), delta);
        const float r1 = fmaf(vx_eff, vx_eff, a1 * a1), r2 = fmaf(vx_eff, vx_eff, a2 * a2);
        const float af_a1 = -vx_eff / r1, af_ve = a1 / r1, ar_a2 = vx_eff / r2, ar_ve = -a2 / r2;
        // Fy = D sin(C atan(B alpha))
        const float qf = __fmul_rn(p.Bf, alpha_f), qr = __fmul_rn(p.Br, alpha_r);
        const float Ff = p.Df * cosf(__fmul_rn(p.Cf, atanf(qf))) * (p.Cf * p.Bf) / fmaf(qf, qf, 1.0f) *
                         inside_(af_raw, -p.maxAlpha, p.maxAlpha);               // d Fy_f / d alpha_f (raw)
        const float Fr = p.Dr * cosf(__fmul_rn(p.Cr, atanf(qr))) * (p.Cr * p.Br) / fmaf(qr, qr, 1.0f);
        const float Ff_vx = Ff * af_ve * ve_vx, Ff_vy = Ff * af_a1, Ff_om = Ff_vy * p.lf;
        const float Fr_vx = Fr * ar_ve * ve_vx, Fr_vy = -(Fr * ar_a2), Fr_om = Fr * ar_a2 * p.lr;
        const float Fx_vx = (-(p.Cm2 * d) - 2.0f * p.Cr2 * vx_eff) * ve_vx;      // d Frx / d vx
        const float im = 1.0f / p.m, iz = 1.0f / p.Iz, lc = p.lf * cdl;
        const float A[6][4] = {
            {-xd[1], cphi, -sphi, 0.0f},
            {xd[0], sphi, cphi, 0.0f},
            {0.0f, 0.0f, 0.0f, 1.0f},
            {0.0f, (Fx_vx - Ff_vx * sdl) * im, om - Ff_vy * sdl * im, vy - Ff_om * sdl * im},
            {0.0f, (Fr_vx + Ff_vx * cdl) * im - om, (Fr_vy + Ff_vy * cdl) * im, (Fr_om + Ff_om * cdl) * im - vx},
            {0.0f, (Ff_vx * lc - Fr_vx * p.lr) * iz, (Ff_vy * lc - Fr_vy * p.lr) * iz,
             (Ff_om * lc - Fr_om * p.lr) * iz}};
        const float pre[4] = {m_phi, m_vx, m_vy, m_om};
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) J->A[i][c] = A[i][c] * pre[c];
    }
}

__device__ __forceinline__ void veh_step(const KP& p, const traj_knet_limits& L, float Ts, const float* x, float d,
                                         float delta, float* xn) {
    veh_step_t<false>(p, L, Ts, x, d, delta, xn, nullptr);
}

// kalman_net.py:145-162 for one sequence: x_post (normalized) -> prior (normalized), m1y, dy = y - m1y
__device__ __forceinline__ void prior_one(const KP& p, const traj_knet_limits& L, float Ts, const float* xp, float d,
                                          float delta, const float* yv, int ystride, const float* xm,
                                          const float* xs, const float* ym, const float* ys, const float* um,
                                          const float* us, float* prior, float* m1y, float* dyo) {
    float x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = __fadd_rn(__fmul_rn(xp[i], xs[i]), xm[i]);   // _denorm_x
    if (um && us) {   // _denorm_u (only when u statistics were set)
        d = __fadd_rn(__fmul_rn(d, us[0]), um[0]);
        delta = __fadd_rn(__fmul_rn(delta, us[1]), um[1]);
    }
    float xn[6];
    veh_step(p, L, Ts, x, d, delta, xn);
    // renormalize; h = rows 0,1,3,4,5 (:136-153)
#pragma unroll
    for (int i = 0; i < 6; ++i) prior[i] = __fdiv_rn(__fsub_rn(xn[i], xm[i]), xs[i]);
    const int hr[5] = {0, 1, 3, 4, 5};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float my = __fdiv_rn(__fsub_rn(xn[hr[j]], ym[j]), ys[j]);
        if (m1y) m1y[j] = my;
        if (dyo) dyo[j] = __fsub_rn(yv[j * ystride], my);
    }
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// One state of the posterior (kalman_net.py:169-178): prior + gamma * sum_j KG[i][j] dy[j], the sum in j order from 0.
// Ki: row i of the gain, its n elements ks floats apart (global rows: 1, the step kernels' k-major LDS: KS).  The
// callers (knet_update_kernel, knet_back_front_kernel) keep their own loops over the six states and their own stores.
__device__ __forceinline__ float posterior_one(const float* Ki, int ks, int n, const float* dy, float prior,
                                               float gamma) {
    float s = 0.0f;
    for (int j = 0; j < n; ++j) s = __fadd_rn(s, __fmul_rn(Ki[j * ks], dy[j]));
    return __fadd_rn(prior, __fmul_rn(gamma, s));
}

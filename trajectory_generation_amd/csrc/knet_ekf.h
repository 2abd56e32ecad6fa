// knet_ekf.h -- the EKF baseline in float64 (traj_ekf_run_f64), one thread per sequence.  Included by knet.hip inside
// its anonymous namespace, after knet_ekf_step.h (the step itself: KPd, veh_f, ekf_step).

__global__ __launch_bounds__(64) void ekf_kernel(KPd p, double Ts, int B, int T, const double* __restrict__ y,
                                                 const double* __restrict__ u, const double* __restrict__ x0,
                                                 const double* __restrict__ P0, const double* __restrict__ Q,
                                                 const double* __restrict__ R, double* __restrict__ xo) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[6], P[6][6];
    for (int i = 0; i < 6; ++i) {
        x[i] = x0[6 * b + i];
        for (int j = 0; j < 6; ++j) P[i][j] = (i == j) ? P0[i] : 0.0;
    }
    for (int t = 0; t < T; ++t) {
        const double d = u[((size_t)b * 2 + 0) * T + t], de = u[((size_t)b * 2 + 1) * T + t];
        double yv[5];
        for (int a = 0; a < 5; ++a) yv[a] = y[((size_t)b * 5 + a) * T + t];
        ekf_step(p, Ts, x, P, d, de, yv, Q, R);
        for (int i = 0; i < 6; ++i) xo[((size_t)b * 6 + i) * T + t] = x[i];
    }
}

// mpc_sizes.h -- per-instance scratch sizes of the scratch-using MPC solvers (mpc_general.h, mpc_long.h, mpc_split.h),
// shared by the kernels that carve the scratch and by the host routing that sizes it (mpc_route.h).  Plain C++17: a
// host compiler reads it without the HIP headers.
#pragma once
#include <cstddef>

#include "../../include/trajmpc.h"

#ifdef __HIPCC__
#define TGMPC_HD __host__ __device__
#else
#define TGMPC_HD
#endif

namespace tgmpc {

constexpr int GEN_NMAX = 2 * TRAJ_MAX_N;      // general solver: n whose Cholesky factor is kept in LDS
constexpr int LONG_NKL = 128;                 // long-horizon kernel: n up to which K^-1 lives in LDS

// per-instance scratch of solve_gen_kernel, in doubles (m <= 10 N rows; n > GEN_NMAX: + the n x n factor)
TGMPC_HD inline size_t gen_ws_doubles(int N) {
    const size_t n = 2 * (size_t)N, m = 10 * (size_t)N;
    return n * n + m * n + 6 * (size_t)(N + 1) * n + 6 * (size_t)(N + 1) + 3 * n + 20 * n + 24 * m + 64 +
           (n > (size_t)GEN_NMAX ? n * n : 0);
}

TGMPC_HD inline int long_ld(int n) { return (n + 7) & ~7; }
// long-horizon kernel, per-instance scratch (doubles): P, and K^-1 when it does not fit LDS
TGMPC_HD inline size_t long_ws_doubles(int N) {
    const int n = 2 * N, ld = long_ld(n);
    return (size_t)ld * ld * (n > LONG_NKL ? 2 : 1);
}

// row-split kernel: the capacity H (half a row) by n = 2N
TGMPC_HD inline int split_h(int n) { return n <= 80 ? 40 : (n <= 96 ? 48 : 64); }
// per-instance scratch (doubles): the scaled P, NRW rows x 2H
TGMPC_HD inline size_t split_ws_doubles(int N) {
    const int H = split_h(2 * N);
    return (size_t)(32 * ((2 * H + 31) / 32)) * (2 * H);
}

}  // namespace tgmpc

// spline.h -- the natural cubic spline piece coefficients of one trajectory (batch.spline_natural), for host and
// device: one lane, or one loop iteration, builds the [nk - 1, 4] rows (a, b, c, d) that path_eval (mpc_common.h)
// reads, y = a + t (b + t (c + t d)) with t = x - xk[j].
//
//   second derivatives M    the (nk - 2) interior equations  h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1]
//                           = 6 ((y[i+1] - y[i]) / h[i] - (y[i] - y[i-1]) / h[i-1]),  M[0] = M[nk-1] = 0, by the Thomas
//                           algorithm (the matrix is strictly diagonally dominant: no pivoting is needed)
//   the four columns        as spline_natural writes them:  y[i],  (y[i+1] - y[i]) / h[i] - h[i] (2 M[i] + M[i+1]) / 6,
//                           M[i] / 2,  (M[i+1] - M[i]) / (6 h[i])
//
// The forward sweep keeps its two records per equation (c', d') in columns 2 and 3 of the output row of that equation;
// the back substitution reads them before it writes the row.  So there is no knot cap and no private array that a
// lane would index dynamically (scratch memory on the GPU).
//
// spline_natural solves the same system with LAPACK (LU with partial pivoting), so the two agree to rounding, not bit
// for bit: tests/test_workload_host.py holds both against an exact rational solve.
//
// float64 only, +, -, *, / in the written order, no libm.  Built with -ffp-contract=off like the rest of the library:
// no product here may fuse into an fma, and the host-compiled and device-compiled text give the same bits.
// The same text compiles with hipcc (host and gfx950) and with a plain host C++17 compiler.
#ifndef TGMPC_SPLINE_H
#define TGMPC_SPLINE_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPL_HD __host__ __device__ __forceinline__
#else
#define SPL_HD inline
#endif

namespace tgspline {

// false for +-inf and NaN (no libm: v - v is 0 exactly for every finite v and NaN otherwise)
SPL_HD bool spl_finite(double v) { return v - v == 0.0; }

// 2 <= nk <= kmax, every knot and ordinate finite, knots strictly increasing
SPL_HD bool spline_knots_ok(int nk, int kmax, const double* xk, const double* yk) {
    if (nk < 2 || nk > kmax) return false;
    bool ok = spl_finite(xk[0]) && spl_finite(yk[0]);
    for (int i = 1; i < nk; ++i) ok = ok && spl_finite(xk[i]) && spl_finite(yk[i]) && xk[i] > xk[i - 1];
    return ok;
}

// coef [nk - 1, 4] from knots that spline_knots_ok accepts
SPL_HD void spline_coef(int nk, const double* xk, const double* yk, double* coef) {
    // forward sweep over the interior equations i = 1 .. nk - 2: c'[i] -> coef[4 i + 2], d'[i] -> coef[4 i + 3]
    double cp = 0.0, dp = 0.0;
    for (int i = 1; i < nk - 1; ++i) {
        const double hl = xk[i] - xk[i - 1], hr = xk[i + 1] - xk[i];
        const double rhs = 6.0 * ((yk[i + 1] - yk[i]) / hr - (yk[i] - yk[i - 1]) / hl);
        const double den = 2.0 * (hl + hr) - hl * cp;     // cp = 0 at i = 1: the first row has no sub-diagonal
        cp = hr / den;
        dp = (rhs - hl * dp) / den;
        coef[4 * i + 2] = cp;
        coef[4 * i + 3] = dp;
    }
    // back substitution from the last piece down; Mn = M[i + 1], M[nk - 1] = M[0] = 0
    double Mn = 0.0;
    for (int i = nk - 2; i >= 0; --i) {
        const double Mi = i >= 1 ? coef[4 * i + 3] - coef[4 * i + 2] * Mn : 0.0;
        const double h = xk[i + 1] - xk[i];
        coef[4 * i + 0] = yk[i];
        coef[4 * i + 1] = (yk[i + 1] - yk[i]) / h - h * (2.0 * Mi + Mn) / 6.0;
        coef[4 * i + 2] = Mi / 2.0;
        coef[4 * i + 3] = (Mn - Mi) / (6.0 * h);
        Mn = Mi;
    }
}

// One trajectory's row coef [kmax - 1, 4] as PathSet.build leaves it: the pieces of a kind-2 trajectory, zeros past
// them and in every row of another kind.  Returns 1 (and a zero row) for a kind-2 trajectory whose knots
// spline_knots_ok refuses, 0 otherwise.
SPL_HD int spline_coef_row(int kind, int nk, int kmax, const double* xk, const double* yk, double* coef) {
    const bool spline = kind == 2;
    const bool ok = spline && spline_knots_ok(nk, kmax, xk, yk);
    const int pieces = ok ? nk - 1 : 0;
    if (ok) spline_coef(nk, xk, yk, coef);
    for (int i = 4 * pieces; i < 4 * (kmax - 1); ++i) coef[i] = 0.0;
    return spline && !ok ? 1 : 0;
}

}  // namespace tgspline

#endif

// mpc_osqp_rules.h -- the scalar OSQP rules every condensed solve kernel applies around its own linear algebra
// (mpc_solve.h, mpc_split.h, mpc_long.h): uniform decisions on block-reduced residuals, and the per-row rho and
// active-set rules.  Nothing here touches LDS, a lane index or a kernel argument.
#pragma once
#include "mpc_common.h"

namespace tgmpc {

// residuals (OSQP update_info, unscaled norms; compute_rho_estimate's scaled norms):
//   pr, eps_p from max(|Ax|, |z|), dr, eps_d from max(|Px|, |A'y|, |q|) (unscaled); prs, drs, pn, dn (scaled)
struct Res { double pr, dr, eps_p, eps_d, prs, drs, pn, dn; };

// a row's rho: RHO_MIN for a free row, RHO_EQ_OVER_INEQ rho for an equality, rho otherwise
__device__ __forceinline__ double rho_for(double l, double u, double rho) {
    if (l <= -INFTY * MIN_SCALING && u >= INFTY * MIN_SCALING) return RHO_MIN;
    if (u - l < RHO_TOL) return RHO_EQ_OVER_INEQ * rho;
    return rho;
}

// OSQP compute_rho_estimate on the scaled norms, clamped to [RHO_MIN, RHO_MAX]
__device__ __forceinline__ double rho_estimate(double rho, const Res& r) {
    const double est = rho * sqrt((r.prs / (r.pn + DIV_TOL)) / (r.drs / (r.dn + DIV_TOL) + DIV_TOL));
    return fmin(fmax(est, RHO_MIN), RHO_MAX);
}
__device__ __forceinline__ bool needs_refactor(double est, double rho, double tol) {
    return est > rho * tol || est < rho / tol;
}

// the status at the iteration cap (an exact-mode continuation round that runs out of iterations still meets eps)
__device__ __forceinline__ int status_at_cap(int rounds, const Res& r) {
    return (rounds > 0 && r.pr <= r.eps_p && r.dr <= r.eps_d)     ? TRAJ_STATUS_OPTIMAL
           : (r.pr <= 10.0 * r.eps_p && r.dr <= 10.0 * r.eps_d) ? TRAJ_STATUS_OPTIMAL_INACCURATE
                                                                 : TRAJ_STATUS_USER_LIMIT;
}

// OSQP active sets: lower (-1) if z - l < -y, upper (+1) if u - z < y
__device__ __forceinline__ int active_sign(double z, double l, double u, double y) {
    return (z - l < -y) ? -1 : ((u - z < y) ? 1 : 0);
}

// exact mode: can this pass's certificate count?  The passes are 1 .. polish_max_pass, so with polish_max_pass = 0 none
// does -- the point stays uncertified and the continuation rounds run (the oracle's and mpc_general.h's pass loop)
__device__ __forceinline__ bool pass_counts(const traj_mpc_config& c) { return c.polish_max_pass >= 1; }

// after an uncertified or failed polish: continue ADMM to a 100x tighter tolerance, then polish again?
__device__ __forceinline__ bool polish_continues(const traj_mpc_config& c, int rounds, int iter) {
    return rounds < c.polish_max_rounds && iter < c.max_iter;
}

}  // namespace tgmpc

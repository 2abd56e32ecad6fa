// gen_model.h -- the bicycle model of the open-loop generators (generation_type1.py / generation_type2.py), shared by
// openloop.hip (simulation of given controls) and piecewise.hip (the type-2 state machine), so that both evaluate
// it identically.
#pragma once
#include "physics.h"

namespace tgmpc {

// generation_type1.py:38-68 (CLAMP_REAR = false) and generation_type2.py:52-86 (CLAMP_REAR = true): against
// physics.h's tire_forces / f_cont_sc, vx_eff carries no sign, Frx is formed with vx_eff, only type 2 clamps the
// rear slip angle, and the accelerations divide by m and Iz.
template <bool CLAMP_REAR>
__device__ __forceinline__ void gen_f_cont(const VP& p, const double* x, double d, double delta, double* xd) {
    const double phi = x[2], vx = x[3], vy = x[4], omega = x[5];
    const double avx = fabs(vx);
    const double vx_eff = (p.vx_zero > avx) ? p.vx_zero : avx;   // python max(abs(vx), vx_zero)
    double alpha_f = -pm_atan2(omega * p.lf + vy, vx_eff) + delta;
    double alpha_r = pm_atan2(omega * p.lr - vy, vx_eff);
    alpha_f = clampd(alpha_f, -p.maxAlpha, p.maxAlpha);
    if (CLAMP_REAR) alpha_r = clampd(alpha_r, -p.maxAlpha, p.maxAlpha);
    const double Fy_f = p.Df * pm_tire_sin(p.Cf * pm_atan(p.Bf * alpha_f));
    const double Fy_r = p.Dr * pm_tire_sin(p.Cr * pm_atan(p.Br * alpha_r));
    const double Frx = (p.Cm1 - p.Cm2 * vx_eff) * d - p.Cr0 - p.Cr2 * (vx_eff * vx_eff);
    double sd, cd, sphi, cphi;
    pm_sincos(delta, &sd, &cd);
    pm_sincos(phi, &sphi, &cphi);
    xd[0] = vx * cphi - vy * sphi;
    xd[1] = vx * sphi + vy * cphi;
    xd[2] = omega;
    xd[3] = (Frx - Fy_f * sd + p.m * vy * omega) / p.m;
    xd[4] = (Fy_r + Fy_f * cd - p.m * vx * omega) / p.m;
    xd[5] = (Fy_f * p.lf * cd - Fy_r * p.lr) / p.Iz;
}

}  // namespace tgmpc

// mpc_launch.h -- the fused closed-loop launch (traj_closed_loop_run), shared by the per-capacity translation
// units: mpc_inst.hip (every capacity, 2 waves per SIMD) and mpc_inst_w3.hip (NN = 40 at 3 waves per SIMD).
#pragma once
#include "mpc_host.h"
#include "mpc_solve.h"

namespace tgmpc {

// One workgroup per resident slot (occupancy x CUs), each taking (step, instance) items from the queue; at
// least ceil(B / TRAJ_FUSED_MAX_PER_WG) workgroups.  The production instance has no diagnostics compiled in;
// a.dbg / a.dbg_items select the DIAG one, whose residency can differ -- each has its own slot count.
template <int NN, int WPS>
int launch_fused(const KArgs& a, hipStream_t st) {
    const dim3 sblock(((NN + 63) / 64) * 64);
    const bool diag = a.dbg != nullptr || a.dbg_items != nullptr;
    static PerDevice slots[2];
    constexpr int WAVES = (NN + 63) / 64;
    constexpr int cap = 4 * WPS / WAVES;   // WPS waves per SIMD, 4 SIMDs, WAVES waves per workgroup
    const int n = diag ? resident_slots(slots[1], solve_kernel<NN, true, true, true, WPS>, (int)sblock.x, cap)
                       : resident_slots(slots[0], solve_kernel<NN, true, true, false, WPS>, (int)sblock.x, cap);
    if (!n) return TRAJ_E_LAUNCH;
    const dim3 grid(fused_grid(n, a.B, a.fused_grid));
    if (diag) hipLaunchKernelGGL((solve_kernel<NN, true, true, true, WPS>), grid, sblock, 0, st, a);
    else hipLaunchKernelGGL((solve_kernel<NN, true, true, false, WPS>), grid, sblock, 0, st, a);
    return launched();
}

}  // namespace tgmpc

// mpc_inst.hip -- one translation unit per horizon capacity (compiled with -DTGMPC_NN=<NN>), so
// the fully unrolled instantiations of the MPC kernels build in parallel.
#include "mpc_launch.h"

#ifndef TGMPC_NN
#error "compile with -DTGMPC_NN=<capacity>"
#endif

#define TGMPC_CAT2(a, b) a##b
#define TGMPC_CAT(a, b) TGMPC_CAT2(a, b)

namespace tgmpc {

#if TGMPC_NN == 40
int launch_fused_w3_40(const KArgs& a, hipStream_t st);   // mpc_inst_w3.hip
void preload_fused_w3_40();                                // mpc_inst_w3.hip
#endif

int TGMPC_CAT(launch_mpc_, TGMPC_NN)(const KArgs& a, hipStream_t st, Mode mode) {
    constexpr int NN = TGMPC_NN;
    dim3 grid(a.B), sblock(((NN + 63) / 64) * 64);
    switch (mode) {
        case Mode::Fused: {
#if TGMPC_NN == 40
            // the first fused launch at this capacity loads BOTH instances' code objects, so a later launch of the
            // other one (the opt-in 3-wave instance, traj_debug_fused_waves(3)) does not pay that inside its own call
            static PerDevice loaded;
            (void)once_per_device(loaded, [](int) {
                preload_fused_w3_40();
                return preload(&solve_kernel<NN, true, true, false, 2>);
            });
            if (a.wps == 3) return launch_fused_w3_40(a, st);
#endif
#if TGMPC_NN > 64
            // capacity 80: one wave per SIMD (the default, a.wps = 1) unless the lean two-wave instance (2 waves per
            // SIMD, 4 instances per CU, opt-in) is asked for with traj_debug_fused_waves(2); any other value runs the
            // default
            if (a.wps != 2) return launch_fused<NN, 1>(a, st);
#endif
            return launch_fused<NN, 2>(a, st);
        }
        case Mode::ClosedStep: hipLaunchKernelGGL((solve_kernel<NN, true>), grid, sblock, 0, st, a); break;
        case Mode::StepInlin:
            hipLaunchKernelGGL((solve_kernel<NN, false, false, true, 2, true>), grid, sblock, 0, st, a);
            break;
        case Mode::Step:
        case Mode::Qp: hipLaunchKernelGGL((solve_kernel<NN, false>), grid, sblock, 0, st, a); break;
    }
    return launched();
}

}  // namespace tgmpc

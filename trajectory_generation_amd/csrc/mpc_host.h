// mpc_host.h -- the host side between the C ABI and hipLaunchKernelGGL, shared by trajmpc.hip, the per-capacity and
// row-split launchers (mpc_launch.h, mpc_inst.hip, mpc_inst_w3.hip, split_inst.hip) and, for its two launch helpers,
// closed_obs.hip and closed_stats.hip.  Host code only: nothing here reaches a kernel's text.  One convention: every
// launcher returns TRAJ_OK or TRAJ_E_LAUNCH (include/trajmpc.h), through launched().
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

#include "../../include/trajmpc.h"
#include "mpc_common.h"
#include "mpc_route.h"

namespace tgmpc {

// what launch_mpc's kernel does: the MPC step (linearization launched before it), the QP half (A / B / g given), one
// closed-loop step (linearization launched by the caller), the fused closed loop of a.nsteps steps (linearization
// inside), the MPC step with the linearization inside (one launch; the records go to the workspace's A / B / g)
enum class Mode { Step, Qp, ClosedStep, Fused, StepInlin };

// after a hipLaunchKernelGGL
inline int launched() { return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH; }
inline unsigned nblk(int n, int per) { return (unsigned)(((long long)n + per - 1) / per); }

// A positive int computed once per device of the process (an attribute set, a code object loaded, a slot count):
// compute(dev) returns it, or 0 for a failure, which is returned and not kept.  The table's entries are atomics --
// several host threads may call in, and at worst two of them compute.  A device index outside the table (none below 64
// devices) computes on every call and is never an error.
using PerDevice = std::atomic<int>[64];
template <class F>
int once_per_device(PerDevice& table, F&& compute) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const bool kept = dev >= 0 && dev < 64;
    int v = kept ? table[dev].load(std::memory_order_acquire) : 0;
    if (!v) {
        v = compute(dev);
        if (v > 0 && kept) table[dev].store(v, std::memory_order_release);
    }
    return v;
}

// loads a kernel's code object without launching it (HIP loads them lazily: milliseconds of host time otherwise)
template <class K>
int preload(K kernel) {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess;
}

// the fused closed loop's resident slots on the current device: workgroups per CU by the occupancy API (at least 1, at
// most cap) times CUs; 0 for a failure
template <class K>
int resident_slots(PerDevice& table, K kernel, int block, int cap = 1 << 30) {
    return once_per_device(table, [&](int dev) {
        int nb = 0, ncu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 0;
        return (nb < 1 ? 1 : (nb > cap ? cap : nb)) * (ncu < 1 ? 1 : ncu);
    });
}

// the fused closed loop's grid: one workgroup per resident slot (or a.fused_grid of them, traj_debug_fused_grid), at
// most B and at least ceil(B / TRAJ_FUSED_MAX_PER_WG)
inline int fused_grid(int slots, int B, int asked) {
    int G = asked > 0 ? asked : slots;
    if (G > B) G = B;
    const int minG = (B + TRAJ_FUSED_MAX_PER_WG - 1) / TRAJ_FUSED_MAX_PER_WG;
    return G < minG ? minG : G;
}

// the part of the kernel arguments every entry point shares; the rest is zero
inline KArgs kargs(const traj_vehicle_params* p, const traj_mpc_config* c, int B, long long* dbg) {
    KArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = *p; a.c = *c;
    a.B = B; a.dbg = dbg;
    return a;
}

// the workspace's base part by its layout (mpc_route.h): the linearization's hand-off doubles as the QP's A / B / g
inline void carve_workspace(KArgs& a, void* ws, const WsLayout& w) {
    const auto at = [ws](size_t off) { return (double*)((char*)ws + off); };
    a.Ad = a.wsA = at(w.A); a.Bd = a.wsB = at(w.Bm); a.gd = a.wsg = at(w.g);
    a.wsXF = at(w.xf); a.wsWarm = at(w.warm);
}

inline bool paths_ok(const traj_paths* ps) {
    return ps && ps->kind && ps->pc && (ps->kmax < 2 || (ps->nk && ps->xk && ps->coef));
}
inline PathArgs path_args(const traj_paths* ps) { return {ps->kmax, ps->kind, ps->pc, ps->nk, ps->xk, ps->coef}; }

}  // namespace tgmpc

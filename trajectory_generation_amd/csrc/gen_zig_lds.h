// gen_zig_lds.h -- the ziggurat tables of gen_zig_tables.h as a translation unit of the library needs them: the
// host's copy (zig_host_*), the device's (zig_dev_*) and the kernels' copy of it in LDS (6 KB: lanes index the tables
// with a random layer).  hipcc only; each including file gets its own static copies.
#pragma once
#include <hip/hip_runtime.h>

#include "gen_rng.h"

namespace tgmpc {

// the tables twice: the host's copy (traj_gen_rng_draw_host) and the device's (the source of the LDS copy)
#define GEN_ZIG_DECL static const
#define GEN_ZIG_NAME(x) zig_host_##x
#include "gen_zig_tables.h"
#undef GEN_ZIG_DECL
#undef GEN_ZIG_NAME
#define GEN_ZIG_DECL static __device__ const
#define GEN_ZIG_NAME(x) zig_dev_##x
#include "gen_zig_tables.h"
#undef GEN_ZIG_DECL
#undef GEN_ZIG_NAME

constexpr int ZIG_N = 256;

struct ZigLds {
    double wi[ZIG_N];
    uint64_t ki[ZIG_N];
    double fi[ZIG_N];
};

// every thread of the block takes part; ends with a barrier
__device__ __forceinline__ void zig_load(ZigLds& t) {
    for (int i = threadIdx.x; i < ZIG_N; i += blockDim.x) {
        t.wi[i] = zig_dev_wi[i];
        t.ki[i] = zig_dev_ki[i];
        t.fi[i] = zig_dev_fi[i];
    }
    __syncthreads();
}

inline ZigTables zig_host_tables() { return ZigTables{zig_host_wi, (const uint64_t*)zig_host_ki, zig_host_fi}; }

}  // namespace tgmpc

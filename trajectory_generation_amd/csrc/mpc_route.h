// mpc_route.h -- which MPC solver an entry point runs and how much caller-owned workspace it needs: the one place
// that decides it.  Every entry point of trajmpc.hip takes one Switches snapshot, computes one Route from it and reads
// nothing else; the workspace queries return the same Route's `need`.  Host-only, plain C++17 (no HIP types).
//
// The tiers (include/trajmpc.h):
//   General  state bounds with a finite side, or TRAJ_MAX_N_LONG < N <= TRAJ_MAX_N_GENERAL (mpc_general.h);
//   Long     no state bounds, TRAJ_MAX_N < N <= TRAJ_MAX_N_LONG and not on the row-split kernel (mpc_long.h);
//   Split    no state bounds, split_min_n <= N <= split_max_n (mpc_split.h; defaults 21 .. 64) -- the QP entry keeps
//            the capacity-80 kernel up to TRAJ_MAX_N whatever split_min_n says;
//   Reg      the register-resident kernels, N <= TRAJ_MAX_N (mpc_solve.h).
// Workspace: the step's and the closed loop's begins with the base part (ws_base_bytes); the solver's scratch follows
// at scratch_off.  The QP entry's workspace is only the scratch.
#pragma once
#include <cstddef>

#include "../../include/trajmpc.h"
#include "mpc_sizes.h"

namespace tgmpc {

enum class Tier { Reg, Split, Long, General };
enum class Entry { Step, Qp, ClosedStep, ClosedRun };

// the debug switches that routing depends on (traj_debug_split_min_n / _split_max_n / _step_linearize): an entry
// point reads them once, so that the workspace it validates is the one its launch uses
struct Switches {
    int split_min_n, split_max_n, step_inlin;
};

struct Route {
    int err;               // TRAJ_OK or TRAJ_E_ARG (a null or invalid configuration, B < 0); the rest holds for TRAJ_OK
    Tier tier;
    bool inlin;            // Step on Reg / Split: the linearization inside the solve launch
    bool fused;            // ClosedRun on Reg / Split: one fused launch; otherwise one launch sequence per step
    size_t base;           // ws_base_bytes (0 for the QP entry)
    size_t scratch_off;    // the solver's scratch inside the caller's workspace ...
    size_t scratch_bytes;  // ... and its size (Long / General: the general solver's allowance, sb_bytes)
    size_t need;           // bytes the entry point requires
};

constexpr double BOUND_INF = 1e30;   // a state bound at or beyond it adds no rows (INFTY of mpc_common.h)

// state bounds (mpc_6stati.py:208-213) with at least one finite side
inline bool state_bounds_active(const traj_mpc_config* c) {
    for (int i = 0; i < 6; ++i) {
        if (c->has_x_lo && c->x_lo[i] > -BOUND_INF) return true;
        if (c->has_x_hi && c->x_hi[i] < BOUND_INF) return true;
    }
    return false;
}

inline int check_cfg(const traj_mpc_config* c) {
    if (!c) return TRAJ_E_ARG;
    if (c->N < 1 || c->N > TRAJ_MAX_N_GENERAL) return TRAJ_E_ARG;
    if (!(c->Ts > 0.0) || c->max_iter < 1 || c->check_interval < 1 || c->scaling_iters < 0) return TRAJ_E_ARG;
    if (c->polish_mode != 0 && c->polish_mode != 1) return TRAJ_E_ARG;
    // the solver settings OSQP itself validates (osqp_api: validate_settings), each written so that NaN fails
    if (!(c->rho > 0.0) || !(c->sigma > 0.0) || !(c->delta > 0.0)) return TRAJ_E_ARG;
    if (!(c->alpha > 0.0 && c->alpha < 2.0)) return TRAJ_E_ARG;
    if (!(c->eps_abs >= 0.0) || !(c->eps_rel >= 0.0) || (c->eps_abs == 0.0 && c->eps_rel == 0.0)) return TRAJ_E_ARG;
    if (!(c->eps_prim_inf > 0.0) || !(c->adaptive_rho_tol >= 1.0) || !(c->cert_tol >= 0.0)) return TRAJ_E_ARG;
    if (c->polish_refine_iter < 0 || c->polish_max_pass < 0 || c->polish_max_rounds < 0) return TRAJ_E_ARG;
    return TRAJ_OK;
}

// The base part of the workspace, as byte offsets from its start -- the one statement of where each region lies:
//   doubles  A [B,N,36] | Bm [B,N,12] | g [B,N,6] (the linearization's hand-off) | xf [B,N,12] (the rollout record) |
//            warm [B,4] (the warm-start records)
//   ints     order [B] (the closed loop's solve order) | the fused run's step queue, queue_bytes from q_count:
//            q_count (next work item) | q_err (error flag) | q_done [B] (steps completed) | q_claimed [B]
// total is the base part's size, a multiple of 8.
struct WsLayout {
    size_t A, Bm, g, xf, warm, order, q_count, q_err, q_done, q_claimed, queue_bytes, total;
};
inline WsLayout layout(int B, int N) {
    const size_t b = (size_t)B, bn = b * (size_t)N, d = sizeof(double), i = sizeof(int);
    WsLayout w;
    w.A = 0;
    w.Bm = w.A + bn * 36 * d;
    w.g = w.Bm + bn * 12 * d;
    w.xf = w.g + bn * 6 * d;
    w.warm = w.xf + bn * 12 * d;
    w.order = w.warm + b * 4 * d;
    w.q_count = w.order + b * i;
    w.q_err = w.q_count + i;
    w.q_done = w.q_err + i;
    w.q_claimed = w.q_done + b * i;
    w.queue_bytes = w.q_claimed + b * i - w.q_count;
    w.total = (w.q_count + w.queue_bytes + 7) & ~(size_t)7;
    return w;
}
inline size_t ws_base_bytes(int B, int N) { return layout(B, N).total; }
// the row-split kernel's P scratch inside the workspace (after the base part): every horizon it can run, whatever the
// routing, so that traj_mpc_workspace_bytes does not depend on a debug switch (+ 2 doubles: 16-byte alignment slack)
inline size_t split_bytes(int B, int N) {
    return (N >= TRAJ_SPLIT_MIN_N && N <= TRAJ_MAX_N_SPLIT) ? ((size_t)B * split_ws_doubles(N) + 2) * sizeof(double) : 0;
}
// the general solver's scratch; the long-horizon kernel's fits in it (long_ws_doubles <= gen_ws_doubles past TRAJ_MAX_N)
inline size_t sb_bytes(int B, int N) { return (size_t)B * gen_ws_doubles(N) * sizeof(double); }
// the closed loop on the general solver: its scratch after the base part, then the step's window [B, N+1, 3], u_cmd
// [B, 2] and a status row [B] (int) -- and never less than traj_mpc_workspace_bytes, which traj_closed_loop_check takes
inline size_t closed_sb_bytes(int B, int N) {
    const size_t e = ws_base_bytes(B, N) + sb_bytes(B, N) +
                     ((size_t)B * (3 * (size_t)(N + 1) + 2) + ((size_t)B + 1) / 2) * sizeof(double);
    const size_t w = ws_base_bytes(B, N) + split_bytes(B, N);
    return e > w ? e : w;
}

inline Route route(const traj_mpc_config* c, int B, Entry e, const Switches& s) {
    Route r{};
    r.err = B < 0 ? TRAJ_E_ARG : check_cfg(c);
    if (r.err) return r;
    const int N = c->N;
    const bool bounds = state_bounds_active(c);
    const bool closed = e == Entry::ClosedStep || e == Entry::ClosedRun;
    if (bounds || N > TRAJ_MAX_N_LONG) r.tier = Tier::General;
    else if (N >= s.split_min_n && N <= s.split_max_n && (e != Entry::Qp || N > TRAJ_MAX_N)) r.tier = Tier::Split;
    else r.tier = N > TRAJ_MAX_N ? Tier::Long : Tier::Reg;
    const bool scratch_after = r.tier == Tier::Long || r.tier == Tier::General;   // past the row-split region
    r.inlin = e == Entry::Step && s.step_inlin && !scratch_after;
    r.fused = e == Entry::ClosedRun && !scratch_after;
    r.base = e == Entry::Qp ? 0 : ws_base_bytes(B, N);
    r.scratch_off = r.base;
    if (e == Entry::Qp) {
        // (the row-split kernel's share of it would do at 41..64; the entry has always asked for the whole)
        r.scratch_bytes = r.tier == Tier::Reg ? 0 : sb_bytes(B, N);
        r.need = r.scratch_bytes;
    } else {
        r.scratch_bytes = scratch_after ? sb_bytes(B, N) : (r.tier == Tier::Split ? split_bytes(B, N) : 0);
        if (!closed) r.need = r.base + r.scratch_bytes;
        else if (r.tier == Tier::General) r.need = closed_sb_bytes(B, N);
        // the closed loop's workspace is traj_mpc_workspace_bytes (the row-split region whichever kernel runs), the
        // long-horizon kernel's scratch over and after it
        else r.need = r.base + split_bytes(B, N) + (r.tier == Tier::Long ? sb_bytes(B, N) : 0);
    }
    return r;
}

}  // namespace tgmpc

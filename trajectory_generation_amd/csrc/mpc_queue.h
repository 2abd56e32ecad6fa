// mpc_queue.h -- the order of the fused closed loop's work queue (traj_closed_loop_run): item q <-> (step, rank), rank =
// the previous launch's cost order.  Integers only: the fused kernels (mpc_solve.h, mpc_split.h) and a host compiler
// (tests/sanitize/san_queue.cpp) read the same text.
//
// Plain order: all ranks of step 0, then of step 1, ...  With a lead (lead_steps > 0, heavy = ranks < lead_h, the
// instances with the most ADMM iterations in the previous launch): the heavy instances' first lead steps come first,
// then level s holds the heavy instances' step s + lead followed by the light instances' step s -- the long chains are
// not held back by the level front.  Every instance's steps stay in increasing queue order, so an item only ever waits
// for an item drawn before it: no deadlock.
#pragma once

#if defined(__HIPCC__)
#define QUEUE_HD __host__ __device__ __forceinline__
#else
#define QUEUE_HD inline
#endif

namespace tgmpc {

struct QueueOrder {
    int Bq, S;     // instances, steps
    int L, H;      // lead steps (<= S) of the H heavy ranks; both 0 without a lead
    int P, full;   // items of the lead prefix; items of the full levels (every rank present)

    QUEUE_HD QueueOrder(int B, int nsteps, int lead_steps, int lead_h) : Bq(B), S(nsteps) {
        L = (lead_h > 0) ? (lead_steps < S ? lead_steps : S) : 0;
        H = (L > 0) ? lead_h : 0;
        P = L * H;
        full = (S - L) * Bq;
    }
    QUEUE_HD int total() const { return Bq * S; }
    // item q -> (st, rk); returns the queue level of q
    QUEUE_HD int decode(int q, int& st, int& rk) const {
        if (q < P) {
            st = q / H;
            rk = q - st * H;
            return 0;
        }
        const int q1 = q - P;
        if (q1 < full) {
            const int lv = q1 / Bq;
            rk = q1 - lv * Bq;
            st = (rk < H) ? lv + L : lv;
            return lv;
        }
        const int q2 = q1 - full, lv = (S - L) + q2 / (Bq - H);
        rk = H + (q2 - (lv - (S - L)) * (Bq - H));
        st = lv;
        return lv;
    }
    QUEUE_HD int encode(int st, int rk) const {
        if (rk < H) return (st < L) ? st * H + rk : P + (st - L) * Bq + rk;
        return (st < S - L) ? P + st * Bq + rk : P + full + (st - (S - L)) * (Bq - H) + (rk - H);
    }
    QUEUE_HD int level_of(int st, int rk) const { return (rk < H) ? (st > L ? st - L : 0) : st; }
};

}  // namespace tgmpc

#undef QUEUE_HD

// mpc_solve.h -- kernel 2 of the MPC step: condensed TV-LQ QP + OSQP-style ADMM + polish.
//
// Reference hot path: MPC/mpc_6stati.py:180-275 (QP build, prob.solve(OSQP), status, info), with
// the linearization (A_k, B_k, g_k) produced by mpc_linearize.h (or given by the caller for
// traj_mpc_qp_batch) and read from global memory.
//   3. the TV-LQ QP             :180-250  condensed over U (X eliminated by the dynamics)
//   4. the solve                :252-262  OSQP's ADMM (Ruiz scaling, sigma/alpha, adaptive rho,
//                                          OSQP termination) + polish, as restated in oracle/
//   5. status / info            :257-275  u_cmd = U[:,0] or u_prev; X_opt by the linear model
//
// Layout (DESIGN.md "Kernel"): thread i (< n = 2N) owns QP variable i = 2k + channel, its box row
// and its rate row.  The KKT matrix K = P + sigma I + A' diag(rho) A lives ROW-PER-LANE in
// registers and is inverted in place by the symmetric sweep operator (n pivots, each a broadcast
// of one column through LDS), so every ADMM iteration is one dense register mat-vec (n FMAs per
// lane) plus two +-2 neighbour exchanges for the banded constraint rows.  The scaled cost matrix P
// (needed for residuals, rho updates and polish) is kept in LDS as a packed upper triangle.
// Everything is float64, like the reference.
#pragma once
#include "mpc_common.h"
#include "mpc_frame.h"
#include "mpc_linearize.h"
#include "mpc_osqp_rules.h"
#include "mpc_queue.h"

#ifndef TGMPC_PRIO_ITERS
#define TGMPC_PRIO_ITERS 100   // fused run: ADMM iterations after which a solve's wave takes issue priority
#endif

#ifndef TGMPC_KCH
#define TGMPC_KCH 8            // CMP: broadcast values per chunk of the ADMM mat-vec
#endif
#ifndef TGMPC_PCH
#define TGMPC_PCH 4            // CMP: pivot-row double2 per chunk of the sweep
#endif
#ifndef TGMPC_NSTASH
#define TGMPC_NSTASH 3         // 3-wave instance: ADMM iterate rows parked in LDS across the factorization (of 5)
#endif
#ifndef TGMPC_L2W_WPE
#define TGMPC_L2W_WPE 2        // waves per SIMD the lean two-wave instance is built for
#endif
#ifndef TGMPC_KCH_W2
#define TGMPC_KCH_W2 8         // fused one-wave instance at 2 waves per SIMD: broadcast values per mat-vec chunk
#endif
#ifndef TGMPC_PCH_W2
#define TGMPC_PCH_W2 4         // fused one-wave instance at 2 waves per SIMD: pivot-row double2 per chunk
#endif
#ifndef TGMPC_SWEEP_UNROLL
#define TGMPC_SWEEP_UNROLL 8   // one-wave sweep, fused instances: pivots per unrolled loop body (1: rolled, NN register
                               // moves per pivot; 8: +0.9 % over 4 at 20 steps, r04)
#endif
#ifndef TGMPC_SWEEP_UNROLL_STEP
#define TGMPC_SWEEP_UNROLL_STEP 4   // the same for the per-step kernels (8 there spills 20-24 B/lane)
#endif
#ifndef TGMPC_SWEEP_UNROLL2
#define TGMPC_SWEEP_UNROLL2 4  // two-wave sweep (capacity 80): the same
#endif
#ifndef TGMPC_SWEEP_2D
#define TGMPC_SWEEP_2D 1       // fused capacity-40 instance at 2 waves per SIMD: K^-1 swept as 8 x 8 blocks of (NN/8)^2 entries, one
#endif                         // block per lane, all 64 lanes busy (0: the row-per-lane receiver sweep); same values bit for bit
#ifndef TGMPC_KMUL_64
#define TGMPC_KMUL_64 1        // the same instance (needs TGMPC_SWEEP_2D): K^-1 v as 160 chains of 10 fma, one per (row, column
#endif                         // class mod 4), dealt over all 64 lanes (0: 4 chains per row on lanes < NN); same values bit for bit
#define TGMPC_PRAGMA_(x) _Pragma(#x)
#define TGMPC_PRAGMA(x) TGMPC_PRAGMA_(x)
#ifndef TGMPC_KCH80
#define TGMPC_KCH80 40         // capacity 80, one wave per SIMD: broadcast values per chunk of the ADMM mat-vec (round 5,
                               // under the max-ILP scheduler: 40 0.965-0.969 M at config 3, 16 0.952, 80 0.946, 20 0.935,
                               // 8 0.933; profiles/r05_cap80_knobs_ab.txt)
#endif
#ifndef TGMPC_PCH80
#define TGMPC_PCH80 4          // capacity 80, one wave per SIMD: pivot-row double2 per chunk of the sweep
#endif
#ifndef TGMPC_PCH2
#define TGMPC_PCH2 4           // L2W: pivot-row double2 per chunk of the two-wave sweep
#endif

namespace tgmpc {

// Fused closed loop: an instance's state (x, u_prev, warm record) passes between workgroups -- on any XCD
// -- without agent-scope release/acquire fences.  A release at agent scope writes back the whole XCD L2
// (buffer_wbl2), which at one hand-off per work item flushed the solve's spill lines to HBM (10.4 GB per
// 200-step launch).  Instead (MI355X_MICROARCH.md, cross-workgroup publish): the state is stored with
// coherent (sc1) stores, the storing lane waits for them (vmcnt(0)), then stores the step counter sc1;
// the consumer polls the counter with sc1 loads and reads the state with sc1 loads.
// (st_coh / ld_coh: mpc_common.h)

// =====================================================================================
// NN = capacity in QP variables (>= 2N); CLOSED = closed-loop step (window from the state, plant
// update, history).  A_k, B_k, g_k are read from a.Ad / a.Bd / a.gd ([B,N,36], [B,N,12], [B,N,6]).
// =====================================================================================
// DIAG: the diagnostics (a.dbg stamps, a.dbg_items timeline) are compiled in; the fused launch uses the
// DIAG = false instance unless a diagnostic buffer is set (their counters cost registers in every phase)
// WPS: waves per SIMD the register allocation is held to (fused one-wave kernels: 2, or 3 -- 168 VGPRs, the
// compact LDS image; mpc_inst_w3.hip).
// INLIN: the linearization runs in the workgroup (block_linearize, stage records in LDS) -- the fused closed loop,
// and the step entry point (traj_mpc_step_batch: one launch per call instead of rollout + Jacobian + solve; the
// records are copied to the workspace's A/B/g for X_opt).  Same values as rollout_kernel + jac_kernel.
template <int NN, bool CLOSED, bool FUSED = false, bool DIAG = true, int WPS = 2, bool INLIN = FUSED>
// (one wave per instance: WPS waves per SIMD; capacity 80, two waves per instance: one wave per SIMD, or, fused
// with WPS = 2, two -- the lean two-wave instance below)
__global__ __launch_bounds__(((NN + 63) / 64) * 64) __attribute__((amdgpu_waves_per_eu(
    NN <= 64 ? WPS : ((FUSED && WPS >= 2) ? TGMPC_L2W_WPE : 1)))) void solve_kernel(const KArgs a0) {
    constexpr int WAVES = (NN + 63) / 64;
    static_assert(WAVES <= 2, "one or two waves per instance");
    constexpr int NT = WAVES * 64;
    constexpr int NM = NN / 2;          // max horizon
    constexpr int NP0 = NN * (NN + 1) / 2;

    // CMP (fused, one wave): the compact LDS image -- at most 13 KB, so that 12 workgroups (3 waves per
    // SIMD) fit a CU's 160 KB.  One wave's LDS operations complete in program order, so buffers whose
    // lives do not overlap share one region (see s_scr).
    constexpr bool CMP = FUSED && WAVES == 1;
    // LEAN (the 3-wave instance): values parked in / re-formed from LDS around the factorization, a rolled P v
    // -- register savings the 2-wave instance does without (same arithmetic, same results)
    // L2W (fused, two waves per instance at capacity 80, WPS = 2): 4 instances per CU instead of 2 -- 256
    // registers per lane and <= 40 KB of LDS: cold rows of NN, the sweep's pivot columns in the exchange region,
    // the window in s_big past the stage records, chunked pivot-row / broadcast reads and the LEAN parking
    constexpr bool L2W = FUSED && WAVES == 2 && WPS >= 2;
    constexpr bool LEAN = (CMP && WPS >= 3) || L2W;
    static_assert(!L2W || CLOSED, "the lean two-wave instance is the fused closed loop");
    // FULLP: the scaled P kept in LDS as the FULL symmetric matrix, row t at s_P + PS t (the packed upper triangle
    // otherwise): every row read -- the K build, P v in the residual checks and the polish, the row after the
    // penalties -- is NN / 2 contiguous ds_read_b128 from one base address instead of NN scattered reads with
    // per-entry address selects, and the scaled rows are written back whole.  The same values in the same
    // arithmetic (each lane reads exactly the entries it read from the packed triangle, which every writer keeps
    // symmetric bit for bit), so the results do not change.  Costs (NN - 1) NN / 2 doubles more LDS: 6.2 KB at
    // capacity 40 -- the fused 2-wave instance's image grows to 19.0 KB, still 8 workgroups per CU; the 3-wave
    // instance's 12.8 KB budget and the per-step kernels' staging tail keep the packed form.
    // (and the fused capacity-80 instance at one wave per SIMD: 73 KB per workgroup, 2 per CU as before)
    constexpr bool FULLP = FUSED && !LEAN;
    // FULLP row stride PS = NN + 2 doubles (2 PS = 4 mod 8 dwords): a row-per-lane 16-byte read puts 16 consecutive
    // lanes on 16 distinct 4-bank groups (stride NN = 40 maps every 4th lane to the same banks: 16-way conflicts)
    constexpr int PSPAD = 2;
    constexpr int PS = FULLP ? NN + PSPAD : NN;
    // SW2D: the factorization sweep over an 8 x 8 grid of lanes, each holding a BSW x BSW block of K (see the sweep).
    // The fused capacity-40 instance at two waves per SIMD; the 3-wave, lean, per-step and other
    // capacities' instances keep the row-per-lane sweep (identical arithmetic: they cross-check this one).
    constexpr bool SW2D = TGMPC_SWEEP_2D && CMP && !LEAN && FULLP && NN == 40;
    constexpr int BSW = NN / 8;
    constexpr int ST2 = NN + 2;   // SW2D: row stride of the staging area that turns blocks back into rows
    // K64: the ADMM / polish mat-vec K^-1 v by column class.  Row r's sum is four independent chains, chain c over the
    // columns = c mod 4 in ascending order; lane 16 c + m runs chain c of up to three rows (slots), so all 64 lanes
    // issue useful fma: 30 per mat-vec instead of 40, 5 broadcast reads instead of 20, 30 doubles of K^-1 instead of
    // 40.  Row 5 q + k lives in lane m = q + 8 (k & 1) (k = 4: m = q), slot k / 2: lanes m < 8 hold three rows, the
    // others two and an exact zero slot.  The four partial sums of a row go through LDS to lane r, which adds them in
    // the row form's association -- the same operations on the same operands, so the same bits.
    constexpr bool K64 = TGMPC_KMUL_64 && SW2D;
    constexpr int KCL = NN / 4;                   // entries of a row per column class
    constexpr int KPA = NN;                       // s_u: partials of classes 0, 1 at KPA + 2 r + c (after the vector)
    constexpr int KPB = KPA + 2 * 64;             //      classes 2, 3 at KPB + 2 r + (c - 2); lanes >= NN read in bounds
    constexpr int KPD = KPB + 2 * 64;             //      32 words nobody reads, for the absent slots' stores
    static_assert(!FULLP || (2 * PS) % 8 == 4, "conflict-free row stride");
    constexpr int NP = FULLP ? NN * PS : NP0;
    __shared__ double s_pref0[(CMP || L2W) ? 2 : 3 * (NM + 1)];
    __shared__ double s_vref0[(CMP || L2W) ? 2 : NM + 1];
    __shared__ double s_x0[6], s_up[2];
    __shared__ int s_item;
    // one region, two lives: A_k, B_k, g_k of every stage staged for the condensing (fused: stage records
    // [A_k 36 | B_k 12 | g_k 6], which also hold block_linearize's scratch for the stage), then (once P is
    // formed) the scaled P as a packed upper triangle (row-major) + per-lane cold values (rows of CS; CMP:
    // NN wide: the spare lanes read the next row's values, or lane CS-1's pair, and never use them)
    constexpr int CS = (WAVES == 1 || L2W) ? NN : NT;
    // the two-wave receiver sweep (capacity 80; the lean two-wave instance too): rows start shifted by SP2 lanes
    constexpr bool RECV2 = WAVES == 2;
    constexpr int SP2 = 64 * WAVES - NN;
    constexpr int NCOLD = 11 * CS;   // 5 single rows + 3 pair rows (see the cold values below)
    constexpr int NLIN = 54 * NM;
    // (L2W: the window -- X*, Y*, phi*, vref, sin / cos(phi*) -- after the stage records, read up to the condensing)
    constexpr int NLINW = NLIN + (L2W ? 6 * (NM + 1) : 0);
    constexpr int NBIG0 = (NP + NCOLD > NLINW) ? NP + NCOLD : NLINW;
    constexpr int NDMA = INLIN ? 0 : 2 * NT * ((27 * NM + NT - 1) / NT);   // the LDS-DMA staging tail (below)
    constexpr int NBIG = NBIG0 > NDMA ? NBIG0 : NDMA;
    __shared__ __attribute__((aligned(16))) double s_big[NBIG];
    double* const s_P = s_big;
    double* const s_cold = s_big + NP;
    __shared__ double s_xh[CLOSED ? 6 : (NM + 1) * 6];   // X_opt by the linear model (not in the closed loop)
    __shared__ double s_sc0[(CMP || L2W) ? 2 : (NM + 1) * 2];
    // exchange buffers: 4 rotating slots of NN (+ 2 more for the two-wave condensing's 2 x 3 NN), and for
    // two waves 3 fixed slots (4, 5, 6) for the ADMM loop's three exchanges, so no rotating index lives
    // across that loop (at NN = 80 it was spilled and reloaded from scratch in every exchange)
    constexpr int NEX = (WAVES > 1) ? (4 * NN + 3 * NT > 6 * NN ? 4 * NN + 3 * NT : 6 * NN) : (CMP ? 4 * NN : 6 * NN);
    // sweep pivot columns: 2 slots of 2 NN + 2 doubles
    constexpr int NSW = 2 * (2 * NN + 2);
    constexpr int FS = 16 * ((NN + 15) / 16);
    constexpr int NFS = (WAVES > 1) ? 0 : (CMP ? 1 : 2) * 4 * FS;   // condensing F_k rows: slots of 4 x FS (one wave)
    // CMP: one scratch region for the exchange / broadcast slots (ADMM, Ruiz, polish), the sweep's pivot
    // columns (factorization), the condensing's F rows and the residual transposition (8 NN + 8) -- each
    // phase leaves nothing there the next one reads.  Otherwise: exchange + sweep buffers, and s_F apart.
    constexpr int NSCR0 = (NEX > NSW) ? NEX : NSW;
    constexpr int NWIN = CMP ? 6 * (NM + 1) : 0;   // CMP: the window and sin/cos(phi*) after the F slot
    constexpr int NSCR1 = (NFS + NWIN > 8 * NN) ? NFS + NWIN : 8 * NN;
    // CMP: the ADMM iterate (x, z, y: 5 rows of NN) is parked past the pivot columns during each K build + sweep
    // (the 3-wave instance parks TGMPC_NSTASH of the 5 rows: with 3 the LDS image is <= 12,800 B, so 12 workgroups
    // fit a CU's 160 KB at gfx950's 1,280-byte allocation granule instead of 11)
    constexpr int NSTR = (CMP && LEAN) ? TGMPC_NSTASH : 5;
    constexpr int NSTASH = LEAN ? ((NSW + 1) & ~1) + NSTR * NN : 0;
    constexpr int NU0 = CMP ? ((NSCR0 > NSCR1) ? NSCR0 : NSCR1) : (L2W ? NSCR0 : NEX + NSW);
    constexpr int NU1 = NU0 > NSTASH ? NU0 : NSTASH;
    // SW2D: 8 staged rows of K^-1 (one local block row of every lane) in the region the sweep leaves dead
    constexpr int NU = (SW2D && 8 * ST2 > NU1) ? 8 * ST2 : NU1;
    __shared__ __attribute__((aligned(16))) double s_u[NU];
    static_assert(!K64 || (KPD + 32 <= NU && KCL % 2 == 0 && KPA % 2 == 0), "K64: the partial sums' area");
    double* const s_ex = s_u;                     // exchange / broadcast buffers
    double* const s_sw = (CMP || L2W) ? s_u : s_u + NEX;   // sweep pivot columns (16-byte aligned: NEX is even)
    __shared__ __attribute__((aligned(16))) double s_F0[(CMP || WAVES > 1) ? 2 : NFS];
    double* const s_F = CMP ? s_u : s_F0;         // condensing: F_k rows; residual maxima
    // the reference window (X*, Y*, phi*) and vref of the stages, sin / cos(phi*_k): CMP keeps them in s_u past
    // the F slot -- read only up to the condensing (the closed loop reports no X_opt or objective)
    double* const s_pref = CMP ? s_u + NFS : (L2W ? s_big + NLIN : s_pref0);
    double* const s_vref = CMP ? s_u + NFS + 3 * (NM + 1) : (L2W ? s_big + NLIN + 3 * (NM + 1) : s_vref0);
    double* const s_sc = CMP ? s_u + NFS + 4 * (NM + 1) : (L2W ? s_big + NLIN + 4 * (NM + 1) : s_sc0);
    __shared__ double s_red[WAVES > 1 ? 16 * WAVES : 2];
    __shared__ int s_flag[4];
    // PARK: stage 0's atan2, rear tire sine and sin / cos(phi_0) of the in-workgroup linearization, kept for the plant
    // update at the item's end (plant_update_parked) -- 32 bytes that outlive the solve.  The 3-wave instance's image
    // has 24 bytes to spare: it keeps the plant that evaluates f(x_0, u_cmd) whole.
    constexpr bool PARK = CLOSED && INLIN && !(CMP && WPS >= 3);
    __shared__ double s_park[PARK ? 4 : 1];
    // The static LDS image of a fused one-wave instance (CMP): s_big, s_u, s_x0, s_up, s_xh, s_item (padded to 8 bytes),
    // s_flag and (PARK) s_park -- the 2-double placeholders above and s_red have no reader there and take no space.
    // It decides the occupancy the kernel is tuned for, of a CU's 160 KB: at capacity 40, 8 workgroups (2 waves per
    // SIMD) need <= 20,480 B and 12 (the 3-wave instance) <= 12,800 B; the images are 19,816 B and 12,776 B, the
    // compiler's group_segment_fixed_size.
    constexpr int LDS_CMP = sizeof(s_big) + sizeof(s_u) + sizeof(s_x0) + sizeof(s_up) + sizeof(s_xh) + 8 + sizeof(s_flag) +
                            (PARK ? sizeof(s_park) : 0);
    static_assert(!(CMP && NN == 40 && WPS == 2) || LDS_CMP <= 20480, "LDS image: 8 workgroups per CU");
    static_assert(!(CMP && NN == 40 && WPS >= 3) || LDS_CMP <= 12800, "LDS image: 12 workgroups per CU");

    // Fused closed loop (traj_closed_loop_run): nsteps steps of this instance in one launch -- the
    // state, u_prev and the warm-start rho stay on chip and the linearization runs in the
    // workgroup (block_linearize), so no instance waits for the slowest one of a step.  The whole
    // body is the loop body, with the thread index passed through an opaque move each step so that
    // nothing per-lane is hoisted out of the loop (it would stay live across the solve and spill).
    constexpr bool fused = FUSED;
    // fused: the grid is the resident workgroups; each takes work items (step, rank) from a queue in
    // order -- all ranks of step 0, then of step 1, ... (rank = the previous launch's cost order) --
    // and waits, if it must, until the instance's previous step is complete.  The instance state
    // (x, u_prev, warm-start record) passes between workgroups through global memory -- coherent (sc1) stores
    // drained with vmcnt(0), then the per-instance step counter stored sc1; the consumer polls the counter and
    // reads the state with sc1 loads (st_coh / ld_coh above, the hand-off at the end of the item) -- so a slow
    // solve delays only its instance
    // and every slot stays busy until the queue is drained.
    bool more = true;
    int item_of_wave = 0;   // fused: the current work item (diagnostics)
    int ra_step = 0, ra_rank = 0;   // fused: the instance (rank) this workgroup just stepped, and its next step
    for (int step = 0; more; ++step) {
    // fused: the arguments are read through a pointer the compiler cannot see through, so nothing
    // derived from them (weights, reciprocals, per-stage predicates, address offsets) is hoisted out of
    // the step loop -- hoisted, those values stay live across the whole solve and spill
    typedef __attribute__((address_space(4))) const KArgs* KArgsPtr;   // constant (kernarg) space: s_load
    // (a0 is the kernel's only argument: it sits at offset 0 of the kernarg segment; &a0 would copy it
    // to private memory)
    KArgsPtr ap = FUSED ? (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr() : (KArgsPtr) nullptr;
    if constexpr (FUSED) asm volatile("" : "+s"(ap));
    const KArgs& a = FUSED ? *(const KArgs*)ap : a0;
    long long* const dbg = DIAG ? a.dbg : nullptr;               // diagnostics, or null
    long long* const dbg_items = DIAG ? a.dbg_items : nullptr;
    int b = (CLOSED && a.perm) ? a.perm[blockIdx.x] : (int)blockIdx.x;
    if constexpr (FUSED) {
        const QueueOrder qo(a.B, a.nsteps, a.lead_steps, a.lead_h);   // item q <-> (step, rank): mpc_queue.h
        // Run-ahead (a.run_ahead > 0): the workgroup that completed (step - 1, rank) claims the instance's next
        // step itself while that step is at most run_ahead levels past the draw front -- an instance whose steps
        // are cheap runs ahead of the level order, so a long chain (a solve at the iteration cap late in the
        // launch) starts its heavy steps earlier.  Every item is claimed exactly once: a per-instance counter
        // (queue[2 + B + b] = steps of b claimed) taken by compare-and-swap from the value `step`, by the
        // run-ahead or by the drawer of q; a drawer whose item was run ahead draws again.  The drawer of (s, b)
        // waits, if it must, only for the claim of (s - 1, b), whose queue item was drawn before its own.
        __syncthreads();
        if (threadIdx.x == 0) {
            int* const claim = a.queue + 2 + qo.Bq;
            const int total = qo.total();
            int got = -1;
            if (a.run_ahead > 0 && ra_step > 0 && ra_step < qo.S) {
                int fs, fr;
                const int front = __hip_atomic_load(&a.queue[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int flv = (front < total) ? qo.decode(front, fs, fr) : qo.S;
                const int rlv = qo.level_of(ra_step, ra_rank);
                const int rb = a.perm ? a.perm[ra_rank] : ra_rank;
                if (rlv <= flv + a.run_ahead && atomicCAS(&claim[rb], ra_step, ra_step + 1) == ra_step) {
                    got = qo.encode(ra_step, ra_rank);
                    if (dbg_items) dbg_items[4 * (size_t)got] = __builtin_amdgcn_s_memrealtime();
                }
            }
            while (got < 0) {
                const int q = atomicAdd(&a.queue[0], 1);
                if (q >= total) { got = q; break; }
                const long long t_draw = __builtin_amdgcn_s_memrealtime();
                if (a.run_ahead <= 0) { got = q; }
                int qs, qr;
                qo.decode(q, qs, qr);
                const int qb = a.perm ? a.perm[qr] : qr;
                int spins = 0;
                for (; got < 0;) {
                    const int cl = __hip_atomic_load(&claim[qb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cl > qs) break;                                              // run ahead: draw again
                    if (cl == qs) {
                        if (atomicCAS(&claim[qb], qs, qs + 1) == qs) { got = q; break; }
                        continue;
                    }
                    __builtin_amdgcn_s_sleep(1);   // (s - 1, b) drawn, its claim not yet made
                    if (++spins > a.spin_limit) {
                        __hip_atomic_store(&a.queue[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        got = q;
                        break;
                    }
                }
                if (got >= 0 && dbg_items) dbg_items[4 * (size_t)q] = t_draw;   // (a run-ahead item: its claimer's)
            }
            s_item = got;
        }
        __syncthreads();
        const int q = s_item;
        if (q >= a.B * a.nsteps) break;
        int rank;
        qo.decode(q, step, rank);
        ra_step = step + 1;
        ra_rank = rank;
        item_of_wave = q;
        b = a.perm ? a.perm[rank] : rank;
        // issue priority (s_setprio): the wave that works on a long chain gets the SIMD first -- see the
        // ADMM loop; every item starts at the default priority
        __builtin_amdgcn_s_setprio(0);
        if (threadIdx.x == 0 && step > 0) {
            int spins = 0;
            while (__hip_atomic_load(&a.queue[2 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < step) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > a.spin_limit) {   // bounded: a lost hand-off is reported, never a hang
                    // (traj_closed_loop_run's caller gets TRAJ_E_HANDOFF from traj_closed_loop_check)
                    __hip_atomic_store(&a.queue[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
        __syncthreads();
        if (dbg_items && threadIdx.x == 0) {   // diagnostics: item timeline (traj_debug_set_item_stamps)
            dbg_items[4 * (size_t)q + 1] = __builtin_amdgcn_s_memrealtime();
            dbg_items[4 * (size_t)q + 3] = blockIdx.x;
        }
        if (dbg && threadIdx.x == 0 && step == 0) {   // diagnostics: start, HW_ID, XCC_ID
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            dbg[(size_t)b * 32 + 22] = __builtin_amdgcn_s_memrealtime();
            dbg[(size_t)b * 32 + 24] = hw;
            dbg[(size_t)b * 32 + 25] = xcc;
        }
    } else {
        more = false;
    }
    const int tstep = a.t + step;
    const traj_vehicle_params& p = a.p;
    const traj_mpc_config& c = a.c;
    int t = threadIdx.x;
    if constexpr (FUSED) asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"((int)threadIdx.x));
    const int lane = t & 63, wid = t >> 6;
    const int N = c.N, n = 2 * N;
    const double Ts = c.Ts;
    const bool own = t < n;             // owns variable / rows t
    const int kk = t >> 1, ch = t & 1;  // stage and channel of variable t
    int xb = 0;                         // rotating exchange buffer
    auto stamp = [&](int i, long long v) {
        if (dbg && t == 0) dbg[(size_t)b * 32 + i] = v;
    };
    stamp(0, __builtin_amdgcn_s_memtime());

    // ---- block helpers -------------------------------------------------------------
    auto exch = [&](double v, int delta) -> double {   // value of variable t+delta (0 outside)
        if constexpr (WAVES == 1) {
            // delta is +-2 at every call site: two DPP wave shifts, no LDS round trip.  Shifting down, an own
            // lane t >= 2 reads own lane t - 2 and lanes 0, 1 get the DPP bound's 0, so only the upward shift
            // zeroes the source (lanes n, n + 1 feed own lanes n - 2, n - 1)
            const double vm = (delta > 0 && !own) ? 0.0 : v;
            const double r = (delta > 0) ? lane_up2(vm) : lane_dn2(vm);
            return own ? r : 0.0;
        } else {
            double* buf = s_ex + (xb & 3) * NN;
            xb++;
            if (own) buf[t] = v;
            __syncthreads();
            int s = t + delta;
            return (own && s >= 0 && s < n) ? buf[s] : 0.0;
        }
    };
    auto bcast = [&](double v) -> double* {            // publish v_t for all, returns buffer
        // (CMP: one slot -- the previous broadcast's reads precede this write in the wave's LDS order)
        double* buf = CMP ? s_ex : s_ex + (xb & 3) * NN;
        if constexpr (!CMP) xb++;
        // (every lane < NN writes: entries n .. NN-1 are the zero padding the register loops over NN read,
        // and in the compact image another phase may have used the slot)
        if (t < NN) buf[t] = own ? v : 0.0;
        __syncthreads();
        return buf;
    };
    // two waves, ADMM loop: the same exchange / broadcast through a fixed slot (see NEX).  The exchange
    // slots are NT wide and every lane writes: a non-own lane's value is never read by an own lane (reads
    // stop at s < n), and what non-own lanes receive only ever reaches non-own lanes -- so no lane flag
    // has to stay live across the loop
    auto exch_at = [&](double v, int delta, int slot) -> double {
        double* buf = s_ex + 4 * NN + (slot - 4) * NT;
        buf[t] = v;
        __syncthreads();
        const int s = t + delta;
        return (s >= 0 && s < n) ? buf[s] : 0.0;
    };
    auto bcast_at = [&](double v, int slot) -> double* {
        double* buf = s_ex + 4 * NN + (slot - 4) * NT;
        if (own) buf[t] = v;
        __syncthreads();
        return buf;
    };
    auto block_max = [&](auto& v) {                   // in-place max over the block (uniform result)
        constexpr int V = sizeof(v) / sizeof(double);
        if (WAVES == 1) {
            wave_max_dpp<V>(v);
        } else {
            wave_max<V>(v);
            if (lane == 0)
                for (int i = 0; i < V; ++i) s_red[wid * V + i] = v[i];
            __syncthreads();
            for (int i = 0; i < V; ++i) {
                double m = s_red[i];
                for (int w = 1; w < WAVES; ++w) m = fmax(m, s_red[w * V + i]);
                v[i] = m;
            }
            __syncthreads();
        }
    };
    auto block_sum = [&](double v) -> double {
        if (WAVES == 1) {
            v = wave_sum_dpp(v);
        } else {
            v = wave_sum(v);
            if (lane == 0) s_red[wid] = v;
            __syncthreads();
            double s = 0.0;
            for (int w = 0; w < WAVES; ++w) s += s_red[w];
            __syncthreads();
            v = s;
        }
        return v;
    };

    // ---- 0. inputs -----------------------------------------------------------------
    if (t == 0) { s_flag[0] = 0; s_flag[1] = 0; }
    // exchange buffers start at zero: entries >= n are the zero padding the unguarded
    // register loops over the full capacity NN rely on
    for (int i = t; i < NEX; i += NT) s_ex[i] = 0.0;
    for (int i = t; i < NFS; i += NT) s_F[i] = 0.0;
    load_state<CLOSED, FUSED>(a, b, t, s_x0, s_up);
    {
        // (the row's address from the uniform instance and step: scalar, none of it in the lanes' registers)
        const double* vr = vref_at(a, __builtin_amdgcn_readfirstlane(b), __builtin_amdgcn_readfirstlane(tstep));
        for (int i = t; i < N + 1; i += NT) s_vref[i] = vr[i];
    }
    if (!CLOSED)
        for (int i = t; i < 3 * (N + 1); i += NT) s_pref[i] = a.path_ref[(size_t)3 * (N + 1) * b + i];
    __syncthreads();
    if (CLOSED) {
        build_window(a, b, N, Ts, s_x0, s_vref, s_pref, t, NT);
        __syncthreads();
    }
    {
        int bad = 0;
        for (int i = t; i < 3 * (N + 1); i += NT) bad |= !isfinite(s_pref[i]);
        for (int i = t; i < N + 1; i += NT) bad |= !isfinite(s_vref[i]);
        if (t < 6) bad |= !isfinite(s_x0[t]);
        if (t < 2) bad |= !isfinite(s_up[t]);
        if (bad) s_flag[0] = 1;
    }

    stamp(1, __builtin_amdgcn_s_memtime());
    const double* gA = a.Ad + (size_t)b * N * 36;   // this instance's linearization
    const double* gB = a.Bd + (size_t)b * N * 12;
    const double* gg = a.gd + (size_t)b * N * 6;
    stamp(2, __builtin_amdgcn_s_memrealtime());   // 100 MHz wall clock (comparable across XCDs)
    // ---- 3. condensed QP (:180-250) --------------------------------------------------
    // A_k, B_k, g_k staged in LDS (coalesced copy); rows are then read as uniform broadcasts
    if constexpr (INLIN) {
        // A_k, B_k, g_k as stage records (LREC doubles each) in s_big
        // (with the sin / cos of the window's phi*_k on its up-front sincos lanes, and the plant's stage-0 values parked)
        block_linearize<NT, true, PARK>(t, p, N, Ts, s_x0, s_up, s_big, dbg ? dbg + (size_t)b * 32 : nullptr,
                                        s_pref + 2, s_sc, s_park);
        if constexpr (!FUSED) {
            // the step entry point reports X_opt by the linear model (read back from A/B/g at the end)
            double* const wA = const_cast<double*>(gA);
            double* const wB = const_cast<double*>(gB);
            double* const wg = const_cast<double*>(gg);
            for (int i = t; i < 54 * N; i += NT) {
                const int k = i / 54, e = i - 54 * k;
                const double v = s_big[LREC * k + e];
                if (e < 36) wA[36 * k + e] = v;
                else if (e < 48) wB[12 * k + e - 36] = v;
                else wg[6 * k + e - 48] = v;
            }
        }
    } else {
    if (((reinterpret_cast<uintptr_t>(gA) | reinterpret_cast<uintptr_t>(gB) | reinterpret_cast<uintptr_t>(gg)) & 15) == 0) {
        // LDS-DMA (global_load_lds_dwordx4): 16 bytes per lane straight into LDS, all chunks in flight
        // at once (one L2/MALL latency, no VGPRs); the three blocks are contiguous in s_big as double2
        // [A 18N | B 6N | g 3N].  Chunk r lands at s_big2[r NT + lane]; lanes past the end re-load
        // the last element into the unused tail of s_big (NBIG >= 2 NT ceil(27 NM / NT)).
        constexpr int MAXV = (27 * NM + NT - 1) / NT;
        static_assert(NBIG >= 2 * NT * MAXV, "s_big too small for the LDS-DMA staging tail");
        const int nA = 18 * N, nB = 6 * N, nT = 27 * N;
#pragma unroll
        for (int r = 0; r < MAXV; ++r) {
            const int i = min(t + r * NT, nT - 1);
            const double2* src = (i < nA) ? reinterpret_cast<const double2*>(gA) + i
                               : (i < nA + nB) ? reinterpret_cast<const double2*>(gB) + (i - nA)
                                               : reinterpret_cast<const double2*>(gg) + (i - nA - nB);
            __builtin_amdgcn_global_load_lds(src, reinterpret_cast<double2*>(s_big) + r * NT + wid * 64, 16, 0, 0);
        }
    } else {
        for (int i = t; i < 36 * N; i += NT) s_big[i] = gA[i];
        for (int i = t; i < 12 * N; i += NT) s_big[36 * N + i] = gB[i];
        for (int i = t; i < 6 * N; i += NT) s_big[48 * N + i] = gg[i];
    }
    }
    stamp(16, __builtin_amdgcn_s_memtime());
    // stage k's A_k at cA + RA k, B_k at cB + RB k, g_k at cg + RG k (fused: block_linearize's stage records)
    constexpr int RA = INLIN ? LREC : 36, RB = INLIN ? LREC : 12, RG = INLIN ? LREC : 6;
    const double* const cA = s_big;
    const double* const cB = s_big + (INLIN ? 36 : 36 * N);
    const double* const cg = s_big + (INLIN ? 48 : 48 * N);
    // sin / cos of phi*_k for every stage (lane-parallel; INLIN: block_linearize formed them)
    if constexpr (!INLIN) {
        for (int k = t; k <= N; k += NT) {
            double sk, ck;
            pm_sincos(s_pref[3 * k + 2], &sk, &ck);
            s_sc[2 * k] = sk;
            s_sc[2 * k + 1] = ck;
        }
    }
    __syncthreads();
    stamp(17, __builtin_amdgcn_s_memtime());

    // P = sum_k G_k' C_k' 2W C_k G_k and q = sum_k G_k' C_k' 2W e_k, accumulated stage by stage:
    // lane t carries column t of the input sensitivity G_k (6-vector); the free response xh_k and
    // its tracking errors e_k are uniform and computed by every lane.  With the weights split as
    // sqrt(2W), F_k = sqrt(2W) C_k G_k (3 x n per stage) and P = sum_k F_k' F_k.
    //   one wave: P accumulates on the matrix cores -- per stage one k=4 step of
    //     v_mfma_f64_16x16x4 per upper-triangle 16x16 tile (rows 0..2 of the step = F_k, row 3 = 0);
    //     each lane reads just the 1-3 F values of its operand slots;
    //   two waves (NN = 80): each lane accumulates its row, F_t F_j (3 FMAs per entry).
    // Both give an exactly symmetric P (each unordered pair is formed once / by a commutative product).
    double Prow[NN];
    double qi = 0.0;
    // (a fresh copy of the lane index per use, so that nothing derived from it is kept live across phases;
    // lanes >= NN read in-range LDS words for their masked-off rows)
    auto opaque_t = [&]() -> int {
        int r;
        asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(t));
        return r;
    };
    // Row tt of the packed upper triangle, entry j: P(j, tt) = s_P[C_j + tt] for j < tt (C_j uniform) and
    // P(tt, j) = s_P[rt + j] for j >= tt (rt = prow_base(tt), the lane's row start).
    auto prow_entry = [&](int j, int tt, int rt) -> double {
        const int cj = j * NN - (j * (j - 1)) / 2 - j;
        return s_P[(j < tt) ? tt + cj : rt + j];
    };
    auto prow_base = [&](int tt) -> int { return tt * NN - (tt * (tt - 1)) / 2 - tt; };
    auto paddr = [&](int j, int tt) -> int {   // packed upper triangle: P(i, j), i <= j
        return (j < tt) ? (j * NN - (j * (j - 1)) / 2 - j + tt) : (tt * NN - (tt * (tt - 1)) / 2 - tt + j);
    };
    {
        const double sw0 = sqrt(2.0 * c.q_c), sw1 = sqrt(2.0 * c.q_phi), sw2 = sqrt(2.0 * c.q_vx);
        // FREE lane (a spare lane past the variables, when there is one) carries the free response
        // xh as its "G column": the same A_k G FMAs every lane already issues, started from g_k
        // (same operation order as a separate xh recursion, bit for bit); the other lanes read the
        // four components they need back with v_readlane.
        constexpr bool FREE_LANE = WAVES == 1 && NN < 64;   // v_readlane: same wave
        constexpr int FL = NT - 1;
        double xh[6], G[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 6; ++i) xh[i] = s_x0[i];
        if (FREE_LANE && t == FL)
            for (int i = 0; i < 6; ++i) G[i] = s_x0[i];
        constexpr int NB = (NN + 15) / 16;          // 16-wide column blocks (MFMA path)
        constexpr int NTILE = NB * (NB + 1) / 2;
        constexpr int FS = 16 * NB;
        typedef double d4 __attribute__((ext_vector_type(4)));
        d4 acc[WAVES == 1 ? NTILE : 1];
        if constexpr (WAVES == 1) {
#pragma unroll
            for (int i = 0; i < NTILE; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
        } else {
#pragma unroll
            for (int j = 0; j < NN; ++j) Prow[j] = 0.0;
        }
        const int mr = (t >> 4) & 3, mc = t & 15;   // MFMA operand slot of this lane: k-row, column
        // Row r of A_k x (+ v0) as the chain v = fma(A[r][cc], x[cc], v), cc = 0..5.  In the closed loop A_k comes
        // from the in-library linearization, whose structural entries are exact (mpc_linearize.h: f does not read
        // X, Y; f_0, f_1 do not read omega; f_2 = omega; f_3..5 do not read phi -- the central differences of those
        // columns are exactly 0, so A = I + Ts J holds exact 1s and 0s there): rows 0 / 1 = [1 0 a a a 0] /
        // [0 1 a a a 0], row 2 = [0 0 1 0 0 a], rows 3..5 = [0 0 0 a a a].  The chain then skips the zero terms
        // and adds the unit ones (fma(1, x, v) = v + x, fma(0, x, v) = v for finite x): the same values (up to
        // the sign of a zero) with 16 fmas and 3 adds instead of 36 fmas.  The QP entry point (caller's A_k) and
        // the step keep the full chain.
        constexpr bool SPARSE_A = CLOSED;
        auto arow = [&](const double* Ak, int r, const double* x, double v) -> double {
            if constexpr (SPARSE_A) {
                if (r <= 1) {
                    v = v + x[r];
#pragma unroll
                    for (int cc = 2; cc < 5; ++cc) v = fma(Ak[6 * r + cc], x[cc], v);
                } else if (r == 2) {
                    v = v + x[2];
                    v = fma(Ak[6 * 2 + 5], x[5], v);
                } else {
#pragma unroll
                    for (int cc = 3; cc < 6; ++cc) v = fma(Ak[6 * r + cc], x[cc], v);
                }
            } else {
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) v = fma(Ak[6 * r + cc], x[cc], v);
            }
            return v;
        };
        for (int k = 0; k < N; ++k) {
            const double* Ak = cA + RA * k;
            if constexpr (!FREE_LANE) {
                // free response xh_{k+1} = A_k xh_k + g_k (uniform)
                double xn[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) xn[r] = arow(Ak, r, xh, cg[RG * k + r]);
#pragma unroll
                for (int r = 0; r < 6; ++r) xh[r] = xn[r];
            }
            // input sensitivities: columns of inputs applied before stage k propagate, stage k's
            // inputs enter through B_k
            // (branch-free: every lane forms A_k G, then selects -- no divergent exec juggling)
            {
                // (a lane whose input has not entered yet holds G = +0, and A_k G started from +0 is +0 exactly: every
                // lane but the two entering ones takes A_k G -- one select per row instead of two)
                const bool fl = FREE_LANE && t == FL;
                const bool enter = own && (kk == k);
                double Gn[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const double v = arow(Ak, r, G, fl ? cg[RG * k + r] : 0.0);
                    const double bv = cB[RB * k + 2 * r + ch];
                    Gn[r] = enter ? bv : v;
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) G[r] = Gn[r];
                if constexpr (FREE_LANE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) xh[r] = readlane_d(G[r], FL);
                }
            }
            // stage k+1 outputs: tracking errors of the free response, weighted sensitivities
            const int k1 = k + 1;
            const double sk = s_sc[2 * k1], ck = s_sc[2 * k1 + 1];
            const double e0 = sk * (xh[0] - s_pref[3 * k1]) - ck * (xh[1] - s_pref[3 * k1 + 1]);
            const double e1 = xh[2] - s_pref[3 * k1 + 2];
            const double e2 = xh[3] - s_vref[k1];
            const double F0 = sw0 * (sk * G[0] - ck * G[1]), F1 = sw1 * G[2], F2 = sw2 * G[3];
            qi += sw0 * F0 * e0 + sw1 * F1 * e1 + sw2 * F2 * e2;
            if constexpr (WAVES == 1) {
                double* fb = s_F + (CMP ? 0 : (k & 1) * 4 * FS);   // 2 rotating slots (CMP: 1); row 3 and columns >= n stay 0
                if (own) { fb[t] = F0; fb[FS + t] = F1; fb[2 * FS + t] = F2; }
                __syncthreads();
                double opv[NB];
#pragma unroll
                for (int ib = 0; ib < NB; ++ib) opv[ib] = fb[mr * FS + 16 * ib + mc];
                // F_k's columns >= 2 (k + 1) are exact zeros (the inputs of later stages): a tile whose column block
                // starts there adds +-0 to its accumulator and is skipped (bit-identical; stages 0..7 touch one
                // tile of 6 at capacity 40, 56 MFMAs per instance instead of 120 at N = 20)
                int ti = 0;
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
#pragma unroll
                    for (int jb = ib; jb < NB; ++jb, ++ti)
                        if (16 * jb < 2 * k + 2)
                            acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(opv[ib], opv[jb], acc[ti], 0, 0, 0);
            } else {
                double* buf = s_ex + (xb & 1) * 3 * NN;   // 2 rotating slots of 3*NN
                xb++;
                if (own) { buf[t] = F0; buf[NN + t] = F1; buf[2 * NN + t] = F2; }
                __syncthreads();
                // the three F rows in chunks of 8 entries, each chunk's reads then its FMAs (the scheduler would
                // otherwise issue all 240 reads beside the 160 registers of Prow); same FMAs, same order.
                // F_k's columns >= 2 (k + 1) are exact zeros (the inputs of later stages do not move x_{k+1}):
                // their three fmas add exact zeros to the row and are skipped, 8 columns at a time (a uniform
                // branch; bit-identical -- about half of the stage loop's fmas at N = 40)
                const double2* b2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(buf, 16));
#pragma unroll
                for (int c0 = 0; c0 < NN; c0 += 8) {
                    if (c0 >= 2 * k + 2) continue;
                    double2 f0[4], f1[4], f2[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f0[i] = b2[c0 / 2 + i];
                        f1[i] = b2[(NN + c0) / 2 + i];
                        f2[i] = b2[(2 * NN + c0) / 2 + i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        Prow[c0 + 2 * i] = fma(F0, f0[i].x, fma(F1, f1[i].x, fma(F2, f2[i].x, Prow[c0 + 2 * i])));
                        Prow[c0 + 2 * i + 1] = fma(F0, f0[i].y, fma(F1, f1[i].y, fma(F2, f2[i].y, Prow[c0 + 2 * i + 1])));
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
                }
            }
        }
        __syncthreads();
        stamp(18, __builtin_amdgcn_s_memtime());
        if constexpr (WAVES == 1) {
            // accumulator tiles (lane: row 16 ib + mr + 4 reg, column 16 jb + mc) -> packed P -> rows
            int ti = 0;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib)
#pragma unroll
                for (int jb = ib; jb < NB; ++jb, ++ti)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = 16 * ib + ((t >> 4) & 3) + 4 * reg, j = 16 * jb + mc;
                        if constexpr (FULLP) {
                            if (i <= j && j < NN) {
                                s_P[i * PS + j] = acc[ti][reg];
                                s_P[j * PS + i] = acc[ti][reg];
                            }
                        } else {
                            if (i <= j && j < NN) s_P[i * NN - (i * (i - 1)) / 2 + (j - i)] = acc[ti][reg];
                        }
                    }
            __syncthreads();
        }
    }
    // input penalties U'RU and dU'Rd dU (dU_0 = U_0 - u_prev)
    double Rs[4], Rds[4];
    Rs[0] = c.R[0]; Rs[3] = c.R[3]; Rs[1] = Rs[2] = 0.5 * (c.R[1] + c.R[2]);
    Rds[0] = c.Rd[0]; Rds[3] = c.Rd[3]; Rds[1] = Rds[2] = 0.5 * (c.Rd[1] + c.Rd[2]);
    // this thread's rows of Rs / Rds (selects, not a dynamic index: keeps them in registers)
    const double Rs0 = ch ? Rs[2] : Rs[0], Rs1 = ch ? Rs[3] : Rs[1];
    const double Rd0 = ch ? Rds[2] : Rds[0], Rd1 = ch ? Rds[3] : Rds[1];
    const double dmul = (kk < N - 1) ? 2.0 : 1.0;
    if constexpr (WAVES == 1) {
        // One wave: the penalty band goes into the packed P in LDS before the rows are read back.  Row t's
        // upper-triangle entries that get a term: the diagonal; for channel 0 its stage partner (t + 1) and
        // the next stage's two inputs (t + 2, t + 3); for channel 1 the next stage's (t + 1, t + 2).  Each
        // lower entry is the upper entry of another row with the same term bit for bit (Rs[1] = Rs[2],
        // Rds[1] = Rds[2]), so adding each entry once gives the rows the per-entry loop gave.
        if (own) {
            // (FULLP: each upper entry's mirror gets the same sum -- the two were equal bit for bit)
            const int rb0 = FULLP ? t * PS : t * NN - (t * (t - 1)) / 2 - t;   // row t: P(t, j) at rb0 + j (j >= t)
            auto addp = [&](int j, double v) {
                const double nv = s_P[rb0 + j] + v;
                s_P[rb0 + j] = nv;
                if constexpr (FULLP) s_P[j * PS + t] = nv;
            };
            s_P[rb0 + t] = s_P[rb0 + t] + (2.0 * (ch ? Rs1 : Rs0) + 2.0 * (ch ? Rd1 : Rd0) * dmul);
            if (ch == 0) {
                addp(t + 1, 2.0 * Rs1 + 2.0 * Rd1 * dmul);
                if (t + 2 < n) addp(t + 2, -2.0 * Rd0);
                if (t + 3 < n) addp(t + 3, -2.0 * Rd1);
            } else {
                if (t + 1 < n) addp(t + 1, -2.0 * Rd0);
                if (t + 2 < n) addp(t + 2, -2.0 * Rd1);
            }
        }
        __syncthreads();
        const int tt = opaque_t();
        if constexpr (FULLP) {
            const int tr = tt < NN ? tt : NN - 1;
            lds_load_all<NN>(s_P + tr * PS, Prow);
#pragma unroll
            for (int j = 0; j < NN; ++j) Prow[j] = own ? Prow[j] : 0.0;
        } else {
#pragma unroll
            for (int j = 0; j < NN; ++j) Prow[j] = own ? s_P[paddr(j, tt)] : 0.0;
        }
    } else if (own) {
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            const int kj = j >> 1;
            const double rs = (j & 1) ? Rs1 : Rs0, rd = (j & 1) ? Rd1 : Rd0;
            double add = (kj == kk) ? 2.0 * rs + 2.0 * rd * dmul : 0.0;
            add = (j < n && (kj == kk - 1 || kj == kk + 1)) ? -2.0 * rd : add;
            Prow[j] += add;
        }
    }
    stamp(19, __builtin_amdgcn_s_memtime());
    if (own && kk == 0) qi -= 2.0 * (Rd0 * s_up[0] + Rd1 * s_up[1]);

    // constraint rows owned by t: box (U_t) and rate (U_t - U_{t-2}, or U_0 - u_prev)
    double lb = ch ? c.u_lo[1] : c.u_lo[0], ub = ch ? c.u_hi[1] : c.u_hi[0];
    double lr = ch ? c.du_lo[1] : c.du_lo[0], ur = ch ? c.du_hi[1] : c.du_hi[0];
    if (kk == 0) { lr += s_up[ch]; ur += s_up[ch]; }
    const bool has_prev = kk > 0;  // rate row couples t-2
    // non-finite data -> solver error
    {
        int bad = 0;
        if (own) {
            bad |= !isfinite(qi);
#pragma unroll
            for (int j = 0; j < NN; ++j) bad |= !isfinite(Prow[j]);
        }
        if (bad) s_flag[0] = 1;
    }
    // exact feasibility of the box+rate chain (interval propagation); decides INFEASIBLE up front
    if (t < 2) {
        double lo = s_up[t], hi = s_up[t];
        const double dlo = t ? c.du_lo[1] : c.du_lo[0], dhi = t ? c.du_hi[1] : c.du_hi[0];
        const double ulo = t ? c.u_lo[1] : c.u_lo[0], uhi = t ? c.u_hi[1] : c.u_hi[0];
        for (int k = 0; k < N; ++k) {
            double nlo = lo + dlo, nhi = hi + dhi;
            if (nlo < ulo) nlo = ulo;
            if (nhi > uhi) nhi = uhi;
            if (!(nlo <= nhi)) { s_flag[1] = 1; }
            lo = nlo;
            hi = nhi;
        }
    }
    __syncthreads();
    const int early = s_flag[0] ? TRAJ_STATUS_SOLVER_ERROR : (s_flag[1] ? TRAJ_STATUS_INFEASIBLE : -1);

    int status = TRAJ_STATUS_SOLVER_ERROR, iter = 0, pol = 0;
    double xsol = 0.0;  // unscaled U_t at exit

    stamp(4, __builtin_amdgcn_s_memtime());
    if (early < 0) {
        // ---- 4a. Ruiz equilibration + cost scaling (OSQP scale_data) ---------------
        // Prow / qi carry D P D and D q; the cost factor cs (uniform, > 0) is applied once at the end,
        // so the column norms of the scaled P are cs * cn with cn = max_j |Prow_j|, tracked in the
        // scaling pass itself (one pass over the row per iteration instead of four).
        double D = 1.0, Eb = 1.0, Er = 1.0, cs = 1.0;
        // (maxima in 4 interleaved partials: max is exact, so this is the sequential result with a quarter
        // of its dependent chain)
        double cn;
        {
            double c4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < NN; ++j) c4[j & 3] = vmax_abs(c4[j & 3], Prow[j]);
            cn = vmax(vmax(c4[0], c4[1]), vmax(c4[2], c4[3]));
        }
        const double ninv = 1.0 / n;   // (the mean column norm: cdiv, mpc_common.h)
        for (int it = 0; it < c.scaling_iters; ++it) {
            double Er_up = exch(Er, +2);     // E of rate row t+2
            double D_dn = exch(D, -2);       // D of variable t-2
            double a_b = Eb * D, a_r = Er * D, a_rm = has_prev ? Er * D_dn : 0.0, a_rp = Er_up * D;
            const double pn = cs * cn;
            double coln = vmax(pn, vmax_abs(vmax_abs2(a_b, a_r), a_rp));
            // (limit_scaling keeps the arguments in [1e-4, 1e4]: sqrt_n / rcp_n are sqrt and 1 / x bit for bit there)
            double Dt = own ? rcp_n(sqrt_n(limit_scaling(coln))) : 1.0;
            double Etb = rcp_n(sqrt_n(limit_scaling(fabs(a_b))));
            double Etr = rcp_n(sqrt_n(limit_scaling(vmax_abs2(a_r, a_rm))));
            // the broadcast D read in chunks of RCH, each chunk's reads in flight at once (CMP: 8, so that the
            // row of P and the chunk fit the 3-wave register budget; capacity 80: 8 as well; the per-step one-wave
            // kernels: the whole vector)
            double c4[4] = {0.0, 0.0, 0.0, 0.0};
            constexpr int RCH = (CMP || WAVES > 1) ? 8 : NN;
            static_assert(NN % RCH == 0, "chunked broadcast");
            const double* dvb = bcast(Dt);
#pragma unroll
            for (int c0 = 0; c0 < NN; c0 += RCH) {
                double Dv[RCH];
                lds_load_all<RCH>(dvb + c0, Dv);
#pragma unroll
                for (int j = 0; j < RCH; ++j) {
                    const double v = Prow[c0 + j] * (Dt * Dv[j]);
                    Prow[c0 + j] = v;
                    c4[(c0 + j) & 3] = vmax_abs(c4[(c0 + j) & 3], v);
                }
            }
            cn = vmax(vmax(c4[0], c4[1]), vmax(c4[2], c4[3]));
            qi *= Dt;
            D *= Dt;
            Eb *= Etb;
            Er *= Etr;
            // cost scaling of the scaled data cs (P, q)
            double mean = cdiv(block_sum(own ? cs * cn : 0.0), (double)n, ninv);
            double qv[1] = {own ? fabs(cs * qi) : 0.0};
            block_max(qv);
            double ct = fmax(mean, limit_scaling(qv[0]));
            ct = rcp_n(limit_scaling(ct));
            cs *= ct;
        }
#pragma unroll
        for (int j = 0; j < NN; ++j) Prow[j] *= cs;
        qi *= cs;
        const double csinv = uniformize(1.0 / cs);   // uniform (held in SGPRs, not in VGPRs)
        const double D_dn = exch(D, -2);
        // (a_rp(t) = Er(t+2) D(t) is a_rm(t+2) bit for bit: where it is needed it is taken from lane t+2 --
        // exch(a_rm, +2), or the product a_rm w formed on lane t+2 -- instead of living in a register)
        double a_b = Eb * D, a_r = Er * D, a_rm = has_prev ? Er * D_dn : 0.0;   // (CMP: re-formed, see reload)
        // Cold per-lane values go to LDS and are re-read (volatile: never hoisted into registers)
        // where needed -- residual checks, the K build, polish, the ADMM loop's clamps -- keeping the ADMM
        // loop's live set down to the inverse row + ~12 doubles.  Single rows: D, E_box, E_rate, a_r(t+2), q.
        // Pair rows (lane t: [2t], [2t+1], one ds_read_b128): (1 / rho_box, 1 / rho_rate) and the scaled
        // bounds (lb, ub), (lr, ur) of the box and rate rows.
        enum { C_D = 0, C_EB, C_ER, C_ARUP, C_Q };
        enum { P_RHOI = 0, P_BB, P_BR };
        typedef double dpair __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(3))) volatile dpair* LdsVD2;
        const int tc = t < CS ? t : CS - 1;
        auto pair = [&](int i) -> dpair { return ((LdsVD2)(s_cold + 5 * CS))[i * CS + tc]; };
        auto set_pair = [&](int i, double x0, double x1) {
            if (t < CS) ((LdsVD2)(s_cold + 5 * CS))[i * CS + t] = dpair{x0, x1};
        };
        {
            // scaled bounds
            const double slb = (lb > -INFTY) ? lb * Eb : -INFTY, sub = (ub < INFTY) ? ub * Eb : INFTY;
            const double slr = (lr > -INFTY) ? lr * Er : -INFTY, sur = (ur < INFTY) ? ur * Er : INFTY;
            const double a_r_up0 = exch(a_r, +2);
            if (t < CS) {   // (rows of CS: lanes >= CS read the next row's values, never use them)
                double* cw = s_cold + t;
                cw[C_D * CS] = D; cw[C_EB * CS] = Eb; cw[C_ER * CS] = Er;
                cw[C_ARUP * CS] = a_r_up0;
                cw[C_Q * CS] = qi;
            }
            set_pair(P_BB, slb, sub);
            set_pair(P_BR, slr, sur);
        }
        // (an LDS-typed volatile pointer: ds_read with a 32-bit address -- a generic volatile pointer
        // becomes a flat load with a 64-bit address per value)
        typedef __attribute__((address_space(3))) volatile double* LdsVD;
        auto cold = [&](int i) -> double { return ((LdsVD)s_cold)[i * CS + t]; };
        // the unscaled bounds of rows t (as formed above from the configuration; exact-mode certificate)
        // (both channels' values as scalar loads, then a select: a select of the two ADDRESSES is what the compiler
        // forms otherwise -- a per-lane 64-bit address hoisted out of the solve and spilled)
        auto raw_bounds = [&](double& lb_, double& ub_, double& lr_, double& ur_) {
            lb_ = ch ? uniformize(c.u_lo[1]) : uniformize(c.u_lo[0]);
            ub_ = ch ? uniformize(c.u_hi[1]) : uniformize(c.u_hi[0]);
            lr_ = ch ? uniformize(c.du_lo[1]) : uniformize(c.du_lo[0]);
            ur_ = ch ? uniformize(c.du_hi[1]) : uniformize(c.du_hi[0]);
            if (kk == 0) { lr_ += s_up[ch]; ur_ += s_up[ch]; }
        };
        // scaled P to LDS (row stride PS)
        // packed upper triangle: P(i, j), i <= j, at i*NN - i(i-1)/2 + (j - i); rows >= n are zero
        if constexpr (FULLP) {
            // the whole row (symmetric bit for bit: lane t's D_t D_j products equal lane j's), 16-byte stores
            if (t < NN) {
                double2* const w2 = reinterpret_cast<double2*>(__builtin_assume_aligned(s_P + t * PS, 16));
#pragma unroll
                for (int j = 0; j < NN; j += 2)
                    w2[j / 2] = double2{own ? Prow[j] : ((j == t) ? 1.0 : 0.0),
                                        own ? Prow[j + 1] : ((j + 1 == t) ? 1.0 : 0.0)};   // identity on padding rows
            }
        } else if (t < NN) {
            const int rt = t * NN - (t * (t - 1)) / 2 - t;
#pragma unroll
            for (int j = 0; j < NN; ++j)
                if (j >= t) s_P[rt + j] = own ? Prow[j] : ((j == t) ? 1.0 : 0.0);   // identity on padding rows
        }
        __syncthreads();
        stamp(5, __builtin_amdgcn_s_memtime());
        // ---- helpers over the scaled problem ----------------------------------------
        // A x (box, rate) for the vector v owned row-wise
        auto Ax = [&](double v, double& zb, double& zr) {
            double vdn = exch(v, -2);
            zb = a_b * v;
            zr = a_r * v - a_rm * vdn;
        };
        // A' w for w = (wb, wr)
        auto ATw = [&](double wb, double wr) -> double {
            const double rp_up = exch(a_rm * wr, +2);   // a_rp(t) wr(t+2), formed on lane t+2
            return a_b * wb + a_r * wr - rp_up;
        };
        auto Pmul = [&](double v) -> double {  // (P v)_t  (rows >= n are zero)
            double* vb = bcast(v);
            const int tt = opaque_t();
            double sa[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if constexpr (FULLP && WAVES > 1) {
                // contiguous row, ROLLED over blocks of 8 (see below); same products in the same chains
                const double2* pr2 = reinterpret_cast<const double2*>(
                    __builtin_assume_aligned(s_P + (tt < NN ? tt : NN - 1) * PS, 16));
                const double2* vb2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(vb, 16));
#pragma nounroll
                for (int c0 = 0; c0 < NN; c0 += 8) {
                    double2 pv[4], vv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { pv[i] = pr2[c0 / 2 + i]; vv[i] = vb2[c0 / 2 + i]; }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        sa[2 * i] = fma(pv[i].x, vv[i].x, sa[2 * i]);
                        sa[2 * i + 1] = fma(pv[i].y, vv[i].y, sa[2 * i + 1]);
                    }
                }
            } else if constexpr (LEAN || WAVES > 1) {
                // a ROLLED loop over blocks of 8 (the row of K^-1 stays live across this: fully unrolled, the
                // scheduler issues all 80 reads at once and the ADMM loop around it spills); same sums, same order
                static_assert(NN % 8 == 0, "Pmul blocks");
                const int rt = prow_base(tt);
#pragma nounroll
                for (int c0 = 0; c0 < NN; c0 += 8) {
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) sa[jj] = fma(prow_entry(c0 + jj, tt, rt), vb[c0 + jj], sa[jj]);
                }
            } else if constexpr (FULLP) {
                // the row and the broadcast in chunks of 8 (16-byte reads), same products in the same chains
                const double2* pr2 = reinterpret_cast<const double2*>(
                    __builtin_assume_aligned(s_P + (tt < NN ? tt : NN - 1) * PS, 16));
                const double2* vb2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(vb, 16));
#pragma unroll
                for (int c0 = 0; c0 < NN; c0 += 8) {
                    double2 pv[4], vv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { pv[i] = pr2[c0 / 2 + i]; vv[i] = vb2[c0 / 2 + i]; }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        sa[(c0 + 2 * i) & 7] = fma(pv[i].x, vv[i].x, sa[(c0 + 2 * i) & 7]);
                        sa[(c0 + 2 * i + 1) & 7] = fma(pv[i].y, vv[i].y, sa[(c0 + 2 * i + 1) & 7]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NN; ++j) sa[j & 7] = fma(s_P[paddr(j, tt)], vb[j], sa[j & 7]);
            }
            return own ? ((sa[0] + sa[1]) + (sa[2] + sa[3])) + ((sa[4] + sa[5]) + (sa[6] + sa[7])) : 0.0;
        };
        double Krow[NN];
        double Kb[SW2D ? BSW * BSW : 1];   // SW2D: the lane's block of K during the factorization, row-major
        // K64: the lane's column class of up to three rows of K^-1 (slot s: Kc[5 s .. 5 s + 4], ascending columns), and
        // where its partial sums go in s_u (kw0: slots 0 and 1, 4 words apart; kw2: slot 2, or a word nobody reads)
        v2d_t Kc[K64 ? 3 * KCL / 2 : 1];
        int kw0 = 0, kw2 = 0;
        auto Kmul = [&](double v, int slot = -1) -> double {  // (K^{-1} v)_t, KC independent FMA chains
            // (round 2 chose 4: one wave issues an f64 op about every 8 cycles, 8 chains measured far slower in the
            // fused instance, and at capacity 80 0.87 M vs 0.93 M at config 3, round 5; every instance of a capacity
            // uses the same chains, so fused and per-step stay bit-identical)
            constexpr int KC = 4;
            if constexpr (K64) {
                // lane t publishes v_t class-major (column j at (j % 4) KCL + j / 4; the padding 0.0 as in bcast), so a
                // lane's class is KCL contiguous words; the chains start from +0.0 and run all KCL terms, like the row
                // form's, whatever n is
                if (t < NN) s_ex[(t & 3) * KCL + (t >> 2)] = own ? v : 0.0;
                __syncthreads();
                const double2* v2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(s_ex + KCL * (t >> 4), 16));
                double2 vc[KCL / 2];
#pragma unroll
                for (int i = 0; i < KCL / 2; ++i) vc[i] = v2[i];
                double pa[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int i = 0; i < KCL / 2; ++i) {
#pragma unroll
                    for (int s = 0; s < 3; ++s) pa[s] = fma(Kc[s * (KCL / 2) + i].x, vc[i].x, pa[s]);
#pragma unroll
                    for (int s = 0; s < 3; ++s) pa[s] = fma(Kc[s * (KCL / 2) + i].y, vc[i].y, pa[s]);
                }
                s_u[kw0] = pa[0];
                s_u[kw0 + 4] = pa[1];
                s_u[kw2] = pa[2];
                __syncthreads();
                const double2 pl = *reinterpret_cast<const double2*>(__builtin_assume_aligned(s_u + KPA + 2 * t, 16));
                const double2 ph = *reinterpret_cast<const double2*>(__builtin_assume_aligned(s_u + KPB + 2 * t, 16));
                double r = (pl.x + pl.y) + (ph.x + ph.y);
                asm volatile("" : "+v"(r));
                return own ? r : 0.0;
            }
            double sa[KC];
#pragma unroll
            for (int i = 0; i < KC; ++i) sa[i] = 0.0;
            const double* vbuf = (slot >= 0) ? bcast_at(v, slot) : bcast(v);
            if constexpr (WAVES == 1 && !CMP) {
                double vb[NN];
                lds_load_all<NN>(vbuf, vb);
#pragma unroll
                for (int j = 0; j < NN; ++j) sa[j % KC] = fma(Krow[j], vb[j], sa[j % KC]);
            } else {
                // NN = 80: the whole vector in flight (160 VGPRs beside the 160 of Krow) spills inside the
                // ADMM loop; CMP: the 3-wave budget (168) holds the row and a chunk.  CH values at a time
                // (the next chunk's reads issued before this chunk's FMAs), same FMA order
                constexpr int CH = LEAN ? TGMPC_KCH : (CMP ? TGMPC_KCH_W2 : TGMPC_KCH80);
                static_assert(NN % CH == 0 && CH % 2 == 0, "chunked broadcast");
                const double2* v2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(vbuf, 16));
                double2 vb[CH / 2];
#pragma unroll
                for (int i = 0; i < CH / 2; ++i) vb[i] = v2[i];
#pragma unroll
                for (int c0 = 0; c0 < NN; c0 += CH) {
                    double2 vn[CH / 2];
#pragma unroll
                    for (int i = 0; i < CH / 2; ++i) if (c0 + CH < NN) vn[i] = v2[(c0 + CH) / 2 + i];
#pragma unroll
                    for (int i = 0; i < CH / 2; ++i) {
                        sa[(c0 + 2 * i) % KC] = fma(Krow[c0 + 2 * i], vb[i].x, sa[(c0 + 2 * i) % KC]);
                        sa[(c0 + 2 * i + 1) % KC] = fma(Krow[c0 + 2 * i + 1], vb[i].y, sa[(c0 + 2 * i + 1) % KC]);
                    }
#pragma unroll
                    for (int i = 0; i < CH / 2; ++i) vb[i] = vn[i];
                }
                // the reads one chunk ahead of the FMAs that use them (a read group per chunk, then the FMAs of
                // the previous chunk); without this the scheduler issues every read first
                __builtin_amdgcn_sched_group_barrier(0x100, CH / 2, 0);
#pragma unroll
                for (int c0 = 0; c0 < NN; c0 += CH) {
                    if (c0 + CH < NN) __builtin_amdgcn_sched_group_barrier(0x100, CH / 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, CH, 0);
                }
            }
            double r = (sa[0] + sa[1]) + (sa[2] + sa[3]);
            // (opaque: keeps the compiler from turning the select into a branch around the whole mat-vec)
            asm volatile("" : "+v"(r));
            return own ? r : 0.0;
        };
        // residuals (Res of mpc_osqp_rules.h).  Norms that only ever enter as a max of several are combined in the
        // lane first, so 8 maxima cross the wave
        auto residuals = [&](double x, double zb, double zr, double yb, double yr) -> Res {
            double px = Pmul(x);   // (first: its temporaries then coexist with no other)
            double axb, axr;
            Ax(x, axb, axr);
            double aty = ATw(yb, yr);
            double v[8];
            if (own) {
                double dres = px + qi + aty;
                const double Dinv = rcp_n(cold(C_D)), Ebinv = rcp_n(cold(C_EB)), Erinv = rcp_n(cold(C_ER));
                v[0] = vmax_abs2(Ebinv * (axb - zb), Erinv * (axr - zr));   // prim res
                v[1] = vmax(vmax_abs2(Ebinv * axb, Erinv * axr), vmax_abs2(Ebinv * zb, Erinv * zr));
                v[2] = fabs(Dinv * dres) * csinv;
                v[3] = vmax(fabs(Dinv * px) * csinv, vmax(fabs(Dinv * aty) * csinv, fabs(Dinv * qi) * csinv));
                v[4] = vmax_abs2(axb - zb, axr - zr);
                v[5] = fabs(dres);
                v[6] = vmax(vmax_abs2(axb, axr), vmax_abs2(zb, zr));
                v[7] = vmax_abs(vmax_abs2(aty, qi), px);
            } else {
                for (int i = 0; i < 8; ++i) v[i] = 0.0;
            }
            if constexpr (WAVES == 1) {
                // one wave: transposed through LDS (s_F, free during the solve).  Lane 8 i + p takes the max
                // of value i over lanes [p NN/8, (p+1) NN/8), three DPP steps join the 8 parts, and the 8
                // maxima come back as one broadcast read -- ~30 instructions where 8 butterflies take ~180.
                // NaN anywhere in a value makes that maximum NaN (as wave_max_dpp).
                static_assert(NN % 8 == 0 && 8 * NN <= (CMP ? NU : NFS), "s_F too small");
                constexpr int PL = NN / 8;
                bool nan[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) nan[i] = __ballot(v[i] != v[i]) != 0;
                if (t < NN) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) s_F[i * NN + t] = v[i];
                }
                __syncthreads();
                const double* src = s_F + (t >> 3) * NN + (t & 7) * PL;
                double m = src[0];
#pragma unroll
                for (int k = 1; k < PL; ++k) m = vmax(m, src[k]);
                m = vmax(m, dpp_d<0xB1>(m));    // lane ^ 1
                m = vmax(m, dpp_d<0x4E>(m));    // lane ^ 2
                m = vmax(m, dpp_d<0x141>(m));   // half-row mirror: quads of one 8-lane group
                __syncthreads();
                if ((t & 7) == 0) s_F[t >> 3] = m;
                __syncthreads();
                double mv[8];
                lds_load_all<8>(s_F, mv);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = nan[i] ? __builtin_nan("") : mv[i];
                __syncthreads();
            } else if constexpr (!LEAN) {
                // two waves: the same transposed reduction over the exchange buffers (free here: every product of
                // this check is in registers once the first barrier is passed) -- 8 values x NN rows, lane 8 i + p
                // of wave 0 takes rows [p NN/8, (p+1) NN/8) of value i, three DPP steps, 8 maxima back; block_max's
                // 6 x 8 cross-lane shuffles per wave are gone.  A NaN-propagating max (the values are >= +0, so the
                // order of the maxima does not matter, bit for bit)
                static_assert(NN % 8 == 0 && 8 * NN + 8 <= NEX, "s_ex too small");
                constexpr int PL = NN / 8;
                auto nmax = [](double a_, double b_) { return (a_ > b_ || a_ != a_) ? a_ : b_; };
                double* const tb = s_ex;
                __syncthreads();
                if (t < NN) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) tb[i * NN + t] = v[i];
                }
                __syncthreads();
                if (t < 64) {
                    const double* src = tb + (t >> 3) * NN + (t & 7) * PL;
                    double m = src[0];
#pragma unroll
                    for (int k = 1; k < PL; ++k) m = nmax(m, src[k]);
                    m = nmax(m, dpp_d<0xB1>(m));    // lane ^ 1
                    m = nmax(m, dpp_d<0x4E>(m));    // lane ^ 2
                    m = nmax(m, dpp_d<0x141>(m));   // half-row mirror: quads of one 8-lane group
                    if ((t & 7) == 0) tb[8 * NN + (t >> 3)] = m;
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = tb[8 * NN + i];
                __syncthreads();
            } else {
                block_max(v);
            }
            // (the results are uniform: held in SGPRs, uniformize, not in VGPRs across the solve)
            Res r;
            r.pr = uniformize(v[0]);
            r.eps_p = uniformize(c.eps_abs + c.eps_rel * v[1]);
            r.dr = uniformize(v[2]);
            r.eps_d = uniformize(c.eps_abs + c.eps_rel * v[3]);
            r.prs = uniformize(v[4]); r.drs = uniformize(v[5]); r.pn = uniformize(v[6]); r.dn = uniformize(v[7]);
            return r;
        };

        // ---- 4b/4c. ADMM (OSQP osqp_solve) + polish (polish.c) --------------------------
        // A state machine around ONE factorization site (so the register-resident inverse is
        // never handed to an out-of-line call): each pass of the outer loop builds
        //   K = P + ks I + A' diag(kb, kr) A
        // (ADMM: kb/kr = rho, ks = sigma; polish: kb/kr = active/delta, ks = delta) and inverts it
        // in place with the symmetric sweep operator, then runs the phase until it needs a new K.
        constexpr int PH_ADMM = 0, PH_POLISH = 1, PH_DONE = 2;
        int phase = PH_ADMM;
        double rho = c.rho;
        double x = 0.0, zb = 0.0, zr = 0.0, yb = 0.0, yr = 0.0;
        // Warm start (closed loop, t > 0): start from the rho the previous step's solve adapted to
        // (iterates start at zero as cold; shifting the previous primal/dual point was measured to
        // lengthen the iteration tail).  mpc_6stati.py:256 asks OSQP for warm_start=True, a no-op
        // there because a new Problem is built every call; the polished optimum does not depend on rho.
        if (CLOSED && c.warm_start && tstep > 0) {
            if (a.wsWarm) {
                const double* wv = a.wsWarm + 4 * (size_t)b;
                const double w0 = FUSED ? ld_coh(wv) : wv[0], w1 = FUSED ? ld_coh(wv + 1) : wv[1];
                if (w1 != 0.0) rho = fmin(fmax(w0, RHO_MIN), RHO_MAX);
            }
        }
        double rb, rr;   // rho of the box and rate rows (their inverses: pair row P_RHOI)
        auto rho_rows = [&]() {
            const dpair bb = pair(P_BB), br = pair(P_BR);
            rb = rho_for(bb.x, bb.y, rho);
            rr = rho_for(br.x, br.y, rho);
            set_pair(P_RHOI, 1.0 / rb, 1.0 / rr);
        };
        rho_rows();
        // LEAN: the per-lane constants of the ADMM loop re-formed from LDS at the K build and after the sweep (the
        // same products of the same values, bit for bit), so that none of them is live across the factorization
        auto reload = [&]() {
            if constexpr (LEAN) {
                const double Dl = cold(C_D), Ebl = cold(C_EB), Erl = cold(C_ER);
                a_b = Ebl * Dl;
                a_r = Erl * Dl;
                const double Ddn = exch(Dl, -2);
                a_rm = (t >= 2) ? Erl * Ddn : 0.0;
                qi = cold(C_Q);
                const dpair bb = pair(P_BB), br = pair(P_BR);
                rb = rho_for(bb.x, bb.y, rho);
                rr = rho_for(br.x, br.y, rho);
            }
        };
        Res r = {0, 0, 0, 0, 0, 0, 0, 0};
        int rounds = 0, ps = 0, actb = 0, actr = 0;
        double escale = 1.0;
        const double alpha = c.alpha, sig = c.sigma, dl = c.delta;
        const double dlinv = 1.0 / dl;   // (quotients by delta: cdiv, mpc_common.h)
        iter = 1;
        int nfact = 0;
        // diagnostics (traj_debug_set_stamps): cycles in residual checks / sweeps / polish
        const bool prof = dbg != nullptr;
        long long cyc_res = 0, cyc_sweep = 0, cyc_pol = 0, n_res = 0, t_mark = 0;
        bool pol_open = false;
        auto tic = [&]() { if (prof) t_mark = __builtin_amdgcn_s_memtime(); };
        auto toc = [&](long long& acc) { if (prof) acc += __builtin_amdgcn_s_memtime() - t_mark; };
        // LEAN: the iterate is parked in LDS (past the sweep's pivot columns) from before the K build to after the
        // sweep -- the factorization is the kernel's register peak, and values live across it are spilled.  The
        // 3-wave instance parks z and y_b (NSTR = 3) and keeps x, y_r in registers: its scratch stays at 256 B
        // and the LDS image at 12,776 B (12 workgroups per CU; all five rows: 13,128 B, 11)
        typedef __attribute__((address_space(3))) volatile double* LdsVDs;
        auto stash = [&]() {
            if constexpr (LEAN) {
                LdsVDs sp = (LdsVDs)(s_u + ((NSW + 1) & ~1));
                if (t < NN) {
                    sp[t] = zb; sp[NN + t] = zr; sp[2 * NN + t] = yb;
                    if (NSTR > 3) sp[3 * NN + t] = yr;
                    if (NSTR > 4) sp[4 * NN + t] = x;
                }
            }
        };
        auto unstash = [&]() {
            if constexpr (LEAN) {
                LdsVDs sp = (LdsVDs)(s_u + ((NSW + 1) & ~1));
                zb = sp[tc]; zr = sp[NN + tc]; yb = sp[2 * NN + tc];
                if (NSTR > 3) yr = sp[3 * NN + tc];
                if (NSTR > 4) x = sp[4 * NN + tc];
            }
        };
        while (phase != PH_DONE) {
            if (pol_open) { toc(cyc_pol); pol_open = false; }
            ++nfact;
            stash();
            reload();
            // ---- build K (row t) ----
            const double kb = (phase == PH_ADMM) ? rb : (actb ? dlinv : 0.0);
            const double kr = (phase == PH_ADMM) ? rr : (actr ? dlinv : 0.0);
            const double ks = (phase == PH_ADMM) ? sig : dl;
            {
                const double kr_up = exch(kr, +2);
                const double a_rp = exch(a_rm, +2);   // = Er(t+2) D(t), bit for bit
                const double dii = ks + kb * a_b * a_b + kr * a_r * a_r + kr_up * a_rp * a_rp;
                // (t, t+2); by symmetry also the (t+2, t) entry: lane t+2's -kr a_r a_rm is the same product
                // of the same values (kr_up = kr(t+2), cold(C_ARUP) = a_r(t+2), a_rp = Er(t+2) D(t) = a_rm(t+2))
                const double dp = -kr_up * cold(C_ARUP) * a_rp;
                // The band goes into the packed P in LDS (each own lane adds its diagonal and its (t, t+2)
                // entry), every lane reads its row as it stands -- no per-entry selects -- and the two entries
                // are restored.  Padding rows n..NN-1 hold the identity in s_P; lanes >= NN hold exact zero rows
                // (the receivers of the one-wave sweep below).
                const int tt = opaque_t();
                const int pdg = FULLP ? tt * PS + tt : paddr(tt, tt), psp = FULLP ? tt * PS + tt + 2 : paddr(tt + 2, tt);
                const int psm = (tt + 2) * PS + tt;   // FULLP: the mirror of (t, t + 2)
                const bool has_sp = own && (t + 2 < n);
                double o_dg = 0.0, o_sp = 0.0;
                if (own) {
                    o_dg = s_P[pdg];
                    s_P[pdg] = o_dg + dii;
                    if (has_sp) {
                        o_sp = s_P[psp];
                        s_P[psp] = o_sp + dp;
                        if constexpr (FULLP) s_P[psm] = o_sp + dp;
                    }
                }
                __syncthreads();
                if constexpr (SW2D) {
                    // lane 8 g + s holds K[BSW g + k][BSW s + l] (padding rows and columns: the identity, from s_P)
                    const double* const blk = s_P + (BSW * (tt >> 3)) * PS + BSW * (tt & 7);
#pragma unroll
                    for (int k = 0; k < BSW; ++k) {
#pragma unroll
                        for (int l = 0; l < BSW; ++l) Kb[k * BSW + l] = blk[k * PS + l];
                    }
                } else if constexpr (RECV2) {
                    // two-wave receiver sweep: lane t holds row t - SP2 (lanes < SP2: exact zero rows)
                    const int r = tt - SP2;
                    const int rr = r >= 0 ? r : 0;
#pragma unroll
                    for (int j = 0; j < NN; ++j) Krow[j] = (r >= 0) ? s_P[FULLP ? rr * PS + j : paddr(j, rr)] : 0.0;
                } else if constexpr (FULLP) {
                    // (lanes >= NN: exact zero rows, the one-wave sweep's receivers)
                    lds_load_all<NN>(s_P + (tt < NN ? tt : NN - 1) * PS, Krow);
                    if (t >= NN) {
#pragma unroll
                        for (int j = 0; j < NN; ++j) Krow[j] = 0.0;
                    }
                } else if (t < NN) {
#pragma unroll
                    for (int j = 0; j < NN; ++j) Krow[j] = s_P[paddr(j, tt)];
                } else {
#pragma unroll
                    for (int j = 0; j < NN; ++j) Krow[j] = 0.0;
                }
                __syncthreads();
                if (own) {
                    s_P[pdg] = o_dg;
                    if (has_sp) {
                        s_P[psp] = o_sp;
                        if constexpr (FULLP) s_P[psm] = o_sp;
                    }
                }
            }
            // ---- sweep: Krow <- row t of K^{-1} (symmetric sweep operator, NN pivots) ----
            // Rolled pivot loop with the row ROTATED so that the current pivot column is always
            // register 0: before pivot pv, Krow[j] = K[t][(pv + j) mod NN] (after NN pivots the
            // rotation is back to the identity).  Column pv is published twice (cb[t], cb[t + NN])
            // so the pivot row in rotated order is the contiguous slice cb[pv .. pv + NN)
            // (K symmetric: K[pv][c] = K[c][pv]).  Padding pivots (>= n) are identity and exact.
            bool ok = true;
            tic();
            if constexpr (SW2D) {
                // One-wave sweep with K held as 8 x 8 blocks: lane 8 g + s holds the BSW x BSW block of rows
                // BSW g .. and columns BSW s .., so all 64 lanes carry data (the row form below: NN of 64) and a
                // lane reads 2 BSW + 1 values per pivot instead of a whole pivot row.  The arithmetic is the row
                // form's, entry by entry: with c = column p as published by the lanes that hold it (c_r = K_rp, used
                // as the pivot column AND, by symmetry, as the pivot row -- K is not bitwise symmetric during the
                // sweep, and the row form never reads the true row), dinv = rcp_nr(c_p):
                //     K_ij <- fma3(-(c_i dinv), c_j, K_ij)   (i, j != p; the sign flip is exact wherever it is applied)
                //     K_pj <- fma3(dinv, c_j, +0.0)          (the row form's receiver lane: an exact zero row)
                //     K_ip <- c_i dinv,   K_pp <- -dinv.
                // The lanes holding column p + 1 form it first and publish it (two alternating slots; one wave's LDS
                // operations complete in program order).  The pivot loop is unrolled over whole blocks of BSW pivots,
                // so the local row / column p % BSW is a static register: no rotation.  Afterwards the blocks go back
                // to rows through LDS (below).
                const int tq = opaque_t();
                const int g = tq >> 3, s = tq & 7;
                if (s == 0) {
#pragma unroll
                    for (int k = 0; k < BSW; ++k) s_sw[BSW * g + k] = Kb[k * BSW];
                }
                __syncthreads();
                // Two blocks of pivots per loop body (2 BSW pivots: the slot of a pivot is static), and the next
                // pivot's reads issued right after its column is published, ahead of this pivot's other FMAs (the
                // reads after the last pivot fetch words nobody uses).
                const double* const cgp = s_sw + BSW * g;
                const double* const csp = s_sw + BSW * s;
                double cg[BSW], cs[BSW];
#pragma unroll
                for (int k = 0; k < BSW; ++k) cg[k] = cgp[k];
#pragma unroll
                for (int k = 0; k < BSW; ++k) cs[k] = csp[k];
                double d = s_sw[0];
#pragma unroll 1
                for (int pb2 = 0; pb2 < 8; pb2 += 2) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int pb = pb2 + h;
                        const bool prow = (g == pb), pcol = (s == pb);
#pragma unroll
                        for (int q = 0; q < BSW; ++q) {
                            const int pv = pb * BSW + q;
                            const int nsl = (((h * BSW + q) & 1) ^ 1) * NN;   // the next pivot's slot (2 BSW pb2 is even)
                            ok = ok && (d > 0.0);
                            const double dinv = rcp_nr(d);
                            // f = c_i dinv: the update's factor is -f (the fma's source modifier: fma3n), the new pivot
                            // column is f itself
                            double f[BSW];
#pragma unroll
                            for (int k = 0; k < BSW; ++k) f[k] = cg[k] * dinv;
                            if (prow) {
                                // the pivot row: K_pj <- dinv c_j + 0 (factor -(-dinv)), K_pp <- -dinv
                                f[q] = -dinv;
#pragma unroll
                                for (int l = 0; l < BSW; ++l) Kb[q * BSW + l] = 0.0;
                            }
                            // the next pivot's column first, published at once
                            const int q1 = (q + 1) % BSW;
#pragma unroll
                            for (int k = 0; k < BSW; ++k) Kb[k * BSW + q1] = fma3n(f[k], cs[q1], Kb[k * BSW + q1]);
                            if (pv + 1 < NN && (q + 1 < BSW ? pcol : (s == pb + 1))) {
                                double* const nb = s_sw + nsl + BSW * g;
#pragma unroll
                                for (int k = 0; k < BSW; ++k) nb[k] = Kb[k * BSW + q1];
                            }
                            __syncthreads();
                            double ng[BSW], ns[BSW];
#pragma unroll
                            for (int k = 0; k < BSW; ++k) ng[k] = cgp[nsl + k];
#pragma unroll
                            for (int k = 0; k < BSW; ++k) ns[k] = csp[nsl + k];
                            const double nd = s_sw[nsl + pv + 1];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int k = 0; k < BSW; ++k) {
#pragma unroll
                                for (int l = 0; l < BSW; ++l)
                                    if (l != q1) Kb[k * BSW + l] = fma3n(f[k], cs[l], Kb[k * BSW + l]);
                            }
                            if (pcol) {
#pragma unroll
                                for (int k = 0; k < BSW; ++k) Kb[k * BSW + q] = f[k];
                            }
#pragma unroll
                            for (int k = 0; k < BSW; ++k) {
                                cg[k] = ng[k];
                                cs[k] = ns[k];
                            }
                            d = nd;
                        }
                    }
                }
                // K^-1 = -(swept K); then back to rows for the ADMM (Kmul and the rest keep the row-per-lane form):
                // in round k every lane writes local row k of its block to a row-major staging area (8 rows, stride
                // ST2) in the scratch region -- the pivot columns are dead after the last pivot, the F slots and the
                // window since the condensing -- and the lanes r with r % BSW == k read row r whole, under an exec
                // mask (lds_load10_masked; lanes >= NN read row 0's slot: defined values they never use).
#pragma unroll
                for (int i = 0; i < BSW * BSW; ++i) Kb[i] = -Kb[i];
                static_assert(NN == 40, "the masked row read is written for 2 x 10 ds_read_b128");
                typedef __attribute__((address_space(3))) double* LdsD;
                if constexpr (K64) {
                    // K64: the staged rows are class-major (column j at (j % 4) KCL + j / 4), and lane 16 c + m takes
                    // the KCL entries of class c of staged row m % 8 -- in rounds 0 and 1 into slot 0 (lanes m < 8,
                    // then m >= 8), rounds 2 and 3 into slot 1, round 4 into slot 2 (m < 8): a static slot and a
                    // constant exec mask per round.  Slot 2 of the lanes m >= 8 keeps its exact zeros.
                    static_assert(BSW == 5 && KCL == 10, "five staging rounds, five ds_read_b128 per class");
                    const int lc = tq >> 4, lm = tq & 15;
                    const unsigned ra = (unsigned)(__UINTPTR_TYPE__)(LdsD)(s_u + (lm & 7) * ST2 + KCL * lc);
                    int wo[BSW];
#pragma unroll
                    for (int l = 0; l < BSW; ++l) {
                        const int col = BSW * s + l;
                        wo[l] = g * ST2 + (col & 3) * KCL + (col >> 2);
                    }
#pragma unroll
                    for (int i = 0; i < 3 * KCL / 2; ++i) Kc[i] = v2d_t{0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < BSW; ++k) {
                        __syncthreads();
#pragma unroll
                        for (int l = 0; l < BSW; ++l) s_u[wo[l]] = Kb[k * BSW + l];
                        __syncthreads();
                        const unsigned long long rm = (k & 1) ? 0xFF00FF00FF00FF00ull : 0x00FF00FF00FF00FFull;
                        lds_load5_masked<0>(ra, rm, Kc + (k >> 1) * (KCL / 2));
                    }
                    // the partial sums' words: row 5 (m % 8) + m / 8 (slot 0), + 2 (slot 1), + 4 (slot 2, m < 8)
                    const int r0 = BSW * (lm & 7) + (lm >> 3);
                    kw0 = ((lc & 2) ? KPB : KPA) + 2 * r0 + (lc & 1);
                    kw2 = (lm < 8) ? kw0 + 8 : KPD + 8 * lc + (lm & 7);
                    asm volatile("" : "+v"(kw0), "+v"(kw2));
                } else {
                    const int rk = tq % BSW, rg = (tq < NN) ? tq / BSW : 0;
                    const unsigned ra = (unsigned)(__UINTPTR_TYPE__)(LdsD)(s_u + rg * ST2);
                    v2d_t kr[NN / 2];
#pragma unroll
                    for (int i = 0; i < NN / 2; ++i) kr[i] = v2d_t{0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < BSW; ++k) {
                        __syncthreads();
                        double* const wr = s_u + g * ST2 + BSW * s;
#pragma unroll
                        for (int l = 0; l < BSW; ++l) wr[l] = Kb[k * BSW + l];
                        __syncthreads();
                        const unsigned long long rm = __ballot(rk == k);
                        lds_load10_masked<0>(ra, rm, kr);
                        lds_load10_masked<160>(ra, rm, kr + 10);
                    }
#pragma unroll
                    for (int i = 0; i < NN / 2; ++i) {
                        Krow[2 * i] = kr[i].x;
                        Krow[2 * i + 1] = kr[i].y;
                    }
                }
            } else if constexpr (WAVES == 1) {
                // One-wave sweep, ONE fma per entry and pivot.  The new pivot row (K_pj / d) is not
                // formed in place (that needs a second operation on the pivot lane only) but in a
                // RECEIVER lane holding an exact zero row: every lane computes
                //     Krow[j] <- fma(be, pivot_row[j], Krow[j]),
                // be = -K_tp / d on row lanes, 1 / d on the receiver (0 + pr/d, exact), and the old
                // pivot lane's row is dropped.  Receivers are the spare lanes NN..63 (pivots < 64-NN),
                // then the former pivot lanes 0.. (re-zeroed once), so row r ends in lane (r + NN) mod
                // 64 and one ds_bpermute rotation puts it back in lane r.  The values are those of forming
                // the pivot row in place, bit for bit (fma(be, pr, 1 * K) and fma(1/d, pr, 0 * K)).
                // Rotated registers as above (pivot column in register 0); the update is written as
                // three-address v_fma_f64 (fma3), so the rotation costs no register copies.
                // Row lanes publish their column entry under the ROW they hold (rho), twice.
                constexpr int SB = 2 * NN + 2;
                constexpr int SPARE = 64 - NN;
                static_assert(NN <= 2 * SPARE, "receivers: the spare lanes, then the first dropped rows' lanes");
                int rho = t < NN ? t : -1;    // row held by this lane (-1: zero or dropped)
                if (t < NN) {
                    s_sw[t] = Krow[0];
                    s_sw[t + NN] = Krow[0];
                }
                // unrolled by TGMPC_SWEEP_UNROLL: the register rotation is static inside the unrolled body, so
                // realigning the row costs NN register moves per TGMPC_SWEEP_UNROLL pivots instead of per pivot
                constexpr int SWU = FUSED ? TGMPC_SWEEP_UNROLL : TGMPC_SWEEP_UNROLL_STEP;
#pragma unroll SWU
                for (int pv = 0; pv < NN; ++pv) {
                    if (NN > SPARE && pv == SPARE) {
                        // lanes 0..SPARE-1 all pivoted (dropped rows): zero them, they receive next
                        if (t < SPARE) {
#pragma unroll
                            for (int j = 0; j < NN; ++j) Krow[j] = 0.0;
                        }
                    }
                    __syncthreads();
                    const int o = pv & 1;
                    const double* prow = s_sw + o * SB + o + pv;
                    const double2* prow2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(prow, 16));
                    // CMP: the pivot row in chunks of PC double2, the next chunk's reads issued before this
                    // chunk's FMAs (the whole row beside Krow does not fit the 3-wave budget)
                    constexpr int PC = LEAN ? TGMPC_PCH : (CMP ? TGMPC_PCH_W2 : NN / 2 - 1);
                    static_assert(PC > 0, "pivot-row chunk");
                    const double2 p0 = prow2[0];
                    double2 pr[PC];
#pragma unroll
                    for (int i = 0; i < PC; ++i) if (1 + i < NN / 2) pr[i] = prow2[1 + i];
                    const double d = p0.x;
                    ok = ok && (d > 0.0);
                    const double dinv = rcp_nr(d);
                    const int rl = pv < SPARE ? NN + pv : pv - SPARE;   // receiver lane (uniform)
                    const bool recv = (t == rl);
                    const double fd = Krow[0] * dinv;
                    const double be = recv ? dinv : -fd;
                    const double k0 = recv ? -dinv : fd;
                    rho = recv ? pv : ((t == pv) ? -1 : rho);
                    const double n0 = fma3(be, p0.y, Krow[1]);
                    if (rho >= 0) {
                        double* nb = s_sw + (o ^ 1) * SB + (o ^ 1);
                        nb[rho] = n0;
                        nb[rho + NN] = n0;
                    }
                    // Krow[j - 1] <- be * (pivot row)[j] + Krow[j], j = 2 .. NN-1: double2 i = 1 .. NN/2 - 1
#pragma unroll
                    for (int c = 1; c < NN / 2; c += PC) {
                        double2 pn[PC];
#pragma unroll
                        for (int i = 0; i < PC; ++i) if (c + PC + i < NN / 2) pn[i] = prow2[c + PC + i];
#pragma unroll
                        for (int i = 0; i < PC; ++i) {
                            if (c + i < NN / 2) {
                                const int j = 2 * (c + i);
                                Krow[j - 1] = fma3(be, pr[i].x, Krow[j]);
                                Krow[j] = fma3(be, pr[i].y, Krow[j + 1]);
                            }
                        }
#pragma unroll
                        for (int i = 0; i < PC; ++i) pr[i] = pn[i];
                    }
                    Krow[0] = n0;
                    Krow[NN - 1] = k0;
                }
                // row r sits in lane (r + NN) mod 64: rotate it back to lane r
                const int src = ((t + NN) & 63) << 2;
#pragma unroll
                for (int j = 0; j < NN; ++j) {
                    const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(Krow[j]));
                    const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(Krow[j]));
                    Krow[j] = __hiloint2double(hi, lo);
                    __builtin_amdgcn_sched_barrier(0);   // one register at a time (no batch of 80 temporaries)
                }
            } else {
                // Two-wave sweep (capacity 80; the lean two-wave instance too), ONE fma per entry and pivot: the receiver
                // form of the one-wave sweep above.  Rows start SHIFTED: lane t holds row t - SP2 (SP2 = 128 - NN
                // spare lanes first, holding exact zero rows).  Pivot pv's new row K_pj / d is formed in
                // receiver lane pv -- a spare lane while pv < SP2; the lanes SP2..NN-1 held rows 0..NN-SP2-1,
                // all dropped by pivot NN - SP2 and zeroed then -- so row r ends in lane r: no final
                // permutation across the waves.  Same values as forming the pivot row in place (see above).
                constexpr int SB = 2 * NN + 2;
                static_assert(RECV2 && NN <= 2 * SP2, "receivers: the spare lanes, then the first dropped rows' lanes");
                int rho = (t >= SP2) ? t - SP2 : -1;   // row held by this lane (-1: zero or dropped)
                if (rho >= 0) {
                    s_sw[rho] = Krow[0];
                    s_sw[rho + NN] = Krow[0];
                }
                TGMPC_PRAGMA(unroll TGMPC_SWEEP_UNROLL2)
                for (int pv = 0; pv < NN; ++pv) {
                    if (NN > SP2 && pv == NN - SP2) {
                        if (t >= SP2 && t < NN) {
#pragma unroll
                            for (int j = 0; j < NN; ++j) Krow[j] = 0.0;
                        }
                    }
                    __syncthreads();
                    const int o = pv & 1;
                    const double* prow = s_sw + o * SB + o + pv;
                    const double2* prow2 = reinterpret_cast<const double2*>(__builtin_assume_aligned(prow, 16));
                    // the pivot row in chunks of PC double2, the next chunk's reads issued before this chunk's FMAs
                    // (the row of K^-1 and the whole pivot row do not fit 256 registers)
                    constexpr int PC = L2W ? TGMPC_PCH2 : TGMPC_PCH80;
                    static_assert(PC > 0, "pivot-row chunk");
                    const double2 p0 = prow2[0];
                    double2 pr[PC];
#pragma unroll
                    for (int i = 0; i < PC; ++i) if (1 + i < NN / 2) pr[i] = prow2[1 + i];
                    const double d = p0.x;
                    ok = ok && (d > 0.0);
                    const double dinv = rcp_nr(d);
                    const bool recv = (t == pv);
                    const double fd = Krow[0] * dinv;
                    const double be = recv ? dinv : -fd;
                    const double k0 = recv ? -dinv : fd;
                    rho = recv ? pv : ((t == SP2 + pv) ? -1 : rho);
                    const double n0 = fma3(be, p0.y, Krow[1]);
                    if (rho >= 0) {
                        double* nb = s_sw + (o ^ 1) * SB + (o ^ 1);
                        nb[rho] = n0;
                        nb[rho + NN] = n0;
                    }
#pragma unroll
                    for (int c = 1; c < NN / 2; c += PC) {
                        double2 pn[PC];
#pragma unroll
                        for (int i = 0; i < PC; ++i) if (c + PC + i < NN / 2) pn[i] = prow2[c + PC + i];
#pragma unroll
                        for (int i = 0; i < PC; ++i) {
                            if (c + i < NN / 2) {
                                const int j = 2 * (c + i);
                                Krow[j - 1] = fma3(be, pr[i].x, Krow[j]);
                                Krow[j] = fma3(be, pr[i].y, Krow[j + 1]);
                            }
                        }
#pragma unroll
                        for (int i = 0; i < PC; ++i) pr[i] = pn[i];
                    }
                    Krow[0] = n0;
                    Krow[NN - 1] = k0;
                }
            }
            // (L2W: the pivot columns share the exchange region -- no wave writes an exchange slot before the
            // other has read the last pivot row)
            if constexpr (L2W) __syncthreads();
            if constexpr (!SW2D) {
#pragma unroll
                for (int j = 0; j < NN; ++j) Krow[j] = -Krow[j];
            }
            toc(cyc_sweep);
            unstash();
            reload();
            if (!ok) {
                if (phase == PH_ADMM) { status = TRAJ_STATUS_SOLVER_ERROR; break; }
                // failed reduced-KKT factorization = unsuccessful polish (polish.c): the ADMM
                // solution and status stand; exact mode continues ADMM like an uncertified pass
                if (c.polish_mode == 1 && polish_continues(c, rounds, iter)) {
                    ++rounds;
                    escale *= 1e-2;
                    ++iter;
                    phase = PH_ADMM;
                } else {
                    phase = PH_DONE;
                }
                continue;
            }

            if (phase == PH_ADMM) {
                bool converged = false, refactor = false;
                int chk = c.check_interval - (iter - 1) % c.check_interval;
                const double oma = uniformize(1.0 - alpha);
                for (; iter <= c.max_iter; ++iter) {
                    // OSQP's update_xz_tilde / update_x / update_z / update_y, each product-sum as an fma
                    // (the iteration is f64-issue bound: 69 f64 ops instead of 86; the oracle keeps OSQP's
                    // separate multiplies -- ulp-level differences, like its Cholesky vs this inverse)
                    // rhs = sig x - q + A'(rho z - y)
                    const double wb = fma(rb, zb, -yb), wr = fma(rr, zr, -yr);
                    // a_rp(t) wr(t+2) formed on lane t+2 (a_rm(t+2) = a_rp(t) bit for bit)
                    const double rp_up = (WAVES > 1) ? exch_at(a_rm * wr, +2, 4) : exch(a_rm * wr, +2);
                    const double atw = fma(a_b, wb, fma(a_r, wr, -rp_up));
                    double xt = Kmul(fma(sig, x, atw - qi), WAVES > 1 ? 5 : -1);
                    const double xt_dn = (WAVES > 1) ? exch_at(xt, -2, 6) : exch(xt, -2);
                    const double ztb = a_b * xt, ztr = fma(a_r, xt, -(a_rm * xt_dn));
                    double xn = fma(alpha, xt, oma * x);
                    double zrb = fma(alpha, ztb, oma * zb);
                    double zrr = fma(alpha, ztr, oma * zr);
                    const dpair ri = pair(P_RHOI), bb = pair(P_BB), br = pair(P_BR);   // (LDS, see the cold values)
                    double nzb = clamp_mm(fma(ri.x, yb, zrb), bb.x, bb.y), nzr = clamp_mm(fma(ri.y, yr, zrr), br.x, br.y);
                    yb = fma(rb, zrb - nzb, yb);
                    yr = fma(rr, zrr - nzr, yr);
                    x = xn;
                    zb = nzb;
                    zr = nzr;
                    if (--chk == 0) {
                        chk = c.check_interval;
#if TGMPC_PRIO_ITERS > 0
                        // a long solve is the critical path of its instance's step chain (the fused run
                        // ends with the slowest chain): its wave issues ahead of the SIMD's other wave
                        if (FUSED && iter >= TGMPC_PRIO_ITERS) __builtin_amdgcn_s_setprio(3);
#endif
                        tic();
                        r = residuals(x, zb, zr, yb, yr);
                        toc(cyc_res);
                        ++n_res;
                        if (r.pr <= escale * r.eps_p && r.dr <= escale * r.eps_d) { converged = true; break; }
                        if (c.adaptive_rho) {
                            const double est = rho_estimate(rho, r);
                            if (needs_refactor(est, rho, c.adaptive_rho_tol)) {
                                rho = uniformize(est);
                                rho_rows();
                                refactor = true;
                                ++iter;
                                break;
                            }
                        }
                    }
                }
                if (refactor && iter <= c.max_iter) continue;
                if (converged) status = TRAJ_STATUS_OPTIMAL;
                else {
                    iter = c.max_iter;
                    r = residuals(x, zb, zr, yb, yr);
                    status = status_at_cap(rounds, r);
                }
                if (status == TRAJ_STATUS_OPTIMAL && c.polish) {
                    const dpair bb = pair(P_BB), br = pair(P_BR);
                    actb = own ? active_sign(zb, bb.x, bb.y, yb) : 0;
                    actr = own ? active_sign(zr, br.x, br.y, yr) : 0;
                    ps = 1;
                    phase = PH_POLISH;
                } else {
                    phase = PH_DONE;
                }
                continue;
            }

            // ---- PH_POLISH: Krow = row of M^{-1}, M = P + dI + Ar'Ar/d (eliminated reduced KKT) ----
            tic();
            pol_open = true;
            {
                double slb, sub, slr, sur;   // scaled bounds (re-read from LDS where used)
                auto bounds = [&]() {
                    const dpair bb2 = pair(P_BB), br2 = pair(P_BR);
                    slb = bb2.x; sub = bb2.y; slr = br2.x; sur = br2.y;
                };
                bounds();
                const double bb = actb < 0 ? slb : (actb > 0 ? sub : 0.0);
                const double br = actr < 0 ? slr : (actr > 0 ? sur : 0.0);
                double px_ = 0.0, pyb = 0.0, pyr = 0.0;
                // (-q through an opaque copy formed here: hoisted out of the phase loop, the negated q was live
                // across the whole solve and spilled)
                double nqi = qi;
                asm volatile("" : "+v"(nqi));
                nqi = -nqi;
                double r1 = nqi, r2b = actb ? bb : 0.0, r2r = actr ? br : 0.0;
                double axb = 0.0, axr = 0.0;
                for (int rf = 0; rf <= c.polish_refine_iter; ++rf) {
                    double tv = Kmul(r1 + ATw(actb ? cdiv(r2b, dl, dlinv) : 0.0, actr ? cdiv(r2r, dl, dlinv) : 0.0));
                    double tb, tr;
                    Ax(tv, tb, tr);
                    px_ += tv;
                    if (actb) pyb += cdiv(tb - r2b, dl, dlinv);
                    if (actr) pyr += cdiv(tr - r2r, dl, dlinv);
                    if (rf == c.polish_refine_iter) break;
                    double Pxv = Pmul(px_);
                    double atyv = ATw(pyb, pyr);
                    r1 = nqi - Pxv - atyv;
                    Ax(px_, axb, axr);
                    r2b = actb ? bb - axb : 0.0;
                    r2r = actr ? br - axr : 0.0;
                }
                Ax(px_, axb, axr);
                if (c.polish_mode == 0) {
                    // z = proj(Ax + y), y = Ax + y - z (OSQP project_normalcone); accept if residuals drop
                    double ztb = axb + pyb, ztr = axr + pyr;
                    bounds();
                    double nzb = clampd(ztb, slb, sub), nzr = clampd(ztr, slr, sur);
                    double nyb = ztb - nzb, nyr = ztr - nzr;
                    Res rp = residuals(px_, nzb, nzr, nyb, nyr);
                    bool okp = (rp.pr < r.pr && rp.dr < r.dr) || (rp.pr < r.pr && r.dr < 1e-10) ||
                               (rp.dr < r.dr && r.pr < 1e-10);
                    if (okp) {
                        x = px_; zb = nzb; zr = nzr; yb = nyb; yr = nyr;
                        pol = 1;
                    }
                    phase = PH_DONE;
                    continue;
                }
                // exact mode: KKT certificate in the unscaled problem
                double Pxv = Pmul(px_);
                double atyv = ATw(pyb, pyr);
                const double tol = c.cert_tol;
                double v[2];
                const double Dinv = 1.0 / cold(C_D), Ebinv = 1.0 / cold(C_EB), Erinv = 1.0 / cold(C_ER);
                double lb, ub, lr, ur;
                raw_bounds(lb, ub, lr, ur);
                bounds();
                v[0] = own ? fabs(Dinv * (Pxv + qi + atyv)) * csinv : 0.0;            // stationarity
                v[1] = own ? fmax(fabs(Dinv * qi), fabs(Dinv * Pxv)) * csinv : 0.0;  // gradient scale
                block_max(v);
                double gsc = fmax(1.0, v[1]);
                int okc = pass_counts(c) && v[0] <= tol * gsc;
                if (own) {
                    double axu = axb * Ebinv, arv = axr * Erinv;
                    if (slb > -INFTY && axu < lb - tol * (1.0 + fabs(lb))) okc = 0;
                    if (sub < INFTY && axu > ub + tol * (1.0 + fabs(ub))) okc = 0;
                    if (slr > -INFTY && arv < lr - tol * (1.0 + fabs(lr))) okc = 0;
                    if (sur < INFTY && arv > ur + tol * (1.0 + fabs(ur))) okc = 0;
                    double ybu = pyb * cold(C_EB) * csinv, yru = pyr * cold(C_ER) * csinv;
                    if (actb < 0 && ybu > tol * gsc) okc = 0;
                    if (actb > 0 && ybu < -tol * gsc) okc = 0;
                    if (actr < 0 && yru > tol * gsc) okc = 0;
                    if (actr > 0 && yru < -tol * gsc) okc = 0;
                }
                double fo[1] = {okc ? 0.0 : 1.0};
                block_max(fo);
                if (fo[0] == 0.0) {
                    x = px_;
                    zb = clampd(axb, slb, sub);
                    zr = clampd(axr, slr, sur);
                    yb = pyb;
                    yr = pyr;
                    pol = ps + 16 * rounds;
                    phase = PH_DONE;
                    continue;
                }
                if (ps < c.polish_max_pass) {
                    // primal-dual active-set update with the OSQP rule on the polished (Ax, y)
                    actb = own ? active_sign(axb, slb, sub, pyb) : 0;
                    actr = own ? active_sign(axr, slr, sur, pyr) : 0;
                    ++ps;
                    continue;
                }
                if (polish_continues(c, rounds, iter)) {
                    // not certified: continue ADMM to a 100x tighter tolerance, then polish again
                    ++rounds;
                    escale *= 1e-2;
                    ++iter;
                    phase = PH_ADMM;
                    continue;
                }
                phase = PH_DONE;
            }
        }
        if (iter > c.max_iter) iter = c.max_iter;
        xsol = cold(C_D) * x;
        if (CLOSED && a.wsWarm && t == 0)
            store_warm<FUSED>(a, b, rho, status == TRAJ_STATUS_OPTIMAL || status == TRAJ_STATUS_OPTIMAL_INACCURATE, iter);
        if (pol_open) toc(cyc_pol);
        stamp(8, nfact);
        stamp(10, ps);
        stamp(11, cyc_res);
        stamp(12, cyc_sweep);
        stamp(13, cyc_pol);
        stamp(14, n_res);
    } else {
        status = early;
        iter = 0;
        if (CLOSED && a.wsWarm && t == 0) store_warm_early<FUSED>(a, b);
    }

    stamp(6, __builtin_amdgcn_s_memtime());
    stamp(9, iter);
    // ---- 5. outputs (:257-275) ------------------------------------------------------
    const bool good = (status == TRAJ_STATUS_OPTIMAL || status == TRAJ_STATUS_OPTIMAL_INACCURATE);
    double* Ubuf = s_ex;  // U (stage-major) for the X rollout
    __syncthreads();
    if (own) Ubuf[t] = xsol;
    __syncthreads();
    // X_opt by the linear model X_{k+1} = A_k X_k + B_k U_k + g_k (s_xh reused); the closed loop
    // returns neither X_opt nor the objective (main.py:94 keeps only u_cmd): skipped there
    rollout_xopt(gA, gB, gg, 36, 12, 6, CLOSED ? 0 : N, Ubuf, s_x0, s_xh, t);
    // objective = cost of :217-250 at (X_opt, U_opt)
    double op = 0.0;
    for (int k = t; k <= (CLOSED ? -1 : N); k += NT)
        stage_cost(c, k, N, s_xh, s_pref, s_vref[k], s_sc[2 * k], s_sc[2 * k + 1], Ubuf, s_up, op);
    double obj = CLOSED ? 0.0 : block_sum(op);
    stamp(7, __builtin_amdgcn_s_memtime());
    stamp(3, __builtin_amdgcn_s_memrealtime());
    double uc0 = good ? Ubuf[0] : s_up[0], uc1 = good ? Ubuf[1] : s_up[1];
    if (CLOSED) {
        // plant x <- x + Ts f(x, u_cmd) (main.py:97), u_prev <- u_cmd (:101)
        if (t == 0) {
            plant_step<FUSED, PARK>(a, b, step, tstep, s_x0, uc0, uc1, status, iter, s_park);
            if (FUSED) {
                if (step == a.nsteps - 1) stamp(23, __builtin_amdgcn_s_memrealtime());   // launch span
                if (dbg_items) dbg_items[4 * (size_t)item_of_wave + 2] = __builtin_amdgcn_s_memrealtime();
                // hand the instance to whichever workgroup takes its next step: the sc1 state stores
                // complete (vmcnt(0)), then the step counter is stored sc1 (no L2 writeback)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&a.queue[2 + b], step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        continue;
    }
    store_outputs(a, b, N, t, NT, good, uc0, uc1, status, obj, iter, pol, own, ch, kk, xsol, s_xh);
    }   // steps / work items
}

}  // namespace tgmpc

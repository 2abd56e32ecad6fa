// san_route.cpp -- csrc/mpc_route.h on the host under AddressSanitizer / UBSan: route() for every horizon -1 .. 1026,
// with and without state bounds, under the four settings of the row-split switches, for the four entries (B = 1 and 7,
// the step's linearization switch both ways), held to the invariants the entry points of trajmpc.hip rely on; and the
// workspace layout (layout()) for B in {0, 1, 7, 4096} and every N in 1 .. 1024, held to its own.
// Prints "san_route ok".
#include <cstdio>
#include <cstring>

#include "../../trajectory_generation_amd/csrc/mpc_route.h"

using namespace tgmpc;

static long long checked = 0;

#define REQUIRE(cond)                                                                                            \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::printf("san_route FAILED: %s (N=%d bounds=%d split=%d..%d entry=%d B=%d)\n", #cond, c.N, bounds, \
                        s.split_min_n, s.split_max_n, (int)e, B);                                                \
            return 1;                                                                                            \
        }                                                                                                        \
    } while (0)

static traj_mpc_config config(int N, bool bounds) {
    traj_mpc_config c;
    std::memset(&c, 0, sizeof(c));
    c.N = N;
    c.Ts = 0.05;
    c.max_iter = 200;
    c.check_interval = 25;
    c.scaling_iters = 10;
    // the solver settings check_cfg holds to OSQP's ranges: traj_default_config's values
    c.eps_abs = 1e-5; c.eps_rel = 1e-5; c.eps_prim_inf = 1e-4;
    c.rho = 0.1; c.sigma = 1e-6; c.alpha = 1.6; c.delta = 1e-6;
    c.polish = 1; c.polish_refine_iter = 3; c.adaptive_rho = 1; c.adaptive_rho_tol = 5.0;
    c.polish_max_pass = 8; c.cert_tol = 1e-9; c.polish_max_rounds = 2;
    if (bounds) {   // x_lo given, one finite entry
        c.has_x_lo = 1;
        for (int i = 0; i < 6; ++i) c.x_lo[i] = -1e30;
        c.x_lo[3] = -1.0;
    }
    return c;
}

static int check(const traj_mpc_config& c, bool bounds, const Switches& s, Entry e, int B) {
    const Route r = route(&c, B, e, s);
    const int N = c.N;
    // what check_cfg has always refused: a horizon outside 1 .. TRAJ_MAX_N_GENERAL (the other fields are valid here)
    REQUIRE((r.err != 0) == (N < 1 || N > TRAJ_MAX_N_GENERAL));
    ++checked;
    if (r.err) {
        REQUIRE(r.err == TRAJ_E_ARG);
        return 0;
    }
    REQUIRE(r.need >= r.scratch_off + r.scratch_bytes);
    REQUIRE(r.scratch_off % 8 == 0);
    REQUIRE(r.scratch_off == r.base);
    REQUIRE((r.base == 0) == (e == Entry::Qp));
    REQUIRE(r.tier != Tier::Split || (N >= 21 && N <= 64 && !bounds));
    REQUIRE(r.tier != Tier::Long || (N >= 41 && N <= 256 && !bounds));
    REQUIRE(r.tier != Tier::Reg || (N <= 40 && !bounds));
    REQUIRE((r.tier == Tier::General) == (bounds || N > 256));
    REQUIRE(r.fused == (e == Entry::ClosedRun && (r.tier == Tier::Reg || r.tier == Tier::Split)));
    REQUIRE(r.inlin == (e == Entry::Step && s.step_inlin && (r.tier == Tier::Reg || r.tier == Tier::Split)));
    // the scratch holds what the tier's kernel carves from it (split_inst.hip aligns its pointer up to 16 bytes)
    const size_t B8 = (size_t)B * sizeof(double);
    if (r.tier == Tier::Split) REQUIRE(r.scratch_bytes >= B8 * split_ws_doubles(N) + 8);
    if (r.tier == Tier::Long) REQUIRE(r.scratch_bytes >= B8 * long_ws_doubles(N));
    if (r.tier == Tier::General) REQUIRE(r.scratch_bytes >= B8 * gen_ws_doubles(N));
    if (r.tier == Tier::Reg) REQUIRE(r.scratch_bytes == 0);
    // the QP entry keeps the capacity-80 kernel up to TRAJ_MAX_N
    if (e == Entry::Qp && N <= 40 && !bounds) REQUIRE(r.tier == Tier::Reg && r.need == 0);
    // the two closed-loop entries share one workspace, never smaller than what traj_closed_loop_check asks for
    if (e == Entry::ClosedRun) REQUIRE(r.need == route(&c, B, Entry::ClosedStep, s).need);
    if (e == Entry::ClosedStep) REQUIRE(r.need >= ws_base_bytes(B, N) + split_bytes(B, N));
    return 0;
}

// the base part's layout: regions in ascending order that do not overlap, doubles 8-byte and ints 4-byte aligned, the
// order B ints and the queue 2 B + 2, and the total what ws_base_bytes returns -- the parent's closed form
static int check_layout(int B, int N) {
#define REQUIRE_L(cond)                                                                \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("san_route FAILED: layout: %s (B=%d N=%d)\n", #cond, B, N);    \
            return 1;                                                                  \
        }                                                                              \
    } while (0)
    const WsLayout w = layout(B, N);
    const size_t b = (size_t)B, bn = b * (size_t)N, d = sizeof(double), i = sizeof(int);
    // {offset, bytes, alignment} in the order of the workspace
    const size_t reg[9][3] = {{w.A, bn * 36 * d, d},    {w.Bm, bn * 12 * d, d}, {w.g, bn * 6 * d, d},
                              {w.xf, bn * 12 * d, d},   {w.warm, b * 4 * d, d}, {w.order, b * i, i},
                              {w.q_count, i, i},        {w.q_err, i, i},        {w.q_done, b * i, i}};
    REQUIRE_L(w.A == 0);
    for (int k = 0; k < 9; ++k) {
        REQUIRE_L(reg[k][0] % reg[k][2] == 0);
        const size_t next = k + 1 < 9 ? reg[k + 1][0] : w.q_claimed;
        REQUIRE_L(reg[k][0] + reg[k][1] <= next);                      // ascending, no overlap
        REQUIRE_L(B == 0 || reg[k][1] == 0 || reg[k][0] < next);
    }
    REQUIRE_L(w.q_claimed % i == 0 && w.q_claimed + b * i <= w.total);
    REQUIRE_L(w.q_count - w.order == b * i);                           // the order: B ints
    REQUIRE_L(w.queue_bytes == (2 * b + 2) * i);                       // the queue: 2 B + 2 ints, from its counter
    REQUIRE_L(w.q_count + w.queue_bytes == w.q_claimed + b * i);
    REQUIRE_L(w.total % 8 == 0);
    REQUIRE_L(w.total == ws_base_bytes(B, N));
    REQUIRE_L(w.total == (66 * bn + 4 * b) * 8 + (((3 * b + 2) * 4 + 7) / 8) * 8);
#undef REQUIRE_L
    ++checked;
    return 0;
}

int main() {
    const int layout_batches[4] = {0, 1, 7, 4096};
    for (int B : layout_batches)
        for (int N = 1; N <= 1024; ++N)
            if (check_layout(B, N)) return 1;
    const int pairs[4][2] = {{21, 64}, {41, 64}, {21, 0}, {41, 0}};
    const Entry entries[4] = {Entry::Step, Entry::Qp, Entry::ClosedStep, Entry::ClosedRun};
    const int batches[2] = {1, 7};
    for (int N = -1; N <= 1026; ++N)
        for (int bounds = 0; bounds < 2; ++bounds)
            for (const auto& pr : pairs)
                for (int inlin = 0; inlin < 2; ++inlin)
                    for (Entry e : entries)
                        for (int B : batches) {
                            const traj_mpc_config c = config(N, bounds);
                            if (check(c, bounds, Switches{pr[0], pr[1], inlin}, e, B)) return 1;
                        }
    // refused whatever the horizon: no configuration, B < 0, an invalid field
    const Switches s{21, 64, 1};
    traj_mpc_config c = config(20, false);
    if (route(nullptr, 4, Entry::Step, s).err != TRAJ_E_ARG || route(&c, -1, Entry::Step, s).err != TRAJ_E_ARG ||
        route(&c, 0, Entry::Step, s).err != TRAJ_OK) {
        std::printf("san_route FAILED: null configuration / B\n");
        return 1;
    }
    c.Ts = 0.0;
    traj_mpc_config c2 = config(20, false);
    c2.polish_mode = 2;
    for (Entry e : entries)
        if (route(&c, 4, e, s).err != TRAJ_E_ARG || route(&c2, 4, e, s).err != TRAJ_E_ARG) {
            std::printf("san_route FAILED: invalid field accepted\n");
            return 1;
        }
    std::printf("san_route ok: %lld routes and layouts\n", checked);
    return 0;
}

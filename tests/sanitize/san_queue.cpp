// san_queue.cpp -- csrc/mpc_queue.h (the fused closed loop's work-queue order) on the host under AddressSanitizer /
// UBSan: QueueOrder over B in {1, 2, 3, 7, 16}, nsteps in {1, 2, 5, 9}, lead_steps in {0, 1, 3, 5, 9, 12} and
// lead_h in 0 .. B, held to what the fused kernels rely on --
//   decode maps 0 .. B nsteps - 1 one to one onto (step, rank), both in range;
//   encode(decode(q)) == q;
//   the level decode returns never decreases in q (and is level_of(step, rank));
//   for every rank the item of step s comes after the item of step s - 1 (an item only ever waits for an item drawn
//   before it: no deadlock).
// Prints "san_queue ok".
#include <cstdio>
#include <vector>

#include "../../trajectory_generation_amd/csrc/mpc_queue.h"

using namespace tgmpc;

#define REQUIRE(cond)                                                                                              \
    do {                                                                                                           \
        if (!(cond)) {                                                                                             \
            std::printf("san_queue FAILED: %s (B=%d nsteps=%d lead_steps=%d lead_h=%d q=%d)\n", #cond, B, S, lead, \
                        lh, q);                                                                                    \
            return 1;                                                                                              \
        }                                                                                                          \
    } while (0)

static int check(int B, int S, int lead, int lh) {
    const QueueOrder qo(B, S, lead, lh);
    int q = -1;
    REQUIRE(qo.total() == B * S);
    std::vector<int> item(B * S, -1);   // [step * B + rank] -> q
    int prev_level = 0;
    for (q = 0; q < qo.total(); ++q) {
        int st = -1, rk = -1;
        const int lv = qo.decode(q, st, rk);
        REQUIRE(st >= 0 && st < S);
        REQUIRE(rk >= 0 && rk < B);
        REQUIRE(item[st * B + rk] == -1);   // one to one (and onto: total() items into total() cells)
        item[st * B + rk] = q;
        REQUIRE(qo.encode(st, rk) == q);
        REQUIRE(lv >= prev_level);
        REQUIRE(lv == qo.level_of(st, rk));
        prev_level = lv;
    }
    for (int rk = 0; rk < B; ++rk)
        for (int st = 1; st < S; ++st) {
            q = item[st * B + rk];
            REQUIRE(q > item[(st - 1) * B + rk]);
        }
    return 0;
}

int main() {
    const int Bs[] = {1, 2, 3, 7, 16}, Ss[] = {1, 2, 5, 9}, leads[] = {0, 1, 3, 5, 9, 12};
    int settings = 0;
    for (int B : Bs)
        for (int S : Ss)
            for (int lead : leads)
                for (int lh = 0; lh <= B; ++lh) {
                    if (check(B, S, lead, lh)) return 1;
                    ++settings;
                }
    std::printf("san_queue ok (%d settings)\n", settings);
    return settings == 816 ? 0 : 1;
}

// san_spline.cpp -- csrc/spline.h on the host under ASan / UBSan (tests/test_workload_host.py builds and runs it).
// Every trajectory gets heap buffers of exactly kmax knots and kmax - 1 rows, so a read past the knots or a write past
// the row is an error: kmax 2 .. 13, nk 0 .. kmax + 1 (refused below 2 and past kmax), the three kinds, a repeated knot
// wherever nk = 5.  The row past the pieces, and every row of another kind or of refused knots, must come back zero.
#include <cstdio>
#include <vector>

#include "../../trajectory_generation_amd/csrc/spline.h"

int main() {
    unsigned s = 1;
    auto u = [&]() {
        s = s * 1664525u + 1013904223u;
        return (double)(s >> 8) / 16777216.0;
    };
    int flagged = 0, rows = 0;
    for (int kmax = 2; kmax <= 13; ++kmax)
        for (int nk = 0; nk <= kmax + 1; ++nk)
            for (int kind = 0; kind < 3; ++kind) {
                std::vector<double> xk(kmax), yk(kmax), coef(4 * (kmax - 1), -7.0);
                double x = -3.0;
                for (int i = 0; i < kmax; ++i) {
                    x += 0.2 + 4.8 * u();
                    xk[i] = x;
                    yk[i] = 6.0 * u() - 3.0;
                }
                const bool repeated = nk == 5 && kmax >= 5;
                if (repeated) xk[3] = xk[2];
                const int f = tgspline::spline_coef_row(kind, nk, kmax, xk.data(), yk.data(), coef.data());
                const bool refuse = kind == 2 && (nk < 2 || nk > kmax || repeated);
                if (f != (refuse ? 1 : 0)) {
                    std::printf("flag %d at kmax %d nk %d kind %d\n", f, kmax, nk, kind);
                    return 1;
                }
                const int pieces = (kind == 2 && !f) ? nk - 1 : 0;
                for (int i = 0; i < 4 * (kmax - 1); ++i)
                    if (i >= 4 * pieces ? coef[i] != 0.0 : (i % 4 == 0 && coef[i] != yk[i / 4])) {
                        std::printf("row entry %d at kmax %d nk %d kind %d\n", i, kmax, nk, kind);
                        return 1;
                    }
                flagged += f;
                ++rows;
            }
    std::printf("san_spline ok: %d rows, %d refused\n", rows, flagged);
    return 0;
}

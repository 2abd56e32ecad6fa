// san_track.cpp -- csrc/track.h on the host under ASan / UBSan (tests/test_track_host.py builds and runs it).
// Every track lives in heap buffers of exactly M + 1 parameters and M pieces, so a read past either is an error.  The
// periodic spline is built here by a dense solve (M <= 16), then project and window run at the edge inputs: s at 0 and
// at L (and past it, and negative), M = 3, a point on every knot, a NaN s_prev, samples 1 and 8, newton 0 and 8, a
// local reach of 0, a point that is not finite, a heading that is not finite, a window several laps long.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../trajectory_generation_amd/csrc/track.h"

using namespace tgtrack;

struct Built {
    std::vector<double> sig, coef, px, py;
    Track view() const { return Track{(int)px.size(), sig.data(), coef.data(), sig.back()}; }
};

static Built build(int M, double rx, double ry, double wob, bool clockwise) {
    Built t;
    t.px.resize(M);
    t.py.resize(M);
    for (int j = 0; j < M; ++j) {
        const double th = 6.283185307179586 * (clockwise ? M - 1 - j : j) / M;
        t.px[j] = rx * std::cos(th);
        t.py[j] = ry * std::sin(th) + wob * std::sin(2.0 * th);
    }
    std::vector<double> h(M);
    t.sig.assign(M + 1, 0.0);
    for (int i = 0; i < M; ++i) {
        const int ip = (i + 1) % M;
        h[i] = std::hypot(t.px[ip] - t.px[i], t.py[ip] - t.py[i]);
        t.sig[i + 1] = t.sig[i] + h[i];
    }
    t.coef.assign((size_t)M * 8, 0.0);
    for (int c = 0; c < 2; ++c) {
        const std::vector<double>& y = c ? t.py : t.px;
        std::vector<double> A((size_t)M * M, 0.0), m(M);
        for (int i = 0; i < M; ++i) {
            const int im = (i + M - 1) % M, ip = (i + 1) % M;
            A[(size_t)i * M + im] += h[im];
            A[(size_t)i * M + i] += 2.0 * (h[im] + h[i]);
            A[(size_t)i * M + ip] += h[i];
            m[i] = 6.0 * ((y[ip] - y[i]) / h[i] - (y[i] - y[im]) / h[im]);
        }
        for (int k = 0; k < M; ++k)   // (strictly diagonally dominant: no pivoting)
            for (int r = k + 1; r < M; ++r) {
                const double f = A[(size_t)r * M + k] / A[(size_t)k * M + k];
                for (int q = k; q < M; ++q) A[(size_t)r * M + q] -= f * A[(size_t)k * M + q];
                m[r] -= f * m[k];
            }
        for (int k = M - 1; k >= 0; --k) {
            for (int q = k + 1; q < M; ++q) m[k] -= A[(size_t)k * M + q] * m[q];
            m[k] /= A[(size_t)k * M + k];
        }
        for (int i = 0; i < M; ++i) {
            const int ip = (i + 1) % M;
            double* q = &t.coef[(size_t)i * 8 + 4 * c];
            q[0] = y[i];
            q[1] = (y[ip] - y[i]) / h[i] - h[i] * (2.0 * m[i] + m[ip]) / 6.0;
            q[2] = m[i] / 2.0;
            q[3] = (m[ip] - m[i]) / (6.0 * h[i]);
        }
    }
    return t;
}

static int fail(const char* what, int M, double v) {
    std::printf("%s at M = %d: %.17g\n", what, M, v);
    return 1;
}

int main() {
    int projections = 0, windows = 0;
    const double nan = std::nan("");
    for (int M = 3; M <= 16; ++M)
        for (int cw = 0; cw < 2; ++cw) {
            const Built b = build(M, 2.0, 1.2, M >= 6 ? 0.25 : 0.0, cw != 0);
            const Track tr = b.view();
            const double L = tr.L;
            // wrap and the piece lookup at the ends
            const double ends[] = {0.0, L, -0.0, std::nextafter(L, 0.0), std::nextafter(0.0, -1.0), -L, 2.0 * L, 7.3 * L, -0.4 * L};
            for (double s : ends) {
                const double w = trk_wrap(s, L);
                if (!(w >= 0.0 && w < L)) return fail("wrap out of range", M, w);
                const int i = trk_piece(tr, w);
                if (i < 0 || i >= M || !(tr.sig[i] <= w)) return fail("piece", M, w);
            }
            if (trk_piece(tr, nan) != 0) return fail("piece of NaN", M, 0);
            const Point p0 = trk_eval(tr, 0.0);
            if (p0.X != b.px[0] || p0.Y != b.py[0]) return fail("P(0) is not the first knot", M, p0.X);
            for (int samples : {1, 8})
                for (int newton : {0, 8})
                    for (double reach : {0.0, 0.5}) {
                        const Search se{samples, reach, 2.0 * reach, newton};
                        // a point on every knot: the knot's own parameter, globally and locally from anywhere near
                        for (int j = 0; j < M; ++j) {
                            const double sp[] = {nan, tr.sig[j], 0.0, std::nextafter(L, 0.0)};
                            for (double s_prev : sp) {
                                const double s = trk_project(tr, se, b.px[j], b.py[j], s_prev);
                                ++projections;
                                if (!(s >= 0.0 && s < L)) return fail("projection out of range", M, s);
                                const bool own = !(s_prev == s_prev) || s_prev == tr.sig[j];
                                if (own && trk_dist2(tr, s, b.px[j], b.py[j]) > 1e-18)
                                    return fail("a point on a knot is not projected onto it", M, s);
                            }
                        }
                        // points that are not finite: a parameter on the track all the same
                        const double bad[][2] = {{nan, 0.0}, {0.0, nan}, {HUGE_VAL, 0.0}, {-HUGE_VAL, HUGE_VAL}};
                        for (const auto& p : bad)
                            for (double s_prev : {nan, 0.3 * L}) {
                                const double s = trk_project(tr, se, p[0], p[1], s_prev);
                                ++projections;
                                if (!(s >= 0.0 && s < L)) return fail("projection of a bad point", M, s);
                            }
                    }
            // windows: from 0, from just below L, several laps long, with headings on other branches and bad ones
            for (int N : {1, 15, 16, 17, 33, 200}) {
                std::vector<double> vr(N + 1, 1.5), pref(3 * (size_t)(N + 1));
                const double starts[] = {0.0, std::nextafter(L, 0.0), 0.37 * L};
                const double phis[] = {0.0, 20.0, -13.0, nan, HUGE_VAL, 1e300};
                for (double s0 : starts)
                    for (double phi : phis)
                        for (int has : {0, 1}) {
                            trk_window(tr, s0, has != 0, phi, vr.data(), N, 0.05, pref.data());
                            ++windows;
                            for (int k = 0; k <= N; ++k) {
                                if (!(pref[3 * k] == pref[3 * k]) || !(pref[3 * k + 2] == pref[3 * k + 2]))
                                    return fail("window holds NaN", M, (double)k);
                                if (k > 0 && std::fabs(pref[3 * k + 2] - pref[3 * k - 1]) > 1.5)
                                    return fail("heading jumps", M, (double)k);
                            }
                            if (has && std::fabs(phi) < 100.0 && std::fabs(pref[2] - phi) > 3.1415926535897936)
                                return fail("heading off the vehicle's branch", M, pref[2]);
                        }
            }
        }
    std::printf("san_track ok: %d projections, %d windows\n", projections, windows);
    return 0;
}

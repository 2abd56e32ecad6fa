// track.h -- closed tracks for the MPC closed loop (include/trajtrack.h), for host and device: a track is a periodic C2
// cubic spline P(s) = (X(s), Y(s)) through M knots, parametrised by cumulative chord length; the vehicle's place on it
// is found by projection, and the MPC's window advances along it in s.  One text: the device kernels (track.hip), the
// host entry points (traj_track_project_host / traj_track_window_host) and the stand-alone sanitizer program
// (tests/sanitize/san_track.cpp) all compile these functions.
//
//   track     sig [M + 1] with sig[0] = 0, sig[i+1] = sig[i] + |P_{i+1} - P_i|, L = sig[M]; coef [M, 2, 4]: piece i of
//             coordinate c is  c0 + t (c1 + t (c2 + t c3)),  t = s - sig[i]  (TrackSet.build solves the cyclic
//             tridiagonal system of the periodic spline in numpy: that is the specification)
//   wrap      wrap(s) = s - L floor(s / L); a result that rounds to L -- or below 0, where the quotient rounded up to
//             an integer -- becomes 0
//   project   candidates c(i, j) = sig[i] + (sig[i+1] - sig[i]) j / S in the order e = i S + j; local search (s_prev not
//             NaN): those whose signed cyclic offset wrap(c - s_prev + L / 2) - L / 2 lies in [-back, fwd]; global search
//             otherwise, and when no local candidate wins.  The smallest squared distance wins, the lowest e on a tie;
//             a distance that is not finite never wins, and with no winner at all the choice is e = 0.  Then `newton`
//             iterations on g = (P - p) . P':  g' = P' . P' + (P - p) . P'';  while g' > 0:
//             s <- wrap(s - clamp(g / g', +-h)), h the chosen piece's candidate spacing; otherwise stop (and stop on a
//             step that is NaN, which only a point that is not finite gives).
//   window   s_0 given, s_{k+1} = s_k + vref_k Ts / |P'(wrap(s_k))| (unwrapped, a serial sum); the reference point is
//             P(wrap(s_k)), a_k = atan2(Y', X'); the heading is unwound onto the vehicle's branch by integer windings
//             n_0 = rint((phi - a_0) / 2 pi) (0 without a heading), n_k = n_{k-1} - rint((a_k - a_{k-1}) / 2 pi),
//             phi*_k = a_k + 2 pi n_k.
//
// Every choice above is made on exact quantities (comparisons, integers), so any mapping of the work onto lanes gives
// the same bits: the candidates may be searched in any partition (trk_better is a total order), the windings are
// integers and may be summed in any order.  float64, built with -ffp-contract=off like the rest of the library; sqrt,
// floor and rint are exact on both sides, so host and device differ by atan2 alone.
#ifndef TGMPC_TRACK_H
#define TGMPC_TRACK_H

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TRK_HD __host__ __device__ __forceinline__
#else
#define TRK_HD inline
#endif

// the device's atan2 is the MPC path's (physics.h pm_atan2) where the including file names it
#if defined(__HIP_DEVICE_COMPILE__) && defined(TRK_DEVICE_ATAN2)
#define TRK_ATAN2(y, x) TRK_DEVICE_ATAN2(y, x)
#else
#define TRK_ATAN2(y, x) atan2(y, x)
#endif

namespace tgtrack {

constexpr double TRK_TWO_PI = 6.283185307179586;
constexpr int TRK_NONE = 0x7fffffff;   // "no candidate": loses every comparison of indices

struct Track {
    int M;                // pieces (= knots)
    const double* sig;    // [M + 1]
    const double* coef;   // [M, 2, 4]
    double L;             // sig[M]
};

struct Search {
    int samples;
    double back, fwd;
    int newton;
};

struct Point {
    double X, Y, dX, dY, ddX, ddY;
};

TRK_HD double trk_nan() { return __builtin_nan(""); }

TRK_HD double trk_wrap(double s, double L) {
    const double r = s - L * floor(s / L);
    return (r >= L || r < 0.0) ? 0.0 : r;
}

// the piece of a wrapped s: the largest i in 0 .. M - 1 with sig[i] <= s (0 for NaN)
TRK_HD int trk_piece(const Track& tr, double s) {
    int lo = 0, hi = tr.M;   // sig[lo] <= s < sig[hi], as far as comparisons hold
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tr.sig[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// P, P', P'' on piece i at t = s - sig[i]
TRK_HD Point trk_eval_piece(const Track& tr, int i, double t) {
    const double* cx = tr.coef + 8 * (size_t)i;
    const double* cy = cx + 4;
    Point q;
    q.X = cx[0] + t * (cx[1] + t * (cx[2] + t * cx[3]));
    q.Y = cy[0] + t * (cy[1] + t * (cy[2] + t * cy[3]));
    q.dX = cx[1] + t * (2.0 * cx[2] + t * (3.0 * cx[3]));
    q.dY = cy[1] + t * (2.0 * cy[2] + t * (3.0 * cy[3]));
    q.ddX = 2.0 * cx[2] + t * (6.0 * cx[3]);
    q.ddY = 2.0 * cy[2] + t * (6.0 * cy[3]);
    return q;
}

// at a wrapped s
TRK_HD Point trk_eval(const Track& tr, double s) {
    const int i = trk_piece(tr, s);
    return trk_eval_piece(tr, i, s - tr.sig[i]);
}

// candidate e = i S + j: its parameter
TRK_HD double trk_candidate(const Track& tr, int S, int e) {
    const int i = e / S, j = e % S;
    return tr.sig[i] + ((tr.sig[i + 1] - tr.sig[i]) * (double)j) / (double)S;
}

// the order of the choice: (d, e) beats (bd, be) -- a total order on finite d, and no d that is not finite beats anything
TRK_HD bool trk_better(double d, int e, double bd, int be) { return d < bd || (d == bd && e < be); }

// One candidate scored against the running local and global bests (d = +inf, e = TRK_NONE to begin with).
TRK_HD void trk_score(const Track& tr, const Search& se, double px, double py, double s_prev, bool local, int e,
                      double& dl, int& el, double& dg, int& eg) {
    const int i = e / se.samples, j = e % se.samples;
    const double t = ((tr.sig[i + 1] - tr.sig[i]) * (double)j) / (double)se.samples;
    const Point q = trk_eval_piece(tr, i, t);
    const double ex = q.X - px, ey = q.Y - py;
    const double d = ex * ex + ey * ey;
    if (trk_better(d, e, dg, eg)) {
        dg = d;
        eg = e;
    }
    if (local) {
        const double off = trk_wrap((tr.sig[i] + t) - s_prev + tr.L / 2.0, tr.L) - tr.L / 2.0;
        if (off >= -se.back && off <= se.fwd && trk_better(d, e, dl, el)) {
            dl = d;
            el = e;
        }
    }
}

TRK_HD int trk_choice(int el, int eg) { return el != TRK_NONE ? el : (eg != TRK_NONE ? eg : 0); }

// the refinement from candidate e
TRK_HD double trk_refine(const Track& tr, const Search& se, double px, double py, int e) {
    const int i = e / se.samples;
    const double h = (tr.sig[i + 1] - tr.sig[i]) / (double)se.samples;
    double s = trk_candidate(tr, se.samples, e);
    for (int it = 0; it < se.newton; ++it) {
        const Point q = trk_eval(tr, s);
        const double ex = q.X - px, ey = q.Y - py;
        const double g = ex * q.dX + ey * q.dY;
        const double gp = (q.dX * q.dX + q.dY * q.dY) + (ex * q.ddX + ey * q.ddY);
        if (!(gp > 0.0)) break;
        const double st = g / gp;
        if (st != st) break;   // (a point that is not finite: the result stays a place on the track)
        s = trk_wrap(s - (st > h ? h : (st < -h ? -h : st)), tr.L);
    }
    return s;
}
// the squared distance of p to P(s), s wrapped
TRK_HD double trk_dist2(const Track& tr, double s, double px, double py) {
    const Point q = trk_eval(tr, s);
    const double ex = q.X - px, ey = q.Y - py;
    return ex * ex + ey * ey;
}

// project(p, s_prev), every candidate in turn
TRK_HD double trk_project(const Track& tr, const Search& se, double px, double py, double s_prev) {
    const bool local = s_prev == s_prev;
    double dl = HUGE_VAL, dg = HUGE_VAL;
    int el = TRK_NONE, eg = TRK_NONE;
    const int n = tr.M * se.samples;
    for (int e = 0; e < n; ++e) trk_score(tr, se, px, py, s_prev, local, e, dl, el, dg, eg);
    return trk_refine(tr, se, px, py, trk_choice(el, eg));
}

// rint(x) as an int; 0 where x is NaN or out of an int's range (a state that is not finite: the solver refuses it)
TRK_HD int trk_rint(double x) { return fabs(x) < 1e9 ? (int)rint(x) : 0; }

// one stage of the window at the unwrapped s: the reference point, the raw heading a, and the next stage's s
TRK_HD void trk_stage(const Track& tr, double s, double vts, double& X, double& Y, double& a, double& s_next) {
    const Point q = trk_eval(tr, trk_wrap(s, tr.L));
    X = q.X;
    Y = q.Y;
    a = TRK_ATAN2(q.dY, q.dX);
    s_next = s + vts / sqrt(q.dX * q.dX + q.dY * q.dY);
}
// the chain alone (what the stage adds to s)
TRK_HD double trk_advance(const Track& tr, double s, double vts) {
    const Point q = trk_eval(tr, trk_wrap(s, tr.L));
    return s + vts / sqrt(q.dX * q.dX + q.dY * q.dY);
}
TRK_HD int trk_wind0(bool has_phi, double phi, double a0) { return has_phi ? trk_rint((phi - a0) / TRK_TWO_PI) : 0; }
TRK_HD int trk_turn(double a, double a_prev) { return trk_rint((a - a_prev) / TRK_TWO_PI); }
TRK_HD double trk_heading(double a, int n) { return a + TRK_TWO_PI * (double)n; }

// the window [N + 1, 3] from s0, serially; vr[k], k = 0 .. N - 1 are read
TRK_HD void trk_window(const Track& tr, double s0, bool has_phi, double phi, const double* vr, int N, double Ts,
                       double* pref) {
    double s = s0, a_prev = 0.0;
    int n = 0;
    for (int k = 0; k <= N; ++k) {
        double X, Y, a, sn;
        trk_stage(tr, s, k < N ? vr[k] * Ts : 0.0, X, Y, a, sn);
        n = k == 0 ? trk_wind0(has_phi, phi, a) : n - trk_turn(a, a_prev);
        pref[3 * k] = X;
        pref[3 * k + 1] = Y;
        pref[3 * k + 2] = trk_heading(a, n);
        a_prev = a;
        s = sn;
    }
}

}  // namespace tgtrack

#endif

"""The closed tracks' rules in plain numpy / Python float64: the specification the track tests compare against, never
the code under test.  (Python's float arithmetic is IEEE double, one rounding per operation, in the written order.)

Geometry    knots P_0 .. P_{M-1}, P_M = P_0; sig_0 = 0, sig_{i+1} = sig_i + |P_{i+1} - P_i|, L = sig_M; piece i per
            coordinate c0 + t (c1 + t (c2 + t c3)), t = s - sig_i; second derivatives from the cyclic tridiagonal
            system of the periodic spline.
wrap        s - L floor(s / L); a result that rounds to L (or falls below 0, where the quotient rounded up) becomes 0.
project     candidates c(i, j) = sig_i + (sig_{i+1} - sig_i) j / S, evaluated on piece i at t = (sig_{i+1} - sig_i) j / S;
            local: those with wrap(c - s_prev + L/2) - L/2 in [-back, fwd], global if s_prev is NaN or none wins; the
            smallest squared distance, the lowest (i, j) on a tie; `newton` iterations on g = (P - p) . P' with
            g' = P' . P' + (P - p) . P'': while g' > 0, s <- wrap(s - clamp(g / g', +-h)), else stop.
window      s_{k+1} = s_k + vref_k Ts / |P'(wrap(s_k))|; (X*, Y*) = P(wrap(s_k)); a_k = atan2(Y', X');
            n_0 = rint((phi - a_0) / 2 pi) (0 without phi), n_k = n_{k-1} - rint((a_k - a_{k-1}) / 2 pi),
            phi*_k = a_k + 2 pi n_k.
"""
import math

import numpy as np

TWO_PI = 6.283185307179586


def circuit_knots(M=12):
    """The 12-knot test circuit P_j = (2 cos th_j, 1.2 sin th_j + 0.25 sin 2 th_j), counter-clockwise."""
    th = 2.0 * np.pi * np.arange(M) / M
    return np.stack([2.0 * np.cos(th), 1.2 * np.sin(th) + 0.25 * np.sin(2.0 * th)], axis=1)


def circle_knots(M=16, R=2.0):
    th = 2.0 * np.pi * np.arange(M) / M
    return np.stack([R * np.cos(th), R * np.sin(th)], axis=1)


def build(knots):
    """(sig [M+1], coef [M,2,4]) of the periodic spline, by a dense solve of the cyclic system."""
    P = np.asarray(knots, dtype=np.float64)
    M = len(P)
    Pn = np.vstack([P[1:], P[:1]])
    h = np.sqrt(((Pn - P) ** 2).sum(axis=1))
    sig = np.zeros(M + 1)
    for i in range(M):
        sig[i + 1] = sig[i] + h[i]
    A = np.zeros((M, M))
    rhs = np.zeros((M, 2))
    for i in range(M):
        im, ip = (i - 1) % M, (i + 1) % M
        A[i, im] += h[im]
        A[i, i] += 2.0 * (h[im] + h[i])
        A[i, ip] += h[i]
        rhs[i] = 6.0 * ((P[ip] - P[i]) / h[i] - (P[i] - P[im]) / h[im])
    m = np.linalg.solve(A, rhs)
    coef = np.zeros((M, 2, 4))
    for i in range(M):
        ip = (i + 1) % M
        coef[i, :, 0] = P[i]
        coef[i, :, 1] = (P[ip] - P[i]) / h[i] - h[i] * (2.0 * m[i] + m[ip]) / 6.0
        coef[i, :, 2] = m[i] / 2.0
        coef[i, :, 3] = (m[ip] - m[i]) / (6.0 * h[i])
    return sig, coef


def wrap(s, L):
    r = s - L * math.floor(s / L)
    return 0.0 if (r >= L or r < 0.0) else r


def eval_piece(coef, i, t):
    """(X, Y, X', Y', X'', Y'') on piece i at t."""
    out = []
    for c in (coef[i, 0], coef[i, 1]):
        c0, c1, c2, c3 = (float(v) for v in c)
        out.append((c0 + t * (c1 + t * (c2 + t * c3)), c1 + t * (2.0 * c2 + t * (3.0 * c3)), 2.0 * c2 + t * (6.0 * c3)))
    (X, dX, ddX), (Y, dY, ddY) = out
    return X, Y, dX, dY, ddX, ddY


def eval_at(sig, coef, M, s):
    """At a wrapped s: the piece is the largest i in 0 .. M-1 with sig_i <= s."""
    i = int(np.clip(np.searchsorted(sig[:M + 1], s, side="right") - 1, 0, M - 1))
    return eval_piece(coef, i, s - float(sig[i]))


def project(sig, coef, M, p, s_prev=None, samples=8, back=0.5, fwd=1.0, newton=8):
    """-> (s, (i, j) of the chosen candidate, iterations that moved s)."""
    L = float(sig[M])
    px, py = float(p[0]), float(p[1])
    cand = []
    for i in range(M):
        hi = float(sig[i + 1]) - float(sig[i])
        for j in range(samples):
            t = (hi * float(j)) / float(samples)
            X, Y = eval_piece(coef, i, t)[:2]
            cand.append((i, j, float(sig[i]) + t, (X - px) * (X - px) + (Y - py) * (Y - py)))
    d = np.array([c[3] for c in cand])
    d = np.where(np.isfinite(d), d, np.inf)
    pick = None
    if s_prev is not None and not math.isnan(s_prev):
        ok = [k for k, c in enumerate(cand) if -back <= wrap(c[2] - s_prev + L / 2.0, L) - L / 2.0 <= fwd]
        if ok and np.isfinite(d[ok]).any():
            pick = ok[int(np.argmin(d[ok]))]          # (argmin: the first of equal minima)
    if pick is None:
        pick = int(np.argmin(d)) if np.isfinite(d).any() else 0
    i, j, s, _ = cand[pick]
    h = (float(sig[i + 1]) - float(sig[i])) / float(samples)
    moved = 0
    for _ in range(newton):
        X, Y, dX, dY, ddX, ddY = eval_at(sig, coef, M, s)
        ex, ey = X - px, Y - py
        g = ex * dX + ey * dY
        gp = (dX * dX + dY * dY) + (ex * ddX + ey * ddY)
        if not gp > 0.0:
            break
        st = g / gp
        if math.isnan(st):      # (only a point that is not finite)
            break
        s = wrap(s - (h if st > h else (-h if st < -h else st)), L)
        moved += 1
    return s, (i, j), moved


def window(sig, coef, M, s0, phi, vref, N, Ts):
    """-> (path_ref [N+1,3], windings [N+1] ints, the raw headings a [N+1])."""
    L = float(sig[M])
    pref, wind, raw = np.zeros((N + 1, 3)), [], []
    s, n, a_prev = float(s0), 0, 0.0
    for k in range(N + 1):
        X, Y, dX, dY = eval_at(sig, coef, M, wrap(s, L))[:4]
        a = math.atan2(dY, dX)
        if k == 0:
            n = 0 if phi is None else int(np.rint((float(phi) - a) / TWO_PI))
        else:
            n = n - int(np.rint((a - a_prev) / TWO_PI))
        pref[k] = (X, Y, a + TWO_PI * float(n))
        wind.append(n)
        raw.append(a)
        if k < N:
            s = s + (float(vref[k]) * Ts) / math.sqrt(dX * dX + dY * dY)
        a_prev = a
    return pref, np.array(wind), np.array(raw)


def tracking_errors(sig, coef, M, X, S):
    """e_c, e_phi [T1] of the states X [T1,6] at the places S [T1] (lateral_error's formula; the wrapped heading
    difference)."""
    L = float(sig[M])
    ec, ep = np.zeros(len(S)), np.zeros(len(S))
    for t in range(len(S)):
        Xr, Yr, dX, dY = eval_at(sig, coef, M, wrap(float(S[t]), L))[:4]
        a = math.atan2(dY, dX)
        ec[t] = math.sin(a) * (X[t, 0] - Xr) - math.cos(a) * (X[t, 1] - Yr)
        ep[t] = math.atan2(math.sin(X[t, 2] - a), math.cos(X[t, 2] - a))
    return ec, ep


def points_near(sig, coef, M, n, spread, seed):
    """n points within `spread` of the track: a uniform s and a lateral offset along the normal."""
    rng = np.random.default_rng(seed)
    L = float(sig[M])
    pts = np.zeros((n, 2))
    for b in range(n):
        X, Y, dX, dY = eval_at(sig, coef, M, rng.uniform(0.0, L))[:4]
        nrm = math.hypot(dX, dY)
        off = rng.uniform(-spread, spread)
        pts[b] = (X - off * dY / nrm, Y + off * dX / nrm)
    return pts


def rel(g, r):
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)))) if g.size else 0.0


def cyc(a, b, L):
    """|a - b| on the circle of length L."""
    d = np.abs(np.asarray(a) - np.asarray(b)) % L
    return np.minimum(d, L - d)

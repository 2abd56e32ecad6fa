"""The QP of one MPC step (MPC/mpc_6stati.py:180-250) in plain numpy float64 -- TEST INFRASTRUCTURE ONLY.

No project code and no solver: given the linearization A_k, B_k, g_k and a control sequence U, the state sequence
the equality constraints force (:186-192), the objective (:224-250) and the distance of the point from the inequality
rows (:195-221).  Whatever a solver returns as X_opt / objective for its own U_opt can be checked against these with
no second solver in between.

Optimality needs no solver either.  ``condensed`` eliminates the states (X = X_free + G u) and returns the QP as
J(u) = 1/2 u' P u + q' u + c0, lo <= A u <= hi -- box, rate and state rows; P is positive definite because R, Rd > 0.
``dual_bound`` evaluates the Lagrange dual d(y) = min_u L(u, y) in closed form: weak duality makes d(y) <= J* for
every y >= 0, whatever produced y.  ``certificate`` guesses y for a given point from the point's own active rows (a
least-squares fit of the stationarity condition, wrong-signed rows dropped) -- a heuristic, not a solver: a bad guess
only makes d smaller, never invalid.  A point with J(u) - d(y) <= tol is thereby PROVED optimal to tol.

``rollout`` and ``cost`` return, beside their value, its abs-sum scale -- the same expression evaluated on absolute
values, i.e. the size of the terms a float64 evaluation rounds (the idiom of tests/_knet_ref.py).  An error bar
proportional to it follows the growth of the unstable plant at Ts = 0.05 instead of being one flat number.

``kw`` is a plain dict of mpc_step's keyword arguments (q_c, q_phi, q_vx, R, Rd, u_bounds, du_bounds, x_lo, x_hi);
absent keys take the reference's defaults (:128-140).
"""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(q_c=6.0, q_phi=0.5, q_vx=0.5, R=np.diag([0.02, 2.0]), Rd=np.diag([0.01, 5.0]),
                u_bounds=((-1.0, 1.0), (-0.6, 0.6)), du_bounds=((-0.5, 0.5), (-0.3, 0.3)), x_lo=None, x_hi=None)


def _kw(kw, key):
    v = (kw or {}).get(key)
    return DEFAULTS[key] if v is None else v


def rollout(x0, Ad, Bd, g, U):
    """X [6,N+1] with X[:,0] = x0, X[:,k+1] = Ad[k] X[:,k] + Bd[k] U[:,k] + g[k] (:186-192), and its abs-sum scale S
    [6,N+1]: the same recurrence on |Ad|, |Bd|, |g|, |U|, |x0|.  Ad [N,6,6], Bd [N,6,2], g [N,6], U [2,N]."""
    U = np.asarray(U, dtype=np.float64)
    N = U.shape[1]
    X = np.zeros((6, N + 1))
    S = np.zeros((6, N + 1))
    X[:, 0] = x0
    S[:, 0] = np.abs(x0)
    for k in range(N):
        X[:, k + 1] = Ad[k] @ X[:, k] + Bd[k] @ U[:, k] + g[k]
        S[:, k + 1] = np.abs(Ad[k]) @ S[:, k] + np.abs(Bd[k]) @ np.abs(U[:, k]) + np.abs(g[k])
    return X, S


def cost(X, U, u_prev, path_ref, vref, kw=None):
    """The objective of :224-250 at (X [6,N+1], U [2,N]) and its abs-sum scale: the lateral, heading and speed terms
    at k = 0..N (k = 0 is a constant of the problem, k = N the terminal cost), U_k' R U_k and dU_k' Rd dU_k at
    k = 0..N-1 with the full 2x2 R, Rd and dU_0 = U_0 - u_prev."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    pr = np.asarray(path_ref, dtype=np.float64)
    q_c, q_phi, q_vx = (float(_kw(kw, k)) for k in ("q_c", "q_phi", "q_vx"))
    R = np.asarray(_kw(kw, "R"), dtype=np.float64).reshape(2, 2)
    Rd = np.asarray(_kw(kw, "Rd"), dtype=np.float64).reshape(2, 2)
    Xr, Yr, Pr = pr[:, 0], pr[:, 1], pr[:, 2]
    s, c = np.sin(Pr), np.cos(Pr)
    ec = s * (X[0] - Xr) - c * (X[1] - Yr)                                       # lateral_error (:111-117)
    ec_a = np.abs(s) * (np.abs(X[0]) + np.abs(Xr)) + np.abs(c) * (np.abs(X[1]) + np.abs(Yr))
    J = q_c * np.sum(ec ** 2) + q_phi * np.sum((X[2] - Pr) ** 2) + q_vx * np.sum((X[3] - vref) ** 2)
    Ja = (abs(q_c) * np.sum(ec_a ** 2) + abs(q_phi) * np.sum((np.abs(X[2]) + np.abs(Pr)) ** 2)
          + abs(q_vx) * np.sum((np.abs(X[3]) + np.abs(vref)) ** 2))
    Up = np.concatenate([np.asarray(u_prev, dtype=np.float64).reshape(2, 1), U[:, :-1]], axis=1)
    dU = U - Up
    dUa = np.abs(U) + np.abs(Up)
    J += np.einsum("ik,ij,jk->", U, R, U) + np.einsum("ik,ij,jk->", dU, Rd, dU)
    Ja += np.einsum("ik,ij,jk->", np.abs(U), np.abs(R), np.abs(U)) + np.einsum("ik,ij,jk->", dUa, np.abs(Rd), dUa)
    return float(J), float(Ja)


def violation(U, u_prev, kw=None, X=None):
    """How far (U, X) lies outside the inequality rows of :195-221: (box, rate, state, scale).  box / rate / state
    are the largest violations (0 when inside) of the magnitude rows, of the rate rows (dU_0 against u_prev) and --
    with x_lo / x_hi in kw and X given -- of the state rows at k = 0..N; scale is max ||[U; dU]||_inf (with X:
    ||[U; dU; X]||_inf), the size OSQP's relative primal tolerance multiplies."""
    U = np.asarray(U, dtype=np.float64)
    ub = np.asarray(_kw(kw, "u_bounds"), dtype=np.float64)        # [2, (lo, hi)]
    db = np.asarray(_kw(kw, "du_bounds"), dtype=np.float64)
    dU = U - np.concatenate([np.asarray(u_prev, dtype=np.float64).reshape(2, 1), U[:, :-1]], axis=1)

    def outside(V, lo, hi):
        return float(max(np.max(lo - V), np.max(V - hi), 0.0))

    box = outside(U, ub[:, :1], ub[:, 1:])
    rate = outside(dU, db[:, :1], db[:, 1:])
    scale = max(np.abs(U).max(), np.abs(dU).max())
    state = 0.0
    x_lo, x_hi = _kw(kw, "x_lo"), _kw(kw, "x_hi")
    if X is not None and (x_lo is not None or x_hi is not None):
        X = np.asarray(X, dtype=np.float64)
        lo = np.full(6, -np.inf) if x_lo is None else np.asarray(x_lo, dtype=np.float64).reshape(6)
        hi = np.full(6, np.inf) if x_hi is None else np.asarray(x_hi, dtype=np.float64).reshape(6)
        state = outside(X, lo[:, None], hi[:, None])
        scale = max(scale, np.abs(X).max())
    return box, rate, state, float(scale)


def _blocks(M2, N):
    """blockdiag(M2, ..., M2), N times."""
    return np.kron(np.eye(N), M2)


def condensed(x0, Ad, Bd, g, u_prev, path_ref, vref, kw=None):
    """The same QP with the states eliminated: P, q, c0, A, lo, hi, n_state with J(U) = 1/2 u' P u + q' u + c0 and
    lo <= A u <= hi, u stage-major (u[2k + ch] = U[ch, k]).  X(U) = X_free + G u: X_free is rollout at U = 0 and
    G [N+1, 6, 2N] follows the stage recurrence G_{k+1} = Ad[k] G_k, + Bd[k] in the columns of stage k.  The residual
    rows of `cost` (lateral, heading, speed at k = 0..N) are affine in u; the input terms take the symmetric parts of
    R and Rd with dU_0 = U_0 - u_prev.  Rows of A: the box on U, the rate rows D u (the u_prev offset moved into
    lo / hi), then one row per (bounded state i -- either side finite --, stage k = 1..N): G[k, i] against
    x_lo[i] - X_free[i, k] and x_hi[i] - X_free[i, k].  n_state counts those last rows."""
    Ad, Bd, g = (np.asarray(a, dtype=np.float64) for a in (Ad, Bd, g))
    N = Ad.shape[0]
    n = 2 * N
    up = np.asarray(u_prev, dtype=np.float64).reshape(2)
    Xf, _ = rollout(x0, Ad, Bd, g, np.zeros((2, N)))
    G = np.zeros((N + 1, 6, n))
    for k in range(N):
        G[k + 1] = Ad[k] @ G[k]
        G[k + 1][:, 2 * k:2 * k + 2] += Bd[k]
    pr = np.asarray(path_ref, dtype=np.float64)
    vr = np.asarray(vref, dtype=np.float64).reshape(N + 1)
    q_c, q_phi, q_vx = (float(_kw(kw, k)) for k in ("q_c", "q_phi", "q_vx"))
    R = np.asarray(_kw(kw, "R"), dtype=np.float64).reshape(2, 2)
    Rd = np.asarray(_kw(kw, "Rd"), dtype=np.float64).reshape(2, 2)
    s, c = np.sin(pr[:, 2])[:, None], np.cos(pr[:, 2])[:, None]
    # residual = M u + r0, weights w
    M = np.concatenate([s * G[:, 0] - c * G[:, 1], G[:, 2], G[:, 3]])
    r0 = np.concatenate([s[:, 0] * (Xf[0] - pr[:, 0]) - c[:, 0] * (Xf[1] - pr[:, 1]), Xf[2] - pr[:, 2], Xf[3] - vr])
    w = np.repeat([q_c, q_phi, q_vx], N + 1)
    D = np.eye(n) - np.eye(n, k=-2)                            # dU = D u + d0
    d0 = np.zeros(n)
    d0[:2] = -up
    Rs, Rds = _blocks((R + R.T) / 2, N), _blocks((Rd + Rd.T) / 2, N)
    P = 2.0 * (M.T @ (w[:, None] * M) + Rs + D.T @ Rds @ D)
    q = 2.0 * (M.T @ (w * r0) + D.T @ (Rds @ d0))
    c0 = float(np.sum(w * r0 * r0) + d0 @ Rds @ d0)
    ub = np.asarray(_kw(kw, "u_bounds"), dtype=np.float64)        # [2, (lo, hi)]
    db = np.asarray(_kw(kw, "du_bounds"), dtype=np.float64)
    A = [np.eye(n), D]
    lo = [np.tile(ub[:, 0], N), np.tile(db[:, 0], N) - d0]
    hi = [np.tile(ub[:, 1], N), np.tile(db[:, 1], N) - d0]
    x_lo, x_hi = _kw(kw, "x_lo"), _kw(kw, "x_hi")
    xl = np.full(6, -np.inf) if x_lo is None else np.asarray(x_lo, dtype=np.float64).reshape(6)
    xh = np.full(6, np.inf) if x_hi is None else np.asarray(x_hi, dtype=np.float64).reshape(6)
    n_state = 0
    for i in np.where(np.isfinite(xl) | np.isfinite(xh))[0]:
        A.append(G[1:, i])
        lo.append(xl[i] - Xf[i, 1:])
        hi.append(xh[i] - Xf[i, 1:])
        n_state += N
    return P, q, c0, np.concatenate(A), np.concatenate(lo), np.concatenate(hi), n_state


def objective(P, q, c0, u):
    return float(0.5 * u @ P @ u + q @ u + c0)


def stage_major(U):
    """U [2,N] -> u [2N], u[2k + ch] = U[ch, k]."""
    return np.asarray(U, dtype=np.float64).T.reshape(-1)


def dual_bound(P, q, c0, A, lo, hi, y_plus, y_minus, scale=False):
    """Weak duality: for ANY y_plus, y_minus >= 0 (taken only on finite hi / lo, negative parts dropped) and
    v = q + A' (y_plus - y_minus), d = c0 - 1/2 v' P^-1 v - hi . y_plus + lo . y_minus = min_u L(u, y) <= J(u) at
    every feasible u.  How y was found does not enter.  scale: return (d, its abs-sum scale) -- with w = P^-1 v,
    |c0| + 1/2 |w|' |P| |w| + |hi| . y_plus + |lo| . y_minus: a backward-stable solve returns (P + E)^-1 v with |E| a
    rounding multiple of |P|, which moves v' P^-1 v by w' E w to first order."""
    yp = np.where(np.isfinite(hi), np.maximum(y_plus, 0.0), 0.0)
    ym = np.where(np.isfinite(lo), np.maximum(y_minus, 0.0), 0.0)
    v = q + A.T @ (yp - ym)
    w = np.linalg.solve(P, v)
    bh, bl = np.where(yp > 0, hi, 0.0) * yp, np.where(ym > 0, lo, 0.0) * ym
    d = float(c0 - 0.5 * v @ w - np.sum(bh) + np.sum(bl))
    if not scale:
        return d
    aw = np.abs(w)
    return d, float(abs(c0) + 0.5 * aw @ np.abs(P) @ aw + np.sum(np.abs(bh)) + np.sum(np.abs(bl)))


def certificate(P, q, c0, A, lo, hi, u, n_state=0):
    """Multipliers for the point u from its own active set, and the dual bound they give.  Rows at a bound
    (|A u - bound| <= 1e-7 (1 + |bound|)) are candidates; lam = lstsq(A_act', -(P u + q)); rows whose multiplier has
    the wrong sign (lam < 0 at hi, > 0 at lo) are dropped; at most 20 rounds; what is left is clipped to the right
    sign.  The iteration need not be right for the bound to be: whatever y comes out, d <= J*.  Returns
    dict(J, d, d_scale: dual_bound's scale, y_plus, y_minus, n_state_active: state rows (the last n_state) carrying a
    positive multiplier)."""
    r = A @ u
    m = len(r)
    at_hi = np.isfinite(hi) & (np.abs(r - hi) <= 1e-7 * (1.0 + np.abs(hi)))
    at_lo = np.isfinite(lo) & (np.abs(r - lo) <= 1e-7 * (1.0 + np.abs(lo)))
    act = at_hi | at_lo
    grad = P @ u + q
    lam = np.zeros(m)
    for _ in range(20):
        lam[:] = 0.0
        idx = np.where(act)[0]
        if len(idx) == 0:
            break
        lam[idx] = np.linalg.lstsq(A[idx].T, -grad, rcond=None)[0]
        wrong = act & (((lam < 0) & ~at_lo) | ((lam > 0) & ~at_hi))
        if not wrong.any():
            break
        act &= ~wrong
    yp = np.where(at_hi, np.maximum(lam, 0.0), 0.0)
    ym = np.where(at_lo, np.maximum(-lam, 0.0), 0.0)
    ns = int(((yp + ym)[m - n_state:] > 0).sum()) if n_state else 0
    d, da = dual_bound(P, q, c0, A, lo, hi, yp, ym, scale=True)
    return dict(J=objective(P, q, c0, u), d=d, d_scale=da, y_plus=yp, y_minus=ym, n_state_active=ns)


def linearization(O, x0, u_prev, N, Ts, p=None):
    """The time-varying model of :165-178 from the oracle's physics: nominal_rollout at constant u_prev, then
    linearize_discretize per stage.  x0 [B,6], u_prev [B,2] -> Ad [B,N,6,6], Bd [B,N,6,2], g [B,N,6]; p is a dict of
    vehicle-parameter overrides (or None)."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 6)
    u_prev = np.asarray(u_prev, dtype=np.float64).reshape(-1, 2)
    B = x0.shape[0]
    op = O.params(p) if p else None
    Ad, Bd, g = np.zeros((B, N, 6, 6)), np.zeros((B, N, 6, 2)), np.zeros((B, N, 6))
    for b in range(B):
        xb = O.nominal_rollout(x0[b], u_prev[b], N, Ts, op)
        for k in range(N):
            Ad[b, k], Bd[b, k], g[b, k] = O.linearize_discretize(xb[:, k], u_prev[b], Ts, op)
    return Ad, Bd, g

"""The QP of one MPC step (MPC/mpc_6stati.py:180-250) in plain numpy float64 -- TEST INFRASTRUCTURE ONLY.

No project code and no solver: given the linearization A_k, B_k, g_k and a control sequence U, the state sequence
the equality constraints force (:186-192), the objective (:224-250) and the distance of the point from the inequality
rows (:195-221).  Whatever a solver returns as X_opt / objective for its own U_opt can be checked against these with
no second solver in between.

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

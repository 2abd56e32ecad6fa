"""tests/_qp_ref.py (the QP of one MPC step in plain numpy) pinned to the reference's goldens, and the GPU output
tests' case table (tests/_mpc_checks.py) walked on the CPU with the oracle standing where the kernel will.

This is where the two constants of tests/_mpc_checks.py are measured: every check prints its worst error-over-bar
ratio (bar with C = 1; run with -s) and asserts 4 x ratio <= C_X / C_J.  Measured here (float64, x86-64):

  goldens (qp_N20/N40 x Ts 0.02/0.05, the reference's own A, B, g and an IPM + exact KKT optimum):
      objective 0.036, violation <= 7.5e-13, X 0.107 of 1e-11 (1 + S) (a solver's output: see test_qp_ref_vs_golden)
  oracle over the case table, both polish modes: X 0.108 (N = 1), objective 0.0847,
      violation 0.94 of the eps bar (unpolished), 3.1e-4 of 1e-9 (polished); worst asserted optimality gap 5.0e-10
  the weak-duality certificate (tests/_mpc_checks.py certify_point; C_D = 0.06 and C_JC = 0.19 are 4 x the worst of
      this walk and of tests/test_settings_ref.py's): gap 5.0e-10 (N = 41, OSQP mode), 7.6e-11 on state-bound rows,
      certified points 4.1e-14; lower side 0.0148 (N = 20, Ts = 0.05, a settings row), condensed objective 0.0462;
      dual bound against the IPM's optimum 4.2e-11; 6 to 11 instances per state-bound row with multipliers on state
      rows; margin LP |t*| >= 1.1e-3 (vy, N = 20), status 3 at t* <= -3.3e-2; the closed loop: gap 4.3e-15

The walk also proves, with the oracle alone, the coverage conditions the GPU tests assert: every case has a solved
instance and (from B = 4) an infeasible one; in every polish mode a case lists in `gap` the oracle polishes at least
half (and two) of the solved instances and each of those is within 1e-7 of the IPM optimum and carries a certificate;
a state-bound row has two instances whose state rows carry multipliers, and two on which ignoring the bounds shows.
No row is beyond what the float64 dual bound can prove: the certified points of every row, N = 300 and Ts = 0.05
at N = 48 / 64 included, are certified to 1e-8 (asserted), so the certificate is asserted on the GPU wherever the
IPM gap is.  The verdicts (status <= 1 / 3) are checked against a margin LP, not OSQP's certificate.

What the seeds avoid.  The seeds in the table were taken, from 17 up, where the ORACLE meets those conditions.
Rejected seeds show a property of the solver both sides share, not of any output epilogue: the condensed problem of
a long or fast-diverging horizon is so ill conditioned (the rollout's abs-sum scale reaches 1e18 at N = 200) that
ADMM's relative criteria stop it after 25 iterations, and a "polished" point can be far from the optimum.  In OSQP
mode (polish accepted by a residual comparison) from N = 48 on: N = 48, Ts = 0.02, seed 17, B = 12, instance 7: 3.3e-6
relative; N = 64, Ts = 0.05, seed 18, B = 8, instance 0: 3.1e4 x the optimal cost.  In exact mode (the 1e-9 KKT
certificate of the condensed problem) at N = 200, seed 17, B = 6, instance 5: 13 x the optimal cost.  The IPM on the
sparse form solves each of them (status 0, <= 20 iterations), and numpy's cost of numpy's rollout of its U_opt confirms
its objective.  Rows whose `gap` is (1,) assert the gap on certified points only, for that reason.
"""
import numpy as np
import pytest

from tests import _mpc_checks as M
from tests import _qp_ref as Q

QP_FILES = ["qp_N20_Ts005", "qp_N20_Ts002", "qp_N40_Ts005", "qp_N40_Ts002"]


# ------------------------------------------------------------------ _qp_ref against hand-written arithmetic

def test_cost_and_violation_by_hand():
    """N = 2 written out term by term: the k = 0 state terms, both off-diagonals of R and Rd, dU_0 against u_prev."""
    X = np.array([[1.0, 2.0, 3.0], [0.5, -1.0, 2.0], [0.1, 0.2, -0.3], [1.0, 1.5, 2.0], [0, 0, 0], [0, 0, 0]])
    U = np.array([[0.2, -0.4], [0.1, 0.3]])
    up = np.array([0.5, -0.1])
    pr = np.array([[0.9, 0.4, 0.05], [2.2, -0.8, 0.25], [2.5, 2.5, -0.2]])
    vr = np.array([1.2, 1.4, 1.6])
    kw = dict(q_c=3.0, q_phi=0.7, q_vx=1.3, R=[[2.0, 0.5], [0.5, 1.0]], Rd=[[4.0, -1.0], [-1.0, 3.0]],
              u_bounds=((-0.3, 0.25), (-0.6, 0.2)), du_bounds=((-0.5, 0.5), (-0.3, 0.15)))
    J = 0.0
    for k in range(3):
        ec = np.sin(pr[k, 2]) * (X[0, k] - pr[k, 0]) - np.cos(pr[k, 2]) * (X[1, k] - pr[k, 1])
        J += 3.0 * ec ** 2 + 0.7 * (X[2, k] - pr[k, 2]) ** 2 + 1.3 * (X[3, k] - vr[k]) ** 2
    for k in range(2):
        u = U[:, k]
        du = u - (up if k == 0 else U[:, k - 1])
        J += 2.0 * u[0] ** 2 + 2 * 0.5 * u[0] * u[1] + 1.0 * u[1] ** 2
        J += 4.0 * du[0] ** 2 - 2 * 1.0 * du[0] * du[1] + 3.0 * du[1] ** 2
    Jq, Ja = Q.cost(X, U, up, pr, vr, kw)
    assert abs(Jq - J) <= 8 * M.EPS * Ja and Ja >= abs(J)
    # a non-symmetric R is its symmetric part
    assert abs(Q.cost(X, U, up, pr, vr, dict(kw, R=[[2.0, 0.9], [0.1, 1.0]]))[0] - Jq) <= 8 * M.EPS * Ja
    box, rate, state, scale = Q.violation(U, up, kw)
    # U_0[1] = 0.3 > 0.2 (box, 0.1); U_0[0] = -0.4 < -0.3 (0.1); dU_1[0] = -0.6 < -0.5 (0.1); dU_0[1] = 0.2 > 0.15 (0.05);
    # dU_1[1] = 0.2 > 0.15
    assert box == pytest.approx(0.1, abs=1e-15) and rate == pytest.approx(0.1, abs=1e-15) and state == 0.0
    assert scale == pytest.approx(0.6, abs=1e-15)
    lo, hi = [-np.inf] * 6, [np.inf] * 6
    lo[3], hi[1] = 1.1, 1.5                                    # vx(0) = 1.0 below 1.1; Y(2) = 2.0 above 1.5
    box, rate, state, scale = Q.violation(U, up, dict(kw, x_lo=lo, x_hi=hi), X)
    assert state == pytest.approx(0.5, abs=1e-15) and scale == 3.0
    assert Q.violation(np.zeros((2, 2)), np.zeros(2), None, X)[:3] == (0.0, 0.0, 0.0)


def test_rollout_by_hand():
    rng = np.random.default_rng(0)
    Ad, Bd, g = rng.normal(size=(3, 6, 6)), rng.normal(size=(3, 6, 2)), rng.normal(size=(3, 6))
    x0, U = rng.normal(size=6), rng.normal(size=(2, 3))
    X, S = Q.rollout(x0, Ad, Bd, g, U)
    x = x0.copy()
    for k in range(3):
        x = np.array([sum(Ad[k, r, c] * x[c] for c in range(6)) + Bd[k, r, 0] * U[0, k] + Bd[k, r, 1] * U[1, k]
                      + g[k, r] for r in range(6)])
        assert np.all(np.abs(X[:, k + 1] - x) <= 16 * M.EPS * S[:, k + 1])
    assert np.array_equal(X[:, 0], x0) and np.all(S >= np.abs(X))


def test_condensed_and_dual_bound_by_hand():
    """N = 3, random model: the condensed objective is cost(rollout(U), U) at random U (non-symmetric R, Rd); the rows
    of A are U, dU (u_prev moved into the bounds) and the bounded states at k = 1..N, one-sided bounds included; the
    dual bound of ANY y >= 0 lies below J at every feasible point (weak duality), an infinite side takes no
    multiplier, and a one-variable QP has the dual worked out by hand."""
    rng = np.random.default_rng(1)
    N = 3
    Ad, Bd, g = rng.normal(size=(N, 6, 6)) * 0.5, rng.normal(size=(N, 6, 2)), rng.normal(size=(N, 6)) * 0.1
    x0, up = rng.normal(size=6), np.array([0.1, -0.05])
    pr, vr = rng.normal(size=(N + 1, 3)), rng.normal(size=N + 1)
    lo, hi = [-np.inf] * 6, [np.inf] * 6
    lo[3], hi[3], hi[2] = -50.0, 60.0, 70.0                    # vx two-sided, heading above only
    kw = dict(q_c=3.0, q_phi=0.7, q_vx=1.3, R=[[2.0, 0.9], [0.1, 1.0]], Rd=[[4.0, -1.5], [-0.5, 3.0]],
              u_bounds=((-0.3, 0.25), (-0.6, 0.2)), du_bounds=((-0.5, 0.5), (-0.3, 0.15)), x_lo=lo, x_hi=hi)
    P, q, c0, A, lo_r, hi_r, ns = Q.condensed(x0, Ad, Bd, g, up, pr, vr, kw)
    assert ns == 2 * N and A.shape == (4 * N + ns, 2 * N) and np.allclose(P, P.T) and np.linalg.eigvalsh(P).min() > 0
    feas = []
    for _ in range(200):
        U = rng.uniform(-0.3, 0.2, size=(2, N))
        u = Q.stage_major(U)
        assert np.array_equal(u, [U[0, 0], U[1, 0], U[0, 1], U[1, 1], U[0, 2], U[1, 2]])
        X, _ = Q.rollout(x0, Ad, Bd, g, U)
        J, Ja = Q.cost(X, U, up, pr, vr, kw)
        assert abs(Q.objective(P, q, c0, u) - J) <= 1e-13 * Ja
        r = A @ u
        assert np.array_equal(r[:2 * N], u)
        dU = U - np.concatenate([up[:, None], U[:, :-1]], axis=1)
        # rate rows: D u within [lo, hi] exactly when dU is within du_bounds
        assert np.allclose(r[2 * N:4 * N] - lo_r[2 * N:4 * N], Q.stage_major(dU) - np.tile([-0.5, -0.3], N), atol=1e-14)
        assert np.allclose(hi_r[2 * N:4 * N] - r[2 * N:4 * N], np.tile([0.5, 0.15], N) - Q.stage_major(dU), atol=1e-14)
        # state rows: heading (upper side only) then vx, k = 1..N
        assert np.allclose(hi_r[4 * N:] - r[4 * N:], np.concatenate([70.0 - X[2, 1:], 60.0 - X[3, 1:]]), atol=1e-12)
        assert np.all(np.isinf(lo_r[4 * N:5 * N])) and np.allclose(r[5 * N:] - lo_r[5 * N:], X[3, 1:] + 50.0, atol=1e-12)
        if np.all(r >= lo_r) and np.all(r <= hi_r):
            feas.append(J)
    assert len(feas) >= 5
    for _ in range(50):
        d = Q.dual_bound(P, q, c0, A, lo_r, hi_r, rng.exponential(size=len(lo_r)) * 3, rng.exponential(size=len(lo_r)) * 3)
        assert np.isfinite(d) and d <= min(feas)
    # min u^2 - 4 u, u <= 1: J* = -3 at u = 1, y = 2; d(y) = -(y - 4)^2 / 4 - y
    P1, q1, A1 = np.array([[2.0]]), np.array([-4.0]), np.array([[1.0]])
    for y in (0.0, 1.0, 2.0, 3.5):
        d = Q.dual_bound(P1, q1, 0.0, A1, np.array([-np.inf]), np.array([1.0]), np.array([y]), np.array([7.0]))
        assert d == pytest.approx(-(y - 4.0) ** 2 / 4.0 - y, abs=1e-15) and d <= -3.0 + 1e-15
    ce = Q.certificate(P1, q1, 0.0, A1, np.array([-np.inf]), np.array([1.0]), np.array([1.0]), 1)
    assert ce["J"] == -3.0 and ce["d"] == pytest.approx(-3.0, abs=1e-15) and ce["y_plus"][0] == pytest.approx(2.0)
    assert ce["n_state_active"] == 1
    # a feasible point that is not the optimum is not certified: u = 0.5 has no active row, d = min_u J = -4
    ce = Q.certificate(P1, q1, 0.0, A1, np.array([-np.inf]), np.array([1.0]), np.array([0.5]), 1)
    assert ce["J"] == -1.75 and ce["d"] == -4.0 and ce["n_state_active"] == 0


# ------------------------------------------------------------------ against the reference's goldens

@pytest.mark.parametrize("name", QP_FILES)
def test_qp_ref_vs_golden(name):
    """The reference's own A, B, g and the golden optimum: cost(golden X_opt, U_opt) is the golden objective within a
    quarter of the bar the kernels are held to, and the optimum is feasible to 1e-9.  rollout(golden U_opt) is the
    golden X_opt to 1e-11 (1 + S): the golden X_opt is itself a solver's output (sparse-form IPM + exact KKT solve),
    whose equality rows hold to the fixture's recorded KKT residual (`stationarity`, <= 1.4e-12), not to rounding --
    zero rows of S carry 1e-13 there -- so it pins the recurrence (stage order, the g term, the B U term) at that
    residual and takes no part in sizing C_X.  This is what makes tests/_qp_ref.py a restatement of the reference and
    not of the kernels."""
    gd = np.load(f"tests/golden/{name}.npz")
    N = int(gd["N"])
    fac = (N + 8) * M.EPS
    w = M.Worst()
    assert gd["stationarity"].max() <= 1.4e-12
    for b in range(len(gd["x0"])):
        X, S = Q.rollout(gd["x0"][b], gd["Ad"][b], gd["Bd"][b], gd["g"][b], gd["U_opt"][b])
        w.add("X / 1e-11 (1 + S)", np.max(np.abs(X - gd["X_opt"][b]) / (1e-11 * (1 + S))))
        J, Ja = Q.cost(gd["X_opt"][b], gd["U_opt"][b], gd["u_prev"][b], gd["path_ref"][b], gd["vref"][b])
        w.add("J", M._ratio(abs(J - gd["objective"][b]), fac * Ja))
        box, rate, state, _ = Q.violation(gd["U_opt"][b], gd["u_prev"][b])
        w.add("viol", max(box, rate, state))
    print(f"golden {name}: worst error / bar (C = 1): {w}")
    assert w.r["X / 1e-11 (1 + S)"] <= 1.0 and 4 * w.r["J"] <= M.C_J and w.r["viol"] <= 1e-9


# ------------------------------------------------------------------ the GPU tests' case table, oracle as the kernel

@pytest.mark.parametrize("case", M.table(), ids=lambda c: c.id)
def test_case_table_with_oracle(oracle_lib, case):
    """Every check of tests/test_mpc_outputs.py on the oracle's outputs, with the bars at a quarter (4 x worst <= C),
    and the coverage conditions with the oracle alone."""
    O = oracle_lib
    kw = M.SETTINGS[case.settings][0]
    assert O.cfg().eps_abs == M.EPS_ABS and O.cfg().eps_rel == M.EPS_REL
    with O.tire_sine(1):
        lin = M.lin_of(O, case)
        for mode in (0, 1):
            o = M.oracle_step(O, case, mode)
            # (the oracle leaves X_opt / U_opt of an unsolved instance untouched: no NaN contract here)
            w = M.check_outputs(o, case, lin, c_x=M.C_X / 4, c_j=M.C_J / 4, nan_contract=False)
            if case.B >= 4:
                assert o["status"][1] == 3
            sb = M.state_bounded(kw)
            gap, cert = None, ""
            if mode in case.gap and not sb:
                gap = M.check_gap(O, o, case, lin)
            if mode in case.gap or sb:
                # the certificate at a quarter of its constants, with its coverage; certified (exact-mode) points to 1e-8:
                # no row is beyond what the float64 bound can prove
                cg, wc, n_state, bound = M.check_certificate(o, case, lin, c_d=M.C_D / 4, c_jc=M.C_JC / 4)
                assert mode == 0 or cg <= 1e-8, (case.id, "float64 limit of the dual bound", cg)
                w.merge(wc)
                cert = f", certificate gap {cg:.2e}, state rows with a multiplier on {n_state}"
                if not sb:      # the new reference tied to the one pinned to the goldens
                    x0, up, pr, vr = M.inputs_of(case)
                    c = O.cfg(N=case.N, Ts=case.Ts, ipm_tol=1e-12, ipm_max_iter=100, **kw)
                    tie = max(abs(d - J) / abs(J) for b, d in bound.items() for J in
                              [O.qp_ipm(x0[b], up[b], pr[b], vr[b], lin[0][b], lin[1][b], lin[2][b], c)["objective"]])
                    assert tie <= M.GAP_TOL, (case.id, mode, "dual bound vs the IPM's optimum", tie)
                    cert += f", |d - J*_ipm| / |J*| {tie:.2e}"
            ok = o["status"] <= 1
            print(f"oracle {case.id} mode {mode}: solved {ok.sum()}/{case.B}, polished {(ok & (o['polished'] > 0)).sum()}, "
                  f"worst error / bar (C = 1): {w}" + ("" if gap is None else f", worst gap {gap:.2e}") + cert)


SB_CASES = [c for c in M.table() if M.state_bounded(M.SETTINGS[c.settings][0])]


@pytest.mark.parametrize("case", SB_CASES, ids=lambda c: c.id)
def test_state_rows_have_teeth(oracle_lib, case):
    """What a solver that ignored the state rows would return: on at least two instances of every state-bound row the
    optimum of the same instance WITHOUT the bounds breaks a state row by more than 1e-3 while the bounded optimum
    costs more than the unbounded one by more than 1e-5 relative -- 100 x the bar the certificate holds the GPU to."""
    O = oracle_lib
    kw = M.SETTINGS[case.settings][0]
    x0, up, pr, vr = M.inputs_of(case)
    with O.tire_sine(1):
        lin = M.lin_of(O, case)
        for mode in (0, 1):
            o, f = M.oracle_step(O, case, mode), M.oracle_step(O, case._replace(settings="default"), mode)
            both = (o["status"] <= 1) & (o["polished"] > 0) & (f["status"] <= 1) & (f["polished"] > 0)
            hits = []
            for b in np.where(both)[0]:
                Xf, _ = Q.rollout(x0[b], lin[0][b], lin[1][b], lin[2][b], f["U_opt"][b])
                Xb, _ = Q.rollout(x0[b], lin[0][b], lin[1][b], lin[2][b], o["U_opt"][b])
                broken = Q.violation(f["U_opt"][b], up[b], kw, Xf)[2]
                Jf, Jb = (Q.cost(X, r["U_opt"][b], up[b], pr[b], vr[b], kw)[0] for X, r in ((Xf, f), (Xb, o)))
                if broken > 1e-3 and Jb - Jf > 1e-5 * abs(Jf):
                    hits.append((broken, (Jb - Jf) / abs(Jf)))
            assert len(hits) >= 2, (case.id, mode, hits)
            print(f"oracle {case.id} mode {mode}: the unbounded optimum breaks a state row on {len(hits)} instances (by "
                  f"{min(h[0] for h in hits):.2e} .. {max(h[0] for h in hits):.2e}), the bounds cost "
                  f"{min(h[1] for h in hits):.2e} .. {max(h[1] for h in hits):.2e} relative")


def _lp_margin(qp, x0, kw):
    """max t with lo + t <= A u <= hi - t over the rows of the condensed QP, and x_lo + t <= x0 <= x_hi - t for the
    constant k = 0 state rows: t* > 0 iff the QP has a strictly feasible point."""
    from scipy.optimize import linprog
    _, _, _, A, lo, hi, _ = qp
    n = A.shape[1]
    fh, fl = np.isfinite(hi), np.isfinite(lo)
    Aub = np.block([[A[fh], np.ones((fh.sum(), 1))], [-A[fl], np.ones((fl.sum(), 1))]])
    bub = np.concatenate([hi[fh], -lo[fl]])
    xl = np.asarray(kw.get("x_lo") if kw.get("x_lo") is not None else [-np.inf] * 6, dtype=np.float64)
    xh = np.asarray(kw.get("x_hi") if kw.get("x_hi") is not None else [np.inf] * 6, dtype=np.float64)
    cap = min(10.0, float(np.min(x0 - xl)), float(np.min(xh - x0)))
    cost = np.zeros(n + 1)
    cost[n] = -1.0
    r = linprog(cost, A_ub=Aub, b_ub=bub, bounds=[(None, None)] * n + [(-1e3, cap)], method="highs")
    assert r.status == 0, r.message
    return float(r.x[n])


@pytest.mark.parametrize("case", M.table(), ids=lambda c: c.id)
def test_statuses_vs_margin_lp(oracle_lib, case):
    """The oracle's feasibility verdicts -- which the GPU tests demand of the kernels instance by instance -- against
    something that is not OSQP's certificate: the margin LP (scipy's HiGHS, used here only).  status <= 1 needs
    t* > 0, status 3 needs t* < 0, in both polish modes; no instance may be borderline (|t*| < 1e-6)."""
    O = oracle_lib
    kw = M.SETTINGS[case.settings][0]
    x0 = M.inputs_of(case)[0]
    with O.tire_sine(1):
        lin = M.lin_of(O, case)
        st = [M.oracle_step(O, case, mode)["status"] for mode in (0, 1)]
    t = np.array([_lp_margin(M.qp_of(case, lin, b), x0[b], kw) for b in range(case.B)])
    assert (np.abs(t) >= 1e-6).all(), (case.id, "borderline", t)
    for s in st:
        assert (t[s <= 1] > 0).all() and (t[s == 3] < 0).all(), (case.id, s, t)
        assert np.isin(s, (0, 1, 2, 3)).all(), s
    s = st[0]
    print(f"oracle {case.id}: LP margin t* >= {t[s <= 1].min():.2e} where status <= 1 ({(s <= 1).sum()})"
          + (f", <= {t[s == 3].max():.2e} where status 3 ({(s == 3).sum()})" if (s == 3).any() else "")
          + (f", status 2 on {(s == 2).sum()} (t* {t[s == 2].min():.2e} ..)" if (s == 2).any() else ""))


def test_closed_loop_vcap_with_oracle(oracle_lib):
    """The closed loop tests/test_mpc_outputs.py certifies (tests/_mpc_checks.py VCAP_LOOP), with the oracle's closed
    loop and step standing where the GPU's will: the coverage summed over the steps and the certificate at a quarter
    of its constants, in both polish modes."""
    from trajectory_generation_amd.batch import spline_natural
    from trajectory_generation_amd.workload import make_workload
    O, L = oracle_lib, M.VCAP_LOOP
    N, Ts = L["N"], L["Ts"]
    w = make_workload(L["B"], N, Ts, kind="spline", seed=L["seed"])
    paths = [O.Path(2, (0, 0, 0, 0), xk=kn[0], coef=spline_natural(kn[0], kn[1]).reshape(-1)) if k == 2
             else O.Path(int(k), c) for k, c, kn in zip(w["kinds"], w["pcs"], w["knots"])]
    vr = np.tile(w["vref"], (L["B"], 1))
    with O.tire_sine(1):
        for mode in (0, 1):
            c = O.cfg(N=N, Ts=Ts, warm_start=0, polish_mode=mode, **M.VCAP)
            r = O.closed_loop_batch(paths, w["x0"], w["u0"], w["vref"], L["T"], c)
            g, wc, n_ok, n_pol, n_state = M.certify_visited(
                O, lambda x, u, pr, v: O.mpc_step_batch(x, u, pr, v, c), r["X"], r["U"], np.asarray(w["u0"]).reshape(-1, 2),
                lambda xs: np.stack([O.ref_window(p, x, N, Ts, w["vref"]) for p, x in zip(paths, xs)]), vr, mode,
                c_d=M.C_D / 4, c_jc=M.C_JC / 4)
            print(f"oracle closed loop vcap mode {mode}: solved {n_ok}/{L['B'] * L['T']}, polished {n_pol}, state rows "
                  f"with a multiplier on {n_state}, max vx {r['X'][:, :, 3].max():.3f}, certificate gap {g:.2e}, worst error / bar "
                  f"(C = 1): {wc}")

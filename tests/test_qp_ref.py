"""tests/_qp_ref.py (the QP of one MPC step in plain numpy) pinned to the reference's goldens, and the GPU output
tests' case table (tests/_mpc_checks.py) walked on the CPU with the oracle standing where the kernel will.

This is where the two constants of tests/_mpc_checks.py are measured: every check prints its worst error-over-bar
ratio (bar with C = 1; run with -s) and asserts 4 x ratio <= C_X / C_J.  Measured here (float64, x86-64):

  goldens (qp_N20/N40 x Ts 0.02/0.05, the reference's own A, B, g and an IPM + exact KKT optimum):
      objective 0.036, violation <= 7.5e-13, X 0.107 of 1e-11 (1 + S) (a solver's output: see test_qp_ref_vs_golden)
  oracle over the case table, both polish modes: X 0.108 (N = 1), objective 0.0847,
      violation 0.94 of the eps bar (unpolished), 3.1e-4 of 1e-9 (polished); worst asserted optimality gap 5.0e-10

The walk also proves, with the oracle alone, the coverage conditions the GPU tests assert: every case has a solved
instance and (from B = 4) an infeasible one; in every polish mode a case lists in `gap` the oracle polishes at least
half (and two) of the solved instances and each of those is within 1e-7 of the IPM optimum.

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
            gap = None
            if mode in case.gap and "x_lo" not in kw:
                gap = M.check_gap(O, o, case, lin)
            ok = o["status"] <= 1
            print(f"oracle {case.id} mode {mode}: solved {ok.sum()}/{case.B}, polished {(ok & (o['polished'] > 0)).sum()}, "
                  f"worst error / bar (C = 1): {w}" + ("" if gap is None else f", worst gap {gap:.2e}"))

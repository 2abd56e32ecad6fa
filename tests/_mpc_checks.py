"""Case table and output checks shared by tests/test_qp_ref.py (CPU: the oracle stands where the kernel will) and
tests/test_mpc_outputs.py (GPU: every solver tier of mpc_step) -- TEST INFRASTRUCTURE ONLY.

The checks hold a solver's outputs to the QP itself (tests/_qp_ref.py), not to another solver:
  * X_opt against the numpy rollout of the solver's own U_opt, elementwise, bar C_X (N + 8) 2^-52 S with S the
    rollout's abs-sum scale;
  * objective against the numpy cost of the solver's own (X_opt, U_opt), bar C_J (N + 8) 2^-52 scale;
  * u_cmd = U_opt[:, 0] and X_opt[:, 0] = x0 bitwise;
  * the inequality rows: 1e-9 where polished, else eps_abs + eps_rel max||[U; dU]||_inf -- OSQP's unscaled primal
    criterion: the returned point is x, whose distance to the box is at most ||Ax - z||_inf;
  * status > 1: X_opt, U_opt, objective NaN and u_cmd = u_prev (mpc_6stati.py:257-262);
  * polished points without state rows: |cost(U) - J*| <= 1e-7 |J*| with J* from the oracle's sparse-form Riccati
    IPM (a different algorithm, pinned to the reference goldens by test_sparse_structured_ipm_vs_golden); 1e-7 is
    the project's objective bar (tests/test_oracle_golden.py);
  * polished points, state rows or not: the weak-duality certificate (certify_point) -- a dual bound d <= J* from
    multipliers fitted to the point's own active rows, J - d <= 1e-7 |J|, in numpy alone.  This is what holds the
    general solver's state-bound solves and the bounded closed loop's steps to the optimum, which the IPM (it has
    no state rows) cannot; on the other tiers it stands beside the IPM, whose code is the project's.

C_X and C_J are 4x the worst error-over-bar ratio that tests/test_qp_ref.py measures on the CPU for the oracle over
this case table (that test asserts 4 x worst <= C; the goldens' objective is held to the same quarter bar): the margin
is for a GPU epilogue summing in another order and contracting to fma.  Measured worst ratios: X 0.108 (oracle, N = 1),
objective 0.0847 (oracle; goldens 0.036).  The golden X_opt is a solver's output, exact to its recorded KKT residual
(1.4e-12) and not to rounding, so it pins the rollout at 1e-11 (1 + S) and takes no part in C_X.  Neither constant is
taken from a kernel's numbers (the kernels measure X 0.108, objective 0.152: DESIGN.md section 2, "Output checks").
The certificate's C_D and C_JC are made by the same rule (below, beside certify_point).

The solver-settings rows (tests/_settings_cases.py) run the same checks with the row's own eps_abs / eps_rel in the
unpolished bar (10 x for status 1, OSQP's "inaccurate" criterion), their own pair of constants C_X_SET / C_J_SET made
by the same rule, and the polished 1e-9 bar, the gap and the certificate only where that table lists them; parity /
pooled hold a call to the oracle under the same settings with the bars of tests/test_gpu_parity.py.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import _qp_ref as Q
from tests._cases import random_instances

EPS = 2.0 ** -52
C_X = 0.44
C_J = 0.34
GAP_TOL = 1e-7
POLISHED_VIOL = 1e-9
EPS_ABS = EPS_REL = 1e-5        # traj_mpc_config / OSQP defaults (asserted against the config in the tests)

SB_VX = ([-np.inf, -np.inf, -np.inf, 0.38, -np.inf, -np.inf], [np.inf, np.inf, np.inf, 1.52, np.inf, np.inf])

# non-default mpc_step arguments (section C): off-diagonal R / Rd, asymmetric boxes, q_*, vehicle parameters
NONDEFAULT = dict(q_c=11.0, q_phi=0.2, q_vx=1.7, R=[[.05, .03], [.03, 1.1]], Rd=[[.04, -.1], [-.1, 3.0]],
                  u_bounds=((-.4, .9), (-.35, .5)), du_bounds=((-.3, .45), (-.2, .15)))
NONDEFAULT_PARAMS = {"m": 0.05, "Iz": 3.1e-5, "lf": 0.03}
# a non-symmetric R with NONDEFAULT's symmetric part (the header: the symmetric part is used)
NONSYM_R = [[.05, .05], [.01, 1.1]]
_INF = np.inf


def _sb(lo, hi):
    return dict(x_lo=[-_INF if v is None else v for v in lo], x_hi=[_INF if v is None else v for v in hi])


# further kinds of state bound: "wide" is tests/test_gpu_parity.py's SB (vx, vy, omega); one state each for omega and
# vy; "phi_hi" bounds one side only, of a state the cost rows also touch (the path's heading passes 0.3 where the
# window runs out to |x| > 1.5: tests/_cases.py)
SETTINGS = {"default": ({}, None),
            "vx": (dict(x_lo=SB_VX[0], x_hi=SB_VX[1]), None),
            "wide": (_sb([None, None, None, 0.35, -0.3, -3.0], [None, None, None, 1.6, 0.3, 3.0]), None),
            "omega": (_sb([None] * 5 + [-1.0], [None] * 5 + [1.0]), None),
            "vy": (_sb([None] * 4 + [-0.05, None], [None] * 4 + [0.05, None]), None),
            "phi_hi": (dict(x_hi=[_INF, _INF, 0.3, _INF, _INF, _INF]), None),
            "nondefault": (NONDEFAULT, NONDEFAULT_PARAMS),
            "nonsym": (dict(NONDEFAULT, R=NONSYM_R), NONDEFAULT_PARAMS)}


def state_bounded(kw):
    """The mpc_step arguments carry state rows (the general solver runs)."""
    return kw.get("x_lo") is not None or kw.get("x_hi") is not None


class Case(NamedTuple):
    """One row of the table.  route: how the kernel is selected ("default"; "cap80": traj_debug_split_min_n(41) on
    the step entry; "long_lds": traj_debug_split_max_n(0)).  gap: the polish modes in which the optimality gap and
    the certificate are asserted with their coverage condition (state-bound rows: the certificate in both; (1,):
    certified points only -- at Ts = 0.05 from N = 48 up and at N >= 200 OSQP mode accepts its polish too rarely, and
    what it accepts need not be the optimum: tests/test_qp_ref.py)."""
    kernel: str
    N: int
    Ts: float
    B: int
    seed: int
    route: str = "default"
    settings: str = "default"
    gap: tuple = (0, 1)
    variant: str = ""           # "hinf": instance 2 is infeasible along the horizon (inputs_of)

    @property
    def id(self):
        return (f"{self.kernel}-N{self.N}-Ts{self.Ts}" + ("" if self.settings == "default" else f"-{self.settings}"))


# seeds: from 17 up, taken where the ORACLE ALONE -- on the CPU, tests/test_qp_ref.py -- polishes at least half (and two)
# of the status <= 1 instances in every mode listed in `gap`, each of those within 1e-7 of the IPM's optimum and
# certified, (state-bound rows) has two instances whose state rows carry multipliers, two on which the unbounded
# optimum breaks a state row, and no instance the margin LP calls borderline, and (the general solver's rows) stops
# well before the iteration cap; what the rejected seeds show is in that file's docstring
QP_CASES = [
    Case("onewave", 1, 0.02, 16, 17), Case("onewave", 8, 0.02, 16, 17), Case("onewave", 20, 0.02, 16, 17),
    Case("onewave", 20, 0.05, 16, 17),
    Case("cap80", 21, 0.02, 12, 17), Case("cap80", 33, 0.02, 12, 17), Case("cap80", 33, 0.05, 12, 19),
    Case("cap80", 40, 0.02, 12, 17),
    Case("split48", 41, 0.02, 12, 17), Case("split48", 48, 0.02, 12, 19),
    Case("split48", 48, 0.05, 12, 19, gap=(1,)),
    Case("split64", 49, 0.02, 12, 19), Case("split64", 64, 0.02, 8, 17), Case("split64", 64, 0.05, 8, 22, gap=(1,)),
    Case("long_lds", 48, 0.02, 12, 19, route="long_lds"),
    Case("long", 65, 0.02, 8, 17), Case("long", 128, 0.02, 6, 17),
    Case("long512", 129, 0.02, 6, 17), Case("long512", 200, 0.02, 6, 28, gap=(1,)),
    Case("general", 300, 0.02, 3, 35, gap=(1,)),
    Case("general_sb", 20, 0.02, 16, 17, settings="vx"), Case("general_sb", 40, 0.02, 12, 17, settings="vx"),
    Case("general_sb", 65, 0.02, 8, 21, settings="vx"),
    # the other kinds of state bound (SETTINGS); "wide" at Ts = 0.05: ADMM's certificate decides 5 of the 16 instances.
    # ("omega" at N = 40, Ts = 0.02 is left out: the oracle runs to the iteration cap on an instance of seed 17)
    Case("general_sb", 20, 0.02, 16, 17, settings="wide"), Case("general_sb", 20, 0.05, 16, 17, settings="wide"),
    Case("general_sb", 20, 0.02, 16, 17, settings="omega"),
    Case("general_sb", 20, 0.02, 16, 17, settings="vy"), Case("general_sb", 40, 0.02, 12, 17, settings="vy"),
    Case("general_sb", 20, 0.02, 16, 17, settings="phi_hi"),
]
# the step entry: 21 <= N <= 40 runs the row-split kernel (H = 40) by default and the capacity-80 kernel on request
STEP_CASES = ([c._replace(kernel="split40") if c.kernel == "cap80" else c for c in QP_CASES]
              + [Case("cap80", 21, 0.02, 12, 17, route="cap80"), Case("cap80", 40, 0.02, 12, 17, route="cap80")])
NONDEFAULT_CASES = [Case("onewave", 12, 0.02, 12, 31, settings="nondefault"),
                    Case("cap80_split40", 33, 0.02, 12, 31, settings="nondefault"),
                    Case("split48", 48, 0.02, 12, 31, settings="nondefault"),
                    Case("long", 80, 0.02, 8, 31, settings="nondefault")]


def table():
    """Every distinct set of inputs the GPU tests run (the CPU survey walks them with the oracle)."""
    seen, out = set(), []
    for c in QP_CASES + STEP_CASES + NONDEFAULT_CASES:
        key = (c.N, c.Ts, c.B, c.seed, c.settings)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def inputs(N, Ts, B, seed):
    """random_instances with, from B = 4 up, one infeasible row (u_prev[0] = 3.0: the rate chain cannot reach the box,
    mpc_6stati.py:197-205) so that the NaN / fallback branch of each epilogue runs.  Shared: never written to."""
    x0, up, pr, vr = random_instances(seed, B, N, Ts)
    if B >= 4:
        up[1, 0] = 3.0
    return x0, up, pr, vr


def inputs_of(case):
    """The case's inputs.  variant "hinf" (a case with a lower vx bound): instance 2 starts just inside the bound
    under full braking, which the rate limit keeps at -0.5 or below for the first step, so that the bound's k = 1 row
    cannot be met -- infeasible along the horizon, found by ADMM's certificate and not up front.  Never written to."""
    if case.variant == "":
        return inputs(case.N, case.Ts, case.B, case.seed)
    assert case.variant == "hinf"
    return _inputs_hinf(case.N, case.Ts, case.B, case.seed, float(SETTINGS[case.settings][0]["x_lo"][3]))


@functools.lru_cache(maxsize=None)
def _inputs_hinf(N, Ts, B, seed, vx_lo):
    x0, up, pr, vr = (a.copy() for a in inputs(N, Ts, B, seed))
    x0[2, 3] = vx_lo + 1e-4
    up[2, 0] = -1.0
    return x0, up, pr, vr


_LIN = {}


def lin_of(O, case):
    """The oracle's linearization of the case's inputs (computed once per input set)."""
    key = (case.N, case.Ts, case.B, case.seed, case.settings in ("nondefault", "nonsym"), case.variant)
    if key not in _LIN:
        x0, up, _, _ = inputs_of(case)
        _LIN[key] = Q.linearization(O, x0, up, case.N, case.Ts, SETTINGS[case.settings][1])
    return _LIN[key]


_ORC = {}


def oracle_step(O, case, mode, row=None):
    """The oracle's mpc_step_batch on the case's inputs (computed once per input set, mode and solver-settings row
    -- (name, keyword arguments) of tests/_settings_cases.py; the caller holds O.tire_sine(1) where it compares with
    the GPU)."""
    key = (case.N, case.Ts, case.B, case.seed, case.settings, case.variant, mode, row[0] if row else None)
    if key not in _ORC:
        kw, par = SETTINGS[case.settings]
        _ORC[key] = O.mpc_step_batch(*inputs_of(case), O.cfg(N=case.N, Ts=case.Ts, polish_mode=mode, **kw,
                                                             **(row[1] if row else {})), O.params(par) if par else None)
    return _ORC[key]


class Worst:
    """The worst error-over-bar ratio seen per check (bar with C = 1), for the printed survey."""

    def __init__(self):
        self.r = {}

    def add(self, name, v):
        self.r[name] = max(self.r.get(name, 0.0), float(v))

    def merge(self, other):
        for k, v in other.r.items():
            self.add(k, v)

    def __str__(self):
        return ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.r.items()))


def _ratio(err, bar):
    """max err / bar, elementwise; 0 / 0 (an exact value with a zero scale) counts as 0."""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(np.max(r))


def check_outputs(o, case, lin=None, c_x=C_X, c_j=C_J, nan_contract=True, solver=None, polished_bar=True):
    """Every consistency, feasibility and contract check on the outputs `o` (numpy arrays) of one call, on EVERY
    instance.  lin = (Ad, Bd, g): the linearization the solver was given (QP entry point) -- without it X_opt is
    only used as the cost's argument.  solver: the solver settings the call ran with (a row of
    tests/_settings_cases.py; its eps_abs / eps_rel make the unpolished bar, the defaults where it has none).
    polished_bar: hold polished points to 1e-9 (False: to the unpolished bar -- the rows where the oracle's own
    polish does not reach 1e-9).  Returns the Worst ratios (C = 1); asserts with c_x / c_j."""
    x0, up, pr, vr = inputs_of(case)
    eps_abs, eps_rel = (solver or {}).get("eps_abs", EPS_ABS), (solver or {}).get("eps_rel", EPS_REL)
    kw = SETTINGS[case.settings][0]
    N, w = case.N, Worst()
    fac = (N + 8) * EPS
    st = o["status"]
    assert (st <= 1).any(), "no instance solved"
    for b in range(case.B):
        tag = f"{case.id} b={b}"
        if st[b] > 1:
            assert np.array_equal(o["u_cmd"][b], up[b]), tag
            if nan_contract:
                assert np.isnan(o["objective"][b]) and np.isnan(o["X_opt"][b]).all() and np.isnan(o["U_opt"][b]).all(), tag
            continue
        X, U = o["X_opt"][b], o["U_opt"][b]
        assert np.isfinite(X).all() and np.isfinite(U).all() and np.isfinite(o["objective"][b]), tag
        assert np.array_equal(o["u_cmd"][b], U[:, 0]), tag
        assert np.array_equal(X[:, 0], x0[b]), tag
        if lin is not None:
            Xr, S = Q.rollout(x0[b], lin[0][b], lin[1][b], lin[2][b], U)
            rx = _ratio(np.abs(X - Xr), fac * S)
            w.add("X", rx)
            assert rx <= c_x, (tag, "X_opt vs rollout(U_opt)", rx, c_x,
                               np.unravel_index(np.argmax(np.abs(X - Xr) / (S + 1e-300)), X.shape))
        J, Ja = Q.cost(X, U, up[b], pr[b], vr[b], kw)
        rj = _ratio(abs(o["objective"][b] - J), fac * Ja)
        w.add("J", rj)
        assert rj <= c_j, (tag, "objective vs cost(X_opt, U_opt)", rj, c_j, o["objective"][b], J)
        box, rate, state, scale = Q.violation(U, up[b], kw, X)
        # OSQP's criterion at eps (status 0) or at 10 eps (status 1, "optimal_inaccurate")
        bar_admm = (eps_abs + eps_rel * scale) * (10.0 if st[b] == 1 else 1.0)
        bar = POLISHED_VIOL if o["polished"][b] > 0 and polished_bar else bar_admm
        w.add("viol_polished" if o["polished"][b] > 0 and polished_bar else "viol_admm", max(box, rate, state) / bar)
        assert max(box, rate, state) <= bar, (tag, "violation", box, rate, state, bar, int(o["polished"][b]))
    return w


BOTH_POL_TOL = 1e-6             # tests/test_gpu_parity.py _agreement: max |dU_opt| where both sides polished


def agreement_floor(N, mode):
    """The fraction of instances on which iteration counts and polish outcomes must agree, pooled over a case's rows:
    tests/test_gpu_parity.py _agreement's (0.98 in OSQP mode, 0.95 in exact mode) and, past N = 64, the long-horizon
    tests' (test_long_horizon_vs_oracle 0.95, test_long_horizon_exact_mode_and_qp_batch_vs_oracle 0.9)."""
    if N > 64:
        return 0.95 if mode == 0 else 0.9
    return 0.98 if mode == 0 else 0.95


def parity(got, want, row, up=None, polish_subset=False):
    """One solver-settings row of one case: `got` against `want` (the oracle with the row's settings).  Statuses
    identical on every instance; iteration counts equal, and polish outcomes equal, each on more than half of the
    status <= 1 instances; max |dU_opt| <= 1e-6 where both polished.  up (the GPU side): an unsolved instance has
    u_cmd = u_prev and NaN outputs.  polish_subset: the documented departure of tests/_settings_cases.py
    UNREFINED -- in place of equal polish outcomes, `got` polishes only where `want` does, and the outcome takes
    no part in the pooled bar.  Returns (solved, iters equal, polish equal) for the pooled bar (pooled)."""
    assert np.array_equal(got["status"], want["status"]), (row, "status", got["status"], want["status"])
    ok = want["status"] <= 1
    n = int(ok.sum())
    pg, pw = got["polished"] > 0, want["polished"] > 0
    ie, pe = int((got["iters"] == want["iters"])[ok].sum()), int((pg == pw)[ok].sum())
    assert 2 * ie > n, (row, "iters", ie, n, got["iters"], want["iters"])
    if polish_subset:
        assert not (pg & ~pw)[ok].any(), (row, "polished where the oracle is not", pg, pw)
        pe = n
    assert 2 * pe > n, (row, "polished", pe, n, pg, pw)
    both = ok & pg & pw
    du = np.abs(got["U_opt"][both] - want["U_opt"][both]).max(axis=(1, 2)) if both.any() else np.zeros(0)
    assert du.max(initial=0.0) <= BOTH_POL_TOL, (row, "U_opt where both polished", du)
    if up is not None:
        bad = ~ok
        assert np.array_equal(got["u_cmd"][bad], up[bad]), (row, "fallback")
        assert (np.isnan(got["objective"][bad]).all() and np.isnan(got["X_opt"][bad]).all()
                and np.isnan(got["U_opt"][bad]).all()), (row, "NaN contract")
    return n, ie, pe


def pooled(stats, N, mode, tag):
    """The pooled bar over all rows of one (case, mode): stats = parity's returns."""
    n, ie, pe = (sum(s[i] for s in stats) for i in range(3))
    floor = agreement_floor(N, mode)
    assert n > 0 and ie >= floor * n and pe >= floor * n, (tag, "pooled agreement", ie, pe, n, floor)
    return ie / n, pe / n


def check_gap(O, o, case, lin, require=True):
    """Polished points against the optimum: |cost(rollout(U_opt), U_opt) - J*| <= 1e-7 |J*|, J* from O.qp_ipm on the
    same A, B, g (status 0 required).  require: the coverage condition -- polished on at least half of the status <= 1
    instances and on at least two.  Returns the worst relative gap."""
    x0, up, pr, vr = inputs_of(case)
    kw = SETTINGS[case.settings][0]
    assert not state_bounded(kw), "the IPM has no state rows: check_certificate"
    ok = o["status"] <= 1
    pol = ok & (o["polished"] > 0)
    if require:
        assert pol.sum() >= 2 and 2 * pol.sum() >= ok.sum(), (case.id, "coverage", int(pol.sum()), int(ok.sum()))
    c = O.cfg(N=case.N, Ts=case.Ts, ipm_tol=1e-12, ipm_max_iter=100, **kw)
    worst = 0.0
    for b in np.where(pol)[0]:
        r = O.qp_ipm(x0[b], up[b], pr[b], vr[b], lin[0][b], lin[1][b], lin[2][b], c)
        assert r["status"] == 0, (case.id, b, "IPM status", r["status"])
        X, _ = Q.rollout(x0[b], lin[0][b], lin[1][b], lin[2][b], o["U_opt"][b])
        J, _ = Q.cost(X, o["U_opt"][b], up[b], pr[b], vr[b], kw)
        gap = abs(J - r["objective"]) / abs(r["objective"])
        worst = max(worst, gap)
        assert gap <= GAP_TOL, (case.id, b, "optimality gap", gap, J, r["objective"])
    return worst


# ---- the weak-duality certificate: optimality with no solver on the other side

# 4 x the oracle's worst ratio over tests/test_qp_ref.py's and tests/test_settings_ref.py's CPU surveys (both assert
# 4 x worst <= C): (b) 0.0148 (N = 20, Ts = 0.05, the "combined" settings row), (c) 0.0462 (N = 8).  Never a kernel's.
C_D = 0.06
C_JC = 0.19


def certify_point(qp, U, J, Ja, N, tag, c_d=C_D, c_jc=C_JC):
    """One point U [2,N] against qp = Q.condensed(...) of its instance; J, Ja = Q.cost(Q.rollout(U), U).  Asserts
      (a) Jc - d <= GAP_TOL |Jc|: Jc the condensed objective at U, d the dual bound of Q.certificate's multipliers --
          d <= J* <= Jc, so the point is proved optimal to the bar;
      (b) Jc - d >= -(|y|_1 viol + c_d (2N + 8) 2^-52 (Ja + Da)): weak duality read the other way -- at a point that
          breaks its rows by at most viol, L(u, y) >= Jc - |y|_1 viol, and rounding does the rest (a d above that
          means the bound itself was formed wrongly).  Da is the dual expression's own abs-sum scale
          (Q.dual_bound): with Ja alone the oracle's own points reach 35 x the C = 1 bar at N = 65 -- d solves with
          the condensed Hessian, and the cost's scale at the point does not follow what that rounds;
      (c) |Jc - J| <= c_jc (2N + 8) 2^-52 (Ja + Jca): the condensed form is the QP that `cost` and `rollout` state.
          Jca is the condensed expression's own abs-sum scale, 1/2 |u|' |P| |u| + |q|' |u| + |c0|: it is evaluated
          about U = 0, where c0, q' u and u' P u cancel down to J (Jca / Ja reaches 350 at N = 49), so Ja alone is
          not the size of what it rounds (against C_J (N + 8) 2^-52 Ja the oracle's own points measure 2.3).
    Returns (relative gap, ratio of (b) with c_d = 1, ratio of (c) with c_jc = 1, state rows with a positive multiplier,
    d)."""
    P, q, c0, A, lo, hi, ns = qp
    u = Q.stage_major(U)
    ce = Q.certificate(P, q, c0, A, lo, hi, u, ns)
    r = A @ u
    viol = float(max(np.max(lo - r), np.max(r - hi), 0.0))
    y1 = float(ce["y_plus"].sum() + ce["y_minus"].sum())
    au = np.abs(u)
    Jca = float(0.5 * au @ np.abs(P) @ au + np.abs(q) @ au + abs(c0))
    fac = (2 * N + 8) * EPS
    gap = ce["J"] - ce["d"]
    rel = gap / abs(ce["J"])
    rd = max(0.0, -gap - y1 * viol) / (fac * (Ja + ce["d_scale"]))
    rjc = abs(ce["J"] - J) / (fac * (Ja + Jca))
    assert rel <= GAP_TOL, (tag, "certificate gap", rel, ce["J"], ce["d"])
    assert rd <= c_d, (tag, "dual bound above the objective", rd, c_d, gap, y1, viol)
    assert rjc <= c_jc, (tag, "condensed objective vs cost(rollout(U), U)", rjc, c_jc, ce["J"], J)
    return rel, rd, rjc, ce["n_state_active"], ce["d"]


_QP = {}


def qp_of(case, lin, b):
    """Q.condensed of instance b of the case on the oracle's linearization (computed once: lin is lin_of's)."""
    key = (case.N, case.Ts, case.B, case.seed, case.settings, case.variant, b)
    if key not in _QP:
        x0, up, pr, vr = inputs_of(case)
        _QP[key] = Q.condensed(x0[b], lin[0][b], lin[1][b], lin[2][b], up[b], pr[b], vr[b], SETTINGS[case.settings][0])
    return _QP[key]


def certify_outputs(o, inputs, lin, kw, N, tag, c_d=C_D, c_jc=C_JC, qp=None):
    """Every instance of one call's outputs `o` with status <= 1 and polished > 0 through certify_point, state rows
    or not.  inputs = (x0, u_prev, path_ref, vref) of the call, lin its linearization, kw its mpc_step arguments;
    qp(b): the condensed QP of instance b where the caller keeps it.  Returns (worst relative gap, Worst ratios of
    (b) and (c), number of instances with a state row carrying a positive multiplier, {b: dual bound})."""
    x0, up, pr, vr = inputs
    pol = (o["status"] <= 1) & (o["polished"] > 0)
    w, worst, n_state, bound = Worst(), -np.inf, 0, {}
    for b in np.where(pol)[0]:
        X, _ = Q.rollout(x0[b], lin[0][b], lin[1][b], lin[2][b], o["U_opt"][b])
        J, Ja = Q.cost(X, o["U_opt"][b], up[b], pr[b], vr[b], kw)
        cond = qp(b) if qp else Q.condensed(x0[b], lin[0][b], lin[1][b], lin[2][b], up[b], pr[b], vr[b], kw)
        rel, rd, rjc, ns, bound[b] = certify_point(cond, o["U_opt"][b], J, Ja, N, f"{tag} b={b}", c_d, c_jc)
        worst = max(worst, rel)
        w.add("D", rd)
        w.add("Jc", rjc)
        n_state += ns > 0
    return worst, w, n_state, bound


def check_certificate(o, case, lin, require=True, c_d=C_D, c_jc=C_JC, min_state=2):
    """certify_outputs on a case of the table.  require: the coverage condition -- check_gap's (polished on at least
    half of the status <= 1 instances and on two) and, with state bounds, at least min_state = two instances with a
    state row carrying a positive multiplier: the certificate then rests on the state rows' signs and on the active
    set the solver chose (min_state = 0: the settings rows tests/_settings_cases.py NO_STATE_ROWS lists, where the
    oracle's own polished points have none).  Returns certify_outputs' tuple."""
    kw = SETTINGS[case.settings][0]
    ok = o["status"] <= 1
    pol = ok & (o["polished"] > 0)
    worst, w, n_state, bound = certify_outputs(o, inputs_of(case), lin, kw, case.N, case.id, c_d, c_jc,
                                               qp=lambda b: qp_of(case, lin, b))
    if require:
        assert pol.sum() >= 2 and 2 * pol.sum() >= ok.sum(), (case.id, "coverage", int(pol.sum()), int(ok.sum()))
        assert not state_bounded(kw) or n_state >= min_state, (case.id, "coverage: state rows with a multiplier", n_state)
    return worst, w, n_state, bound


# the closed loop under a speed cap (tests/test_gpu_parity.py SBC "vcap", its workload: spline paths, seed 5): the
# states the loop itself drives against the cap
VCAP = dict(x_lo=[-np.inf, -np.inf, -np.inf, 0.2, -np.inf, -np.inf], x_hi=[np.inf, np.inf, np.inf, 1.3, np.inf, np.inf])
VCAP_LOOP = dict(N=20, Ts=0.05, B=8, T=8, seed=5)


def certify_visited(O, step, X, U, u0, window, vr, polish_mode, c_d=C_D, c_jc=C_JC):
    """The VCAP_LOOP closed loop's visited states X [B,T+1,6] with applied commands U [B,T,2]: at every step t the
    step entry `step(x, u_prev, path_ref, vref) -> outputs` on the state the loop stood in, its window from
    `window(x positions) -> [B,N+1,3]`; the polished outputs certified on the oracle's linearization at that state.
    Coverage, summed over the steps: polished on at least half of the solved (step, instance) pairs and on two; two with a state row carrying a
    multiplier.  Returns (worst gap, Worst, solved, polished, with state rows)."""
    N, Ts, T = VCAP_LOOP["N"], VCAP_LOOP["Ts"], VCAP_LOOP["T"]
    w, worst, n_ok, n_pol, n_state = Worst(), -np.inf, 0, 0, 0
    for t in range(T):
        xt, ut = X[:, t], (U[:, t - 1] if t > 0 else u0)
        prt = window(xt[:, 0])
        o = step(xt, ut, prt, vr)
        lin = Q.linearization(O, xt, ut, N, Ts)
        g, wc, ns, _ = certify_outputs(o, (xt, ut, prt, vr), lin, VCAP, N, f"vcap mode {polish_mode} t={t}", c_d, c_jc)
        worst = max(worst, g)
        w.merge(wc)
        n_ok += int((o["status"] <= 1).sum())
        n_pol += int(((o["status"] <= 1) & (o["polished"] > 0)).sum())
        n_state += ns
    assert n_pol >= 2 and 2 * n_pol >= n_ok and n_state >= 2, ("vcap coverage", polish_mode, n_ok, n_pol, n_state)
    return worst, w, n_ok, n_pol, n_state

"""The solver-settings table: every OSQP setting of traj_mpc_config off its default, per kernel text -- TEST
INFRASTRUCTURE ONLY.  tests/test_settings_ref.py proves the table on the CPU with the oracle standing where the
kernel will (its docstring holds the survey); tests/test_mpc_settings_gpu.py runs it on the kernels.

A row is a name and the config_struct / O.cfg keyword arguments it adds.  Every setting but warm_start is off its
default in one single-purpose row (with the companion it needs to show: adaptive_rho = 0 beside a rho) and in a
combined row.  The two flags, polish and adaptive_rho, are on in "combined" -- off, they void the settings they gate
-- and off in "combined_off"; OSQP takes 0 or 1 for either, so no other value is used.  eps_abs and eps_rel differ
wherever one of them moves, so that a kernel reading one for the other shows.  No value is one OSQP would refuse.

A case is one of tests/_mpc_checks.py's Case rows with the entry point it runs through and the kernel text it
selects ("solve": mpc_solve.h, "split": mpc_split.h, "long": mpc_long.h, "general": mpc_general.h), at the smallest
horizons that still select it.  TABLE lists, per (case, row), the polish modes the GPU test runs: those in which
the oracle with the row's settings departs from the oracle at defaults by more than tests/_mpc_checks.py parity
allows (the discrimination rule), with at least two solved instances.  POLISHED lists the (case, row, mode) in which
polished points are held to the 1e-9 violation bar, to the weak-duality certificate and, without state bounds, to the
1e-7 optimality gap against the IPM: those where the oracle alone meets them with the coverage condition.  Elsewhere
polished points are held to the unpolished bar.
"""
from __future__ import annotations

from typing import NamedTuple

from tests import _mpc_checks as M

DEFAULTS = dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4, rho=0.1, sigma=1e-6, alpha=1.6, delta=1e-6,
                max_iter=10000, check_interval=25, scaling_iters=10, polish=1, polish_refine_iter=3, adaptive_rho=1,
                adaptive_rho_tol=5.0, polish_max_pass=8, cert_tol=1e-9, polish_max_rounds=2)

ROWS = {
    "eps_loose": dict(eps_abs=1e-3, eps_rel=1e-4),
    "eps_tight": dict(eps_abs=1e-8, eps_rel=1e-7),
    "alpha_1": dict(alpha=1.0),
    "alpha_18": dict(alpha=1.8),
    "rho_lo": dict(rho=0.01, adaptive_rho_tol=1.5),
    "rho_fixed": dict(rho=1.0, adaptive_rho=0),
    "ci_7": dict(check_interval=7),
    "ci_1": dict(check_interval=1),
    "scal_0": dict(scaling_iters=0),
    "scal_1": dict(scaling_iters=1),
    "sigma": dict(sigma=1.0),
    "polish_0": dict(polish=0),
    "refine_0": dict(polish_refine_iter=0),
    "delta": dict(delta=1e-3),
    "cap_60": dict(max_iter=60),
    "cap_400": dict(max_iter=400),                     # the long horizons' cap (60 leaves them one solved instance)
    "cap_10": dict(max_iter=10),                       # below the check interval: no check ever runs (N = 8)
    "cap_nocheck": dict(max_iter=150, check_interval=1000),   # the same past N = 8, where 10 iterations solve nothing
    "cert": dict(cert_tol=0.0),                        # exact mode: no polish certifies, every round runs
    "rounds_0": dict(cert_tol=0.0, polish_max_rounds=0),      # ... and none does (against BASE: cert_tol alone)
    "pass_0": dict(polish_max_pass=0),
    "prim_inf": dict(eps_prim_inf=1e-1),               # the certificate of the "hinf" instance no longer passes
    "combined": dict(eps_abs=1e-6, eps_rel=1e-4, eps_prim_inf=1e-3, alpha=1.3, rho=0.3, sigma=1e-5, check_interval=10,
                     scaling_iters=4, polish_refine_iter=5, delta=1e-7, adaptive_rho_tol=3.0, max_iter=4000,
                     polish_max_pass=4, cert_tol=1e-8, polish_max_rounds=1),
    "combined_off": dict(eps_abs=1e-6, eps_rel=1e-4, eps_prim_inf=1e-3, alpha=1.3, rho=0.3, sigma=1e-5,
                         check_interval=10, scaling_iters=4, max_iter=4000, adaptive_rho=0, polish=0),
}
# the settings a row's discrimination is measured against where the defaults would not single its setting out: the
# row's companion alone
BASE = {"rounds_0": dict(cert_tol=0.0)}
NOCHECK = ("cap_10", "cap_nocheck")                    # coverage: two status 1 instances
THREE_ROWS = ("combined", "ci_7", "cap_60")            # the rows the bit-identity contracts are repeated under
LONG_SOLVES = ("rho_fixed", "cap_60", "eps_tight", "combined")      # the rows run at Ts = 0.05 too
N129_ROWS = ("eps_loose", "alpha_1", "ci_7", "scal_0", "scal_1", "polish_0", "cap_400", "combined")


class SCase(NamedTuple):
    """text: the kernel text the case selects; entry: "step" / "qp"; rows: the candidate rows (None: every row but
    prim_inf, which needs the instance that is infeasible along the horizon); extra: settings every row of the case
    carries unless it sets them itself (max_iter <= 2000 at N = 129, for the oracle's time)."""
    text: str
    entry: str
    case: M.Case
    rows: tuple = None
    extra: tuple = ()

    @property
    def id(self):
        return (f"{self.text}-{self.entry}-{self.case.id}" + ("" if self.case.route == "default" else f"-{self.case.route}")
                + (f"-{self.case.variant}" if self.case.variant else ""))

    def row(self, name):
        """(name, keyword arguments) as tests/_mpc_checks.py oracle_step takes it."""
        kw = {**dict(self.extra), **ROWS[name]}
        if "max_iter" in dict(self.extra):             # the case's cap holds for a row with a larger one
            kw["max_iter"] = min(kw["max_iter"], dict(self.extra)["max_iter"])
        return name, kw

    def base(self, name):
        """What the row is measured against: None (the defaults) or its BASE settings."""
        return (f"{name}-base", {**dict(self.extra), **BASE[name]}) if name in BASE else None


_C = M.Case
SCASES = [
    SCase("solve", "step", _C("onewave", 8, 0.02, 16, 17)),                  # capacity 16
    SCase("solve", "step", _C("onewave", 12, 0.02, 16, 17)),                 # capacity 32
    SCase("solve", "step", _C("onewave", 20, 0.02, 16, 17)),                 # capacity 40
    SCase("solve", "step", _C("onewave", 20, 0.05, 16, 17), rows=LONG_SOLVES),
    SCase("solve", "qp", _C("cap80", 33, 0.02, 12, 17)),                     # the two-wave capacity 80
    SCase("solve", "step", _C("cap80", 33, 0.02, 12, 17, route="cap80")),
    SCase("split", "step", _C("split40", 33, 0.02, 12, 17)),                 # H = 40
    SCase("split", "step", _C("split48", 41, 0.02, 12, 17)),
    SCase("split", "step", _C("split64", 49, 0.02, 12, 19)),
    SCase("long", "step", _C("long", 65, 0.02, 8, 17)),                      # 256 threads
    SCase("long", "step", _C("long512", 129, 0.02, 6, 17), rows=N129_ROWS, extra=(("max_iter", 2000),)),
    SCase("general", "step", _C("general_sb", 20, 0.02, 16, 17, settings="vx")),
    SCase("general", "step", _C("general_sb", 20, 0.02, 16, 17, settings="vx", variant="hinf"),
          rows=("prim_inf", "combined")),
    SCase("general", "step", _C("general_sb", 65, 0.02, 8, 21, settings="vx"), rows=("combined",)),
]
TEXTS = ("solve", "split", "long", "general")
BY_ID = {sc.id: sc for sc in SCASES}


def candidates():
    """Every (case, row name) the survey walks."""
    return [(sc, r) for sc in SCASES for r in (sc.rows if sc.rows is not None else [x for x in ROWS if x != "prim_inf"])]


# the output-check constants of the settings rows: 4 x the oracle's worst error-over-bar ratio over this table, measured
# by tests/test_settings_ref.py on the CPU (X 0.170: N = 12, scaling_iters = 0; objective 0.102: N = 12, polish = 0)
C_X_SET = 0.69
C_J_SET = 0.41
# (the certificate's constants C_D / C_JC of tests/_mpc_checks.py cover this table too: the same survey measures them)
# (case, row) whose polished points, the oracle's own, have no state row with a multiplier: under max_iter = 60 only
# the instances the bounds leave alone converge.  Their certificate is asserted without that coverage condition
NO_STATE_ROWS = {("general-step-general_sb-N20-Ts0.02-vx", "cap_60")}
# (row, text) without a discriminating case.  The three cap purposes are each one setting read at several horizons:
# max_iter = 60 leaves the long horizons one solved instance (cap_400 is their cap row; it shows nothing new on the
# general solver's N = 20, where cap_60 stands); 10 iterations reach status 1 only at N = 8 (cap_nocheck is the row
# without a check elsewhere).  eps_prim_inf is read only where an instance can be infeasible along the horizon: without
# state rows the box and rate chain are decided up front, and with them the general solver runs.
PARITY_ONLY = {("cap_60", "long"), ("cap_400", "general"), ("cap_10", "split"), ("cap_10", "long"),
               ("cap_10", "general"), ("prim_inf", "solve"), ("prim_inf", "split"), ("prim_inf", "long")}
# ---- what the CPU survey (tests/test_settings_ref.py) left: TABLE[case id][row] = polish modes with discrimination,
# POLISHED[case id][row] = the modes among them in which the 1e-9 bar and (no state bounds) the gap are asserted
TABLE = {
    "solve-step-onewave-N8-Ts0.02": {"alpha_1": (0, 1), "alpha_18": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "cap_60": (0, 1), "cap_10": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "solve-step-onewave-N12-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "solve-step-onewave-N20-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "solve-step-onewave-N20-Ts0.05": {"rho_fixed": (0, 1), "eps_tight": (0, 1), "combined": (0, 1)},
    "solve-qp-cap80-N33-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "solve-step-cap80-N33-Ts0.02-cap80": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "split-step-split40-N33-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "split-step-split48-N41-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0,), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "split-step-split64-N49-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "long-step-long-N65-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_400": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "long-step-long512-N129-Ts0.02": {"eps_loose": (0, 1), "alpha_1": (0, 1), "ci_7": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "polish_0": (0, 1), "combined": (0, 1)},
    "general-step-general_sb-N20-Ts0.02-vx": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "polish_0": (0, 1), "refine_0": (0, 1), "delta": (0, 1), "cap_60": (0, 1), "cap_nocheck": (0, 1), "cert": (1,), "rounds_0": (1,), "pass_0": (1,), "combined": (0, 1), "combined_off": (0, 1)},
    "general-step-general_sb-N20-Ts0.02-vx-hinf": {"prim_inf": (0, 1), "combined": (0, 1)},
    "general-step-general_sb-N65-Ts0.02-vx": {"combined": (0, 1)},
}
POLISHED = {
    "solve-step-onewave-N8-Ts0.02": {"alpha_1": (0, 1), "alpha_18": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "sigma": (0, 1), "cap_60": (0, 1), "combined": (0, 1)},
    "solve-step-onewave-N12-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "sigma": (0, 1), "combined": (0, 1)},
    "solve-step-onewave-N20-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "delta": (0,), "combined": (0, 1)},
    "solve-step-onewave-N20-Ts0.05": {"rho_fixed": (0, 1), "eps_tight": (0, 1), "combined": (0, 1)},
    "solve-qp-cap80-N33-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "combined": (0, 1)},
    "solve-step-cap80-N33-Ts0.02-cap80": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "combined": (0, 1)},
    "split-step-split40-N33-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "cap_60": (0, 1), "cap_400": (0, 1), "combined": (0, 1)},
    "split-step-split48-N41-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0,), "sigma": (0, 1), "cap_400": (0, 1), "combined": (0, 1)},
    "split-step-split64-N49-Ts0.02": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "delta": (0,), "cap_400": (0, 1), "combined": (0, 1)},
    "long-step-long-N65-Ts0.02": {"eps_loose": (1,), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "cap_400": (0, 1), "combined": (1,)},
    "long-step-long512-N129-Ts0.02": {"eps_loose": (0, 1), "alpha_1": (0, 1), "ci_7": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "combined": (0, 1)},
    "general-step-general_sb-N20-Ts0.02-vx": {"eps_loose": (0, 1), "eps_tight": (0, 1), "alpha_1": (0, 1), "alpha_18": (0, 1), "rho_lo": (0, 1), "rho_fixed": (0, 1), "ci_7": (0, 1), "ci_1": (0, 1), "scal_0": (0, 1), "scal_1": (0, 1), "sigma": (0, 1), "delta": (0,), "cap_60": (0, 1), "combined": (0, 1)},
    "general-step-general_sb-N20-Ts0.02-vx-hinf": {"prim_inf": (0, 1), "combined": (0, 1)},
    "general-step-general_sb-N65-Ts0.02-vx": {"combined": (0, 1)},
}


def surviving():
    """(case, row name, modes) the GPU test runs."""
    return [(BY_ID[cid], r, modes) for cid, rows in TABLE.items() for r, modes in rows.items()]


def unrefined(sc, row, mode):
    """The one departure by design.  With polish_refine_iter = 0 in OSQP mode the polish is one solve of the
    delta-regularized KKT system and nothing corrects it.  mpc_solve.h, mpc_split.h and mpc_long.h solve it by a
    multiply with the explicit K^-1 they keep, which is not backward stable as the oracle's (and mpc_general.h's)
    triangular solves are: its residuals are larger by the system's condition number, and OSQP's acceptance test (the
    polished residuals below ADMM's) passes less often.  The oracle with its polish solve replaced by a multiply with
    the inverse it forms from the same factor polishes exactly the kernels' instances (N 12 / 20 / 33 / 41 / 49 / 65:
    0 / 3 / 1 / 0 / 2 / 2 of the oracle's 1 / 4 / 5 / 5 / 5 / 4) with the same iteration counts; one refinement step
    removes the difference.  Asserted instead: the kernel polishes only where the oracle does."""
    return row == "refine_0" and mode == 0 and sc.text != "general"


def min_state(sc, row):
    """check_certificate's coverage: the instances that must carry a multiplier on a state row."""
    return 0 if (sc.id, row) in NO_STATE_ROWS else 2


def polished_modes(sc, row):
    return POLISHED.get(sc.id, {}).get(row, ())

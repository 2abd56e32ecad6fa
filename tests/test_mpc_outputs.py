"""X_opt, objective and the optimum of every MPC solver tier against the QP itself (tests/_qp_ref.py: plain numpy, no
solver): optimality by a weak-duality certificate, state rows included, and against the oracle's sparse-form Riccati
IPM (another algorithm) where there are none.

mpc_step has five hand-written solvers, each with its own output epilogue (X_opt by the linear model, the cost of
mpc_6stati.py:224-250, the scatter into [B,2,N] / [B,6,N+1]): the one-wave register kernel (N <= 20), the two-wave
capacity-80 kernel (21..40: the QP entry point, the step on request), the row-split kernel (21..64; H = 40 / 48 / 64),
the long-horizon kernel (65..256: K^-1 in LDS when it is sent N <= 64, in the caller's scratch past that, 512 threads
past N = 128) and the general solver (state bounds, N > 256).  tests/_mpc_checks.py holds the case table -- the
smallest shapes that open each path -- and the checks; tests/test_qp_ref.py walks the same table on the CPU with the
oracle in the kernel's place, which is where the two bar constants C_X = 0.44 and C_J = 0.34 come from (4 x the
oracle's worst error-over-bar ratio) and where the seeds are shown to meet the coverage conditions.

A (QP entry point, the linearization is the test's): on EVERY instance with status <= 1, X_opt = rollout(U_opt)
elementwise, objective = cost(X_opt, U_opt), u_cmd = U_opt[:, 0] and X_opt[:, 0] = x0 bitwise, the inequality rows
to 1e-9 (polished) or OSQP's eps criterion; status > 1: NaN outputs and u_cmd = u_prev; polished points within 1e-7
of the IPM's optimum (coverage: at least half of the solved instances and two) and, with or without state rows,
certified to 1e-7 by a dual bound (tests/_mpc_checks.py certify_point; state-bound rows -- a vx band, vx + vy + omega,
omega, vy, a one-sided heading bound -- in both modes, with two instances whose state rows carry multipliers, and
parity with the oracle beside it).
B (step entry point, the linearization is the kernel's): objective, feasibility and contract as in A; X_opt against the
oracle's on all stages where both polished, 1e-5 (1 + |X|) -- 10 x the U bar, the ratio of test_oracle_golden.py; the
certificate on the oracle's linearization.  The speed-capped closed loop: the step entry's polished outputs certified
on every state 8 steps of the loop visit.
C: both with non-default weights (off-diagonal R / Rd), asymmetric boxes, q_* and vehicle parameters, plus parity with
the oracle under the same settings; a non-symmetric R gives the symmetrized R's outputs bit for bit.
D: batch independence and determinism past N = 20 (row-split, long, general).
E: every tier's entry points on a workspace of exactly the size their query returns, a guard behind it untouched.

Measured on an MI355X, worst error / bar with C = 1 (the CPU oracle's in brackets): X 0.108 (0.108), objective 0.152
(0.0847), violation 0.94 of the eps bar / 0.018 of 1e-9, optimality gap 5.0e-10, step-entry X_opt against the oracle's
8.5e-9; certificate gap 5.0e-10 (5.0e-10) over the table, 7.6e-11 (7.6e-11) on state-bound rows and 5.1e-11 (4.3e-15) on
the closed loop's 39 polished steps, 37 of them with active state rows; its lower side 0.0157 (0.0148) of the C = 1
bar, the condensed objective 0.0462 (0.0462).  Most of the file's time is the N = 300 row: the general solver takes
about 6 s per call at 600 variables.
"""
import contextlib

import numpy as np
import pytest
import torch

from tests import _mpc_checks as M
from tests._cases import random_instances

pytestmark = pytest.mark.gpu

TB = pytest.importorskip("trajectory_generation_amd.batch")


@pytest.fixture(autouse=True, scope="module")
def _oracle_gpu_tire_sine(oracle_lib):
    """The oracle evaluates the HIP path's tire sine, as in tests/test_gpu_parity.py."""
    with oracle_lib.tire_sine(1):
        yield


@contextlib.contextmanager
def _route(case):
    """Select the kernel the row names, then restore the library's routing."""
    from trajectory_generation_amd import _lib
    if case.route == "cap80":
        prev = TB.SPLIT_MIN_N
        TB.set_split_min_n(_lib.MAX_N + 1)
        try:
            yield
        finally:
            TB.set_split_min_n(prev)
    elif case.route == "long_lds":
        _lib.check(_lib.lib().traj_debug_split_max_n(0), "traj_debug_split_max_n")
        try:
            yield
        finally:
            _lib.lib().traj_debug_split_max_n(_lib.MAX_N_SPLIT)
    else:
        assert case.route == "default"
        yield


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _cfg(case, mode, settings=None):
    kw, par = M.SETTINGS[settings or case.settings]
    c = TB.config_struct(N=case.N, Ts=case.Ts, polish_mode=mode, **kw)
    assert c.eps_abs == M.EPS_ABS and c.eps_rel == M.EPS_REL
    return c, par


def _parity(g, r, case, mode):
    """Statuses identical; U within 1e-6 where both polished (the step tests' bar)."""
    assert np.array_equal(g["status"], r["status"]), (case.id, mode, g["status"], r["status"])
    both = (g["status"] <= 1) & (g["polished"] > 0) & (r["polished"] > 0)
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    assert du[both].max(initial=0.0) <= 1e-6, (case.id, mode, du)
    return both


def _certificate(o, case, lin, mode, sb, w):
    """check_certificate in the modes of case.gap (state-bound rows: both), its ratios merged into w; the survey text."""
    if not sb and mode not in case.gap:
        return ""
    cg, wc, n_state, _ = M.check_certificate(o, case, lin)
    w.merge(wc)
    return f", certificate gap {cg:.2e}" + (f", state rows with a multiplier on {n_state}" if sb else "")


@pytest.mark.parametrize("case", M.QP_CASES + M.NONDEFAULT_CASES, ids=lambda c: c.id)
def test_qp_entry_outputs_vs_qp(gpu, oracle_lib, case):
    """A (and C): traj_mpc_qp_batch on the oracle's linearization, both polish modes, every check on every instance."""
    x0, up, pr, vr = M.inputs(case.N, case.Ts, case.B, case.seed)
    lin = M.lin_of(oracle_lib, case)
    sb = M.state_bounded(M.SETTINGS[case.settings][0])
    for mode in (0, 1):
        cfg, par = _cfg(case, mode)
        with _route(case):
            o = _np(TB.mpc_qp_batch(x0, up, pr, vr, *lin, cfg, par))
        if case.B >= 4:
            assert o["status"][1] == 3                       # the infeasible row: the epilogue's NaN / fallback branch
        w = M.check_outputs(o, case, lin)
        gap = None if sb or mode not in case.gap else M.check_gap(oracle_lib, o, case, lin)
        cert = _certificate(o, case, lin, mode, sb, w)
        if case.settings != "default":
            _parity(o, M.oracle_step(oracle_lib, case, mode), case, mode)
        ok = o["status"] <= 1
        print(f"gpu qp {case.id} mode {mode}: solved {ok.sum()}/{case.B}, polished {(ok & (o['polished'] > 0)).sum()}, "
              f"worst error / bar (C = 1): {w}" + ("" if gap is None else f", worst gap {gap:.2e}") + cert)


@pytest.mark.parametrize("case", M.STEP_CASES + M.NONDEFAULT_CASES, ids=lambda c: c.id)
def test_step_entry_outputs_vs_qp_and_oracle(gpu, oracle_lib, case):
    """B (and C): traj_mpc_step_batch, the linearization inside the kernel."""
    x0, up, pr, vr = M.inputs(case.N, case.Ts, case.B, case.seed)
    sb = M.state_bounded(M.SETTINGS[case.settings][0])
    for mode in (0, 1):
        cfg, par = _cfg(case, mode)
        with _route(case):
            o = _np(TB.mpc_step_batch(x0, up, pr, vr, cfg, par))
        if case.B >= 4:
            assert o["status"][1] == 3
        w = M.check_outputs(o, case, None)
        # (the oracle's linearization stands for the kernel's, as check_gap takes it for the settings rows' step
        # outputs: the 1e-7 bar absorbs the difference)
        cert = _certificate(o, case, M.lin_of(oracle_lib, case), mode, sb, w)
        r = M.oracle_step(oracle_lib, case, mode)
        both = _parity(o, r, case, mode)
        if mode in case.gap:
            assert both.sum() >= 1, (case.id, mode)
        dx = np.abs(o["X_opt"][both] - r["X_opt"][both]) / (1.0 + np.abs(r["X_opt"][both]))
        assert dx.max(initial=0.0) <= 1e-5, (case.id, mode, dx.max())
        print(f"gpu step {case.id} mode {mode}: solved {(o['status'] <= 1).sum()}/{case.B}, both polished {both.sum()}, "
              f"worst error / bar (C = 1): {w}, X vs oracle {dx.max(initial=0.0):.2e}" + cert)


def test_closed_loop_vcap_visited_states_certified(gpu, oracle_lib):
    """The bounded closed loop's own steps: 8 steps of the speed-capped loop (tests/_mpc_checks.py VCAP_LOOP) and, on
    every state it visits, the step entry's polished outputs proved optimal by the certificate -- the states the loop
    itself drives against the cap.  The loop applied exactly those steps' u_cmd (bit for bit, as
    tests/test_gpu_parity.py test_closed_loop_state_bounds_per_step holds at greater length)."""
    from trajectory_generation_amd.workload import make_workload
    L = M.VCAP_LOOP
    N, Ts, B, T = L["N"], L["Ts"], L["B"], L["T"]
    w = make_workload(B, N, Ts, kind="spline", seed=L["seed"])
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    vr = np.tile(w["vref"], (B, 1))
    for mode in (0, 1):
        cfg = TB.config_struct(N=N, Ts=Ts, warm_start=0, polish_mode=mode, **M.VCAP)
        res = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
        X, U, S = (res[k].cpu().numpy() for k in ("X", "U", "status"))
        t_seen = []

        def step(x, u, pr, v):
            o = _np(TB.mpc_step_batch(x, u, pr, v, cfg))
            t = len(t_seen)
            t_seen.append(t)
            assert np.array_equal(o["u_cmd"], U[:, t]) and np.array_equal(o["status"], S[t]), (mode, t)
            return o

        g, wc, n_ok, n_pol, n_state = M.certify_visited(
            oracle_lib, step, X, U, np.asarray(w["u0"]).reshape(-1, 2),
            lambda xs: TB.ref_window_batch(paths, xs, vr, N, Ts).cpu().numpy(), vr, mode)
        print(f"gpu closed loop vcap mode {mode}: solved {n_ok}/{B * T}, polished {n_pol}, state rows with a multiplier on "
              f"{n_state}, certificate gap {g:.2e}, worst error / bar (C = 1): {wc}")


@pytest.mark.parametrize("case", M.NONDEFAULT_CASES, ids=lambda c: c.id)
def test_nonsymmetric_R_is_its_symmetric_part(gpu, oracle_lib, case):
    """C: include/trajmpc.h says the symmetric part of R is used.  With R = [[.05, .05], [.01, 1.1]] both entry points
    return, bit for bit, the U_opt, u_cmd, X_opt, status, iteration count and polish flag they return for
    (R + R') / 2, and the objective is still the cost of the point (u' R u is the same number for both)."""
    x0, up, pr, vr = M.inputs(case.N, case.Ts, case.B, case.seed)
    lin = M.lin_of(oracle_lib, case)
    kw, par = M.SETTINGS["nonsym"]
    R = np.asarray(kw["R"])
    nonsym = case._replace(settings="nonsym")
    for mode in (0, 1):
        cn = TB.config_struct(N=case.N, Ts=case.Ts, polish_mode=mode, **kw)
        cs = TB.config_struct(N=case.N, Ts=case.Ts, polish_mode=mode, **dict(kw, R=(R + R.T) / 2))
        for entry in ("step", "qp"):
            run = ((lambda c: TB.mpc_step_batch(x0, up, pr, vr, c, par)) if entry == "step" else
                   (lambda c: TB.mpc_qp_batch(x0, up, pr, vr, *lin, c, par)))
            a, b = run(cn), run(cs)
            # (the objective is evaluated from R as given -- u0 (R00 u0 + R01 u1) + u1 (R10 u0 + R11 u1), mpc_long.h
            # -- so it may round differently; check_outputs holds it to the cost of the point)
            for k in ("U_opt", "u_cmd", "X_opt", "status", "iters", "polished"):
                assert _same(a[k], b[k]), (case.id, mode, entry, k)
            assert (a["status"] <= 1).sum() >= 2
            M.check_outputs(_np(a), nonsym, lin if entry == "qp" else None)


def _same(a, b):
    return torch.equal(a.nan_to_num(), b.nan_to_num()) and torch.equal(a.isnan(), b.isnan())


@pytest.mark.parametrize("N,bounds", [(33, None), (80, None), (20, "vx")], ids=["split-N33", "long-N80", "general-N20-vx"])
def test_batch_independence_past_n20(gpu, N, bounds):
    """D: the row-split kernel runs several instances per workgroup in a work-item loop, the long-horizon and general
    kernels index the caller's scratch by b.  Every output of rows [0, 5, 12] of a B = 13 call equals, bit for bit,
    the call on those three rows alone and three B = 1 calls; a repeated call equals the first (NaN against NaN:
    row 5 is infeasible)."""
    Ts, B, idx = 0.02, 13, [0, 5, 12]
    x0, up, pr, vr = random_instances(8, B, N, Ts)
    up[5, 0] = 3.0
    kw = M.SETTINGS["vx"][0] if bounds else {}
    for mode in (0, 1):
        cfg = TB.config_struct(N=N, Ts=Ts, polish_mode=mode, **kw)
        a = TB.mpc_step_batch(x0, up, pr, vr, cfg)
        a = {k: v.clone() for k, v in a.items()}
        b = TB.mpc_step_batch(x0, up, pr, vr, cfg)
        for k in a:
            assert _same(a[k], b[k]), (mode, "repeat", k)
        st = a["status"].cpu().numpy()
        assert st[5] == 3 and st[0] <= 1 and st[12] <= 1, st
        c = TB.mpc_step_batch(x0[idx], up[idx], pr[idx], vr[idx], cfg)
        for k in a:
            assert _same(a[k][idx], c[k]), (mode, "rows alone", k)
        for j, i in enumerate(idx):
            d = TB.mpc_step_batch(x0[i:i + 1], up[i:i + 1], pr[i:i + 1], vr[i:i + 1], cfg)
            for k in a:
                assert _same(a[k][i:i + 1], d[k]), (mode, "B = 1", i, k)


# ---- E: every tier on exactly the workspace its query asks for

GUARD_BYTES, GUARD_FILL = 4096, 0xA5


def _guarded_workspace(need, dev):
    """`need` zeroed bytes followed by a 4 KiB guard of a fixed bit pattern."""
    buf = torch.zeros(need + GUARD_BYTES, dtype=torch.uint8, device=dev)
    buf[need:] = GUARD_FILL
    return buf


def _guard_intact(buf, need):
    torch.cuda.synchronize()
    return bool((buf[need:] == GUARD_FILL).all())


@contextlib.contextmanager
def _split_min_n(n_min):
    prev = TB.SPLIT_MIN_N
    if n_min is not None:
        TB.set_split_min_n(n_min)
    try:
        yield
    finally:
        TB.set_split_min_n(prev)


TIER_CASES = [("reg-N20", 20, {}, None), ("split-N24", 24, {}, None), ("cap80-N24", 24, {}, 41),
              ("split-N41", 41, {}, None), ("split-N64", 64, {}, None), ("long-N65", 65, {}, None),
              ("long-N130", 130, {}, None), ("general-N20-vx", 20, M.SETTINGS["vx"][0], None)]


@pytest.mark.parametrize("name,N,kw,min_n", TIER_CASES, ids=[c[0] for c in TIER_CASES])
def test_step_and_closed_step_on_exactly_the_queried_workspace(gpu, name, N, kw, min_n):
    """E: traj_mpc_step_workspace_bytes / traj_closed_loop_workspace_bytes are what the entry points use, per tier
    (csrc/mpc_route.h).  The C entry point called directly on a workspace of exactly the queried size leaves the 4 KiB
    guard behind it untouched, and its outputs are those of the batch API on the same inputs, bit for bit."""
    import ctypes as C

    from trajectory_generation_amd import _lib
    L, p, B, Ts = _lib.lib(), _lib.default_params(), 3, 0.05
    cfg = TB.config_struct(N=N, Ts=Ts, max_iter=200, **kw)
    x0, up, pr, vr = (TB._dev(a) for a in random_instances(11, B, N, Ts))
    with _split_min_n(min_n):
        # the step
        ref = TB.mpc_step_batch(x0, up, pr, vr, cfg)
        need = int(L.traj_mpc_step_workspace_bytes(C.byref(cfg), B))
        assert need > 0
        ws, o = _guarded_workspace(need, gpu), TB._outputs(B, N, gpu)
        _lib.check(L.traj_mpc_step_batch(
            C.byref(p), C.byref(cfg), B, TB._p(x0), TB._p(up), TB._p(pr), TB._p(vr), TB._p(o["u_cmd"]),
            TB._p(o["status"]), TB._p(o["objective"]), TB._p(o["X_opt"]), TB._p(o["U_opt"]), TB._p(o["iters"]),
            TB._p(o["polished"]), TB._p(ws), need, TB._stream()), "traj_mpc_step_batch")
        assert _guard_intact(ws, need), (name, "step")
        assert (o["iters"] > 0).all() and (o["status"] >= 0).all() and (o["status"] <= 6).all(), (o["iters"], o["status"])
        for k in ref:
            assert _same(ref[k], o[k]), (name, "step", k)
        # one closed-loop step from the same states (t = 0: cold, nothing read from the workspace)
        xy = x0[:, :2].cpu().numpy()   # (parabolas through the states' positions)
        paths = TB.PathSet.build([0] * B, [[y - 0.1 * x * x, 0.0, 0.1, 0.0] for x, y in xy])
        xa, ua, xb, ub = x0.clone(), up.clone(), x0.clone(), up.clone()
        sta, stb = (torch.full((B,), -1, dtype=torch.int32, device=gpu) for _ in range(2))
        TB.closed_loop_step(xa, ua, paths, vr, cfg, status=sta)
        need = int(L.traj_closed_loop_workspace_bytes(C.byref(cfg), B))
        assert need > 0
        ws, ps = _guarded_workspace(need, gpu), paths.struct()
        _lib.check(L.traj_closed_loop_step(
            C.byref(p), C.byref(cfg), C.byref(ps), B, TB._p(xb), TB._p(ub), TB._p(vr), 0, 0, None, None, TB._p(stb),
            None, TB._p(ws), need, TB._stream()), "traj_closed_loop_step")
        assert _guard_intact(ws, need), (name, "closed-loop step")
        assert (stb >= 0).all() and (stb <= 6).all(), stb
        assert not torch.equal(xb, x0)
        assert torch.equal(xa, xb) and torch.equal(ua, ub) and torch.equal(sta, stb), (name, "closed-loop step")


@pytest.mark.parametrize("N", [40, 41], ids=["cap80-N40", "split-N41"])
def test_qp_entry_on_exactly_the_queried_workspace(gpu, N):
    """E for the QP entry: at N = 40 it keeps the capacity-80 kernel and takes no workspace (a guard alone is passed,
    with size 0); at N = 41 the row-split kernel runs on traj_mpc_qp_workspace_bytes.  The linearization is the one at
    (x0, u_prev), repeated over the horizon."""
    import ctypes as C

    from trajectory_generation_amd import _lib
    L, p, B, Ts = _lib.lib(), _lib.default_params(), 3, 0.05
    cfg = TB.config_struct(N=N, Ts=Ts, max_iter=200)
    x0, up, pr, vr = (TB._dev(a) for a in random_instances(12, B, N, Ts))
    lin = [a.unsqueeze(1).expand(B, N, *a.shape[1:]).contiguous() for a in TB.linearize_discretize_batch(x0, up, Ts)]
    ref = TB.mpc_qp_batch(x0, up, pr, vr, *lin, cfg)
    need = int(L.traj_mpc_qp_workspace_bytes(C.byref(cfg), B))
    assert (need == 0) == (N == 40)
    ws, o = _guarded_workspace(need, gpu), TB._outputs(B, N, gpu)
    _lib.check(L.traj_mpc_qp_batch(
        C.byref(p), C.byref(cfg), B, TB._p(x0), TB._p(up), TB._p(pr), TB._p(vr), *[TB._p(a) for a in lin],
        TB._p(o["u_cmd"]), TB._p(o["status"]), TB._p(o["objective"]), TB._p(o["X_opt"]), TB._p(o["U_opt"]),
        TB._p(o["iters"]), TB._p(o["polished"]), TB._p(ws), need, TB._stream()), "traj_mpc_qp_batch")
    assert _guard_intact(ws, need), N
    assert (o["iters"] > 0).all() and (o["status"] >= 0).all() and (o["status"] <= 6).all(), (o["iters"], o["status"])
    for k in ref:
        assert _same(ref[k], o[k]), (N, k)

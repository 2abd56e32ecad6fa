"""HIP path (libtrajmpc.so through its C ABI) vs the oracle and the reference's golden vectors.

Tolerances (DESIGN.md "Parity"):
  * physics (tire_forces, f_cont, rollout, lateral_error): |gpu - ref| <= 1e-12 (1 + |ref|)
    -- same float64 formulas; only libm ulps differ.
  * central-difference Jacobians / A, B, g: <= 1e-8 (1 + |ref|) -- a 1-ulp difference in f is
    divided by 2 eps = 2e-5.
  * QP, OSQP mode (polish_mode 0) and exact mode (1) vs the oracle on the same inputs: statuses
    identical; the polish outcome -- a residual comparison (mode 0) or a 1e-9 KKT certificate
    (mode 1), both borderline-sensitive to roundoff -- agrees for >= 98 % / 95 % of instances and
    the ADMM iteration count likewise; where both polished |dU| <= 1e-6 and the objective agrees to
    1e-7 relative; where neither polished (an eps = 1e-5 ADMM point) |dU| <= 1e-4.
  * exact mode vs the golden KKT-certified optimum: |dU| <= 1e-6 at Ts = 0.02, <= 1e-4 at
    Ts = 0.05 (condition numbers up to 8e8).
  * closed loop: gate (2) whole trajectories at Ts = 0.02 (150 steps): most within
    1e-8, all within 1e-3 at a polish flip and 1e-5 at the end and for MPC/main.py's own case at Ts = 0.05 (1e-7 over 10 steps); gate (1) per-step parity along the GPU trajectory
    for the random spline workload at Ts = 0.05, whose unstable plant amplifies 1e-12 differences
    ~50x per step so that no two float64 implementations keep whole trajectories together.
The QP boundary itself (cvxpy + OSQP) is not importable anywhere here: parity unpinned there,
pinned instead to the exact optimum (golden) and to the oracle's OSQP restatement.
"""
import numpy as np
import pytest
import torch

from tests._cases import random_instances

pytestmark = pytest.mark.gpu

TB = pytest.importorskip("trajectory_generation_amd.batch")


MAX_ITER = 10000   # traj_mpc_config / OSQP max_iter (CVXPY's default)


@pytest.fixture(autouse=True, scope="module")
def _oracle_gpu_tire_sine(oracle_lib):
    """Every GPU-vs-oracle gate in this module runs the oracle with the HIP path's tire sine (physics.h tire_sin_poly,
    the same coefficients and fma order: oracle.tire_sine(1)), so the two sides evaluate the same Pacejka physics and
    an unconverged point (the 10,000-iteration cap) is compared by U like any other.  The polynomial's own distance
    from libm's sine -- the reference's -- is bounded separately (tests/test_oracle_golden.py
    test_tire_sine_poly_vs_libm_and_fixtures, <= 2 ulp) and the GPU physics stays gated against the reference
    fixtures at 1e-12 below."""
    with oracle_lib.tire_sine(1):
        yield


@pytest.fixture
def cap80(gpu):
    """Send 20 < N <= 40 to the two-wave capacity-80 kernel (mpc_solve.h) for one test (the library's default for those
    horizons is the row-split kernel since round 6), then back: its instances keep their own bit-identity tests."""
    prev = TB.SPLIT_MIN_N
    TB.set_split_min_n(41)
    try:
        yield
    finally:
        TB.set_split_min_n(prev)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b))))


@pytest.fixture(scope="module")
def ph():
    return np.load("tests/golden/physics.npz")


# ------------------------------------------------------------------ physics vs reference goldens

def test_tire_forces_f_cont(gpu, ph):
    assert rel(TB.tire_forces_batch(ph["x"], ph["u"]).cpu().numpy(), ph["tire_forces"]) <= 1e-12
    assert rel(TB.f_cont_batch(ph["x"], ph["u"]).cpu().numpy(), ph["f_cont"]) <= 1e-12


def test_numerical_jacobian(gpu, ph):
    Jx, Ju, f = [t.cpu().numpy() for t in TB.numerical_jacobian_batch(ph["x"], ph["u"])]
    assert rel(Jx, ph["Jx"]) <= 1e-8
    assert rel(Ju, ph["Ju"]) <= 1e-8
    assert rel(f, ph["fval"]) <= 1e-12
    # columns X, Y are exactly zero as in the reference (f does not read X, Y)
    assert np.all(Jx[:, :, :2] == ph["Jx"][:, :, :2])


@pytest.mark.parametrize("Ts,tag", [(0.02, "002"), (0.05, "005")])
def test_linearize_discretize(gpu, ph, Ts, tag):
    A, Bm, g = [t.cpu().numpy() for t in TB.linearize_discretize_batch(ph["x"], ph["u"], Ts)]
    assert rel(A, ph["Ad_" + tag]) <= 1e-8
    assert rel(Bm, ph["Bd_" + tag]) <= 1e-8
    assert rel(g, ph["g_" + tag]) <= 1e-8


def test_anchor_values(gpu):
    an = np.load("tests/golden/anchors.npz")
    f = TB.f_cont_batch(an["x"][None], an["u"][None]).cpu().numpy()[0]
    np.testing.assert_allclose(f, [1, 0, 0, -0.17368083, 0.71692105, 30.66255866], atol=1e-7)
    A, Bm, g = [t.cpu().numpy()[0] for t in TB.linearize_discretize_batch(an["x"][None], an["u"][None], 0.05)]
    assert abs(A[5, 4] - 14.203684) < 1e-5 and abs(A[5, 5] + 1.334158) < 1e-5
    assert abs(Bm[5, 1] - 30.010969) < 1e-5 and abs(g[3] + 0.047693) < 1e-5


def test_lateral_error(gpu, ph):
    a = ph["lateral_error_in"]
    e = TB.lateral_error_batch(*[a[:, i] for i in range(5)]).cpu().numpy()
    assert rel(e, ph["lateral_error"]) <= 1e-12


# ------------------------------------------------------------------ full MPC step vs the oracle

def _step_both(O, seed, B, N, Ts, mode, **kw):
    x0, up, pr, vr = random_instances(seed, B, N, Ts)
    g = TB.mpc_step_batch(x0, up, pr, vr, TB.config_struct(N=N, Ts=Ts, polish_mode=mode, **kw))
    g = {k: v.cpu().numpy() for k, v in g.items()}
    r = O.mpc_step_batch(x0, up, pr, vr, O.cfg(N=N, Ts=Ts, polish_mode=mode, **kw))
    return g, r


def _agreement(g, r, both_pol_tol, neither_tol, flag_agree, iters_equal):
    """Statuses identical; the polish outcome (a residual comparison in OSQP mode, a KKT certificate
    in exact mode) agrees except for borderline cases; where both polished the optimum agrees."""
    assert np.array_equal(g["status"], r["status"])
    ok = g["status"] <= 1
    pg, pr = g["polished"] > 0, r["polished"] > 0
    assert np.mean(pg == pr) >= flag_agree
    assert np.mean(g["iters"] == r["iters"]) >= iters_equal
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    both = pg & pr & ok
    assert du[both].max(initial=0.0) <= both_pol_tol
    # (an instance that ran to the 10,000-iteration cap -- exact mode's continuation round keeps "optimal" there when
    # the base eps is met -- is compared by U as well: the oracle evaluates the GPU's tire sine in this module, so a
    # cap point no longer moves with a 2-ulp change of the sine alone, which shifted one such point by 0.12 at N = 40)
    neither = ~pg & ~pr & (g["status"] == 0)
    assert du[neither].max(initial=0.0) <= neither_tol
    dobj = np.abs(g["objective"] - r["objective"]) / np.abs(r["objective"])
    assert dobj[both].max(initial=0.0) <= 1e-7
    # u_cmd is U_opt[:, 0] (mpc_6stati.py:264-275)
    assert np.array_equal(g["u_cmd"][ok], g["U_opt"][ok][:, :, 0])
    return both


@pytest.mark.parametrize("N,Ts,B,min_pol", [(20, 0.05, 512, 0.8), (20, 0.02, 256, 0.95), (40, 0.05, 192, 0.45),
                                            (40, 0.02, 128, 0.8), (33, 0.02, 64, 0.8)])
def test_mpc_step_osqp_mode_vs_oracle(gpu, oracle_lib, N, Ts, B, min_pol):
    g, r = _step_both(oracle_lib, 11, B, N, Ts, 0)
    both = _agreement(g, r, both_pol_tol=1e-6, neither_tol=1e-4, flag_agree=0.98, iters_equal=0.98)
    assert both.mean() >= min_pol


@pytest.mark.parametrize("N,Ts,B,min_cert", [(20, 0.05, 256, 0.95), (20, 0.02, 128, 0.98), (40, 0.02, 64, 0.75)])
def test_mpc_step_exact_mode_vs_oracle(gpu, oracle_lib, N, Ts, B, min_cert):
    g, r = _step_both(oracle_lib, 12, B, N, Ts, 1)
    both = _agreement(g, r, both_pol_tol=1e-6, neither_tol=1e-1, flag_agree=0.95, iters_equal=0.95)
    assert both.mean() >= min_cert


@pytest.mark.parametrize("name", ["qp_N20_Ts005", "qp_N20_Ts002", "qp_N40_Ts005", "qp_N40_Ts002"])
def test_qp_exact_mode_vs_golden_optimum(gpu, oracle_lib, name):
    """QP half only (caller-supplied A, B, g from the reference) vs the golden KKT-certified optimum."""
    gd = np.load(f"tests/golden/{name}.npz")
    N, Ts = int(gd["N"]), float(gd["Ts"])
    o = TB.mpc_qp_batch(gd["x0"], gd["u_prev"], gd["path_ref"], gd["vref"], gd["Ad"], gd["Bd"], gd["g"],
                        TB.config_struct(N=N, Ts=Ts, polish_mode=1))
    o = {k: v.cpu().numpy() for k, v in o.items()}
    r = oracle_lib.mpc_step_batch(gd["x0"], gd["u_prev"], gd["path_ref"], gd["vref"],
                                  oracle_lib.cfg(N=N, Ts=Ts, polish_mode=1))
    assert np.array_equal(o["status"], r["status"]) and np.all(o["status"] <= 1)
    cert = o["polished"] > 0
    assert cert.mean() >= (0.9 if N == 20 else 0.35)
    du = np.abs(o["U_opt"] - gd["U_opt"]).max(axis=(1, 2))
    assert du[cert].max() <= (1e-6 if Ts < 0.03 else 1e-4)
    dobj = np.abs(o["objective"] - gd["objective"]) / np.abs(gd["objective"])
    assert dobj[cert].max() <= 1e-7


def test_full_step_vs_golden_optimum(gpu):
    """Full step (GPU linearization + QP) in exact mode vs the reference-linearized golden optimum."""
    gd = np.load("tests/golden/qp_N20_Ts002.npz")
    N, Ts = int(gd["N"]), float(gd["Ts"])
    o = TB.mpc_step_batch(gd["x0"], gd["u_prev"], gd["path_ref"], gd["vref"],
                          TB.config_struct(N=N, Ts=Ts, polish_mode=1))
    o = {k: v.cpu().numpy() for k, v in o.items()}
    cert = o["polished"] > 0
    assert cert.mean() >= 0.9
    du = np.abs(o["U_opt"] - gd["U_opt"]).max(axis=(1, 2))
    assert du[cert].max() <= 1e-6
    assert rel(o["X_opt"][cert], gd["X_opt"][cert]) <= 1e-6


# ------------------------------------------------------------------ edge cases

def test_infeasible_nonfinite_and_fallback(gpu, oracle_lib):
    N, Ts = 20, 0.05
    x0, up, pr, vr = random_instances(5, 6, N, Ts)
    up[1, 0] = 3.0          # rate chain cannot reach the box: infeasible (mpc_6stati.py:197-205)
    x0[2, 4] = np.nan       # non-finite state -> solver error
    pr[3, 7, 1] = np.inf    # non-finite reference
    vr[4, 2] = np.nan
    g = TB.mpc_step_batch(x0, up, pr, vr, TB.config_struct(N=N, Ts=Ts))
    g = {k: v.cpu().numpy() for k, v in g.items()}
    r = oracle_lib.mpc_step_batch(x0, up, pr, vr, oracle_lib.cfg(N=N, Ts=Ts))
    assert g["status"].tolist() == r["status"].tolist()
    assert g["status"][1] == 3 and g["status"][2] == 6 and g["status"][3] == 6 and g["status"][4] == 6
    for b in (1, 2, 3, 4):   # fallback: u_cmd = u_prev, no solution
        assert np.array_equal(g["u_cmd"][b], up[b])
        assert np.isnan(g["objective"][b]) and np.all(np.isnan(g["U_opt"][b]))
    assert g["status"][0] <= 1 and g["status"][5] <= 1


def test_degenerate_inputs(gpu, oracle_lib):
    """vx = 0 and vx < 0 (the sign(vx) max(|vx|, 0.3) branch), a pinned steering box, N = 1."""
    N, Ts = 20, 0.05
    x0, up, pr, vr = random_instances(6, 4, N, Ts)
    x0[0, 3] = 0.0
    x0[1, 3] = -0.7
    x0[2, 3] = -0.0
    g, r = (TB.mpc_step_batch(x0, up, pr, vr, TB.config_struct(N=N, Ts=Ts)),
            oracle_lib.mpc_step_batch(x0, up, pr, vr, oracle_lib.cfg(N=N, Ts=Ts)))
    g = {k: v.cpu().numpy() for k, v in g.items()}
    assert np.array_equal(g["status"], r["status"])
    both = (g["polished"] > 0) & (r["polished"] > 0)
    assert np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))[both].max(initial=0.0) <= 1e-6
    # equal steering bounds: delta pinned at 0 (u_prev delta within the rate reach)
    up2 = up.copy()
    up2[:, 1] = 0.1
    cfgk = dict(u_bounds=((-1.0, 1.0), (0.0, 0.0)))
    g2 = TB.mpc_step_batch(x0, up2, pr, vr, TB.config_struct(N=N, Ts=Ts, **cfgk))
    ok = g2["status"].cpu().numpy() <= 1
    assert ok.all()
    assert np.abs(g2["U_opt"].cpu().numpy()[:, 1, :]).max() <= 1e-6
    # horizon 1
    x1, u1, p1, v1 = random_instances(7, 8, 1, Ts)
    g1 = TB.mpc_step_batch(x1, u1, p1, v1, TB.config_struct(N=1, Ts=Ts))
    r1 = oracle_lib.mpc_step_batch(x1, u1, p1, v1, oracle_lib.cfg(N=1, Ts=Ts))
    assert np.array_equal(g1["status"].cpu().numpy(), r1["status"])
    np.testing.assert_allclose(g1["U_opt"].cpu().numpy(), r1["U_opt"], atol=1e-6)


def test_batch_composition_and_determinism(gpu):
    """Each instance is independent of its batch neighbours and of B; repeated calls are bitwise equal."""
    N, Ts = 20, 0.05
    x0, up, pr, vr = random_instances(8, 300, N, Ts)
    cfg = TB.config_struct(N=N, Ts=Ts)
    a = TB.mpc_step_batch(x0, up, pr, vr, cfg)
    b = TB.mpc_step_batch(x0, up, pr, vr, cfg)
    for k in a:
        assert torch.equal(a[k].nan_to_num(), b[k].nan_to_num()), k
    idx = [0, 17, 299]
    c = TB.mpc_step_batch(x0[idx], up[idx], pr[idx], vr[idx], cfg)
    for k in ("u_cmd", "U_opt", "status", "iters"):
        assert torch.equal(a[k][idx].nan_to_num(), c[k].nan_to_num()), k
    e = TB.mpc_step_batch(x0[:0], up[:0], pr[:0], vr[:0], cfg)
    assert e["u_cmd"].shape == (0, 2)


# ------------------------------------------------------------------ closed loop (MPC/main.py)

def _oracle_paths(O, w):
    from trajectory_generation_amd.batch import spline_natural
    out = []
    for k, c, kn in zip(w["kinds"], w["pcs"], w["knots"]):
        if k == 2:
            out.append(O.Path(2, (0, 0, 0, 0), xk=kn[0], coef=spline_natural(kn[0], kn[1]).reshape(-1)))
        else:
            out.append(O.Path(int(k), c))
    return out


def test_ref_window_vs_oracle(gpu, oracle_lib):
    from trajectory_generation_amd.workload import make_workload
    for kind in ("spline", "mixed"):
        w = make_workload(32, 20, 0.05, kind=kind, seed=4)
        paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
        xs = w["x0"][:, 0] + np.linspace(-10, 40, 32)       # also outside the knots (extrapolation)
        g = TB.ref_window_batch(paths, xs, np.tile(w["vref"], (32, 1)), 20, 0.05).cpu().numpy()
        ops = _oracle_paths(oracle_lib, w)
        r = np.stack([oracle_lib.ref_window(p, x, 20, 0.05, w["vref"]) for p, x in zip(ops, xs)])
        assert rel(g, r) <= 1e-12


def _closed_loop_both(O, kind, N, Ts, T, warm, B, seed=9, mode=0):
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(B, N, Ts, kind=kind, seed=seed)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=warm, polish_mode=mode)
    res = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    r = O.closed_loop_batch(_oracle_paths(O, w), w["x0"], w["u0"], w["vref"], T,
                            O.cfg(N=N, Ts=Ts, warm_start=warm, polish_mode=mode))
    return w, paths, cfg, res, r


@pytest.mark.parametrize("kind,N,Ts,T,warm", [("mixed", 20, 0.02, 150, 0), ("mixed", 20, 0.02, 150, 1),
                                              ("spline", 40, 0.02, 60, 1)])
def test_closed_loop_trajectories_vs_oracle(gpu, oracle_lib, kind, N, Ts, T, warm):
    """SURVEY.md 8(d) gate (2): whole closed-loop trajectories agree in the stable regime (Ts = 0.02)."""
    w, _, _, res, r = _closed_loop_both(oracle_lib, kind, N, Ts, T, warm, B=16)
    assert np.array_equal(res["status"].T, r["status"])
    err = np.abs(res["X"] - r["X"]).max(axis=2)          # [B, T+1]
    # a borderline polish flip (OSQP's accept/reject of the polished point) moves one step's u to
    # the eps = 1e-5 ADMM point instead of the optimum; the stable plant then contracts the offset
    assert err.max() <= 1e-3, err.max(axis=0)
    assert err[:, -1].max() <= 1e-5, err[:, -1]
    assert np.mean(err.max(axis=1) <= 1e-8) >= 0.75
    assert np.mean(res["iters"].T == r["iters"]) >= 0.95


def test_closed_loop_main_py_case_vs_oracle(gpu, oracle_lib):
    """MPC/main.py itself (parabola y = 0.1 x^2, x0 = [0, .5, 0, 1, 0, 0], Ts = 0.05): 20 steps agree."""
    _, _, _, res, r = _closed_loop_both(oracle_lib, "parabola", 20, 0.05, 20, 1, B=2)
    assert np.array_equal(res["status"].T, r["status"])
    err = np.abs(res["X"] - r["X"]).max(axis=(0, 2))
    # 1e-12 at step 1, growing ~2x per step through the unstable lateral mode
    assert err[:10].max() <= 1e-7 and err.max() <= 1e-4, err


@pytest.mark.parametrize("kind,N,T,B,warm", [("spline", 20, 20, 48, 0), ("spline", 20, 20, 48, 1),
                                             ("mixed", 40, 30, 32, 0)])
def test_closed_loop_per_step_parity_ts005(gpu, oracle_lib, kind, N, T, B, warm):
    """SURVEY.md 8(d) gate (1) at Ts = 0.05, where the plant is unstable (rho(A) up to 6.45) and
    1e-12 differences grow ~50x per step: every step of the GPU closed loop is re-solved by the
    oracle from the GPU's own state and must agree (statuses identical; u_cmd as in the step tests).
    The N = 40 case (BASELINE.json configs[2]) drives some instances into solver errors (the
    40-stage condensed problem of an unstable plant overflows); the oracle reports the same."""
    Ts = 0.05
    w, paths, cfg, res, _ = _closed_loop_both(oracle_lib, kind, N, Ts, T, warm, B)
    vr = np.tile(w["vref"], (B, 1))
    n_same_pol = n = n_it = 0
    for t in range(T):
        xt = res["X"][:, t]
        ut = res["U"][:, t - 1] if t > 0 else w["u0"]
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        g = {k: v.cpu().numpy() for k, v in TB.mpc_step_batch(xt, ut, prt, vr, cfg).items()}
        # the closed-loop kernel applied exactly what the step entry point returns (warm start off)
        if not warm:
            assert np.array_equal(g["u_cmd"], res["U"][:, t])
            assert np.array_equal(g["status"], res["status"][t])
        ro = oracle_lib.mpc_step_batch(xt, ut, prt, vr, oracle_lib.cfg(N=N, Ts=Ts))
        assert np.array_equal(g["status"], ro["status"])
        same = (g["polished"] > 0) == (ro["polished"] > 0)
        du = np.abs(g["u_cmd"] - ro["u_cmd"]).max(axis=1)
        if N == 20:
            assert du[same].max() <= 1e-4
        else:
            # 40-stage problems of the unstable plant reach condition numbers ~1e9:
            # polished optima agree to 1e-6; unpolished eps = 1e-5 ADMM points to 3e-5 when both stop at
            # the same iteration; a different stopping iteration is a different point.  Observed on the
            # row-split kernel (tools/gate_margins.py, profiles/r06_gate_margins.json): 2.5e-7 / 3.0e-6, equal
            # iterations on 99.7 % (round 5's bars, on the capacity-80 kernel: 1e-6 / 1e-3 / 95 %)
            both = (g["polished"] > 0) & (ro["polished"] > 0)
            assert du[both].max(initial=0.0) <= 1e-6
            eq = same & ~both & (g["iters"] == ro["iters"])
            assert du[eq].max(initial=0.0) <= 3e-5
            n_it += int((g["iters"] == ro["iters"]).sum())
        n_same_pol += same.sum()
        n += B
    assert n_same_pol / n >= 0.98
    if N != 20:
        assert n_it / n >= 0.99


@pytest.mark.parametrize("kind,N,T,B", [("spline", 20, 20, 48), ("mixed", 40, 20, 32), ("mixed", 48, 12, 16)])
def test_closed_loop_warm_rho_per_step_vs_warm_oracle(gpu, oracle_lib, kind, N, T, B):
    """The warm-started closed loop (the bench line's semantics: each instance starts its ADMM from the rho its
    previous step adapted to, x = z = y = 0 as cold) gated step by step against the oracle run with the SAME warm
    start: every step of the GPU loop (per-step launches, bit-identical to the fused run) is re-solved by the
    oracle from the GPU's state and the GPU's carried rho (the workspace's warm record after the previous step,
    orc_mpc_step_batch_warm).  Statuses identical; at the GPU's iteration count, u to 1e-6 where the oracle polished and
    to 1e-3 where it did not (every unpolished one to 1e-2), each on >= 98 % (N = 40: 95 %; the rest are polish flips
    and unpolished ADMM points carrying the iterates' rounding); iteration counts equal,
    and the rho each side carries out of the step equal to 1e-4 relative, on as many (rho is a ratio of residual norms
    of a not yet converged iterate: it carries that iterate's rounding, 1e-8 .. 1e-5 relative measured)."""
    from trajectory_generation_amd.workload import make_workload
    Ts = 0.05
    w = make_workload(B, N, Ts, kind=kind, seed=9)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=1)
    fused = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
    dev = fused["X"].device
    x = torch.as_tensor(w["x0"], device=dev).clone()
    u = torch.as_tensor(w["u0"], device=dev).clone()
    vr_d = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=dev).contiguous()
    hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=dev)
    hu = torch.empty((B, T, 2), dtype=torch.float64, device=dev)
    hx[:, 0] = x
    st = torch.empty((T, B), dtype=torch.int32, device=dev)
    it = torch.empty((T, B), dtype=torch.int32, device=dev)
    ws = TB.workspace(B, N, dev, TB._closed_extra(B, cfg))   # (the closed loop's own buffer: past N = 40 with its scratch)
    off = 66 * B * N   # the warm records: 4 doubles per instance after A, B, g and the stage records (trajmpc.hip)
    ocfg = oracle_lib.cfg(N=N, Ts=Ts)
    vr = np.tile(w["vref"], (B, 1))
    rho_prev, valid_prev = np.zeros(B), np.zeros(B, np.int32)
    n = n_it = n_rho = n_pol = n_pol_same = n_eq = n_eq_same = 0
    for t in range(T):
        xt, ut = hx[:, t].cpu().numpy(), (hu[:, t - 1].cpu().numpy() if t > 0 else np.asarray(w["u0"]))
        TB.closed_loop_step(x, u, paths, vr_d, cfg, None, t, hx, hu, st[t], it[t])
        rec = ws[off:off + 4 * B].view(B, 4).cpu().numpy()
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        ro = oracle_lib.mpc_step_batch_warm(xt, ut, prt, vr, rho_prev, valid_prev, ocfg)
        gs, gu, gi = st[t].cpu().numpy(), hu[:, t].cpu().numpy(), it[t].cpu().numpy()
        assert np.array_equal(gs, ro["status"]), (t, gs, ro["status"])
        ok = gs <= 1
        du = np.abs(gu - ro["u_cmd"]).max(axis=1)
        # the loop does not export its per-step polish outcome, so pair by the oracle's: where the oracle polished
        # and the iterations agree, the points agree to 1e-6 but for the borderline polish flips (OSQP's
        # accept / reject of the polished point; the cold gate above meets them as unequal polish outcomes)
        pol = ok & (ro["polished"] > 0) & (gi == ro["iters"])
        n_pol += int(pol.sum())
        n_pol_same += int((du[pol] <= 1e-6).sum())
        eq = ok & (ro["polished"] == 0) & (gi == ro["iters"])
        assert du[eq].max(initial=0.0) <= 1e-2, (t, du[eq].max(initial=0.0))
        n_eq += int(eq.sum())
        n_eq_same += int((du[eq] <= 1e-3).sum())
        n_it += int((gi == ro["iters"]).sum())
        gr, gv = rec[:, 0], (rec[:, 1] != 0).astype(np.int32)
        both = (gv > 0) & (ro["valid"] > 0)
        n_rho += int((np.abs(gr - ro["rho"]) <= 1e-4 * np.abs(ro["rho"]))[both].sum() + (gv == ro["valid"])[~both].sum())
        n += B
        rho_prev, valid_prev = gr.copy(), gv.copy()   # the GPU's carried rho feeds the next step on both sides
    # the per-step launches are the fused run bit for bit (NaN == NaN: a blown-up N = 40 state, if any)
    same = lambda a, b: bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())   # noqa: E731
    assert same(hx, fused["X"]) and same(hu, fused["U"]) and torch.equal(st, fused["status"])
    bar = 0.98 if N == 20 else 0.95
    assert n_it / n >= bar and n_rho / n >= bar, (n_it / n, n_rho / n)
    assert n_pol_same >= bar * n_pol and n_eq_same >= bar * n_eq, (n_pol_same, n_pol, n_eq_same, n_eq)


def test_closed_loop_history_matches_single_steps(gpu):
    """run_closed_loop's device histories equal step-by-step calls of the per-step entry point."""
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 20, 0.05, 5, 16
    w = make_workload(B, N, Ts, kind="spline", seed=2)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=0)
    res = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
    x = np.array(w["x0"])
    u = np.array(w["u0"])
    for t in range(T):
        pr = TB.ref_window_batch(paths, x[:, 0], np.tile(w["vref"], (B, 1)), N, Ts)
        o = TB.mpc_step_batch(x, u, pr, np.tile(w["vref"], (B, 1)), cfg)
        uc = o["u_cmd"].cpu().numpy()
        f = TB.f_cont_batch(x, uc).cpu().numpy()
        x = x + Ts * f
        u = uc
        assert np.array_equal(res["U"].cpu().numpy()[:, t], uc)
        assert np.array_equal(res["X"].cpu().numpy()[:, t + 1], x)


@pytest.mark.parametrize("N,warm,mode,kernel", [(20, 1, 0, None), (20, 0, 0, None), (8, 1, 0, None), (12, 1, 0, None),
                                                (30, 1, 0, 41), (40, 1, 0, 41), (30, 1, 0, 21), (40, 1, 1, 21),
                                                (20, 1, 1, None)])
def test_fused_closed_loop_bit_identical(gpu, N, warm, mode, kernel):
    """traj_closed_loop_run (one launch, in-workgroup linearization, on-chip state) equals the per-step
    launches bit for bit: histories, statuses, iteration counts; also when split into two runs.  Every
    capacity: 16 (N 8), 32 (N 12), 40 (N 20), 80 (N 30 and N 40, kernel 41: the two-wave instance) and the row-split
    kernel (kernel 21, the default for 20 < N <= 40)."""
    from trajectory_generation_amd.workload import make_workload
    prev = TB.SPLIT_MIN_N
    if kernel is not None:
        TB.set_split_min_n(kernel)
    try:
        _fused_closed_loop_bit_identical(gpu, N, warm, mode)
    finally:
        TB.set_split_min_n(prev)


def _fused_closed_loop_bit_identical(gpu, N, warm, mode):
    from trajectory_generation_amd.workload import make_workload
    Ts, T, B = 0.05, 24, 96
    w = make_workload(B, N, Ts, kind="mixed" if N == 40 else "spline", seed=6)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=warm, polish_mode=mode)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    fus = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    for k in ("X", "U", "status", "iters"):
        assert torch.equal(per[k], fus[k]), k
    # two fused launches (t0 = 0 and t0 = 10) continue exactly (warm record carried in the workspace)
    x = torch.as_tensor(w["x0"], device=gpu).clone()
    u = torch.as_tensor(w["u0"], device=gpu).clone()
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
    hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=gpu)
    hu = torch.empty((B, T, 2), dtype=torch.float64, device=gpu)
    hx[:, 0] = x
    st = torch.empty((T, B), dtype=torch.int32, device=gpu)
    it = torch.empty((T, B), dtype=torch.int32, device=gpu)
    TB.closed_loop_run(x, u, paths, vr, cfg, None, 0, 10, hx, hu, st[:10], it[:10])
    TB.closed_loop_run(x, u, paths, vr, cfg, None, 10, T - 10, hx, hu, st[10:], it[10:])
    assert torch.equal(hx, per["X"]) and torch.equal(hu, per["U"])
    assert torch.equal(st, per["status"]) and torch.equal(it, per["iters"])
    # several instances per workgroup (a grid smaller than B), with the heavy/light rank pairing
    from trajectory_generation_amd import _lib
    try:
        _lib.check(_lib.lib().traj_debug_fused_grid(28), "traj_debug_fused_grid")
        fus2 = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    finally:
        _lib.lib().traj_debug_fused_grid(0)
    for k in ("X", "U", "status", "iters"):
        assert torch.equal(per[k], fus2[k]), k


def _same(a, b):
    """Equal bit for bit, NaN == NaN (a diverged trajectory's history holds NaN in both runs)."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()) if a.is_floating_point() else torch.equal(a, b)


@pytest.mark.parametrize("N,warm,mode", [(20, 1, 0), (18, 1, 0), (20, 0, 1)])
def test_fused_three_waves_bit_identical(gpu, N, warm, mode):
    """The 3-waves-per-SIMD fused instance (capacity 40: 168 VGPRs, compact LDS image; opt-in since round 5,
    traj_debug_fused_waves(3)) equals the 2-wave instance and the per-step launches bit for bit; N = 18
    leaves padding rows in the capacity-40 kernel."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    Ts, T, B = 0.05, 200, 96
    w = make_workload(B, N, Ts, kind="spline", seed=11)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=warm, polish_mode=mode)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    runs = {}
    try:
        for wv in (2, 3, 0):   # forced 2, forced 3, by launch length (the default: 2)
            _lib.check(_lib.lib().traj_debug_fused_waves(wv), "traj_debug_fused_waves")
            runs[wv] = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    finally:
        _lib.lib().traj_debug_fused_waves(0)
    for wv, r in runs.items():
        for k in ("X", "U", "status", "iters"):
            assert _same(per[k], r[k]), (wv, k)


def test_fused_capacity80_instances_bit_identical(gpu, cap80):
    """Capacity 80 (N = 40, config 3): the one-wave-per-SIMD fused instance (the default) and the lean two-wave
    instance held to 2 waves per SIMD (traj_debug_fused_waves(2): 39 KB LDS, chunked reads) equal the per-step
    launches bit for bit, solver errors of the unstable N = 40 problems included."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 40, 0.05, 12, 48
    w = make_workload(B, N, Ts, kind="mixed", seed=3)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    runs = {}
    try:
        for wv in (1, 2, 0):   # forced one wave per SIMD, forced lean two-wave, default
            _lib.check(_lib.lib().traj_debug_fused_waves(wv), "traj_debug_fused_waves")
            runs[wv] = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    finally:
        _lib.lib().traj_debug_fused_waves(0)
    for wv, r in runs.items():
        for k in ("X", "U", "status", "iters"):
            assert _same(per[k], r[k]), (wv, k)


@pytest.mark.parametrize("lead", [(0, 0), (3, 500), (1, 999)])
def test_fused_queue_lead_bit_identical(gpu, lead):
    """The fused run's queue order (heavy instances ahead of the level front, traj_debug_queue_lead) moves
    only the schedule: a run continued from a first launch (so that the order has a previous launch to
    rank by) equals the per-step launches bit for bit, whatever the lead."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B, T0 = 20, 0.05, 16, 80, 4
    w = make_workload(B, N, Ts, kind="spline", seed=8)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    x = torch.as_tensor(w["x0"], device=gpu).clone()
    u = torch.as_tensor(w["u0"], device=gpu).clone()
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
    hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=gpu)
    hu = torch.empty((B, T, 2), dtype=torch.float64, device=gpu)
    hx[:, 0] = x
    st = torch.empty((T, B), dtype=torch.int32, device=gpu)
    it = torch.empty((T, B), dtype=torch.int32, device=gpu)
    try:
        _lib.check(_lib.lib().traj_debug_queue_lead(*lead), "traj_debug_queue_lead")
        TB.closed_loop_run(x, u, paths, vr, cfg, None, 0, T0, hx, hu, st[:T0], it[:T0])
        TB.closed_loop_run(x, u, paths, vr, cfg, None, T0, T - T0, hx, hu, st[T0:], it[T0:])
    finally:
        _lib.lib().traj_debug_queue_lead(1, 100)
    assert torch.equal(hx, per["X"]) and torch.equal(hu, per["U"])
    assert torch.equal(st, per["status"]) and torch.equal(it, per["iters"])


@pytest.mark.parametrize("levels,grid", [(0, 0), (1, 28), (64, 0), (64, 28), (4, 12)])
def test_fused_run_ahead_bit_identical(gpu, cap80, levels, grid):
    """Run-ahead (traj_debug_run_ahead: a workgroup keeps its instance for the next step, claimed once through the
    per-instance claim counter; drawers of run-ahead items draw again) moves only the schedule: two fused launches
    (the second ranked by the first) equal the per-step launches bit for bit, with every workgroup slot or a grid
    far smaller than B (many instances per workgroup, many skipped draws), at N = 20 and config 3's N = 40."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    Ts, T, B, T0 = 0.05, 16, 80, 4
    for N, kind in ((20, "spline"), (40, "mixed")):
        w = make_workload(B, N, Ts, kind=kind, seed=12)
        paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
        cfg = TB.config_struct(N=N, Ts=Ts)
        per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
        x = torch.as_tensor(w["x0"], device=gpu).clone()
        u = torch.as_tensor(w["u0"], device=gpu).clone()
        vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
        hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=gpu)
        hu = torch.empty((B, T, 2), dtype=torch.float64, device=gpu)
        hx[:, 0] = x
        st = torch.empty((T, B), dtype=torch.int32, device=gpu)
        it = torch.empty((T, B), dtype=torch.int32, device=gpu)
        try:
            _lib.check(_lib.lib().traj_debug_run_ahead(levels), "traj_debug_run_ahead")
            _lib.check(_lib.lib().traj_debug_fused_grid(grid), "traj_debug_fused_grid")
            TB.closed_loop_run(x, u, paths, vr, cfg, None, 0, T0, hx, hu, st[:T0], it[:T0])
            TB.closed_loop_run(x, u, paths, vr, cfg, None, T0, T - T0, hx, hu, st[T0:], it[T0:])
        finally:
            _lib.lib().traj_debug_run_ahead(0)   # the library default (TGMPC_RUN_AHEAD 0): later tests run the product path
            _lib.lib().traj_debug_fused_grid(0)
        assert _same(hx, per["X"]) and _same(hu, per["U"]), N
        assert torch.equal(st, per["status"]) and torch.equal(it, per["iters"]), N


def test_fused_lost_handoff_is_an_error(gpu):
    """A fused-run workgroup that gives up waiting for an instance's previous step (spin bound, here one
    poll: step 1 items are drawn while step 0 still runs) makes the run an error (TRAJ_E_HANDOFF via
    traj_closed_loop_check), never TRAJ_OK with stale state; the default bound runs clean afterwards."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 20, 0.05, 6, 16
    w = make_workload(B, N, Ts, kind="spline", seed=3)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts)
    try:
        _lib.check(_lib.lib().traj_debug_spin_limit(1), "traj_debug_spin_limit")
        with pytest.raises(RuntimeError, match="hand-off"):
            TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    finally:
        _lib.lib().traj_debug_spin_limit(0)
    ok = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    assert torch.equal(ok["X"], per["X"])


# ------------------------------------------------------------------ drop-in module

def test_dropin_mpc_step_contract(gpu, oracle_lib):
    from trajectory_generation_amd import mpc_6stati as M
    x0, up, pr, vr = random_instances(13, 1, 20, 0.05)
    u, status, info = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20, vref=vr[0])
    assert status in ("optimal", "optimal_inaccurate")
    assert isinstance(u, np.ndarray) and u.shape == (2,)
    assert set(info) == {"status", "objective", "X_opt", "U_opt", "path_ref", "vref"}
    assert info["X_opt"].shape == (6, 21) and info["U_opt"].shape == (2, 20)
    np.testing.assert_array_equal(info["X_opt"][:, 0], x0[0])
    r = oracle_lib.mpc_step(x0[0], up[0], pr[0], vr[0], oracle_lib.cfg(N=20, Ts=0.05))
    np.testing.assert_allclose(u, r["u_cmd"], atol=1e-6)
    # vref None -> x0[3]; scalar vref
    _, s2, i2 = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20)
    assert np.all(i2["vref"] == x0[0, 3])
    _, s3, i3 = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20, vref=1.5)
    assert np.all(i3["vref"] == 1.5)
    # bad path_ref shape -> AssertionError (mpc_6stati.py:151)
    with pytest.raises(AssertionError):
        M.mpc_step(x0[0], up[0], pr[0][:-1], Ts=0.05, N=20)
    # infeasible -> (u_prev, status, {})
    u4, s4, i4 = M.mpc_step(x0[0], [3.0, 0.0], pr[0], Ts=0.05, N=20)
    assert s4 == "infeasible" and i4 == {} and np.array_equal(u4, [3.0, 0.0])
    # non-PSD weight -> cvxpy DCPError inside the reference's try
    u5, s5, i5 = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20, R=np.diag([-1.0, 1.0]))
    assert s5 == "Solver Error: DCPError" and i5 == {}
    # params override (dict copy, :144-146)
    _, s6, i6 = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20, params={"m": 0.05})
    assert s6 in ("optimal", "optimal_inaccurate")
    assert not np.array_equal(i6["U_opt"], info["U_opt"])


@pytest.mark.parametrize("N,Ts,B", [(60, 0.02, 24), (41, 0.05, 16), (60, 0.05, 16), (64, 0.02, 12), (65, 0.02, 8),
                                    (128, 0.02, 4), (21, 0.05, 16), (33, 0.02, 16), (49, 0.05, 12), (200, 0.02, 4)])
def test_long_horizon_vs_oracle(gpu, oracle_lib, N, Ts, B):
    """Horizons past the capacity-40 kernel: 21 <= N <= 64 on the row-split kernel (mpc_split.h; N 21, 41 and 49 open
    its three half-row widths H = 40 / 48 / 64, N = 33 has n = 66 = 2 mod 4), past that the long-horizon kernel (mpc_long.h: the hot
    algorithm with one thread per variable, K^-1 in LDS up to N = 64, in the caller's scratch from N = 65 to
    TRAJ_MAX_N_LONG = 256, N > 128 on its 512-thread instance; include/trajmpc.h horizon tiers): mpc_step takes any N (mpc_6stati.py:125).  Batch entry
    point and the drop-in module against the oracle at the step tests' bars: statuses identical, iteration counts
    equal on >= 95 %, U within 1e-6 where both polished and 1e-4 where neither did; the drop-in returns the batch's
    u_cmd and the reference's fallback contract."""
    from trajectory_generation_amd import mpc_6stati as M
    g, r = _step_both(oracle_lib, 17, B, N, Ts, 0)
    assert np.array_equal(g["status"], r["status"])
    ok = g["status"] <= 1
    assert ok.mean() >= 0.5
    pg, pr = g["polished"] > 0, r["polished"] > 0
    assert np.mean(pg == pr) >= 0.95 and np.mean(g["iters"] == r["iters"]) >= 0.95
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    assert du[pg & pr & ok].max(initial=0.0) <= 1e-6
    assert du[~pg & ~pr & ok].max(initial=0.0) <= 1e-4
    assert np.array_equal(g["u_cmd"][ok], g["U_opt"][ok][:, :, 0])
    assert g["X_opt"].shape == (B, 6, N + 1) and np.array_equal(g["X_opt"][ok][:, :, 0], random_instances(17, B, N, Ts)[0][ok])
    # the drop-in module (the reference's per-call path) on the first instances
    x0, up, pr_, vr = random_instances(17, B, N, Ts)
    for b in range(3):
        u, status, info = M.mpc_step(x0[b], up[b], pr_[b], Ts=Ts, N=N, vref=vr[b])
        assert status == _lib_status(g["status"][b])
        if g["status"][b] <= 1:
            np.testing.assert_array_equal(u, g["u_cmd"][b])
            assert info["X_opt"].shape == (6, N + 1) and info["U_opt"].shape == (2, N)
        else:
            assert np.array_equal(u, up[b]) and info == {}
    d = M.mpc_step_batch(x0, up, pr_, vr, Ts=Ts, N=N)
    assert np.array_equal(d["status"].cpu().numpy(), g["status"])
    assert np.array_equal(d["u_cmd"].cpu().numpy(), g["u_cmd"])


@pytest.mark.parametrize("N,Ts,B", [(48, 0.02, 16), (60, 0.05, 12), (80, 0.02, 6)])
def test_long_horizon_exact_mode_and_qp_batch_vs_oracle(gpu, oracle_lib, N, Ts, B):
    """The long-horizon kernel's exact polish (polish_mode 1: the KKT certificate, active-set passes, continuation
    rounds) against the oracle's, with K^-1 in LDS (N 48, 60) and in the caller's scratch (N 80): statuses identical,
    the certificate outcome and the iteration counts equal on >= 90 %, U within 1e-6 where both certified and 0.1
    where neither did (an eps ADMM point, possibly at the iteration cap).  Then the QP entry point
    (traj_mpc_qp_batch, the caller's A_k, B_k, g_k: here the oracle's own rollout + linearize_discretize,
    mpc_6stati.py:165-178) at the same horizons in both polish modes against the oracle's step on the same inputs."""
    g, r = _step_both(oracle_lib, 19, B, N, Ts, 1)
    assert np.array_equal(g["status"], r["status"])
    ok = g["status"] <= 1
    pg, pr = g["polished"] > 0, r["polished"] > 0
    assert np.mean(pg == pr) >= 0.9 and np.mean(g["iters"] == r["iters"]) >= 0.9
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    assert du[pg & pr & ok].max(initial=0.0) <= 1e-6
    assert du[~pg & ~pr & ok].max(initial=0.0) <= 1e-1
    assert (pg & pr & ok).sum() >= 1
    x0, up, prf, vr = random_instances(19, B, N, Ts)
    Ad, Bd, gd = np.zeros((B, N, 6, 6)), np.zeros((B, N, 6, 2)), np.zeros((B, N, 6))
    for b in range(B):
        xb = oracle_lib.nominal_rollout(x0[b], up[b], N, Ts)
        for k in range(N):
            Ad[b, k], Bd[b, k], gd[b, k] = oracle_lib.linearize_discretize(xb[:, k], up[b], Ts)
    for mode in (0, 1):
        q = {k: v.cpu().numpy() for k, v in
             TB.mpc_qp_batch(x0, up, prf, vr, Ad, Bd, gd, TB.config_struct(N=N, Ts=Ts, polish_mode=mode)).items()}
        ro = oracle_lib.mpc_step_batch(x0, up, prf, vr, oracle_lib.cfg(N=N, Ts=Ts, polish_mode=mode))
        assert np.array_equal(q["status"], ro["status"]), mode
        okq = q["status"] <= 1
        both = okq & (q["polished"] > 0) & (ro["polished"] > 0)
        assert both.sum() >= 1, mode
        dq = np.abs(q["U_opt"] - ro["U_opt"]).max(axis=(1, 2))
        assert dq[both].max(initial=0.0) <= 1e-6, mode
        assert np.array_equal(q["u_cmd"][okq], q["U_opt"][okq][:, :, 0])


@pytest.mark.parametrize("N,Ts", [(8, 0.05), (20, 0.05), (20, 0.02), (30, 0.05), (40, 0.05), (48, 0.05), (64, 0.05)])
def test_step_in_kernel_linearization_bit_identical(gpu, N, Ts):
    """traj_mpc_step_batch runs the linearization inside the solve launch (one launch per call; the capacity-16/40
    kernels copy block_linearize's stage records to the workspace for X_opt, the row-split kernel reads them from LDS);
    it equals the rollout_kernel + jac_kernel + solve sequence bit for bit in every output, at every kernel (capacity
    16 and 40; the row-split kernel at H = 40 (N 30, 40), 48 and 64)."""
    from trajectory_generation_amd import _lib
    x0, up, pr, vr = random_instances(23, 48, N, Ts)
    cfg = TB.config_struct(N=N, Ts=Ts)
    outs = {}
    try:
        for mode in (1, 0):
            _lib.check(_lib.lib().traj_debug_step_linearize(mode), "traj_debug_step_linearize")
            outs[mode] = {k: v.cpu() for k, v in TB.mpc_step_batch(x0, up, pr, vr, cfg).items()}
    finally:
        _lib.lib().traj_debug_step_linearize(1)
    for k in outs[0]:
        a, b = outs[1][k], outs[0][k]
        assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()) if a.is_floating_point() else torch.equal(a, b), k


@pytest.mark.parametrize("N,B", [(65, 3), (130, 2), (300, 1)])
def test_general_solver_past_128_variables_vs_oracle(gpu, oracle_lib, N, B):
    """The general solver (state bounds, mpc_general.h) past n = 128 variables, where its one-wave triangular solves
    hold three or more rows per lane and the Cholesky factor lives in the caller's scratch -- N = 300 past the round-5
    limit of 256 (its instance with 32 rows per lane, TRAJ_MAX_N_GENERAL = 1024): statuses, iteration counts and polish
    outcomes identical to the oracle, U within 1e-6 where both polished (Ts = 0.02, speed band)."""
    x_lo, x_hi = SB["vx"]
    g, r = _sb_both(oracle_lib, 29, B, N, 0.02, 0, x_lo, x_hi)
    assert np.array_equal(g["status"], r["status"])
    assert np.array_equal(g["iters"], r["iters"])
    pg, pr = g["polished"] > 0, r["polished"] > 0
    assert np.array_equal(pg, pr)
    ok = g["status"] <= 1
    assert ok.any()
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    assert du[pg & pr & ok].max(initial=0.0) <= 1e-6
    assert du[~pg & ~pr & ok].max(initial=0.0) <= 1e-4


def _lib_status(code):
    from trajectory_generation_amd._lib import STATUS_STRINGS
    return STATUS_STRINGS[int(code)]


# ------------------------------------------------------------------ state bounds (a9, :208-213)

# absent sides (-inf / inf) mixed with finite ones.  "wide": vx, vy, omega bounded -- at Ts = 0.05 about
# half the instances become infeasible along the horizon (OSQP's certificate); "vx": speed band only,
# all feasible, the optimum moves on 50-80 % of the instances (oracle survey of these seeds)
SB = {"wide": ([-np.inf, -np.inf, -np.inf, 0.35, -0.3, -3.0], [np.inf, np.inf, np.inf, 1.6, 0.3, 3.0]),
      "vx": ([-np.inf, -np.inf, -np.inf, 0.38, -np.inf, -np.inf], [np.inf, np.inf, np.inf, 1.52, np.inf, np.inf])}
SB_LO, SB_HI = SB["wide"]


def _sb_both(O, seed, B, N, Ts, mode, x_lo=SB_LO, x_hi=SB_HI):
    x0, up, pr, vr = random_instances(seed, B, N, Ts)
    kw = dict(x_lo=x_lo, x_hi=x_hi, polish_mode=mode)
    g = TB.mpc_step_batch(x0, up, pr, vr, TB.config_struct(N=N, Ts=Ts, **kw))
    g = {k: v.cpu().numpy() for k, v in g.items()}
    r = O.mpc_step_batch(x0, up, pr, vr, O.cfg(N=N, Ts=Ts, **kw))
    return g, r


@pytest.mark.parametrize("N,Ts,B,mode,bounds", [(20, 0.05, 96, 0, "wide"), (20, 0.05, 96, 0, "vx"),
                                                 (20, 0.02, 64, 0, "wide"), (40, 0.02, 12, 0, "vx"),
                                                 (20, 0.02, 32, 1, "wide")])
def test_state_bounds_vs_oracle(gpu, oracle_lib, N, Ts, B, mode, bounds):
    """The general solver (mpc_general.h) against the oracle's OSQP restatement with state rows: same
    statuses (x0 outside the bounds -> infeasible up front; ADMM's primal-infeasibility certificate
    otherwise), the same polish outcome and iteration counts on >= 95 % of instances, the optimum
    to 1e-6 where both polished; the state bounds hold on the returned X_opt (to the ADMM eps)."""
    x_lo, x_hi = SB[bounds]
    g, r = _sb_both(oracle_lib, 21, B, N, Ts, mode, x_lo, x_hi)
    assert np.array_equal(g["status"], r["status"])
    ok = g["status"] <= 1
    assert ok.mean() >= 0.4                                   # the bounds bind without emptying the set
    pg, pr = g["polished"] > 0, r["polished"] > 0
    assert np.mean(pg == pr) >= 0.95
    assert np.mean(g["iters"] == r["iters"]) >= 0.95
    both = pg & pr & ok
    du = np.abs(g["U_opt"] - r["U_opt"]).max(axis=(1, 2))
    assert du[both].max(initial=0.0) <= 1e-6
    neither = ~pg & ~pr & ok
    assert du[neither].max(initial=0.0) <= 1e-4
    X = g["X_opt"][ok]                                        # [b, 6, N+1]
    lo, hi = np.asarray(x_lo)[None, :, None], np.asarray(x_hi)[None, :, None]
    assert np.all(X[:, :, 1:] >= lo - 1e-3) and np.all(X[:, :, 1:] <= hi + 1e-3)
    bad = ~ok                                                 # fallback (mpc_6stati.py:257-262): u_prev
    x0, up, _, _ = random_instances(21, B, N, Ts)
    assert np.array_equal(g["u_cmd"][bad], up[bad])
    # the bounds are active: the bounded optimum differs from the unbounded one somewhere
    gu = TB.mpc_step_batch(*random_instances(21, B, N, Ts), TB.config_struct(N=N, Ts=Ts, polish_mode=mode))
    assert np.abs(gu["U_opt"].cpu().numpy()[ok] - g["U_opt"][ok]).max() > 1e-3
    print(f"state bounds {bounds} N={N} Ts={Ts} mode={mode}: optimal {ok.mean():.2f}, polished {both.mean():.2f}, "
          f"iters equal {np.mean(g['iters'] == r['iters']):.3f}, U bit-identical "
          f"{np.mean([np.array_equal(a, b) for a, b in zip(g['U_opt'][ok], r['U_opt'][ok])]):.2f}")


def test_state_bounds_edge_cases(gpu, oracle_lib):
    """x0 outside a bound (k = 0 row, :210-213) -> infeasible with the u_prev fallback; all-infinite bounds
    are the unbounded problem (the hot kernel); infeasible through the horizon -> OSQP's certificate."""
    from trajectory_generation_amd import mpc_6stati as M
    x0, up, pr, vr = random_instances(14, 4, 20, 0.05)
    lo = [-np.inf] * 6
    lo[3] = x0[0, 3] + 0.1                                    # vx(0) below its lower bound
    u, st, info = M.mpc_step(x0[0], up[0], pr[0], Ts=0.05, N=20, x_lo=lo)
    assert st == "infeasible" and info == {} and np.array_equal(u, up[0])
    # infinite bounds only: identical to no bounds at all
    a = M.mpc_step(x0[1], up[1], pr[1], Ts=0.05, N=20, x_lo=[-np.inf] * 6, x_hi=[np.inf] * 6)
    b = M.mpc_step(x0[1], up[1], pr[1], Ts=0.05, N=20)
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
    # vx pinned to a narrow band around every x0's speed for the whole horizon, and vx >= 5 (violated at
    # k = 0 by every instance): the statuses -- decided by ADMM's certificate or up front -- are the oracle's
    for x_lo, x_hi in (([-np.inf] * 3 + [1.0, -np.inf, -np.inf], [np.inf] * 3 + [1.0 + 1e-6, np.inf, np.inf]),
                       ([-np.inf] * 3 + [5.0, -np.inf, -np.inf], [np.inf] * 6)):
        g, r = _sb_both(oracle_lib, 14, 16, 20, 0.05, 0, x_lo=x_lo, x_hi=x_hi)
        assert np.array_equal(g["status"], r["status"])
        assert np.array_equal(g["iters"], r["iters"])
    assert (g["status"] == 3).all()
    # the drop-in signature accepts bounds and returns the reference's info dict
    u, st, info = M.mpc_step(x0[3], up[3], pr[3], Ts=0.05, N=20, x_lo=SB_LO, x_hi=SB_HI)
    assert st in ("optimal", "optimal_inaccurate") and info["X_opt"].shape == (6, 21)


def test_state_bound_solves_between_closed_loop_steps(gpu):
    """A state-bound step / QP solve (whose scratch is the caller's workspace) made between two closed-loop
    steps on the same stream leaves the closed loop's state (warm-start records, order, queue) alone: the
    interleaved trajectory equals the uninterrupted one bit for bit (batch.workspace keeps one buffer per
    role)."""
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 20, 0.05, 8, 24
    w = make_workload(B, N, Ts, kind="spline", seed=4)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts)                     # warm start on: state carried between steps
    ref = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    x = torch.as_tensor(w["x0"], device=gpu).clone()
    u = torch.as_tensor(w["u0"], device=gpu).clone()
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
    hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=gpu)
    hu = torch.empty((B, T, 2), dtype=torch.float64, device=gpu)
    hx[:, 0] = x
    st = torch.empty((T, B), dtype=torch.int32, device=gpu)
    it = torch.empty((T, B), dtype=torch.int32, device=gpu)
    sb_cfg = TB.config_struct(N=N, Ts=Ts, x_lo=SB_LO, x_hi=SB_HI)
    x0s, ups, prs, vrs = random_instances(31, 200, N, Ts)      # more instances than the closed loop: a bigger scratch
    for t in range(T):
        TB.closed_loop_step(x, u, paths, vr, cfg, None, t, hx, hu, st[t], it[t])
        TB.mpc_step_batch(x0s, ups, prs, vrs, sb_cfg)          # state-bound step between the closed-loop steps
    for k, v in (("X", hx), ("U", hu), ("status", st), ("iters", it)):
        assert torch.equal(ref[k], v), k


# the closed loop under state bounds: "vcap" caps the speed at 1.3 m/s (the unbounded loop of this workload reaches
# 1.48 within 40 steps at Ts = 0.05); "wide" as above
SBC = {"vcap": ([-np.inf, -np.inf, -np.inf, 0.2, -np.inf, -np.inf], [np.inf, np.inf, np.inf, 1.3, np.inf, np.inf]),
       "wide": SB["wide"], "none": ([-np.inf] * 6, [np.inf] * 6)}


@pytest.mark.parametrize("N,Ts,T,B,bounds", [(20, 0.05, 40, 16, "vcap"), (20, 0.02, 30, 16, "wide"),
                                             (48, 0.02, 8, 6, "vcap"), (160, 0.02, 3, 2, "none"),
                                             (300, 0.02, 2, 2, "none")])
def test_closed_loop_state_bounds_per_step(gpu, oracle_lib, N, Ts, T, B, bounds):
    """State bounds inside the closed loop (mpc_6stati.py:208-213 passed by main.py:94's call; ABI 4: one step per
    launch sequence on the general solver, include/trajmpc.h), and without bounds N = 160 (the long-horizon kernel's
    512-thread instance) and N = 300 (past TRAJ_MAX_N_LONG: the general-solver path): traj_closed_loop_run equals
    step-by-step
    traj_closed_loop_step calls bit for bit; every step applied exactly the step entry point's u_cmd and status on the
    loop's own state (the reference calls mpc_step once per step: cold rho); and every step re-solved by the oracle
    from the GPU's state agrees at test_state_bounds_vs_oracle's bars (statuses identical, U to 1e-6 where both
    polished -- 1e-5 at N = 48 -- 1e-4 where neither did at the same iteration, polish outcome and iterations equal
    on >= 95 %)."""
    from trajectory_generation_amd.workload import make_workload
    x_lo, x_hi = SBC[bounds]
    w = make_workload(B, N, Ts, kind="spline", seed=5)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    # (cold rho, the reference's per-call semantics: the bounded and the general-solver closed loop run it anyway; the
    # long-horizon kernel's closed loop (N = 160) would otherwise carry rho from step to step)
    cfg = TB.config_struct(N=N, Ts=Ts, x_lo=x_lo, x_hi=x_hi, warm_start=0)
    res = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
    ref = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    for k in ("X", "U", "status", "iters"):
        assert _same(res[k], ref[k]), k
    X, U, S = (res[k].cpu().numpy() for k in ("X", "U", "status"))
    vr = np.tile(w["vref"], (B, 1))
    ocfg = oracle_lib.cfg(N=N, Ts=Ts, x_lo=x_lo, x_hi=x_hi)
    n = n_pol = n_it = 0
    for t in range(T):
        xt = X[:, t]
        ut = U[:, t - 1] if t > 0 else w["u0"]
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        g = {k: v.cpu().numpy() for k, v in TB.mpc_step_batch(xt, ut, prt, vr, cfg).items()}
        assert np.array_equal(g["u_cmd"], U[:, t]) and np.array_equal(g["status"], S[t]), t
        ro = oracle_lib.mpc_step_batch(xt, ut, prt, vr, ocfg)
        assert np.array_equal(g["status"], ro["status"]), (t, g["status"], ro["status"])
        ok = g["status"] <= 1
        pg, pr = g["polished"] > 0, ro["polished"] > 0
        du = np.abs(g["u_cmd"] - ro["u_cmd"]).max(axis=1)
        # (N = 48: 1e-5 -- the 96-variable problem with 2 x 48 state rows; one polished point 8.4e-6 apart was
        # measured at step 4 of the N = 48 case, the others at 1e-13)
        assert du[pg & pr & ok].max(initial=0.0) <= (1e-6 if N <= 40 else 1e-5), (t, du)
        assert du[~pg & ~pr & ok & (g["iters"] == ro["iters"])].max(initial=0.0) <= 1e-4, (t, du)
        n += B
        n_pol += int((pg == pr).sum())
        n_it += int((g["iters"] == ro["iters"]).sum())
    assert n_pol / n >= 0.95 and n_it / n >= 0.95, (n_pol / n, n_it / n)
    if bounds == "none":   # (no state rows: nothing below applies)
        return
    # (the statuses are the oracle's, step by step; with state rows OSQP stops unconverged or certifies infeasibility
    # on many steps -- the u_prev fallback then holds, as in the reference -- this only checks the bounds leave
    # solvable steps)
    assert (S <= 1).mean() >= 0.15
    # the bounds move the loop: the unbounded closed loop of the same workload applies other commands
    un = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, TB.config_struct(N=N, Ts=Ts, warm_start=0))
    assert np.abs(un["U"].cpu().numpy() - U).max() > 1e-3
    print(f"closed loop, state bounds {bounds} N={N} Ts={Ts}: optimal {(S <= 1).mean():.2f}, max vx "
          f"{np.nanmax(X[:, :, 3]):.3f} (unbounded {np.nanmax(un['X'].cpu().numpy()[:, :, 3]):.3f})")


def test_closed_loop_step_small_horizon_both_tiers(gpu):
    """The plant update the general tier's per-step path shares with the condensed kernels (csrc/mpc_frame.h:
    closed_sb_plant_kernel is plant_update), next to the window of ref_window_kernel that feeds it: 3
    traj_closed_loop_step calls at N = 4, B = 5, spline paths, once with one finite state bound that is never active
    (vx <= 1e3: the general solver) and once without bounds (the register-resident kernel).  Each run's history row
    t + 1 is bit for bit the state the step leaves in place (and row t of hist_u the u_prev it leaves).  The two runs
    agree at test_closed_loop_state_bounds_per_step's bars for two solvers of one problem, on every one of the 15
    (step, instance) pairs -- the bound is never active, so none is exempt: the statuses are equal and every step is
    either polished on both tiers (the applied u to 1e-6) or on neither at the same iteration count (1e-4) -- and the
    state rows, which integrate those commands (x' = x + Ts f(x, u)), at the loosest bar a command that fed them was
    held to."""
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 4, 0.02, 3, 5
    w = make_workload(B, N, Ts, kind="spline", seed=5)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), dtype=torch.float64, device="cuda").contiguous()
    runs = {}
    for name, x_hi in (("bounded", [np.inf, np.inf, np.inf, 1e3, np.inf, np.inf]), ("none", None)):
        kw = dict(x_lo=[-np.inf] * 6, x_hi=x_hi) if x_hi else {}
        cfg = TB.config_struct(N=N, Ts=Ts, warm_start=0, **kw)
        x = torch.as_tensor(w["x0"], dtype=torch.float64, device="cuda").reshape(B, 6).clone()
        u = torch.as_tensor(w["u0"], dtype=torch.float64, device="cuda").reshape(B, 2).clone()
        hx = torch.full((B, T + 1, 6), float("nan"), dtype=torch.float64, device="cuda")
        hu = torch.full((B, T, 2), float("nan"), dtype=torch.float64, device="cuda")
        hx[:, 0] = x
        st = torch.empty((T, B), dtype=torch.int32, device="cuda")
        it = torch.empty((T, B), dtype=torch.int32, device="cuda")
        pol = np.zeros((T, B), dtype=bool)
        for t in range(T):
            # (the step entry point on the loop's state: the loop applies exactly its u_cmd -- it tells which steps polished)
            prt = TB.ref_window_batch(paths, x[:, 0].cpu().numpy(), vr.cpu().numpy(), N, Ts).cpu().numpy()
            g = TB.mpc_step_batch(x.cpu().numpy(), u.cpu().numpy(), prt, vr.cpu().numpy(), cfg)
            pol[t] = g["polished"].cpu().numpy() > 0
            TB.closed_loop_step(x, u, paths, vr, cfg, None, t, hx, hu, st[t], it[t])
            assert torch.equal(hx[:, t + 1], x) and torch.equal(hu[:, t], u), (name, t)
            assert torch.equal(g["u_cmd"], hu[:, t]), (name, t)
        runs[name] = dict(X=hx.cpu().numpy(), U=hu.cpu().numpy(), S=st.cpu().numpy(), I=it.cpu().numpy(), pol=pol)
    a, b = runs["bounded"], runs["none"]
    assert np.array_equal(a["S"], b["S"]), (a["S"], b["S"])
    bar = np.zeros(B)   # per instance: the loosest bar of the commands so far
    for t in range(T):
        ok = a["S"][t] <= 1
        both, neither = a["pol"][t] & b["pol"][t] & ok, ~a["pol"][t] & ~b["pol"][t] & ok & (a["I"][t] == b["I"][t])
        du = np.abs(a["U"][:, t] - b["U"][:, t]).max(axis=1)
        dx = np.abs(a["X"][:, t + 1] - b["X"][:, t + 1]).max(axis=1)
        print(f"small horizon, both tiers, step {t}: du {du} dx {dx} polished {a['pol'][t]} {b['pol'][t]} "
              f"iters {a['I'][t]} {b['I'][t]}")
        assert du[both].max(initial=0.0) <= 1e-6 and du[neither].max(initial=0.0) <= 1e-4, (t, du)
        assert (both | neither | ~ok).all(), (t, a["pol"][t], b["pol"][t], a["I"][t], b["I"][t])
        # (not ok: both runs keep their u_prev, the statuses being equal -- as far apart as the commands before)
        assert (du[~ok] <= bar[~ok]).all(), (t, du, bar)
        bar = np.maximum(bar, np.where(neither, 1e-4, 1e-6))
        assert (dx <= bar).all(), (t, dx, bar)


# ------------------------------------------------------------------ dataset emitter (f1)

def test_dataset_generate_single_rank(gpu, oracle_lib, tmp_path):
    """dataset.generate (GPU closed loop -> packed history -> CSV) against the C oracle's closed loop of
    the same workload (Ts = 0.02: the stable regime where whole trajectories agree), and the CSVs
    against the histories it returns."""
    import pandas as pd
    from trajectory_generation_amd import dataset as D
    from trajectory_generation_amd.workload import make_workload
    B, T, N, Ts = 6, 30, 20, 0.02
    X, U, st = D.generate(B, T, N=N, Ts=Ts, kind="spline", seed=1, out_prefix=str(tmp_path / "ds"))
    w = make_workload(B, N, Ts, kind="spline", seed=1)
    O = oracle_lib
    r = O.closed_loop_batch(_oracle_paths(O, w), w["x0"], w["u0"], w["vref"], T, O.cfg(N=N, Ts=Ts, warm_start=1))
    assert np.array_equal(st.cpu().numpy(), r["status"].T)
    assert np.abs(X.cpu().numpy() - r["X"]).max() <= 1e-3
    assert st.shape == (T, B)
    # pack_history -> gather_to_root -> unpack_history is an exact copy of the device closed loop
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    direct = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, TB.config_struct(N=N, Ts=Ts))
    assert torch.equal(X, direct["X"]) and torch.equal(U, direct["U"]) and torch.equal(st, direct["status"])
    clean = pd.read_csv(tmp_path / "ds_clean.csv", float_precision="round_trip")
    noisy = pd.read_csv(tmp_path / "ds_noisy.csv", float_precision="round_trip")
    assert len(clean) == B * (T + 1) and list(noisy.columns)[-1] == "trajectory_id"
    np.testing.assert_allclose(clean["phi"].to_numpy().reshape(B, T + 1), X[:, :, 2].cpu().numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(clean["d"].to_numpy().reshape(B, T + 1)[:, :T], U[:, :, 0].cpu().numpy(), rtol=0, atol=0)


def test_native_loader_to_device(gpu, tmp_path):
    """f3 device path: load_vehicle_dataset(native=True, device='cuda') parses both CSVs with the library's
    parallel parser and copies the [n, C, T] float32 blocks from pinned memory to the GPU; the tensors
    equal the pandas loader's (data_loader.py:5-109) bit for bit."""
    from trajectory_generation_amd import dataset as D
    rng = np.random.default_rng(5)
    B, T = 40, 60
    X = np.cumsum(rng.normal(size=(B, T + 1, 6)) * 0.01, axis=1)
    U = rng.normal(size=(B, T, 2)) * 0.1
    p = str(tmp_path / "ds")
    D.write_csv(p, X, U, np.arange(B), 0.01)
    a = D.load_vehicle_dataset(f"{p}_noisy.csv", f"{p}_clean.csv", T_steps=50, native=True, device="cuda")
    b = D.load_vehicle_dataset(f"{p}_noisy.csv", f"{p}_clean.csv", T_steps=50)
    for pa, pb in zip(a, b):
        for ta, tb in zip(pa, pb):
            assert ta.is_cuda and torch.equal(ta.cpu(), tb)


def test_config3_hard_states_vs_fixture(gpu):
    """Config 3's hard states (tests/golden/qp_N40_Ts005_hard.npz, recorded from the reference's own
    rollout): the GPU step gives the fixture's statuses -- the u_prev fallback (mpc_6stati.py:257-262) on
    every step whose reference rollout blows up -- and, where exact mode certifies its point on a control
    row, the sparse-form (interior point) optimum to 1e-4."""
    g = np.load("tests/golden/qp_N40_Ts005_hard.npz")
    N, Ts = int(g["N"]), float(g["Ts"])
    keep = np.isfinite(g["x0"]).all(axis=1)
    x0, up, pr, vr = g["x0"][keep], g["u_prev"][keep], g["path_ref"][keep], g["vref"][keep]
    o = TB.mpc_step_batch(x0, up, pr, vr, TB.config_struct(N=N, Ts=Ts))
    o = {k: v.cpu().numpy() for k, v in o.items()}
    assert np.array_equal(o["status"], g["condensed_status"][keep])
    fail = g["failing"][keep] == 1
    assert np.array_equal(o["u_cmd"][fail], up[fail])
    ok = (~fail) & (g["ipm_status"][keep] == 0) & (g["ref_xbar_max"][keep] < 1e3)
    ox = TB.mpc_step_batch(x0[ok], up[ok], pr[ok], vr[ok], TB.config_struct(N=N, Ts=Ts, polish_mode=1))
    ox = {k: v.cpu().numpy() for k, v in ox.items()}
    cert = ox["polished"] > 0
    assert cert.sum() >= 16
    du = np.abs(ox["U_opt"][cert] - g["U_opt"][keep][ok][cert]).max()
    assert du <= 1e-4, du


@pytest.mark.parametrize("kernel", [41, 21])
def test_config3_iteration_cap_steps_vs_oracle(gpu, oracle_lib, kernel):
    """Config 3's steps at the 10,000-iteration cap (the launch's tail): the bench's own N = 40
    mixed workload (4096 trajectories, dt = 0.05) run 25 steps by the fused closed loop with cold rho (the oracle's
    semantics); every step that ran to the cap (up to 12, spread over the run) is re-solved from the GPU's state by
    the oracle: the same status and the same 10,000 iterations, the u_prev fallback where the status is not optimal,
    and u to 1e-3 where it is (an unpolished ADMM point after 10,000 iterations).  kernel 41: the capacity-80 kernel
    (traj_debug_split_min_n(41)); kernel 21: the row-split kernel, the default since round 6.  On the row-split kernel
    the status at the cap -- optimal_inaccurate or user_limit, OSQP's test of a NON-converged iterate's residuals
    against 10 eps -- may flip between the two on a borderline step (its mat-vec sums in another order: half-row
    partials joined across the lane pair); both still run the 10,000 iterations, and such a step is then compared by
    that (u_prev where the GPU fell back, the GPU's u otherwise); at most one flip per sample."""
    prev = TB.SPLIT_MIN_N
    TB.set_split_min_n(kernel)
    try:
        _config3_iteration_cap_steps(oracle_lib, kernel)
    finally:
        TB.set_split_min_n(prev)


def _config3_iteration_cap_steps(oracle_lib, kernel):
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 40, 0.05, 25, 4096
    w = make_workload(B, N, Ts, kind="mixed")
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=0)
    res = {k: v.cpu().numpy() for k, v in TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg).items()}
    cap = np.argwhere(res["iters"] == MAX_ITER)            # (t, b)
    assert len(cap) >= 3, len(cap)                          # the workload's tail items exist
    cap = cap[np.linspace(0, len(cap) - 1, min(12, len(cap))).round().astype(int)]
    vr = np.tile(w["vref"], (B, 1))
    ocfg = oracle_lib.cfg(N=N, Ts=Ts)
    flips = 0
    for t in np.unique(cap[:, 0]):
        bs = cap[cap[:, 0] == t, 1]
        xt = res["X"][:, t]
        ut = res["U"][:, t - 1] if t > 0 else np.asarray(w["u0"])
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()[bs]
        ro = oracle_lib.mpc_step_batch(xt[bs], ut[bs], prt, vr[bs], ocfg)
        gs, gu = res["status"][t, bs], res["U"][bs, t]
        same = gs == ro["status"]
        if kernel == 41:
            assert same.all(), (t, bs, gs, ro["status"])
        else:   # a flip only between the two max_iter outcomes
            assert np.isin(gs[~same], (1, 2)).all() and np.isin(ro["status"][~same], (1, 2)).all(), (t, bs, gs, ro["status"])
            flips += int((~same).sum())
        assert np.array_equal(ro["iters"], np.full(len(bs), MAX_ITER)), (t, bs, ro["iters"])
        ok = gs <= 1
        assert np.array_equal(gu[~ok], ut[bs][~ok]), (t, bs)
        assert np.abs(gu[ok & same] - ro["u_cmd"][ok & same]).max(initial=0.0) <= 1e-3, (t, bs)
    assert flips <= 1, flips


def test_divergent_dataset_trajectory_step_gate(gpu, oracle_lib):
    """configs[3]'s rare divergent trajectory (id 1854 of the bench workload leaves the
    stable regime at dt = 0.05, vx < 0 from step 9, solver errors from ~step 70 in this build's realization):
    whatever realization a build produces, every step of the GPU closed loop, re-solved from the GPU's own
    state by the step entry point and by the oracle (cold start), has the oracle's status, and u agrees where
    both polished (1e-6) or both stopped unpolished at the same ADMM iteration (1e-3)."""
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T = 20, 0.05, 75
    w = make_workload(4, N, Ts, kind="spline", seed=0, id_offset=1852)   # ids 1852..1855 (per-id seeds)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts)
    res = {k: v.cpu().numpy() for k, v in TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg).items()}
    vr = np.tile(w["vref"], (4, 1))
    n_cmp = 0
    for t in range(T):
        xt = res["X"][:, t]
        ut = res["U"][:, t - 1] if t > 0 else w["u0"]
        if not np.isfinite(xt).all():
            break
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        g = {k: v.cpu().numpy() for k, v in TB.mpc_step_batch(xt, ut, prt, vr, cfg).items()}
        ro = oracle_lib.mpc_step_batch(xt, ut, prt, vr, oracle_lib.cfg(N=N, Ts=Ts))
        assert np.array_equal(g["status"], ro["status"]), (t, g["status"], ro["status"])
        ok = g["status"] <= 1
        both = ok & (g["polished"] > 0) & (ro["polished"] > 0)
        du = np.abs(g["u_cmd"] - ro["u_cmd"]).max(axis=1)
        assert du[both].max(initial=0.0) <= 1e-6, (t, du)
        eq = ok & (g["polished"] == 0) & (ro["polished"] == 0) & (g["iters"] == ro["iters"])
        assert du[eq].max(initial=0.0) <= 1e-3, (t, du)
        n_cmp += int(both.sum() + eq.sum())
    assert n_cmp >= 200


# ------------------------------------------------------------------ the closed loop past N = 40 (long-horizon kernel)

@pytest.mark.parametrize("kind,N,Ts,T,B,warm", [("spline", 60, 0.05, 10, 16, 0), ("mixed", 48, 0.05, 10, 16, 0),
                                                ("spline", 60, 0.02, 12, 16, 0), ("spline", 100, 0.05, 4, 6, 0)])
def test_closed_loop_long_horizon_per_step(gpu, oracle_lib, kind, N, Ts, T, B, warm):
    """MPC/main.py's loop at horizons past the register-resident capacity (mpc_step takes any N, mpc_6stati.py:125;
    the closed loop runs the long-horizon kernel one step per launch sequence, include/trajmpc.h tiers).  SURVEY.md
    8(d) gate (1), at Ts = 0.05 and at main.py's Ts = 0.02 too: at N = 60 whole trajectories are no gate even at
    Ts = 0.02 -- the oracle's own closed loop with libm's and with the polynomial tire sine separates by 0.32 over 40
    steps there (eps = 1e-5 ADMM points amplified over the 60-stage preview) -- so every step of the GPU closed loop is re-solved from the GPU's own state by the step
    entry point (bit-identical to what the loop applied when warm start is off) and by the oracle (with the same
    carried rho when it is on): statuses identical, u to 1e-6 where both polished, to 1e-3 where both stopped
    unpolished at the same iteration, iteration counts equal on >= 95 %.  The fused entry point (traj_closed_loop_run)
    equals the per-step launches bit for bit.  N 48 / 60 run the row-split kernel (mpc_split.h), N = 100 the long-horizon
    one; the warm-started loop past N = 40 is gated in test_closed_loop_warm_rho_per_step_vs_warm_oracle."""
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(B, N, Ts, kind=kind, seed=21)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=warm)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    fus = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=True)
    for k in ("X", "U", "status", "iters"):
        assert _same(per[k], fus[k]), k
    res = {k: v.cpu().numpy() for k, v in per.items()}
    vr = np.tile(w["vref"], (B, 1))
    rho, valid = np.full(B, 0.1), np.zeros(B, np.int32)
    n = n_it = n_pol = n_close = 0
    for t in range(T):
        xt = res["X"][:, t]
        ut = res["U"][:, t - 1] if t > 0 else np.asarray(w["u0"])
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        if not warm:
            g = {k: v.cpu().numpy() for k, v in TB.mpc_step_batch(xt, ut, prt, vr, cfg).items()}
            assert np.array_equal(g["u_cmd"], res["U"][:, t]) and np.array_equal(g["status"], res["status"][t])
            assert np.array_equal(g["iters"], res["iters"][t])
            ro = oracle_lib.mpc_step_batch(xt, ut, prt, vr, oracle_lib.cfg(N=N, Ts=Ts))
        else:
            ro = oracle_lib.mpc_step_batch_warm(xt, ut, prt, vr, rho, valid, oracle_lib.cfg(N=N, Ts=Ts, warm_start=1))
            rho, valid = ro["rho"], ro["valid"]
        assert np.array_equal(res["status"][t], ro["status"]), (t, res["status"][t], ro["status"])
        ok = res["status"][t] <= 1
        du = np.abs(res["U"][:, t] - ro["u_cmd"]).max(axis=1)
        it_eq = res["iters"][t] == ro["iters"]
        pr_ = ro["polished"] > 0
        if not warm:
            # the step entry point's polish flag: where both polished the optimum agrees, where neither did the eps
            # ADMM points agree at the same stopping iteration, and the polish outcome agrees but for borderline flips
            pg = g["polished"] > 0
            assert du[pg & pr_ & ok].max(initial=0.0) <= 1e-6, (t, du)
            assert du[~pg & ~pr_ & it_eq & ok].max(initial=0.0) <= 1e-3, (t, du)
            n_pol += int((pg == pr_).sum())
        else:
            # (no polish flag from the closed loop: u within 1e-6 where the oracle polished on >= 95 %, all within 1e-2)
            n_pol += int(((du <= 1e-6) | ~pr_ | ~ok).sum())
            assert du[ok].max(initial=0.0) <= 1e-2, (t, du)
        n_close += int((du[ok] <= 1e-3).sum() + (~ok).sum())
        n_it += int(it_eq.sum())
        n += B
    assert n_it / n >= 0.95 and n_pol / n >= 0.95 and n_close / n >= 0.98, (n_it / n, n_pol / n, n_close / n)


@pytest.fixture
def split_from_21(gpu):
    """Route 21 <= N <= 40 to the row-split kernel for one test (the step, per-step and fused closed loop), then back."""
    prev = TB.SPLIT_MIN_N
    TB.set_split_min_n(21)
    try:
        yield
    finally:
        TB.set_split_min_n(prev)


@pytest.mark.parametrize("kind,N,T,B,warm", [("mixed", 40, 12, 48, 1), ("mixed", 40, 12, 48, 0), ("spline", 24, 10, 40, 1),
                                             ("spline", 32, 8, 24, 0)])
def test_split_fused_closed_loop_bit_identical(split_from_21, kind, N, T, B, warm):
    """The row-split kernel's fused closed loop (queue, sc1 hand-off, in-workgroup linearization by block_linearize)
    equals its per-step launches (rollout_kernel + jac_kernel + the closed-loop split solve) bit for bit -- histories,
    statuses, iterations -- over two launches (the second ordered by the first, with the lead set), also with a grid far
    smaller than B (many instances per workgroup)."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.workload import make_workload
    Ts = 0.05
    w = make_workload(B, N, Ts, kind=kind, seed=13)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=warm)
    per = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=False)
    for grid in (0, 7):
        dev = per["X"].device
        x = torch.as_tensor(w["x0"], device=dev).clone()
        u = torch.as_tensor(w["u0"], device=dev).clone()
        vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=dev)
        hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=dev)
        hu = torch.empty((B, T, 2), dtype=torch.float64, device=dev)
        hx[:, 0] = x
        st = torch.empty((T, B), dtype=torch.int32, device=dev)
        it = torch.empty((T, B), dtype=torch.int32, device=dev)
        T0 = T // 3
        try:
            _lib.check(_lib.lib().traj_debug_fused_grid(grid), "traj_debug_fused_grid")
            TB.closed_loop_run(x, u, paths, vr, cfg, None, 0, T0, hx, hu, st[:T0], it[:T0])
            TB.closed_loop_run(x, u, paths, vr, cfg, None, T0, T - T0, hx, hu, st[T0:], it[T0:])
        finally:
            _lib.lib().traj_debug_fused_grid(0)
        assert _same(hx, per["X"]) and _same(hu, per["U"]), grid
        assert torch.equal(st, per["status"]) and torch.equal(it, per["iters"]), grid


def test_split_config3_per_step_vs_oracle(split_from_21, oracle_lib):
    """Config 3 (mixed references, N = 40, dt = 0.05) on the row-split kernel: SURVEY.md 8(d) gate (1) as for the
    capacity-80 kernel (test_closed_loop_per_step_parity_ts005): every step of the fused closed loop (cold rho),
    re-solved from the GPU's state by the step entry point (the loop's u, bit for bit) and by the oracle: statuses
    identical, u to 1e-6 where both polished, to 1e-3 where both stopped unpolished at the same iteration, iteration
    counts equal on >= 95 %."""
    from trajectory_generation_amd.workload import make_workload
    N, Ts, T, B = 40, 0.05, 20, 32
    w = make_workload(B, N, Ts, kind="mixed", seed=9)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=Ts, warm_start=0)
    res = {k: v.cpu().numpy() for k, v in TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg).items()}
    vr = np.tile(w["vref"], (B, 1))
    n = n_it = n_pol = 0
    for t in range(T):
        xt = res["X"][:, t]
        ut = res["U"][:, t - 1] if t > 0 else w["u0"]
        prt = TB.ref_window_batch(paths, xt[:, 0], vr, N, Ts).cpu().numpy()
        g = {k: v.cpu().numpy() for k, v in TB.mpc_step_batch(xt, ut, prt, vr, cfg).items()}
        assert np.array_equal(g["u_cmd"], res["U"][:, t]) and np.array_equal(g["status"], res["status"][t])
        ro = oracle_lib.mpc_step_batch(xt, ut, prt, vr, oracle_lib.cfg(N=N, Ts=Ts))
        assert np.array_equal(g["status"], ro["status"]), (t, g["status"], ro["status"])
        ok = g["status"] <= 1
        pg, pr_ = g["polished"] > 0, ro["polished"] > 0
        du = np.abs(g["u_cmd"] - ro["u_cmd"]).max(axis=1)
        assert du[pg & pr_ & ok].max(initial=0.0) <= 1e-6, (t, du)
        assert du[~pg & ~pr_ & ok & (g["iters"] == ro["iters"])].max(initial=0.0) <= 1e-3, (t, du)
        n_it += int((g["iters"] == ro["iters"]).sum())
        n_pol += int((pg == pr_).sum())
        n += B
    assert n_it / n >= 0.95 and n_pol / n >= 0.98, (n_it / n, n_pol / n)

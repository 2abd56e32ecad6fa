"""The closed loop on a state estimate, on the CPU: the host specification of the loop (tests/_obs_ref.py, the C
oracle's MPC step on the EKF's estimate) filters, and the Python wrappers refuse bad shapes and arguments before
anything touches a GPU.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _obs_ref as R
from tests._knet_weights import LIMITS
from trajectory_generation_amd import _lib
from trajectory_generation_amd.workload import make_workload

B, N, TS, T = 16, 12, 0.05, 40


def _ekf_constants():
    from trajectory_generation_amd import knet as K
    return K.EKF_P0, K.EKF_Q, K.EKF_R


def test_host_ekf_step_is_the_oracles_filter():
    """T calls of _obs_ref.ekf_step_host give oracle.knet_oracle.ekf_run's estimates exactly (the same expressions)."""
    from oracle import knet_oracle as KO
    P0, Q, Rn = _ekf_constants()
    p = dict(KO.PARAMS)
    p.update(LIMITS)
    rng = np.random.default_rng(1)
    Tn = 7
    x0 = np.array([[0.3, -0.2, 0.1, 1.0, 0.02, 0.4], [1.0, 0.5, -0.3, 0.6, -0.03, -5.9]])
    U = np.stack([rng.uniform(-0.2, 0.6, (2, Tn)), rng.uniform(-0.3, 0.3, (2, Tn))], 1)
    Y = rng.normal(size=(2, 5, Tn)) * 0.05 + x0[:, R.HR, None]
    ref = KO.ekf_run(p, TS, Y, U, x0, P0, Q, Rn)
    for b in range(2):
        x, P = x0[b].copy(), np.diag(P0).astype(np.float64)
        for t in range(Tn):
            x, P = R.ekf_step_host(p, TS, x, P, U[b, 0, t], U[b, 1, t], Y[b, :, t], Q, Rn)
            assert (x == ref[b, :, t]).all(), (b, t)


def test_host_loop_filters(oracle_lib):
    """B = 16, N = 12, Ts = 0.05, T = 40, spline seed 6, default_rng(7) noise, the limits of tests/_knet_weights:
    every status optimal, and the estimate's pooled MSE on the measured channels below the measurements' own over
    steps >= 5 (0.30 of it when this was written)."""
    from oracle import knet_oracle as KO
    from trajectory_generation_amd.observed import estimation_errors
    P0, Q, Rn = _ekf_constants()
    p = dict(KO.PARAMS)
    p.update(LIMITS)
    w = make_workload(B, N, TS, kind="spline", seed=6)
    noise = np.random.default_rng(7).normal(size=(B, T, 5)) * np.sqrt(np.array(Rn))
    run = R.observed_loop_host(oracle_lib, w, N, TS, T, p, noise, P0, Q, Rn)
    assert (run["status"] == 0).all(), np.argwhere(run["status"] != 0)[:5]
    e = estimation_errors(run, skip=5)
    print(f"host loop: mse_est / mse_meas = {e['ratio']:.3f}; per channel "
          f"{(e['mse_est_ch'][R.HR] / e['mse_meas_ch']).round(3).tolist()}")
    assert e["mse_est"] < e["mse_meas"]
    # the measurement rows are the truth plus the noise, one addition
    assert (run["Y"] == run["X"][:, 1:][:, :, R.HR] + noise).all()


def test_estimation_errors_against_numpy():
    from trajectory_generation_amd.observed import estimation_errors
    rng = np.random.default_rng(0)
    X, Xh, Y = rng.normal(size=(3, 8, 6)), rng.normal(size=(3, 8, 6)), rng.normal(size=(3, 7, 5))
    e = estimation_errors(dict(X=X, Xhat=Xh, Y=Y), skip=2)
    d_est, d_meas = Xh[:, 3:] - X[:, 3:], Y[:, 2:] - X[:, 3:][:, :, R.HR]
    np.testing.assert_allclose(e["mse_est_ch"], (d_est ** 2).mean((0, 1)), rtol=1e-14)
    np.testing.assert_allclose(e["mse_meas_ch"], (d_meas ** 2).mean((0, 1)), rtol=1e-14)
    np.testing.assert_allclose(e["mse_est"], (d_est[:, :, R.HR] ** 2).mean(), rtol=1e-14)
    np.testing.assert_allclose(e["mse_meas"], (d_meas ** 2).mean(), rtol=1e-14)
    np.testing.assert_allclose(e["ratio"], e["mse_est"] / e["mse_meas"], rtol=1e-14)
    with pytest.raises(ValueError):
        estimation_errors(dict(X=X, Xhat=Xh, Y=Y), skip=7)
    with pytest.raises(ValueError):
        estimation_errors(dict(X=X, Xhat=Xh[:, :7], Y=Y))


def test_wrapper_argument_errors_need_no_gpu():
    """Shapes, the estimator's name, Q / R and the schedule are checked before any device work."""
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd import observed as OB
    cfg = TB.config_struct(N=N, Ts=TS)
    x0, u0, vref = np.zeros((4, 6)), np.zeros((4, 2)), np.ones(N + 1)
    bad = [dict(x0=np.zeros((4, 5))), dict(x0=np.zeros(6)), dict(u0=np.zeros((3, 2))), dict(xhat0=np.zeros((4, 5))),
           dict(noise=np.zeros((4, 5, 5))), dict(noise=np.zeros((4, 6, 4))), dict(P0=np.ones(5)),
           dict(P0=np.ones((4, 6))), dict(T=-1), dict(estimator="kalman"), dict(estimator=3),
           dict(Q=[1e-6] * 5), dict(Q=[-1e-6] + [0.0] * 5), dict(Q=[float("nan")] + [0.0] * 5), dict(R=[1.0] * 6),
           dict(R=[0.0] + [1.0] * 4), dict(R=[float("nan")] + [1.0] * 4), dict(vref_step=2),
           dict(vref_step=1, vref=np.ones(6 + N - 1)), dict(vref_step=1, vref=np.ones((3, 6 + N))),
           dict(estimator=lambda t, y, u: None, graph=True)]
    for kw in bad:
        args = dict(x0=x0, u0=u0, paths=None, vref=vref, T=6, cfg=cfg)
        args.update(kw)
        with pytest.raises(ValueError):
            OB.run_closed_loop_observed(**args)
    with pytest.raises(ValueError):
        OB.set_obs_lanes(8)
    o = OB.obs_config("ekf")
    assert o.estimator == _lib.OBS_EKF and list(o.Q) == list(OB.EKF_Q) and list(o.R) == list(OB.EKF_R)
    assert OB.obs_config("truth").estimator == _lib.OBS_TRUTH


def test_entry_points_refuse_before_any_launch():
    """The C entry points' argument errors that can be provoked with no device memory: every one returns TRAJ_E_ARG
    before a launch (the pointers are fake), and B == 0 is TRAJ_OK."""
    L = _lib.lib()
    p, c = _lib.default_params(), _lib.default_config(N, TS)
    lim = _lib.KnetLimits(*[float(LIMITS[k]) for k in ("x_min", "x_max", "y_min", "y_max", "phi_min", "phi_max",
                                                         "vx_min", "vx_max", "vy_min", "vy_max", "omega_min",
                                                         "omega_max")])
    ps = _lib.Paths()
    ps.kmax, ps.kind, ps.pc = 0, 16, 16
    fk, nul = C.c_void_p(16), None
    need = L.traj_closed_loop_obs_workspace_bytes(C.byref(c), 4)
    assert need == (L.traj_closed_loop_workspace_bytes(C.byref(c), 4) + 7) // 8 * 8 + 4 * 6 * 8
    assert L.traj_closed_loop_obs_workspace_bytes(None, 4) == 0
    assert L.traj_closed_loop_obs_workspace_bytes(C.byref(c), -1) == 0

    def cfg_of(est=_lib.OBS_EKF, Q=None, Rr=None):
        o = _lib.ObsConfig()
        o.estimator = est
        o.Q[:] = list(Q if Q is not None else (1e-6,) * 6)
        o.R[:] = list(Rr if Rr is not None else (1e-4,) * 5)
        return o

    def step(**kw):
        a = dict(p=C.byref(p), c=C.byref(c), paths=C.byref(ps), lim=C.byref(lim), o=C.byref(cfg_of()), B=4, x=fk,
                 xh=fk, P=fk, u=fk, vref=fk, row=N + 1, len=N + 1, vs=0, noise=nul, t=0, hT=6, hx=nul, hxh=nul, hu=nul,
                 hy=nul, ws=fk, wb=need)
        a.update(kw)
        return [L.traj_closed_loop_obs_step(a["p"], a["c"], a["paths"], a["lim"], a["o"], a["B"], a["x"], a["xh"],
                                            a["P"], a["u"], a["vref"], a["row"], a["len"], a["vs"], a["noise"], a["t"],
                                            a["hT"], a["hx"], a["hxh"], a["hu"], a["hy"], nul, nul, a["ws"], a["wb"],
                                            nul),
                L.traj_closed_loop_obs_run(a["p"], a["c"], a["paths"], a["lim"], a["o"], a["B"], a["x"], a["xh"],
                                           a["P"], a["u"], a["vref"], a["row"], a["len"], a["vs"], a["noise"], a["t"],
                                           1, a["hT"], a["hx"], a["hxh"], a["hu"], a["hy"], nul, nul, a["ws"], a["wb"],
                                           nul)]

    nan = float("nan")
    cbad = _lib.default_config(N, TS)
    cbad.rho = 0.0
    cases = [dict(p=nul), dict(c=nul), dict(paths=nul), dict(o=nul), dict(B=-1), dict(o=C.byref(cfg_of(est=3))),
             dict(o=C.byref(cfg_of(est=-1))), dict(lim=nul), dict(P=nul), dict(o=C.byref(cfg_of(Rr=(0.0,) + (1.0,) * 4))),
             dict(o=C.byref(cfg_of(Rr=(1.0,) * 4 + (-1.0,)))), dict(o=C.byref(cfg_of(Rr=(nan,) + (1.0,) * 4))),
             dict(o=C.byref(cfg_of(Q=(-1e-9,) + (0.0,) * 5))), dict(o=C.byref(cfg_of(Q=(0.0,) * 5 + (nan,)))),
             dict(x=nul), dict(xh=nul), dict(u=nul), dict(vref=nul), dict(ws=nul), dict(wb=need - 8), dict(c=C.byref(cbad)),
             dict(hx=fk, t=6), dict(hxh=fk, t=-1), dict(hu=fk, t=6), dict(hy=fk, t=7), dict(noise=fk, t=6),
             dict(noise=fk, t=-1), dict(vs=2), dict(len=N), dict(row=3), dict(vs=1, len=N + 3, row=N + 3, t=3),
             dict(vs=1, len=N + 3, row=0, t=-1, hT=0)]
    for kw in cases:
        assert step(**kw) == [_lib.TRAJ_E_ARG] * 2, sorted(kw)
    # a run whose last step leaves the histories or the schedule
    o = cfg_of()
    run = lambda t0, steps, hT, hx, vs, ln: L.traj_closed_loop_obs_run(   # noqa: E731
        C.byref(p), C.byref(c), C.byref(ps), C.byref(lim), C.byref(o), 4, fk, fk, fk, fk, fk, ln, ln, vs, nul, t0, steps,
        hT, hx, nul, nul, nul, nul, nul, fk, need, nul)
    assert run(4, 3, 6, fk, 0, N + 1) == _lib.TRAJ_E_ARG
    assert run(0, 4, 6, nul, 1, N + 3) == _lib.TRAJ_E_ARG
    assert run(0, -1, 6, nul, 0, N + 1) == _lib.TRAJ_E_ARG
    assert run(0, 0, 6, nul, 0, N + 1) == _lib.TRAJ_OK
    # an empty batch: no launch, whatever the pointers
    assert step(B=0, x=nul, xh=nul, P=nul, u=nul, vref=nul, ws=nul, wb=0) == [_lib.TRAJ_OK] * 2
    # the truth and a caller's estimator need neither the limits nor P; a bad R is the EKF's business alone
    # (checked with B = 0: with B > 0 these calls would launch)
    for est in (_lib.OBS_TRUTH, _lib.OBS_EXTERNAL):
        assert step(B=0, o=C.byref(cfg_of(est=est, Rr=(0.0,) * 5)), lim=nul, P=nul) == [_lib.TRAJ_OK] * 2
    # the estimator alone
    def e(**kw):
        a = dict(p=C.byref(p), lim=C.byref(lim), Ts=TS, B=4, x=fk, P=fk, u=fk, y=fk, Q=fk, R=fk)
        a.update(kw)
        return L.traj_ekf_step_f64(a["p"], a["lim"], a["Ts"], a["B"], a["x"], a["P"], a["u"], a["y"], a["Q"], a["R"],
                                   nul)

    for kw in (dict(p=nul), dict(lim=nul), dict(B=-1), dict(Ts=0.0), dict(Ts=nan), dict(x=nul), dict(P=nul), dict(u=nul),
               dict(y=nul), dict(Q=nul), dict(R=nul)):
        assert e(**kw) == _lib.TRAJ_E_ARG, sorted(kw)
    assert e(B=0, x=nul) == _lib.TRAJ_OK
    assert L.traj_debug_obs_lanes(8) == _lib.TRAJ_E_ARG and L.traj_debug_obs_lanes(16) == _lib.TRAJ_OK
    assert L.traj_debug_obs_lanes(_lib.OBS_DEFAULT_LANES) == _lib.TRAJ_OK

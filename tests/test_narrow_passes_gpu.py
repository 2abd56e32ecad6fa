"""The narrow passes of the in-workgroup linearization -- one lane-parallel sincos for the arguments known before the
rollout chain (u1, u1 +- eps, the window's phi*_k), the Jacobian assembly over three lanes per stage, the plant update
from the values stage 0 parks -- leave every result where the path they do not touch has it.  That path is the
per-step closed loop (rollout_kernel + jac_kernel launches, the solve reading A/B/g from the workspace, the plant's own
f(x, u)).  The fused run is compared with it, and the step entry point with its in-workgroup linearization on and off
(traj_debug_step_linearize), as float64 / int bit patterns: B = 5, T = 4."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T, TS, SEED = 5, 4, 0.05, 11
KEYS = ("X", "U", "status", "iters")
STEP_KEYS = ("u_cmd", "status", "objective", "X_opt", "U_opt", "iters", "polished")


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


def _workload(kind, N):
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(B, N, TS, kind=kind, seed=SEED)
    return w, TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])


def _closed(w, paths, cfg, fused, x0=None, u0=None, params=None):
    from trajectory_generation_amd import batch as TB
    r = TB.run_closed_loop(w["x0"] if x0 is None else x0, w["u0"] if u0 is None else u0, paths, w["vref"], T, cfg,
                           params=params, fused=fused)
    return {k: r[k].cpu().numpy() for k in KEYS}


def _step(w, paths, cfg, in_kernel, x0=None, u0=None, params=None):
    """The step entry point on the closed loop's first window, the linearization in the workgroup or as launches."""
    from trajectory_generation_amd import _lib, batch as TB
    x0 = w["x0"] if x0 is None else x0
    u0 = w["u0"] if u0 is None else u0
    vref = np.tile(w["vref"], (B, 1))
    pr = TB.ref_window_batch(paths, np.ascontiguousarray(x0[:, 0]), vref, cfg.N, TS)
    try:
        _lib.check(_lib.lib().traj_debug_step_linearize(int(in_kernel)), "traj_debug_step_linearize")
        o = TB.mpc_step_batch(x0, u0, pr, vref, cfg, params)
        return {k: o[k].cpu().numpy() for k in STEP_KEYS}
    finally:
        _lib.lib().traj_debug_step_linearize(1)


def _check(kind, N, x0=None, u0=None, params=None, **cfg_kw):
    """Fused against per step, step entry point in-workgroup against launches; returns the per-step closed loop."""
    from trajectory_generation_amd import batch as TB
    w, paths = _workload(kind, N)
    cfg = TB.config_struct(N=N, Ts=TS, **cfg_kw)
    want = _closed(w, paths, cfg, False, x0, u0, params)
    _same(_closed(w, paths, cfg, True, x0, u0, params), want, KEYS, "fused")
    _same(_step(w, paths, cfg, 1, x0, u0, params), _step(w, paths, cfg, 0, x0, u0, params), STEP_KEYS, "step")
    return want


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("kind", ["spline", "mixed"])
@pytest.mark.parametrize("N", [20, 7, 1])
def test_fused_and_step_equal_launched_linearization(gpu, N, kind, warm):
    r = _check(kind, N, warm_start=warm)
    assert np.isfinite(r["X"]).all()


@pytest.mark.parametrize("kind", ["spline", "mixed"])
def test_row_split_kernel(gpu, kind):
    """N = 24: the row-split kernel runs block_linearize at its own thread count."""
    _check(kind, 24, warm_start=1)


@pytest.mark.parametrize("kind,warm", [("spline", 1), ("mixed", 0)])
def test_three_wave_instance(gpu, kind, warm):
    """The 3-waves-per-SIMD instance keeps the plant that evaluates f(x_0, u_cmd) whole."""
    from trajectory_generation_amd import _lib
    try:
        _lib.check(_lib.lib().traj_debug_fused_waves(3), "traj_debug_fused_waves")
        _check(kind, 20, warm_start=warm)
    finally:
        _lib.lib().traj_debug_fused_waves(0)


@pytest.mark.parametrize("N", [20, 1])
def test_signed_zeros(gpu, N):
    """-0.0 in phi, vy, omega and in both inputs: the input columns' exact-vector evaluation, on the lanes that own
    the d and delta columns; the last trajectory has -0.0 in u0[1] alone."""
    w, _ = _workload("spline", N)
    x0, u0 = w["x0"].copy(), w["u0"].copy()
    x0[:4, 2] = -0.0
    x0[:4, 4] = -0.0
    x0[:4, 5] = -0.0
    u0[:4] = -0.0
    u0[4, 1] = -0.0
    assert (u0[:, 1] == 0.0).all() and np.signbit(u0[:, 1]).all() and u0[4, 0] != 0.0 and (x0[4, 2:] != 0.0).all()
    r = _check("spline", N, x0=x0, u0=u0)
    assert np.isfinite(r["X"]).all()


def test_pacejka_sine_outside_its_interval(gpu):
    """Cf = 2.5 and a front slip near -0.58 at stage 0: |Cf atan(Bf alpha_f)| > pi / 2, so the rollout lanes and the
    plant take the library sine."""
    from trajectory_generation_amd.batch import REFERENCE_PARAMS
    p = dict(REFERENCE_PARAMS, Cf=2.5)
    w, _ = _workload("spline", 20)
    x0, u0 = w["x0"].copy(), w["u0"].copy()
    x0[:, 3] = 0.5
    x0[:, 4] = np.linspace(0.25, 0.35, B)
    x0[:, 5] = 1.0
    u0[:, 1] = 0.0
    vx_eff = np.sign(x0[:, 3]) * np.maximum(np.abs(x0[:, 3]), p["vx_zero"])
    alpha_f = np.clip(-np.arctan2(x0[:, 5] * p["lf"] + x0[:, 4], vx_eff) + u0[:, 1], -p["maxAlpha"], p["maxAlpha"])
    assert (np.abs(p["Cf"] * np.arctan(p["Bf"] * alpha_f)) > math.pi / 2).all()
    r = _check("spline", 20, x0=x0, u0=u0, params=p)
    assert np.isfinite(r["X"]).all() and np.isfinite(r["U"]).all()


def test_plant_steps_with_u_prev_when_the_solve_is_not_optimal(gpu):
    """One ADMM iteration: no step is optimal, the plant applies u_prev -- on the parked values in the fused run."""
    w, _ = _workload("mixed", 20)
    r = _check("mixed", 20, max_iter=1)
    assert (r["status"] >= 2).all()
    assert np.array_equal(_bits(r["U"]), _bits(np.repeat(w["u0"][:, None, :], T, axis=1)))
    assert np.isfinite(r["X"]).all()

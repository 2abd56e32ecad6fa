"""The 64-lane K^-1 v of the fused capacity-40 instance at two waves per SIMD (TGMPC_KMUL_64: 160 chains of ten fma, one
per row and column class, dealt over all lanes; csrc/mpc_solve.h) leaves every result where the row-per-lane mat-vec
has it.  Two instances keep the row form and run the same arithmetic: the 3-waves-per-SIMD fused instance
(traj_debug_fused_waves(3)) and the per-step closed loop.  The default fused run is compared with both as float64 / int
bit patterns: X, U, status and iteration counts at B = 8, T = 6.  (The capacity-40 instances serve N = 16 .. 20; the
smaller horizons run the other capacities, which must not move either.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T, TS, SEED = 8, 6, 0.05, 23
KEYS = ("X", "U", "status", "iters")


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


def _workload(kind, N):
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(B, N, TS, kind=kind, seed=SEED)
    return w, TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])


def _closed(w, paths, cfg, fused, x0=None, u0=None):
    from trajectory_generation_amd import batch as TB
    r = TB.run_closed_loop(w["x0"] if x0 is None else x0, w["u0"] if u0 is None else u0, paths, w["vref"], T, cfg,
                           fused=fused)
    return {k: r[k].cpu().numpy() for k in KEYS}


def _three_waves(w, paths, cfg, x0=None, u0=None):
    from trajectory_generation_amd import _lib
    try:
        _lib.check(_lib.lib().traj_debug_fused_waves(3), "traj_debug_fused_waves")
        return _closed(w, paths, cfg, True, x0, u0)
    finally:
        _lib.lib().traj_debug_fused_waves(0)


def _check(kind, N, x0=None, u0=None, **cfg_kw):
    """The default fused run against the 3-wave instance and the per-step closed loop; returns the default run."""
    from trajectory_generation_amd import batch as TB
    w, paths = _workload(kind, N)
    cfg = TB.config_struct(N=N, Ts=TS, **cfg_kw)
    got = _closed(w, paths, cfg, True, x0, u0)
    _same(got, _three_waves(w, paths, cfg, x0, u0), "3-wave instance")
    _same(got, _closed(w, paths, cfg, False, x0, u0), "per-step closed loop")
    return got


@pytest.mark.parametrize("pmode", [0, 1])
@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("kind", ["spline", "mixed"])
@pytest.mark.parametrize("N", [20, 17, 13, 5, 1])
def test_fused_equals_row_form_instances(gpu, N, kind, warm, pmode):
    r = _check(kind, N, warm_start=warm, polish_mode=pmode)
    assert np.isfinite(r["X"]).all() and np.isfinite(r["U"]).all()


@pytest.mark.parametrize("rho", [1e-3, 100.0])
@pytest.mark.parametrize("N", [20, 17])
def test_rho_refactorization(gpu, N, rho):
    """A cold start from a rho a factor 100 / 1000 off the default 0.1: the residual checks move rho by far more than
    the tolerance, so K^-1 is staged into the class form again before the polish stages M^-1.  The factorization count
    is read from the solve's diagnostics on the first step (polish off: one factorization + the rho changes).  From
    rho = 100 every item refactors; from 1e-3 the items whose unconstrained optimum is feasible converge at the first
    check (3 of the 8), the others refactor."""
    import torch
    from trajectory_generation_amd import _lib, batch as TB
    r = _check("spline", N, warm_start=0, rho=rho)
    assert np.isfinite(r["X"]).all()
    w, paths = _workload("spline", N)
    cfg = TB.config_struct(N=N, Ts=TS, warm_start=0, rho=rho, polish=0)
    dev = TB.require_gpu()
    x = torch.as_tensor(w["x0"], device=dev).contiguous()
    u = torch.as_tensor(w["u0"], device=dev).contiguous()
    vref = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=dev).contiguous()
    dbg = torch.zeros((B, 32), dtype=torch.int64, device=dev)
    try:
        _lib.check(_lib.lib().traj_debug_set_stamps(C.c_void_p(dbg.data_ptr())), "traj_debug_set_stamps")
        TB.closed_loop_step(x, u, paths, vref, cfg, None, 0)
        torch.cuda.synchronize()
    finally:
        _lib.lib().traj_debug_set_stamps(None)
    nfact = dbg.cpu().numpy()[:, 8]
    assert (nfact >= 2).all() if rho > 1.0 else (nfact >= 2).any(), nfact


@pytest.mark.parametrize("N", [20, 17])
def test_iteration_cap_below_the_first_check(gpu, N):
    """max_iter = 7 < check_interval = 25: every item ends at the cap (status from the residuals there), none is
    polished, and the plant steps with u_prev."""
    w, _ = _workload("mixed", N)
    r = _check("mixed", N, max_iter=7)
    assert (r["status"] >= 2).all() and (r["iters"] == 7).all()
    assert np.array_equal(_bits(r["U"]), _bits(np.repeat(w["u0"][:, None, :], T, axis=1)))
    assert np.isfinite(r["X"]).all()


@pytest.mark.parametrize("N", [20, 17])
def test_signed_zeros(gpu, N):
    """-0.0 in phi, vy, omega and in both inputs."""
    w, _ = _workload("spline", N)
    x0, u0 = w["x0"].copy(), w["u0"].copy()
    x0[:6, 2] = -0.0
    x0[:6, 4] = -0.0
    x0[:6, 5] = -0.0
    u0[:6] = -0.0
    u0[7, 1] = -0.0
    assert np.signbit(u0[:6]).all() and np.signbit(x0[:6, 2]).all()
    r = _check("spline", N, x0=x0, u0=u0)
    assert np.isfinite(r["X"]).all()

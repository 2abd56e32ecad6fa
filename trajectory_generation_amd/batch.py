"""Batched, device-resident API over libtrajmpc.so (torch.cuda tensors in, torch.cuda tensors out).

Every function here launches HIP kernels through the C ABI (include/trajmpc.h); PyTorch only
provides device memory and the current stream.  There is no CPU fallback.

Reference correspondence (DorianaG01/trajectory_generation):
  f_cont_batch / tire_forces_batch / numerical_jacobian_batch /
  linearize_discretize_batch / lateral_error_batch   MPC/mpc_6stati.py:25-117
  mpc_step_batch                                     MPC/mpc_6stati.py:120-275, B instances at once
  mpc_qp_batch                                       the QP half :180-275 with caller (A, B, g)
  ref_window_batch / PathSet                         MPC/main.py:51-68 (geometry: DESIGN.md)
  closed_loop_step / run_closed_loop                 MPC/main.py:85-101, B trajectories at once
  simulate_open_loop                                 generation_traj/generation_type1.py:70-84, :131-137, :287-288
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p, stream as _stream
from ._lib import FsmRules, GenConfig, MpcConfig, Paths, VehicleParams

REFERENCE_PARAMS = {
    "Cm1": 0.287, "Cm2": 0.0545, "Cr0": 0.0518, "Cr2": 0.00035,
    "Br": 3.3852, "Cr": 1.2691, "Dr": 0.1737, "Bf": 2.579, "Cf": 1.2, "Df": 0.192,
    "m": 0.041, "Iz": 27.8e-6, "lf": 0.029, "lr": 0.033, "g": 9.81, "maxAlpha": 0.6, "vx_zero": 0.3,
}


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("trajectory_generation_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def params_struct(params: dict | VehicleParams | None = None) -> VehicleParams:
    if isinstance(params, VehicleParams):
        return params
    p = _lib.default_params()
    for k, v in (params or {}).items():
        if k in REFERENCE_PARAMS:
            setattr(p, k, float(v))
    return p


def config_struct(N=20, Ts=0.02, q_c=6.0, q_phi=0.5, q_vx=0.5, R=None, Rd=None,
                  u_bounds=((-1.0, 1.0), (-0.6, 0.6)), du_bounds=((-0.5, 0.5), (-0.3, 0.3)),
                  x_lo=None, x_hi=None, **solver) -> MpcConfig:
    """mpc_step keyword arguments (mpc_6stati.py:120-143) -> traj_mpc_config."""
    c = _lib.default_config(int(N), float(Ts))
    c.q_c, c.q_phi, c.q_vx = float(q_c), float(q_phi), float(q_vx)
    R = np.diag([0.02, 2.0]) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2)
    Rd = np.diag([0.01, 5.0]) if Rd is None else np.asarray(Rd, dtype=np.float64).reshape(2, 2)
    for i in range(4):
        c.R[i] = float(R.flat[i])
        c.Rd[i] = float(Rd.flat[i])
    for ch in range(2):
        c.u_lo[ch], c.u_hi[ch] = (float(v) for v in u_bounds[ch])
        c.du_lo[ch], c.du_hi[ch] = (float(v) for v in du_bounds[ch])
    if x_lo is not None:
        c.has_x_lo = 1
        for i, v in enumerate(np.asarray(x_lo, dtype=np.float64).reshape(6)):
            c.x_lo[i] = float(v)
    if x_hi is not None:
        c.has_x_hi = 1
        for i, v in enumerate(np.asarray(x_hi, dtype=np.float64).reshape(6)):
            c.x_hi[i] = float(v)
    for k, v in solver.items():
        if not hasattr(c, k):
            raise TypeError(f"unknown solver setting {k!r}")
        setattr(c, k, v)
    return c


def dev_f64(x, shape=None, device=None) -> torch.Tensor:
    """x as a contiguous float64 tensor on the GPU (device, or the current one), reshaped if a shape is given."""
    dev = require_gpu(device)
    t = torch.as_tensor(x, dtype=torch.float64, device=dev)
    if shape is not None:
        t = t.reshape(shape)
    return t.contiguous()


# ---------------------------------------------------------------- physics

def tire_forces_batch(x, u, params=None) -> torch.Tensor:
    x = dev_f64(x, (-1, 6)); u = dev_f64(u, (-1, 2))
    out = torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().traj_tire_forces_batch(C.byref(params_struct(params)), x.shape[0], _p(x), _p(u), _p(out),
                                                 _stream()), "traj_tire_forces_batch")
    return out


def f_cont_batch(x, u, params=None) -> torch.Tensor:
    x = dev_f64(x, (-1, 6)); u = dev_f64(u, (-1, 2))
    out = torch.empty((x.shape[0], 6), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().traj_f_cont_batch(C.byref(params_struct(params)), x.shape[0], _p(x), _p(u), _p(out),
                                            _stream()), "traj_f_cont_batch")
    return out


def numerical_jacobian_batch(x, u, params=None, eps_x=1e-5, eps_u=1e-5):
    x = dev_f64(x, (-1, 6)); u = dev_f64(u, (-1, 2))
    B = x.shape[0]
    Jx = torch.empty((B, 6, 6), dtype=torch.float64, device=x.device)
    Ju = torch.empty((B, 6, 2), dtype=torch.float64, device=x.device)
    f = torch.empty((B, 6), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().traj_numerical_jacobian_batch(C.byref(params_struct(params)), B, _p(x), _p(u),
                                                        float(eps_x), float(eps_u), _p(Jx), _p(Ju), _p(f),
                                                        _stream()), "traj_numerical_jacobian_batch")
    return Jx, Ju, f


def linearize_discretize_batch(xbar, ubar, Ts, params=None):
    x = dev_f64(xbar, (-1, 6)); u = dev_f64(ubar, (-1, 2))
    B = x.shape[0]
    A = torch.empty((B, 6, 6), dtype=torch.float64, device=x.device)
    Bm = torch.empty((B, 6, 2), dtype=torch.float64, device=x.device)
    g = torch.empty((B, 6), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().traj_linearize_discretize_batch(C.byref(params_struct(params)), B, float(Ts), _p(x),
                                                          _p(u), _p(A), _p(Bm), _p(g), _stream()),
               "traj_linearize_discretize_batch")
    return A, Bm, g


def lateral_error_batch(X, Y, Xref, Yref, phiref) -> torch.Tensor:
    ts = [dev_f64(v, (-1,)) for v in (X, Y, Xref, Yref, phiref)]
    out = torch.empty_like(ts[0])
    _lib.check(_lib.lib().traj_lateral_error_batch(ts[0].shape[0], *[_p(t) for t in ts], _p(out), _stream()),
               "traj_lateral_error_batch")
    return out


# ---------------------------------------------------------------- open-loop generators (include/trajgen.h)

def gen_config_struct(model=_lib.GEN_MODEL_TYPE1, Ts=0.01, u_bounds=None, du_bounds=None, clip_state=None,
                      vx_min=None, omega_max=None) -> GenConfig:
    """traj_gen_config: the model's defaults (traj_gen_default_config) with the given fields replaced.
    u_bounds / du_bounds: ((d_lo, d_hi), (delta_lo, delta_hi)) as generation_type1.py:251 writes them;
    a channel with du_bounds (-inf, inf) has no slew limiter."""
    c = _lib.default_gen_config(int(model), float(Ts))
    for ch in range(2):
        if u_bounds is not None:
            c.u_lo[ch], c.u_hi[ch] = (float(v) for v in u_bounds[ch])
        if du_bounds is not None:
            c.du_lo[ch], c.du_hi[ch] = (float(v) for v in du_bounds[ch])
    if clip_state is not None:
        c.clip_state = int(bool(clip_state))
    if vx_min is not None:
        c.vx_min = float(vx_min)
    if omega_max is not None:
        c.omega_max = float(omega_max)
    return c


def simulate_open_loop(x0, u_raw, gen_cfg: GenConfig, params=None) -> dict:
    """B open-loop trajectories in one launch (traj_gen_simulate_batch): slew limiter and output clip of
    generation_type1.py:131-137, :287-288 on u_raw [B,T,2], then the Euler loop of :70-84 from x0 [B,6].
    Returns torch.cuda tensors X [B,T+1,6] (X[:,0] = x0) and U [B,T,2] (the controls that were applied)."""
    x0 = dev_f64(x0, (-1, 6))
    B = x0.shape[0]
    u_raw = dev_f64(u_raw, None, x0.device)
    if u_raw.dim() != 3 or u_raw.shape[0] != B or u_raw.shape[2] != 2:
        raise ValueError(f"u_raw must be [B,T,2] with B = {B}, got {tuple(u_raw.shape)}")
    T = u_raw.shape[1]
    X = torch.empty((B, T + 1, 6), dtype=torch.float64, device=x0.device)
    U = torch.empty((B, T, 2), dtype=torch.float64, device=x0.device)
    _lib.check(_lib.lib().traj_gen_simulate_batch(C.byref(params_struct(params)), C.byref(gen_cfg), B, T, _p(x0),
                                                  _p(u_raw), _p(X), _p(U), _stream()), "traj_gen_simulate_batch")
    return dict(X=X, U=U)


def set_gen_store_form(form: int) -> None:
    """Experiments and tests: the kernel form of the following simulate_open_loop calls (_lib.GEN_FORM_DEFAULT /
    GEN_FORM_STAGED / GEN_FORM_DIRECT, traj_gen_debug_store_form).  Results do not depend on it."""
    _lib.check(_lib.lib().traj_gen_debug_store_form(int(form)), "traj_gen_debug_store_form")


def fsm_rules_struct(rules=None) -> FsmRules:
    """traj_gen_fsm_rules from a generation_type2.ControlRules (or anything with its fields; None: the defaults).
    The two mode distributions of generation_type2.py:109-112 go in as Generator.choice forms them:
    cdf = p.cumsum() / p.cumsum()[-1]."""
    if isinstance(rules, FsmRules):
        return rules
    r = _lib.default_fsm_rules()
    if rules is not None:
        r.v_turn_max, r.v_high = float(rules.v_turn_max), float(rules.v_high)
        r.delta_straight_noise = float(rules.delta_straight_noise)
        for i in range(2):
            r.d_range[i] = float(rules.d_range[i])
            r.delta_turn_range[i] = float(rules.delta_turn_range[i])
    for name, p in (("cdf_after_turn", [0.5, 0.5]), ("cdf_any", [0.35, 0.35, 0.15, 0.15])):
        cdf = np.asarray(p, dtype=np.float64).cumsum()
        cdf /= cdf[-1]
        for i, v in enumerate(cdf):
            getattr(r, name)[i] = float(v)
    return r


def simulate_piecewise(x0, rng_state, T, Ts=0.01, rules=None, params=None, want_rng_state=False) -> dict:
    """B type-2 trajectories of T steps in one launch (traj_gen_piecewise_batch): the state-machine controller of
    generation_type2.py:95-157 on each trajectory's own numpy stream, and the Euler loop of :180-187, from x0 [B,6].
    rng_state [B,4] uint64: np.random.PCG64(seed + i).state as (state >> 64, state & M, inc >> 64, inc & M)
    (generation_type2.pcg64_states; or its int64 CUDA tensor of the same bits).  Returns torch.cuda tensors X [B,T+1,6], U [B,T,2], mode [B,T] uint8 (codes of
    _lib.FSM_MODES) and, with want_rng_state, rng_state [B,4] int64 (the bits of the uint64 words) after the last draw."""
    x0 = dev_f64(x0, (-1, 6))
    B, T = x0.shape[0], int(T)
    if torch.is_tensor(rng_state):      # already on the device (generation_type2.pcg64_states with a device)
        if tuple(rng_state.shape) != (B, 4) or rng_state.dtype != torch.int64:
            raise ValueError(f"rng_state must be [B,4] int64 (the uint64 words' bits) with B = {B}")
        st = rng_state.to(x0.device).contiguous()
    else:
        st = np.ascontiguousarray(rng_state, dtype=np.uint64)
        if st.shape != (B, 4):
            raise ValueError(f"rng_state must be [B,4] uint64 with B = {B}, got {st.shape}")
        st = torch.from_numpy(st.view(np.int64)).to(x0.device)
    X = torch.empty((B, T + 1, 6), dtype=torch.float64, device=x0.device)
    U = torch.empty((B, T, 2), dtype=torch.float64, device=x0.device)
    mode = torch.empty((B, T), dtype=torch.uint8, device=x0.device)
    st_out = torch.empty_like(st) if want_rng_state else None
    cfg = gen_config_struct(_lib.GEN_MODEL_TYPE2, Ts)
    rc = _lib.lib().traj_gen_piecewise_batch(C.byref(params_struct(params)), C.byref(cfg),
                                             C.byref(fsm_rules_struct(rules)), B, T, _p(x0), _p(st), _p(X), _p(U),
                                             _p(mode), _p(st_out), _stream())
    _lib.check(rc, "traj_gen_piecewise_batch")
    out = dict(X=X, U=U, mode=mode)
    if want_rng_state:
        out["rng_state"] = st_out
    return out


def rng_draw_batch(rng_state, n, kind) -> tuple:
    """Tests of csrc/gen_rng.h: every one of the B streams rng_state [B,4] uint64 draws n values of `kind`
    (_lib.RNG_RAW -> uint64, RNG_DOUBLE / RNG_NORMAL -> float64) on the GPU.  Returns (draws [B,n], states [B,4]
    uint64) as numpy arrays."""
    dev = require_gpu()
    st = np.ascontiguousarray(rng_state, dtype=np.uint64)
    B = st.shape[0]
    st_d = torch.from_numpy(st.view(np.int64)).to(dev)
    out = torch.empty((B, int(n)), dtype=torch.int64, device=dev)
    st_out = torch.empty_like(st_d)
    _lib.check(_lib.lib().traj_gen_rng_draw_batch(B, int(n), int(kind), _p(st_d), _p(out), _p(st_out), _stream()),
               "traj_gen_rng_draw_batch")
    h = out.cpu().numpy()
    return (h.view(np.uint64) if kind == _lib.RNG_RAW else h.view(np.float64)), st_out.cpu().numpy().view(np.uint64)


def rng_draw_host(state, n, kind) -> tuple:
    """The same header on the CPU (traj_gen_rng_draw_host): n draws from one stream state [4] uint64."""
    st = np.ascontiguousarray(state, dtype=np.uint64).reshape(4)
    out = np.empty(int(n), dtype=np.uint64 if kind == _lib.RNG_RAW else np.float64)
    st_out = np.empty(4, dtype=np.uint64)
    _lib.check(_lib.lib().traj_gen_rng_draw_host(C.c_void_p(st.ctypes.data), int(kind), int(n),
                                                 C.c_void_p(out.ctypes.data), C.c_void_p(st_out.ctypes.data)),
               "traj_gen_rng_draw_host")
    return out, st_out


# ---------------------------------------------------------------- MPC step

def _outputs(B, N, device):
    f64 = dict(dtype=torch.float64, device=device)
    return dict(u_cmd=torch.empty((B, 2), **f64), status=torch.empty(B, dtype=torch.int32, device=device),
                objective=torch.empty(B, **f64), X_opt=torch.empty((B, 6, N + 1), **f64),
                U_opt=torch.empty((B, 2, N), **f64), iters=torch.empty(B, dtype=torch.int32, device=device),
                polished=torch.empty(B, dtype=torch.int32, device=device))


_WS = {}


# horizons from which the row-split kernel runs (traj_debug_split_min_n; the library default TRAJ_SPLIT_MIN_N)
SPLIT_MIN_N = _lib.SPLIT_MIN_N


def set_split_min_n(n_min: int) -> None:
    """Experiments: run the row-split kernel from horizon n_min on (step and closed loop; 21 .. MAX_N + 1, the latter
    sending 20 < N <= MAX_N back to the capacity-80 kernel).  traj_mpc_workspace_bytes does not depend on it."""
    global SPLIT_MIN_N
    _lib.check(_lib.lib().traj_debug_split_min_n(int(n_min)), "traj_debug_split_min_n")
    SPLIT_MIN_N = int(n_min)


def sized_workspace(nbytes: int, device, role: str = "closed_loop") -> torch.Tensor:
    """Cached device workspace of at least nbytes: what the entry point's own query returns for the configuration and
    batch (traj_mpc_step_workspace_bytes, traj_mpc_qp_workspace_bytes, traj_closed_loop_workspace_bytes).  The library
    decides the solver tier and sizes its scratch (csrc/mpc_route.h); nothing here restates that.

    One buffer per (device, stream, role).  The closed loop keeps state in its workspace between calls (the
    warm-start records, the previous launch's order, the step queue), so the one-shot step / QP entry points
    use a buffer of their own ("step"): a state-bound solve between two closed-loop steps on the same stream
    must not overwrite -- or, by growing the cache, replace -- the closed loop's buffer."""
    nbytes = int(nbytes)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, role)
    ws = _WS.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        new = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        if ws is not None:
            new[:ws.numel()].copy_(ws)   # (stream-ordered) what the smaller buffer held stays in place
        ws = new
        _WS[key] = ws
    return ws


def workspace(B: int, N: int, device, extra_bytes: int = 0, role: str = "closed_loop") -> torch.Tensor:
    """sized_workspace of traj_mpc_workspace_bytes(B, N) + extra_bytes (the closed loop's: closed_extra)."""
    return sized_workspace(int(_lib.lib().traj_mpc_workspace_bytes(int(B), int(N))) + int(extra_bytes), device, role)


def mpc_step_batch(x0, u_prev, path_ref, vref, cfg: MpcConfig, params=None, out: dict | None = None) -> dict:
    """B independent mpc_step calls (mpc_6stati.py:120-275) in one launch.

    x0 [B,6], u_prev [B,2], path_ref [B,N+1,3], vref [B,N+1] (float64, any device; moved to the GPU).
    Returns torch.cuda tensors: u_cmd [B,2], status [B] (int codes, see _lib.STATUS_STRINGS),
    objective [B], X_opt [B,6,N+1], U_opt [B,2,N], iters [B], polished [B]."""
    N = cfg.N
    x0 = dev_f64(x0, (-1, 6))
    B = x0.shape[0]
    dev = x0.device
    u_prev = dev_f64(u_prev, (B, 2), dev)
    path_ref = dev_f64(path_ref, (B, N + 1, 3), dev)
    vref = dev_f64(vref, (B, N + 1), dev)
    o = out if out is not None else _outputs(B, N, dev)
    ws = sized_workspace(_lib.lib().traj_mpc_step_workspace_bytes(C.byref(cfg), B), dev, role="step")
    _lib.check(_lib.lib().traj_mpc_step_batch(
        C.byref(params_struct(params)), C.byref(cfg), B, _p(x0), _p(u_prev), _p(path_ref), _p(vref),
        _p(o["u_cmd"]), _p(o["status"]), _p(o["objective"]), _p(o["X_opt"]), _p(o["U_opt"]), _p(o["iters"]),
        _p(o["polished"]), _p(ws), ws.numel() * 8, _stream()), "traj_mpc_step_batch")
    return o


def mpc_qp_batch(x0, u_prev, path_ref, vref, Ad, Bd, g, cfg: MpcConfig, params=None) -> dict:
    """The QP half of mpc_step (:180-275) with the linearization given: Ad [B,N,6,6], Bd [B,N,6,2], g [B,N,6]."""
    N = cfg.N
    x0 = dev_f64(x0, (-1, 6))
    B = x0.shape[0]
    dev = x0.device
    args = [dev_f64(u_prev, (B, 2), dev), dev_f64(path_ref, (B, N + 1, 3), dev), dev_f64(vref, (B, N + 1), dev),
            dev_f64(Ad, (B, N, 6, 6), dev), dev_f64(Bd, (B, N, 6, 2), dev), dev_f64(g, (B, N, 6), dev)]
    o = _outputs(B, N, dev)
    need = int(_lib.lib().traj_mpc_qp_workspace_bytes(C.byref(cfg), B))
    ws = sized_workspace(need, dev, role="step") if need else None   # (the register-resident kernels take none)
    _lib.check(_lib.lib().traj_mpc_qp_batch(
        C.byref(params_struct(params)), C.byref(cfg), B, _p(x0), *[_p(a) for a in args],
        _p(o["u_cmd"]), _p(o["status"]), _p(o["objective"]), _p(o["X_opt"]), _p(o["U_opt"]), _p(o["iters"]),
        _p(o["polished"]), _p(ws) if ws is not None else None, need, _stream()), "traj_mpc_qp_batch")
    return o


# ---------------------------------------------------------------- closed loop (MPC/main.py)

def d_steady_state(v, params=None):
    """MPC/main.py:9-18 (host arithmetic on a scalar: initial u_prev of the closed loop)."""
    p = dict(REFERENCE_PARAMS)
    p.update(params or {})
    return (p["Cr0"] + p["Cr2"] * v ** 2) / (p["Cm1"] - p["Cm2"] * v)


def vref_ramp(N, Ts, v0=0.8, v_cruise=2.0, tramp=2.0) -> np.ndarray:
    """MPC/main.py:28-32 vref_profile_ramp_cruise."""
    t = np.arange(N + 1) * Ts
    return v0 + (v_cruise - v0) * np.clip(t / tramp, 0.0, 1.0)


def spline_natural(xk, yk):
    """Natural cubic spline piece coefficients (a, b, c, d) per interval, as in oracle/ and DESIGN.md."""
    xk = np.asarray(xk, dtype=np.float64)
    yk = np.asarray(yk, dtype=np.float64)
    n = len(xk)
    h = np.diff(xk)
    M = np.zeros(n)
    if n > 2:
        A = np.zeros((n - 2, n - 2))
        rhs = np.zeros(n - 2)
        for i in range(1, n - 1):
            if i > 1:
                A[i - 1, i - 2] = h[i - 1]
            A[i - 1, i - 1] = 2.0 * (h[i - 1] + h[i])
            if i < n - 2:
                A[i - 1, i] = h[i]
            rhs[i - 1] = 6.0 * ((yk[i + 1] - yk[i]) / h[i] - (yk[i] - yk[i - 1]) / h[i - 1])
        M[1:-1] = np.linalg.solve(A, rhs)
    coef = np.zeros((n - 1, 4))
    coef[:, 0] = yk[:-1]
    coef[:, 1] = (yk[1:] - yk[:-1]) / h - h * (2.0 * M[:-1] + M[1:]) / 6.0
    coef[:, 2] = M[:-1] / 2.0
    coef[:, 3] = (M[1:] - M[:-1]) / (6.0 * h)
    return coef


def spline_natural_stacked(xk, yk):
    """spline_natural for G knot sets of one length at once: xk, yk [G,n] -> coef [G,n-1,4].  The same systems, filled
    with array operations, go through one np.linalg.solve on the stacked [G,n-2,n-2] matrices (LAPACK factors each
    matrix as the per-matrix call does), and the columns are spline_natural's expressions: the same bits
    (tests/test_workload_host.py holds that)."""
    xk = np.asarray(xk, dtype=np.float64)
    yk = np.asarray(yk, dtype=np.float64)
    G, n = xk.shape
    h = np.diff(xk, axis=1)
    M = np.zeros((G, n))
    if n > 2:
        A = np.zeros((G, n - 2, n - 2))
        r = np.arange(n - 2)
        A[:, r, r] = 2.0 * (h[:, :-1] + h[:, 1:])
        A[:, r[1:], r[:-1]] = h[:, 1:-1]
        A[:, r[:-1], r[1:]] = h[:, 1:-1]
        rhs = 6.0 * ((yk[:, 2:] - yk[:, 1:-1]) / h[:, 1:] - (yk[:, 1:-1] - yk[:, :-2]) / h[:, :-1])
        M[:, 1:-1] = np.linalg.solve(A, rhs[:, :, None])[:, :, 0]
    coef = np.zeros((G, n - 1, 4))
    coef[:, :, 0] = yk[:, :-1]
    coef[:, :, 1] = (yk[:, 1:] - yk[:, :-1]) / h - h * (2.0 * M[:, :-1] + M[:, 1:]) / 6.0
    coef[:, :, 2] = M[:, :-1] / 2.0
    coef[:, :, 3] = (M[:, 1:] - M[:, :-1]) / (6.0 * h)
    return coef


def spline_rows(kinds, knots, kmax):
    """PathSet.build's host arrays (nk [B], xk [B,kmax], coef [B,kmax-1,4]): the kind-2 trajectories grouped by knot
    count, one spline_natural_stacked per group; zeros elsewhere."""
    kinds = np.asarray(kinds)
    B = len(kinds)
    xk = np.zeros((B, kmax))
    coef = np.zeros((B, kmax - 1, 4))
    nk = np.zeros(B, np.int32)
    idx = np.nonzero(kinds == 2)[0]
    lens = np.array([len(knots[b][0]) for b in idx], dtype=np.int64)
    for n in np.unique(lens):
        g = idx[lens == n]
        kx = np.array([knots[b][0] for b in g], dtype=np.float64).reshape(len(g), n)
        ky = np.array([knots[b][1] for b in g], dtype=np.float64).reshape(len(g), n)
        nk[g] = n
        xk[g, :n] = kx
        coef[g, :n - 1] = spline_natural_stacked(kx, ky)
    return nk, xk, coef


def spline_coef_host(kinds, nk, xk, yk):
    """csrc/spline.h on the CPU (traj_gen_spline_coef_host): kinds [B], nk [B], xk / yk [B,kmax] -> numpy
    (coef [B,kmax-1,4], flag [B]), the arrays PathSet.build_device computes on the GPU, bit for bit."""
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    nk = np.ascontiguousarray(nk, dtype=np.int32)
    xk = np.ascontiguousarray(xk, dtype=np.float64)
    yk = np.ascontiguousarray(yk, dtype=np.float64)
    B, kmax = xk.shape
    if kinds.shape != (B,) or nk.shape != (B,) or yk.shape != (B, kmax):
        raise ValueError(f"kinds, nk must be [B] and yk [B,kmax] with xk's B = {B}, kmax = {kmax}")
    coef = np.empty((B, max(kmax - 1, 0), 4))
    flag = np.empty(B, dtype=np.int32)
    _lib.check(_lib.lib().traj_gen_spline_coef_host(B, kmax, _p(kinds), _p(nk), _p(xk), _p(yk), _p(coef), _p(flag)),
               "traj_gen_spline_coef_host")
    return coef, flag


@dataclass
class PathSet:
    """Per-trajectory reference geometry on the device (traj_paths).

    kind 0: y = c0 + c1 x + c2 x^2 + c3 x^3 (parabola of MPC/main.py:64-66: c2 = 0.1)
    kind 1: y = c0 sin(c1 x + c2) + c3      (sinusoid of MPC/README.md:73-76: c0 = 0.5, c1 = 0.5)
    kind 2: natural cubic spline through nk knots (linear extrapolation outside)."""
    kind: torch.Tensor
    pc: torch.Tensor
    nk: torch.Tensor
    xk: torch.Tensor
    coef: torch.Tensor

    @property
    def B(self):
        return self.kind.shape[0]

    def struct(self) -> Paths:
        s = Paths()
        s.kmax = int(self.xk.shape[1])
        s.kind, s.pc, s.nk, s.xk, s.coef = (t.data_ptr() for t in (self.kind, self.pc, self.nk, self.xk, self.coef))
        return s

    @staticmethod
    def build(kinds, pcs, knots=None, device=None) -> "PathSet":
        """kinds [B] ints, pcs [B,4], knots: list of (xk, yk) (None for kind 0/1)."""
        dev = require_gpu(device)
        B = len(kinds)
        kmax = max([2] + [len(k[0]) for k in (knots or []) if k is not None])
        nk, xk, coef = spline_rows(kinds, knots, kmax)
        return PathSet(kind=torch.as_tensor(np.asarray(kinds, np.int32), device=dev),
                       pc=torch.as_tensor(np.asarray(pcs, np.float64).reshape(B, 4), device=dev),
                       nk=torch.as_tensor(nk, device=dev), xk=torch.as_tensor(xk, device=dev),
                       coef=torch.as_tensor(coef, device=dev))

    @staticmethod
    def build_device(kinds, pcs, nk, xk, yk, device=None, check=True) -> "PathSet":
        """build from arrays, the coefficients computed on the GPU (traj_gen_spline_coef_batch, csrc/spline.h): kinds
        [B], pcs [B,4], nk [B] knots per trajectory, xk / yk [B,kmax] knot abscissae / ordinates (tensors or arrays;
        rows of kind 0 / 1 and entries past nk are not read).  No host loop.  The coefficients agree with build's to rounding
        (Thomas algorithm against LAPACK's LU), not bit for bit.
        check: read the kernel's flags back (synchronizes) and raise ValueError naming the first kind-2 trajectory with
        nk < 2, nk > kmax, knots that do not strictly increase or a value that is not finite."""
        dev = require_gpu(device)
        kind = torch.as_tensor(kinds, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        B = kind.shape[0]
        nk = torch.as_tensor(nk, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        xk = dev_f64(xk, None, dev)
        yk = dev_f64(yk, None, dev)
        if xk.dim() != 2 or xk.shape[0] != B or xk.shape[1] < 2 or yk.shape != xk.shape or nk.shape[0] != B:
            raise ValueError(f"xk, yk must be [B,kmax] with B = {B}, kmax >= 2 and nk [B]; got {tuple(xk.shape)}, "
                             f"{tuple(yk.shape)}, {tuple(nk.shape)}")
        kmax = xk.shape[1]
        coef = torch.empty((B, kmax - 1, 4), dtype=torch.float64, device=dev)
        flag = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().traj_gen_spline_coef_batch(B, kmax, _p(kind), _p(nk), _p(xk), _p(yk), _p(coef), _p(flag),
                                                         _stream()), "traj_gen_spline_coef_batch")
        if check:
            bad = torch.nonzero(flag)
            if bad.numel():
                b = int(bad[0])
                raise ValueError(f"PathSet.build_device: trajectory {b}: nk = {int(nk[b])} with kmax = {kmax}, or its "
                                 "knots do not strictly increase, or a knot or ordinate is not finite")
        return PathSet(kind=kind, pc=dev_f64(pcs, (B, 4), dev), nk=nk, xk=xk, coef=coef)


def ref_window_batch(paths: PathSet, x_start, vref, N, Ts) -> torch.Tensor:
    """MPC/main.py:51-68 for B trajectories -> path_ref [B,N+1,3]."""
    xs = dev_f64(x_start, (-1,))
    B = xs.shape[0]
    vr = dev_f64(vref, (B, N + 1), xs.device)
    out = torch.empty((B, N + 1, 3), dtype=torch.float64, device=xs.device)
    ps = paths.struct()
    _lib.check(_lib.lib().traj_ref_window_batch(C.byref(ps), B, int(N), float(Ts), _p(xs), _p(vr), _p(out),
                                                _stream()), "traj_ref_window_batch")
    return out


def closed_extra(B: int, cfg: MpcConfig) -> int:
    """Bytes the closed loop needs past traj_mpc_workspace_bytes, by traj_closed_loop_workspace_bytes: the scratch of
    the long-horizon kernel or the general solver (with its window and u_cmd) where cfg runs on one of them."""
    L = _lib.lib()
    need = int(L.traj_closed_loop_workspace_bytes(C.byref(cfg), int(B)))
    return max(0, need - int(L.traj_mpc_workspace_bytes(int(B), int(cfg.N))))


_dev, _closed_extra = dev_f64, closed_extra   # their earlier, private names: callers written against them keep working


def speed_reference(vref, B, N, device, vref_step, need, what):
    """(tensor, vref_row, vref_len, vref_step) of the _sched entry points for either form of a speed reference.  Shapes
    are checked first, on the host (ValueError); a contiguous float64 device tensor of the right shape passes untouched.
    vref_step 0: vref [N+1] (expanded to B rows) or [B,N+1], the same every step -> ([B,N+1], N + 1, N + 1, 0).
    vref_step 1: a schedule sampled at Ts, [L] (one shared row: vref_row = 0, never tiled) or [B,L], L >= need."""
    if vref_step not in (0, 1):
        raise ValueError(f"{what}: vref_step must be 0 (the same window every step) or 1 (a schedule sampled at Ts), "
                         f"got {vref_step!r}")
    shape = tuple(np.shape(vref))
    ready = torch.is_tensor(vref) and vref.is_cuda and vref.dtype == torch.float64 and vref.is_contiguous()
    if vref_step == 0:
        if shape not in ((N + 1,), (1, N + 1), (B, N + 1)):
            raise ValueError(f"{what}: vref must be [N+1] or [B,N+1] with B = {B}, N = {N}, got {shape}")
        if not (ready and shape == (B, N + 1)):
            vref = dev_f64(vref, (-1, N + 1), device)
            if vref.shape[0] != B:
                vref = vref.expand(B, N + 1).contiguous()
        return vref, N + 1, N + 1, 0
    if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] != B):
        raise ValueError(f"{what}: a speed schedule is [L] or [B,L] with B = {B}, got {shape}")
    if shape[-1] < need:
        raise ValueError(f"{what}: the schedule holds {shape[-1]} samples, the call reads {need}")
    L = int(shape[-1])
    return (vref if ready else dev_f64(vref, None, device)), (0 if len(shape) == 1 else L), L, 1


def closed_loop_step(x, u_prev, paths: PathSet, vref, cfg: MpcConfig, params=None, t=0, hist_x=None, hist_u=None,
                     status=None, iters=None, vref_step=0):
    """One step of MPC/main.py:85-101 for all B trajectories; x [B,6], u_prev [B,2] updated in place.
    vref_step=1: vref is a speed schedule [L] or [B,L], L >= t + N + 1, and this step reads vref[b, t + k], k = 0..N
    (traj_closed_loop_step_sched, which serves both forms); 0 (default): vref [N+1] or [B,N+1], the same at every
    step."""
    B = x.shape[0]
    vr, row, L, vs = speed_reference(vref, B, cfg.N, x.device, vref_step, int(t) + cfg.N + 1, "closed_loop_step")
    ps = paths.struct()
    T = hist_u.shape[1] if hist_u is not None else 0
    ws = workspace(B, cfg.N, x.device, closed_extra(B, cfg))
    _lib.check(_lib.lib().traj_closed_loop_step_sched(
        C.byref(params_struct(params)), C.byref(cfg), C.byref(ps), B, _p(x), _p(u_prev), _p(vr), row, L, vs, int(t),
        int(T), _p(hist_x), _p(hist_u), _p(status), _p(iters), _p(ws), ws.numel() * 8, _stream()),
        "traj_closed_loop_step_sched")


def closed_loop_run(x, u_prev, paths: PathSet, vref, cfg: MpcConfig, params=None, t0=0, steps=1, hist_x=None,
                    hist_u=None, status=None, iters=None, check=True, vref_step=0):
    """Steps t0 .. t0+steps-1 of MPC/main.py:85-101 in ONE fused launch (traj_closed_loop_run), bit-identical
    to `steps` closed_loop_step calls; x, u_prev updated in place; status / iters [steps, B].
    check: synchronize and raise RuntimeError if the run lost an instance hand-off (traj_closed_loop_check).
    vref_step=1: vref is a speed schedule [L] or [B,L], L >= t0 + steps + N, and step t reads vref[b, t + k], k = 0..N
    (traj_closed_loop_run_sched, which serves both forms: still one launch); 0 (default): vref [N+1] or [B,N+1], the
    same at every step."""
    B = x.shape[0]
    vr, row, L, vs = speed_reference(vref, B, cfg.N, x.device, vref_step, int(t0) + int(steps) + cfg.N,
                                     "closed_loop_run")
    ps = paths.struct()
    T = hist_u.shape[1] if hist_u is not None else 0
    ws = workspace(B, cfg.N, x.device, closed_extra(B, cfg))
    _lib.check(_lib.lib().traj_closed_loop_run_sched(
        C.byref(params_struct(params)), C.byref(cfg), C.byref(ps), B, _p(x), _p(u_prev), _p(vr), row, L, vs,
        int(t0), int(steps), int(T), _p(hist_x), _p(hist_u), _p(status), _p(iters), _p(ws), ws.numel() * 8,
        _stream()), "traj_closed_loop_run_sched")
    if check:   # synchronizes: a lost instance hand-off raises instead of returning stale trajectories
        _lib.check(_lib.lib().traj_closed_loop_check(_p(ws), ws.numel() * 8, B, cfg.N, _stream()),
                   "traj_closed_loop_run_sched")


def run_closed_loop(x0, u0, paths: PathSet, vref, T, cfg: MpcConfig, params=None, record=True, fused=True,
                    vref_step=0) -> dict:
    """T closed-loop steps (MPC/main.py:85-101) for B trajectories, all on the device: one fused launch
    (closed_loop_run), or one launch sequence per step (fused=False; identical results).

    vref_step=0 (default): vref [N+1] or [B,N+1], read anew at every step, as main.py:87 rebuilds its profile inside
    the loop.  vref_step=1: vref is a speed schedule over the run, [L] (shared by all trajectories, passed as one row)
    or [B,L] with L >= T + N, sampled at Ts: step t takes vref[b, t : t + N + 1] for its window and its q_vx rows.
    Returns X [B,T+1,6] (X[:,0] = x0), U [B,T,2], status [T,B], iters [T,B] (torch.cuda)."""
    B = int(np.shape(x0)[0]) if len(np.shape(x0)) == 2 else 1
    vr = speed_reference(vref, B, cfg.N, None, vref_step, int(T) + cfg.N, "run_closed_loop")[0]
    x = dev_f64(x0, (B, 6)).clone()
    dev = x.device
    u = dev_f64(u0, (B, 2), dev).clone()
    hx = torch.empty((B, T + 1, 6), dtype=torch.float64, device=dev) if record else None
    hu = torch.empty((B, T, 2), dtype=torch.float64, device=dev) if record else None
    if record:
        hx[:, 0] = x
    st = torch.empty((T, B), dtype=torch.int32, device=dev)
    it = torch.empty((T, B), dtype=torch.int32, device=dev)
    if fused:
        closed_loop_run(x, u, paths, vr, cfg, params, 0, T, hx, hu, st, it, vref_step=vref_step)
    else:
        for t in range(T):
            closed_loop_step(x, u, paths, vr, cfg, params, t, hx, hu, st[t], it[t], vref_step=vref_step)
    return dict(X=hx, U=hu, status=st, iters=it, x=x, u=u)


# ---------------------------------------------------------------- the evaluation after the loop (MPC/main.py:107-121)

STATS_SERIES = ("d", "delta", "dd", "ddelta", "e_c", "e_phi", "e_v")   # TRAJ_STATS_SERIES
STATS_FIELDS = ("n", "mean", "M2", "min", "max")                       # TRAJ_STATS_FIELDS
_N, _MEAN, _M2, _MIN, _MAX = range(5)


def stats_views(pooled) -> dict:
    """The named views of a [7,5] record: n, mean, std = sqrt(M2 / n) (numpy's ddof = 0), min, max, each a dict keyed
    by series name."""
    pooled = np.asarray(pooled, dtype=np.float64).reshape(len(STATS_SERIES), len(STATS_FIELDS))
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(pooled[:, _M2] / pooled[:, _N])
    cols = dict(n=pooled[:, _N], mean=pooled[:, _MEAN], std=std, min=pooled[:, _MIN], max=pooled[:, _MAX])
    return {k: {s: float(v[i]) for i, s in enumerate(STATS_SERIES)} for k, v in cols.items()}


def closed_loop_stats(run, paths: PathSet, vref, u0, T=None, mask=None, vref_step=0) -> dict:
    """MPC/main.py:107-121 for a finished run (what run_closed_loop returns, recorded), on the device: the statistics of
    d and delta, of their rates and of the three tracking errors over steps 0 .. T-1 (default: all recorded steps),
    per trajectory and pooled (traj_closed_loop_stats, traj_closed_loop_stats_pool; the series: include/trajmpc.h).

    u0 [B,2]: u_prev before step 0 (the u0 run_closed_loop took); vref as run_closed_loop takes it; mask [B] (bool or
    0 / 1): False leaves a trajectory out of the pooled record.
    vref_step=1: vref is the run's speed schedule [L] or [B,L], L >= T + 1 (what run_closed_loop took), and e_v at step
    t is vx(X[b,t+1]) - vref[b,t+1], the speed the next step's window starts from (traj_closed_loop_stats_sched).
    Returns per_traj [B,7,5] and fails [B] (device tensors), pooled [7,5] (numpy: n, mean, M2, min, max per series),
    fails_total (int) and the views of stats_views(pooled).  The read-back of pooled and the count (one copy of 288
    bytes) is the only synchronisation."""
    X, U = run["X"], run["U"]
    if X is None or U is None:
        raise ValueError("closed_loop_stats needs the recorded histories (run_closed_loop(record=True))")
    dev = X.device if torch.is_tensor(X) and X.is_cuda else None
    # (a schedule's horizon only bounds the row's length: every N >= 1 with N + 1 <= L gives the same record)
    N = 1 if vref_step != 0 else int((np.shape(vref) or (0,))[-1]) - 1
    vr, row, L, vs = speed_reference(vref, int(np.shape(U)[0]), N, dev, vref_step,
                                     (int(np.shape(U)[1]) if T is None else int(T)) + 1, "closed_loop_stats")
    X = dev_f64(X, None, dev)
    dev = X.device
    U = dev_f64(U, None, dev)
    B, hist_T = U.shape[0], U.shape[1]
    if U.dim() != 3 or U.shape[2] != 2 or tuple(X.shape) != (B, hist_T + 1, 6):
        raise ValueError(f"X must be [B,T+1,6] and U [B,T,2], got {tuple(X.shape)}, {tuple(U.shape)}")
    T = hist_T if T is None else int(T)
    if paths.B != B:
        raise ValueError(f"paths holds {paths.B} trajectories, the run {B}")
    if B > 0 and not 1 <= T <= hist_T:
        raise ValueError(f"T = {T}: the statistics take 1 .. {hist_T} of the {hist_T} recorded steps")
    u0 = dev_f64(u0, (B, 2), dev)
    st = run.get("status")
    if st is not None:
        st = torch.as_tensor(st).to(device=dev, dtype=torch.int32).contiguous()
        if st.dim() != 2 or st.shape[0] < T or st.shape[1] != B:
            raise ValueError(f"status must be [>=T,B] = [>={T},{B}], got {tuple(st.shape)}")
    rec = torch.empty((B, len(STATS_SERIES), len(STATS_FIELDS)), dtype=torch.float64, device=dev)
    fails = torch.empty(B, dtype=torch.int32, device=dev)
    ps = paths.struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_closed_loop_stats_sched(
            C.byref(ps), B, N, T, hist_T, _p(X), _p(U), _p(u0), _p(vr), row, L, vs, _p(st), _p(rec), _p(fails),
            _stream()), "traj_closed_loop_stats_sched")
    pooled, fails_total = pool_stats(rec, fails, mask)
    return dict(per_traj=rec, fails=fails, pooled=pooled, fails_total=fails_total, **stats_views(pooled))


def pool_stats(per_traj, fails=None, mask=None) -> tuple:
    """The records per_traj [B,7,5] of the trajectories mask keeps (default: all) merged into one on the device
    (traj_closed_loop_stats_pool), with the sum of their fails [B] (default: 0).  Returns (pooled [7,5] numpy,
    fails_total int): one copy of 288 bytes, which synchronises.  Nothing kept: n = 0, the other fields NaN."""
    S, F = len(STATS_SERIES), len(STATS_FIELDS)
    rec = dev_f64(per_traj, (-1, S, F), per_traj.device if torch.is_tensor(per_traj) and per_traj.is_cuda else None)
    B, dev = rec.shape[0], rec.device
    if fails is not None:
        fails = torch.as_tensor(fails).to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    if mask is not None:
        mask = torch.as_tensor(mask).to(device=dev).reshape(B).to(torch.uint8).contiguous()
    if B == 0:     # no launch
        pooled = np.full((S, F), np.nan)
        pooled[:, _N] = 0.0
        return pooled, 0
    out = torch.empty(S * F + 1, dtype=torch.int64, device=dev)   # the pooled record's bits, then the count
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_closed_loop_stats_pool(
            B, _p(rec), _p(fails), _p(mask), _p(out), C.c_void_p(out.data_ptr() + 8 * S * F), _stream()),
            "traj_closed_loop_stats_pool")
    host = out.cpu().numpy()
    return host[:S * F].view(np.float64).reshape(S, F).copy(), int(host[S * F])


def path_fn_host(kinds, pcs, knots=None):
    """The reference geometry of PathSet.build's arguments as the host specification's path function:
    path_fn(b, xs) -> (y(xs), atan(y'(xs))) for an array xs, in numpy (path_eval's rule, workload.spline_eval's)."""
    kinds = np.asarray(kinds)
    pcs = np.asarray(pcs, dtype=np.float64).reshape(len(kinds), 4)
    coefs = {b: spline_natural(*knots[b]) for b in range(len(kinds)) if kinds[b] == 2}

    def path_fn(b, xs):
        xs = np.asarray(xs, dtype=np.float64)
        c = pcs[b]
        if kinds[b] == 0:
            return c[0] + xs * (c[1] + xs * (c[2] + xs * c[3])), np.arctan(c[1] + xs * (2.0 * c[2] + xs * 3.0 * c[3]))
        if kinds[b] == 1:
            a = c[1] * xs + c[2]
            return c[0] * np.sin(a) + c[3], np.arctan(c[0] * c[1] * np.cos(a))
        xk, cf = np.asarray(knots[b][0], dtype=np.float64), coefs[b]
        nk = len(xk)
        j = np.clip(np.searchsorted(xk, xs, side="right") - 1, 0, nk - 2)
        q = cf[j]
        t = xs - xk[j]
        y = q[:, 0] + t * (q[:, 1] + t * (q[:, 2] + t * q[:, 3]))
        dy = q[:, 1] + t * (2.0 * q[:, 2] + t * 3.0 * q[:, 3])
        lo, hi = xs <= xk[0], xs >= xk[-1]
        h = xk[-1] - xk[-2]
        qe = cf[nk - 2]
        ye = qe[0] + h * (qe[1] + h * (qe[2] + h * qe[3]))
        se = qe[1] + h * (2.0 * qe[2] + h * 3.0 * qe[3])
        y = np.where(lo, cf[0, 0] + cf[0, 1] * (xs - xk[0]), np.where(hi, ye + se * (xs - xk[-1]), y))
        dy = np.where(lo, cf[0, 1], np.where(hi, se, dy))
        return y, np.arctan(dy)

    return path_fn


def closed_loop_series_host(X, U, u0, path_fn, vref0) -> np.ndarray:
    """The seven series of closed_loop_stats as numpy arrays [B,7,T]: X [B,T+1,6], U [B,T,2], u0 [B,2];
    path_fn(b, xs [T]) -> (Y* [T], phi* [T]), the path's ordinate and heading at abscissae xs; vref0 [B] or a scalar,
    the first entry of each trajectory's speed reference, or [B,T]: the speed e_v at step t is taken against, column
    t (for a schedule S read with vref_step = 1 that is S[:, 1:T+1])."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    B, T = U.shape[0], U.shape[1]
    u0 = np.asarray(u0, dtype=np.float64).reshape(B, 2)
    v0 = np.asarray(vref0, dtype=np.float64)
    if v0.ndim == 2:
        if v0.shape != (B, T):
            raise ValueError(f"vref0 per step must be [B,T] = [{B},{T}], got {v0.shape}")
    else:
        v0 = np.broadcast_to(v0, (B,))
    ser = np.empty((B, len(STATS_SERIES), T))
    ser[:, 0:2] = U.transpose(0, 2, 1)
    ser[:, 2:4] = (U - np.concatenate([u0[:, None, :], U[:, :-1]], axis=1)).transpose(0, 2, 1)
    for b in range(B):
        x = X[b, 1:T + 1]
        ys, phis = path_fn(b, x[:, 0])
        ys, phis = np.asarray(ys, dtype=np.float64), np.asarray(phis, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ser[b, 4] = np.sin(phis) * (x[:, 0] - x[:, 0]) - np.cos(phis) * (x[:, 1] - ys)   # X* = X
            ser[b, 5] = np.arctan2(np.sin(x[:, 2] - phis), np.cos(x[:, 2] - phis))
        ser[b, 6] = x[:, 3] - v0[b]
    return ser


def _record_host(v) -> np.ndarray:
    """(n, mean, M2, min, max) of the samples v by numpy's own reductions; NaN past n if one is not finite."""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return np.array([0.0, np.nan, np.nan, np.nan, np.nan])
    if not np.isfinite(v).all():
        return np.array([float(v.size), np.nan, np.nan, np.nan, np.nan])
    return np.array([float(v.size), np.mean(v), np.std(v) ** 2 * v.size, np.min(v), np.max(v)])


def closed_loop_stats_host(X, U, u0, path_fn, vref0, status=None, mask=None) -> dict:
    """The numpy specification of closed_loop_stats (arguments: closed_loop_series_host; status [>=T,B] or None): plain
    np.mean / np.std / np.min / np.max per series, per trajectory and over the kept trajectories' samples together;
    a series with a non-finite sample gets NaN in mean, M2, min and max, as on the device.
    Returns numpy per_traj [B,7,5], fails [B], pooled [7,5], fails_total, series [B,7,T] and stats_views(pooled)."""
    ser = closed_loop_series_host(X, U, u0, path_fn, vref0)
    B, S, T = ser.shape
    keep = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(B).astype(bool)
    per = np.array([[_record_host(ser[b, s]) for s in range(S)] for b in range(B)]).reshape(B, S, len(STATS_FIELDS))
    pooled = np.array([_record_host(ser[keep, s]) for s in range(S)])
    if status is None:
        fails = np.zeros(B, dtype=np.int64)
    else:
        fails = (np.asarray(status)[:T] >= 2).sum(axis=0).astype(np.int64)
    return dict(per_traj=per, fails=fails, pooled=pooled, fails_total=int(fails[keep].sum()), series=ser,
                **stats_views(pooled))


def merge_stats(a, b) -> np.ndarray:
    """Chan's merge of two records [7,5] (or [...,7,5], broadcast): the record of the two sample sets together, in
    float64.  n, min and max are exact; a side with n = 0 leaves the other unchanged; NaN fields stay NaN.  How
    launches, shards and ranks combine their pooled records."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    na, nb = a[..., _N], b[..., _N]
    n = na + nb
    with np.errstate(invalid="ignore", divide="ignore"):
        w = nb / n
        delta = b[..., _MEAN] - a[..., _MEAN]
        out = np.stack([n, a[..., _MEAN] + delta * w, (a[..., _M2] + b[..., _M2]) + (delta * delta) * (na * w),
                        np.minimum(a[..., _MIN], b[..., _MIN]), np.maximum(a[..., _MAX], b[..., _MAX])], axis=-1)
    out = np.where((nb == 0)[..., None], a, out)
    return np.where(((na == 0) & (nb != 0))[..., None], b, out)


def mpc_stats(pooled) -> dict:
    """The four numbers generation_type1 takes as `stats` (generation_type1.py:250's mpc_stats) from a pooled record
    [7,5], or from what closed_loop_stats returns."""
    if isinstance(pooled, dict):
        pooled = pooled["pooled"]
    v = stats_views(pooled)
    return {"d_mean": v["mean"]["d"], "d_std": v["std"]["d"], "delta_mean": v["mean"]["delta"],
            "delta_std": v["std"]["delta"]}

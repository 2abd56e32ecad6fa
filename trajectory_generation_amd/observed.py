"""The MPC closed loop on a state estimate (include/trajobs.h): the controller is fed an estimator's output, the plant
runs on the true state, and the estimator sees noisy measurements of it (X, Y, vx, vy, omega; phi is not measured).

run_closed_loop_observed   the loop with the float64 EKF in it ("ekf"), with the true state ("truth": the plain closed
                           loop, bit for bit) or with any callable estimator (one step per call of it)
knet_estimator             a callable around a KalmanNetNN's own step
estimation_errors          MSE of the estimate and of the measurements against the true state

Per step the library copies x_hat into a control copy, runs traj_closed_loop_step_sched on it unchanged (every solver
tier, the warm start, the speed schedule) and then one observe kernel: plant, measurement, estimator, history rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p, stream as _stream
from .batch import MpcConfig, PathSet, dev_f64, params_struct, require_gpu, sized_workspace, speed_reference
from .knet import EKF_P0, EKF_Q, EKF_R, limits_struct

HR = (0, 1, 3, 4, 5)               # the measured rows of the state (vehicle_model.py:136-153)
ESTIMATORS = {"truth": _lib.OBS_TRUTH, "ekf": _lib.OBS_EKF}
_ROLE = "closed_loop_observed"     # a workspace of its own: never the cached "closed_loop" buffer


def set_obs_lanes(lanes: int) -> None:
    """The EKF step's form in the observe kernel and in ekf_step (traj_debug_obs_lanes): 1 = one thread per filter,
    16 = sixteen lanes per filter; the same bits either way."""
    rc = _lib.lib().traj_debug_obs_lanes(int(lanes))
    if rc != _lib.TRAJ_OK:
        raise ValueError(f"lanes must be 1 or 16, got {lanes!r}")


def obs_config(estimator, Q=EKF_Q, R=EKF_R) -> _lib.ObsConfig:
    """traj_obs_config for an estimator name (or TRAJ_OBS_* code) and the EKF's diagonal Q [6], R [5]."""
    code = ESTIMATORS.get(estimator, estimator) if isinstance(estimator, str) else estimator
    if code not in (_lib.OBS_TRUTH, _lib.OBS_EKF, _lib.OBS_EXTERNAL):
        raise ValueError(f"estimator must be 'ekf', 'truth' or a callable, got {estimator!r}")
    q, r = np.asarray(Q, dtype=np.float64).reshape(-1), np.asarray(R, dtype=np.float64).reshape(-1)
    if q.shape != (6,) or r.shape != (5,):
        raise ValueError(f"Q must hold 6 entries and R 5, got {q.shape[0]} and {r.shape[0]}")
    if not (q >= 0.0).all():
        raise ValueError("Q: every entry must be >= 0")
    if not (r > 0.0).all():
        raise ValueError("R: every entry must be > 0")
    o = _lib.ObsConfig()
    o.estimator = int(code)
    o.Q[:] = q.tolist()
    o.R[:] = r.tolist()
    return o


def _check_shapes(x0, u0, xhat0, noise, P0, T):
    """The argument checks that need no GPU; returns B."""
    sx = tuple(np.shape(x0))
    if len(sx) != 2 or sx[1] != 6:
        raise ValueError(f"x0 must be [B,6], got {sx}")
    B = sx[0]
    if int(T) < 0:
        raise ValueError(f"T must be >= 0, got {T!r}")
    if tuple(np.shape(u0)) != (B, 2):
        raise ValueError(f"u0 must be [B,2] = [{B},2], got {tuple(np.shape(u0))}")
    if xhat0 is not None and tuple(np.shape(xhat0)) != (B, 6):
        raise ValueError(f"xhat0 must be [B,6] = [{B},6], got {tuple(np.shape(xhat0))}")
    if noise is not None and tuple(np.shape(noise)) != (B, int(T), 5):
        raise ValueError(f"noise must be [B,T,5] = [{B},{int(T)},5], got {tuple(np.shape(noise))}")
    if tuple(np.shape(P0)) not in ((6,), (B, 6, 6)):
        raise ValueError(f"P0 must be [6] (a diagonal) or [B,6,6], got {tuple(np.shape(P0))}")
    return B


class _Loop:
    """The buffers of one observed run and its two calls into the library."""

    def __init__(self, x0, u0, paths, vref, T, cfg, params, o, xhat0, noise, P0, vref_step):
        # (first: a bad reference is a ValueError before anything touches the GPU)
        self.vr, self.row, self.L, self.vs = speed_reference(vref, int(np.shape(x0)[0]), cfg.N, None, vref_step,
                                                             int(T) + cfg.N, "run_closed_loop_observed")
        x = dev_f64(x0, (-1, 6))
        dev = x.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.B, self.T, self.cfg, self.paths, self.o, self.dev = x.shape[0], int(T), cfg, paths, o, dev
        B = self.B
        self.x0 = x.clone()
        self.u0 = dev_f64(u0, (B, 2), dev).clone()
        self.xhat0 = self.x0.clone() if xhat0 is None else dev_f64(xhat0, (B, 6), dev).clone()
        P0t = torch.as_tensor(np.asarray(P0, dtype=np.float64), **f64)
        self.P0 = (torch.diag_embed(P0t.expand(B, 6)) if P0t.dim() == 1 else P0t).contiguous().clone()
        self.noise = None if noise is None else dev_f64(noise, (B, self.T, 5), dev)
        self.p = params_struct(params)
        # (a missing limit is limits_struct's KeyError; no params at all misses the first)
        self.lim = limits_struct(params if isinstance(params, dict) else {}) if o.estimator == _lib.OBS_EKF else None
        self.x, self.xhat, self.u, self.P = (torch.empty_like(self.x0), torch.empty_like(self.x0),
                                             torch.empty_like(self.u0), torch.empty_like(self.P0))
        self.X = torch.empty((B, self.T + 1, 6), **f64)
        self.Xhat = torch.empty((B, self.T + 1, 6), **f64)
        self.Y = torch.empty((B, self.T, 5), **f64)
        self.U = torch.empty((B, self.T, 2), **f64)
        self.status = torch.empty((self.T, B), dtype=torch.int32, device=dev)
        self.iters = torch.empty((self.T, B), dtype=torch.int32, device=dev)
        self.ps = paths.struct()
        need = int(_lib.lib().traj_closed_loop_obs_workspace_bytes(C.byref(cfg), B))
        if need == 0 and B > 0:
            raise ValueError("run_closed_loop_observed: invalid MPC configuration")
        self.ws = sized_workspace(need, dev, _ROLE)

    def reset(self):
        """The run's initial state (stream-ordered copies into the buffers the launches read)."""
        self.x.copy_(self.x0)
        self.xhat.copy_(self.xhat0)
        self.u.copy_(self.u0)
        self.P.copy_(self.P0)
        self.X[:, 0] = self.x0
        self.Xhat[:, 0] = self.xhat0

    def _common(self):
        lim = C.byref(self.lim) if self.lim is not None else None
        return (C.byref(self.p), C.byref(self.cfg), C.byref(self.ps), lim, C.byref(self.o), self.B, _p(self.x),
                _p(self.xhat), _p(self.P), _p(self.u), _p(self.vr), self.row, self.L, self.vs, _p(self.noise))

    def _tail(self, st, it):
        return (self.T, _p(self.X), _p(self.Xhat), _p(self.U), _p(self.Y), _p(st), _p(it), _p(self.ws),
                self.ws.numel() * 8, _stream())

    def run(self, t0, steps):
        _lib.check(_lib.lib().traj_closed_loop_obs_run(*self._common(), int(t0), int(steps),
                                                       *self._tail(self.status[t0:], self.iters[t0:])),
                   "traj_closed_loop_obs_run")

    def step(self, t):
        _lib.check(_lib.lib().traj_closed_loop_obs_step(*self._common(), int(t),
                                                        *self._tail(self.status[t], self.iters[t])),
                   "traj_closed_loop_obs_step")

    def result(self):
        return dict(X=self.X, Xhat=self.Xhat, Y=self.Y, U=self.U, status=self.status, iters=self.iters, x=self.x,
                    xhat=self.xhat, u=self.u, P=self.P)


def run_closed_loop_observed(x0, u0, paths: PathSet, vref, T, cfg: MpcConfig, params=None, estimator="ekf", xhat0=None,
                             noise=None, P0=EKF_P0, Q=EKF_Q, R=EKF_R, vref_step=0, graph=False) -> dict:
    """T closed-loop steps for B trajectories with the controller on a state estimate, all on the device.

    estimator  "ekf": the float64 EKF over the clamped vehicle model (knet.ekf_run's filter, one step per loop step;
               its clamp limits are params' LIMIT_KEYS -- a missing key is a KeyError); "truth": the estimate is the true
               state (run_closed_loop, bit for bit); a callable est(t, y [B,5], u [B,2]) -> x_hat [B,6] (float64, real
               units), called once per step with that step's measurement and applied command.
    xhat0      the initial estimate [B,6] (default x0); noise [B,T,5] added to the measurements (default none);
               P0 [6] (a diagonal) or [B,6,6], Q [6], R [5]: the EKF's covariances.
    vref, vref_step  as run_closed_loop takes them.
    graph      capture the whole run once with torch.cuda.graph and replay it (not with a callable); the result then
               carries "replay": a function that runs the captured loop again from the initial state, into the same
               tensors.
    Returns X [B,T+1,6] (truth, X[:,0] = x0), Xhat [B,T+1,6] (Xhat[:,0] = xhat0; Xhat[:,t] is what step t's controller
    saw), Y [B,T,5] (Y[:,t] measures X[:,t+1]), U [B,T,2], status / iters [T,B], and the final x, xhat, u, P.
    closed_loop_stats takes the result as it takes run_closed_loop's."""
    B = _check_shapes(x0, u0, xhat0, noise, P0, T)
    external = callable(estimator)
    if external and graph:
        raise ValueError("graph=True captures library launches only: not with a callable estimator")
    o = obs_config(_lib.OBS_EXTERNAL if external else estimator, Q, R)
    loop = _Loop(x0, u0, paths, vref, T, cfg, params, o, xhat0, noise, P0, vref_step)
    with torch.cuda.device(loop.dev):
        if external:
            loop.reset()
            for t in range(loop.T):
                loop.step(t)
                xh = torch.as_tensor(estimator(t, loop.Y[:, t], loop.U[:, t]), dtype=torch.float64, device=loop.dev)
                if tuple(xh.shape) != (B, 6):
                    raise ValueError(f"the estimator must return [B,6] = [{B},6], got {tuple(xh.shape)}")
                loop.xhat.copy_(xh)
                loop.Xhat[:, t + 1] = loop.xhat
            return loop.result()
        if not graph:
            loop.reset()
            loop.run(0, loop.T)
            return loop.result()
        # every kernel of the sequence loaded before the capture (two steps: the second launches the order kernel)
        loop.reset()
        loop.run(0, min(2, loop.T))
        torch.cuda.synchronize(loop.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loop.run(0, loop.T)

        def replay():
            loop.reset()
            g.replay()
            return out

        out = loop.result()
        out["replay"] = replay
        return replay()


def ekf_step(params: dict, Ts: float, x, P, u, y, Q=EKF_Q, R=EKF_R) -> None:
    """One EKF predict / update in place on x [B,6], P [B,6,6] (float64 device tensors) with u [B,2], y [B,5]
    (traj_ekf_step_f64): the estimator of run_closed_loop_observed alone."""
    dev = require_gpu(x.device if torch.is_tensor(x) and x.is_cuda else None)
    B = x.shape[0]
    if (not torch.is_tensor(x) or not torch.is_tensor(P) or x.dtype != torch.float64 or P.dtype != torch.float64
            or tuple(x.shape) != (B, 6) or tuple(P.shape) != (B, 6, 6) or not x.is_contiguous()
            or not P.is_contiguous()):
        raise ValueError("ekf_step updates contiguous float64 device tensors x [B,6] and P [B,6,6] in place")
    f64 = lambda a, s: torch.as_tensor(a, dtype=torch.float64, device=dev).reshape(s).contiguous()   # noqa: E731
    uu, yy, q, r = f64(u, (B, 2)), f64(y, (B, 5)), f64(Q, (6,)), f64(R, (5,))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_ekf_step_f64(C.byref(params_struct(params)), C.byref(limits_struct(params)),
                                                float(Ts), B, _p(x), _p(P), _p(uu), _p(yy), _p(q), _p(r), _stream()),
                   "traj_ekf_step_f64")


def knet_estimator(model, x0):
    """est(t, y, u) for run_closed_loop_observed around a built KalmanNetNN's own step: InitSequence from x0 [B,6] (real
    units), init_hidden_KNet, then one KNet_step per call, in eval mode and without gradients.  The normalisation is the
    model's: y is normalised with its y statistics, the posterior comes back in real units (float64)."""
    x0 = torch.as_tensor(x0, dtype=torch.float32, device=model.device).reshape(-1, 6)
    B = x0.shape[0]
    model.eval()
    with torch.no_grad():
        model.batch_size = B
        model.init_hidden_KNet()
        model.InitSequence(model._renorm_x(x0.unsqueeze(2)), 0)   # (the model's bridge works on [B,C,1])

    def est(t, y, u):
        with torch.no_grad():
            yn = model._renorm_y(y.to(model.device, torch.float32).reshape(B, 5, 1))
            post = model.KNet_step(yn.contiguous(), u.to(model.device, torch.float32).reshape(B, 2, 1).contiguous())
            return model._denorm_x(post.reshape(B, 6, 1)).reshape(B, 6).to(torch.float64)

    return est


def estimation_errors(run, skip=0) -> dict:
    """MSE of the estimate and of the measurements against the truth over steps >= skip of a finished run: Xhat[:,t+1]
    and Y[:,t] both against X[:,t+1].  Per channel (mse_est_ch [6], mse_meas_ch [5]) and pooled over the five measured
    channels (mse_est, mse_meas; mse_est_all pools all six states); ratio = mse_est / mse_meas."""
    X, Xhat, Y = (np.asarray(run[k].detach().cpu() if torch.is_tensor(run[k]) else run[k], dtype=np.float64)
                  for k in ("X", "Xhat", "Y"))
    T = Y.shape[1]
    if X.shape != Xhat.shape or X.shape[1] != T + 1 or X.shape[2] != 6 or Y.shape[2] != 5 or Y.shape[0] != X.shape[0]:
        raise ValueError(f"X, Xhat must be [B,T+1,6] and Y [B,T,5], got {X.shape}, {Xhat.shape}, {Y.shape}")
    skip = int(skip)
    if not 0 <= skip < max(T, 1):
        raise ValueError(f"skip = {skip}: the run has {T} steps")
    hr = list(HR)
    e_est = (Xhat[:, 1 + skip:] - X[:, 1 + skip:]) ** 2
    e_meas = (Y[:, skip:] - X[:, 1 + skip:, hr]) ** 2
    est_ch, meas_ch = e_est.mean(axis=(0, 1)), e_meas.mean(axis=(0, 1))
    mse_est, mse_meas = float(e_est[:, :, hr].mean()), float(e_meas.mean())
    return dict(mse_est_ch=est_ch, mse_meas_ch=meas_ch, mse_est=mse_est, mse_meas=mse_meas,
                mse_est_all=float(e_est.mean()), ratio=mse_est / mse_meas if mse_meas > 0 else float("nan"))

"""Synthetic closed-loop workloads (BASELINE.json configs).

The reference's only closed-loop caller is MPC/main.py:85-101 (one parabola, one trajectory).
These generators build B independent trajectories of the same loop with the geometry defined
in DESIGN.md "reference paths":
  * spline  (config 2 / 4): natural cubic spline y(x) through 11 knots x in [-6, 34] m (4 m
    spacing), y ~ U(-1, 1) m; linear extrapolation outside the knots.  Deviation from SURVEY.md
    8(d) config 2 (6 knots on x in [0, 12]), deliberate: a trajectory starts at X in [-2, 2] and,
    on the 0.8 -> 2.0 m/s ramp, covers about 17 m in the bench's 205 steps and 22 m in the dataset's
    240 -- with knots on [0, 12] only, it would start on the extrapolated line and spend most of the
    run past the last knot tracking a straight line (trivially easy QPs); the 4 m spacing keeps the
    curvature of 6 knots over 12 m (2.4 m spacing) within a factor of 2.
  * mixed   (config 3): 50 % sinusoid y = A sin(w x + phase) (A = 0.5, w = 0.5 of MPC/README.md:75,
    jittered +-20 %), 50 % parabola y = a x^2 (a = 0.1 of main.py:64-66, drawn in [0.05, 0.15]).
Initial state per trajectory (ranges of generation_type1.py:260-265 / main.py:77): X ~ U(-2, 2),
Y = y(X) + U(-0.5, 0.5), phi = atan(y'(X)) + U(-0.2, 0.2), vx ~ U(0.4, 1.5), vy ~ U(-0.05, 0.05),
omega ~ U(-1, 1); u_prev = [d_ss(vx), 0] (main.py:20-22).  vref = the main.py:28-32 ramp
(0.8 -> 2.0 m/s over 2 s) over the horizon, re-used every step (main.py:87).
Trajectory `tid` draws from numpy.random.default_rng([seed, tid]) so shards are reproducible
for any rank count.
make_track_workload puts the trajectories on shared closed circuits instead (track.TrackSet): headings
all round the compass, which no y(x) path gives.
make_workload is the specification; make_workload_device builds the same workload and its PathSet on the GPU in
one launch (csrc/workload.hip: the same streams and draws, no per-trajectory Python), opt-in.
"""
from __future__ import annotations

import numpy as np

from .batch import d_steady_state, spline_natural, vref_ramp

SPLINE_KNOTS_X = np.linspace(-6.0, 34.0, 11)


def spline_eval(xk, coef, x):
    """y, dy/dx of the natural spline (same rule as the kernel's path_eval)."""
    nk = len(xk)
    if x <= xk[0]:
        return coef[0, 0] + coef[0, 1] * (x - xk[0]), coef[0, 1]
    if x >= xk[-1]:
        q = coef[nk - 2]
        h = xk[-1] - xk[-2]
        ye = q[0] + h * (q[1] + h * (q[2] + h * q[3]))
        se = q[1] + h * (2 * q[2] + h * 3 * q[3])
        return ye + se * (x - xk[-1]), se
    j = min(int(np.searchsorted(xk, x, side="right")) - 1, nk - 2)
    q = coef[j]
    t = x - xk[j]
    return q[0] + t * (q[1] + t * (q[2] + t * q[3])), q[1] + t * (2 * q[2] + t * 3 * q[3])


def _initial_state(rng, y, dy):
    X = rng.uniform(-2.0, 2.0)
    yy, dd = y(X), dy(X)
    return np.array([X, yy + rng.uniform(-0.5, 0.5), np.arctan(dd) + rng.uniform(-0.2, 0.2),
                     rng.uniform(0.4, 1.5), rng.uniform(-0.05, 0.05), rng.uniform(-1.0, 1.0)])


def make_workload(B, N=20, Ts=0.05, kind="spline", seed=0, id_offset=0):
    """Returns dict(kinds [B], pcs [B,4], knots list, x0 [B,6], u0 [B,2], vref [N+1], ids [B])."""
    kinds, pcs, knots, x0 = [], [], [], []
    for i in range(B):
        tid = id_offset + i
        rng = np.random.default_rng([seed, tid])
        if kind == "spline":
            yk = rng.uniform(-1.0, 1.0, len(SPLINE_KNOTS_X))
            coef = spline_natural(SPLINE_KNOTS_X, yk)
            x0.append(_initial_state(rng, lambda x: spline_eval(SPLINE_KNOTS_X, coef, x)[0],
                                     lambda x: spline_eval(SPLINE_KNOTS_X, coef, x)[1]))
            kinds.append(2); pcs.append([0.0] * 4); knots.append((SPLINE_KNOTS_X.copy(), yk))
        elif kind == "mixed":
            if tid % 2 == 0:
                A = 0.5 * rng.uniform(0.8, 1.2); w = 0.5 * rng.uniform(0.8, 1.2); ph = rng.uniform(0, 2 * np.pi)
                c = [A, w, ph, 0.0]
                x0.append(_initial_state(rng, lambda x: A * np.sin(w * x + ph), lambda x: A * w * np.cos(w * x + ph)))
                kinds.append(1)
            else:
                a = rng.uniform(0.05, 0.15)
                c = [0.0, 0.0, a, 0.0]
                x0.append(_initial_state(rng, lambda x: a * x * x, lambda x: 2 * a * x))
                kinds.append(0)
            pcs.append(c); knots.append(None)
        elif kind == "parabola":
            a = 0.1
            x0.append(np.array([0.0, 0.5, 0.0, 1.0, 0.0, 0.0]))   # main.py:77
            kinds.append(0); pcs.append([0.0, 0.0, a, 0.0]); knots.append(None)
        else:
            raise ValueError(kind)
    x0 = np.array(x0)
    u0 = np.stack([np.array([d_steady_state(v), 0.0]) for v in x0[:, 3]])
    return dict(kinds=np.array(kinds, np.int32), pcs=np.array(pcs, np.float64), knots=knots, x0=x0, u0=u0,
                vref=vref_ramp(N, Ts), ids=np.arange(id_offset, id_offset + B))


def track_knots(seed, i, knots=16):
    """Circuit i of make_track_workload, [knots,2], from numpy.random.default_rng([seed, i]): theta_j = 2 pi j / knots,
    r_j = R0 (1 + a2 cos(2 theta_j + psi2) + a3 cos(3 theta_j + psi3)), knots (r cos theta, asp r sin theta) with
    R0 ~ U(1.5, 2.5), a2, a3 ~ U(0, 0.12), psi2, psi3 ~ U(0, 2 pi), asp ~ U(0.6, 1), drawn in that order; an odd i has
    its knots reversed (a clockwise track)."""
    rng = np.random.default_rng([seed, i])
    R0, a2, a3 = rng.uniform(1.5, 2.5), rng.uniform(0.0, 0.12), rng.uniform(0.0, 0.12)
    psi2, psi3, asp = rng.uniform(0.0, 2 * np.pi), rng.uniform(0.0, 2 * np.pi), rng.uniform(0.6, 1.0)
    th = 2.0 * np.pi * np.arange(knots) / knots
    r = R0 * (1.0 + a2 * np.cos(2.0 * th + psi2) + a3 * np.cos(3.0 * th + psi3))
    P = np.stack([r * np.cos(th), asp * r * np.sin(th)], axis=1)
    return np.ascontiguousarray(P[::-1]) if i % 2 else P


def make_track_workload(B, N=20, Ts=0.02, seed=0, n_tracks=8, knots=16, id_offset=0):
    """B trajectories on n_tracks shared closed circuits (track.TrackSet; the loop is track.run_closed_loop_track).

    Track i: track_knots(seed, i, knots) -- the same circuits whatever B and id_offset are.  Trajectory tid = id_offset
    + b drives on track tid % n_tracks and draws from numpy.random.default_rng([seed, n_tracks + tid]), in this order: a
    uniform place s on its track, a lateral offset U(-0.1, 0.1) m along the left normal, a heading offset U(-0.2, 0.2)
    rad from the track's, v ~ U(0.8, 1.5) (vx = vref = v, held constant over the run), vy ~ U(-0.05, 0.05),
    omega ~ U(-1, 1); u0 = (d_steady_state(v), 0).
    Returns dict(knots: list of [knots,2], track_of [B], s0 [B], x0 [B,6], u0 [B,2], vref [B,N+1], ids [B])."""
    from .track import TrackSet
    if int(n_tracks) < 1 or int(knots) < 3 or int(B) < 0:
        raise ValueError(f"need n_tracks >= 1, knots >= 3, B >= 0; got {n_tracks}, {knots}, {B}")
    kn = [track_knots(seed, i, knots) for i in range(n_tracks)]
    ts = TrackSet.build(kn)
    ids = np.arange(id_offset, id_offset + B)
    track_of = (ids % n_tracks).astype(np.int32)
    x0, s0 = np.zeros((B, 6)), np.zeros(B)
    for b, tid in enumerate(ids):
        rng = np.random.default_rng([seed, n_tracks + int(tid)])
        i = int(track_of[b])
        s0[b] = rng.uniform(0.0, ts.L[i])
        X, Y, dX, dY = (float(v) for v in ts.eval_host(i, s0[b]))
        nrm = np.hypot(dX, dY)
        off = rng.uniform(-0.1, 0.1)
        x0[b] = [X - off * dY / nrm, Y + off * dX / nrm, np.arctan2(dY, dX) + rng.uniform(-0.2, 0.2),
                 rng.uniform(0.8, 1.5), rng.uniform(-0.05, 0.05), rng.uniform(-1.0, 1.0)]
    u0 = np.stack([np.array([d_steady_state(v), 0.0]) for v in x0[:, 3]]) if B else np.zeros((0, 2))
    return dict(knots=kn, track_of=track_of, s0=s0, x0=x0, u0=u0, vref=np.repeat(x0[:, 3:4], N + 1, axis=1), ids=ids)


def _workload_args(B, kind, seed, id_offset):
    """(workload code, seed words uint32 [ns], kmax) of the library's workload builders, refusing what
    numpy.random.default_rng([seed, tid]) refuses (a negative int) and what the library does not take."""
    from . import _lib
    if kind not in _lib.WORKLOADS:
        raise ValueError(kind)
    seed, id_offset = int(seed), int(id_offset)
    if seed < 0 or id_offset < 0:
        raise ValueError("expected non-negative integer")      # numpy's words
    ns = max(1, (seed.bit_length() + 31) // 32)
    if ns > _lib.WORKLOAD_MAX_SEED_WORDS:
        raise ValueError(f"seed has {ns} 32-bit words; the device builder takes {_lib.WORKLOAD_MAX_SEED_WORDS}")
    if int(B) < 1 or id_offset + int(B) > 2 ** 63 - 1:
        raise ValueError(f"B = {B}, id_offset = {id_offset}: need B >= 1 and ids below 2^63")
    words = np.array([(seed >> (32 * k)) & 0xffffffff for k in range(ns)], dtype=np.uint32)
    return _lib.WORKLOADS[kind], words, (_lib.WORKLOAD_SPLINE_KNOTS if kind == "spline" else 2)


def workload_rows_host(B, kind="spline", seed=0, id_offset=0, params=None):
    """make_workload's loop on the CPU through the library (traj_gen_workload_host: the text of the GPU builder,
    csrc/workload.hip).  Returns numpy arrays kinds [B], pcs [B,4], nk [B], xk / yk [B,kmax], coef [B,kmax-1,4],
    x0 [B,6], u0 [B,2].  For the tests; make_workload stays the specification."""
    import ctypes as C

    from . import _lib
    from .batch import params_struct
    code, words, kmax = _workload_args(B, kind, seed, id_offset)
    B = int(B)
    o = dict(kinds=np.empty(B, np.int32), pcs=np.empty((B, 4)), nk=np.empty(B, np.int32), xk=np.empty((B, kmax)),
             yk=np.empty((B, kmax)), coef=np.empty((B, kmax - 1, 4)), x0=np.empty((B, 6)), u0=np.empty((B, 2)))
    _lib.check(_lib.lib().traj_gen_workload_host(C.byref(params_struct(params)), code, _lib.ptr(words), len(words),
                                                 int(id_offset), B, kmax, *[_lib.ptr(a) for a in o.values()]),
               "traj_gen_workload_host")
    return o


def make_workload_device(B, N=20, Ts=0.05, kind="spline", seed=0, id_offset=0, device=None, params=None):
    """make_workload built on the GPU in one launch (traj_gen_workload_batch): no per-trajectory Python.

    Returns make_workload's keys with kinds [B], pcs [B,4], x0 [B,6], u0 [B,2] as device tensors, knots=None,
    yk [B,kmax] (the spline kind's knot ordinates; zeros otherwise) and paths, the PathSet of the workload (its
    coefficients by csrc/spline.h); vref [N+1] and ids [B] stay numpy.  The draws, kinds, pcs, knots, X, vx, vy, omega
    are make_workload's bit for bit; u0 within 2 ulp (v * v against the host's v ** 2); Y, phi and the coefficients to
    rounding (Thomas against LAPACK, the device's atan and sincos against the host's).  params: vehicle parameters of
    u0's steady-state throttle (default: the reference's, as make_workload).  ValueError for a negative seed or
    id_offset, as numpy raises, and for a seed of more than six 32-bit words."""
    import ctypes as C

    import torch

    from . import _lib
    from .batch import PathSet, params_struct, require_gpu
    dev = require_gpu(device)
    code, words, kmax = _workload_args(B, kind, seed, id_offset)
    B = int(B)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    kinds, nk = torch.empty(B, **i32), torch.empty(B, **i32)
    pcs, xk, yk = torch.empty((B, 4), **f64), torch.empty((B, kmax), **f64), torch.empty((B, kmax), **f64)
    coef, x0, u0 = torch.empty((B, kmax - 1, 4), **f64), torch.empty((B, 6), **f64), torch.empty((B, 2), **f64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_gen_workload_batch(
            C.byref(params_struct(params)), code, _lib.ptr(words), len(words), int(id_offset), B, kmax,
            *[_lib.ptr(t) for t in (kinds, pcs, nk, xk, yk, coef, x0, u0)], _lib.stream()), "traj_gen_workload_batch")
    return dict(kinds=kinds, pcs=pcs, knots=None, yk=yk, x0=x0, u0=u0, vref=vref_ramp(N, Ts),
                ids=np.arange(id_offset, id_offset + B), paths=PathSet(kind=kinds, pc=pcs, nk=nk, xk=xk, coef=coef))


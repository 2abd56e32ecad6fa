"""The MPC closed loop on closed tracks (include/trajtrack.h): circuits, hairpins and U-turns, which no y(x) path of
batch.PathSet can describe.

TrackSet                 periodic C2 cubic splines through knots, by cumulative chord length, shared among trajectories
track_project_batch      the place of points on their tracks (global, or local from a previous place)
track_window_batch       the MPC's reference window along a track, its heading unwound onto the vehicle's branch
run_closed_loop_track    T closed-loop steps for B trajectories on the device, optionally as one captured graph
tracking_errors          e_c, e_phi, unwrapped progress and laps of a finished run
track_project_host / track_window_host   the same rules on the CPU (csrc/track.h compiled for the host)

Per step the library launches the track kernel (projection, window, the step's vref slice), traj_mpc_step_batch on them
(every solver tier, unchanged) and the plant kernel.  The rules are in csrc/track.h and DESIGN.md section 7j.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr as _p

MIN_KNOTS = 3


def set_track_lanes(lanes: int) -> None:
    """The track kernel's form (traj_debug_track_lanes): 1 = one thread per trajectory, 16 = sixteen lanes per
    trajectory; the same bits either way."""
    if _lib.lib().traj_debug_track_lanes(int(lanes)) != _lib.TRAJ_OK:
        raise ValueError(f"lanes must be 1 or 16, got {lanes!r}")


def search_struct(search=None) -> _lib.TrackSearch:
    """traj_track_search from None (the defaults: samples 8, back 0.5, fwd 1.0, newton 8), a dict of some of those
    keys, or a struct (passed through)."""
    if isinstance(search, _lib.TrackSearch):
        return search
    s = _lib.TrackSearch()
    _lib.check(_lib.lib().traj_track_default_search(C.byref(s)), "traj_track_default_search")
    for k, v in (search or {}).items():
        if k not in ("samples", "back", "fwd", "newton"):
            raise TypeError(f"unknown search setting {k!r}")
        setattr(s, k, v)
    return s


def periodic_spline(knots):
    """The periodic C2 cubic spline through knots [M,2] (P_M = P_0) by cumulative chord length: (sig [M+1],
    coef [M,2,4]) with piece i of coordinate c  c0 + t (c1 + t (c2 + t c3)),  t = s - sig[i].  The second derivatives
    solve the cyclic tridiagonal system  h[i-1] m[i-1] + 2 (h[i-1] + h[i]) m[i] + h[i] m[i+1] = 6 ((y[i+1] - y[i]) /
    h[i] - (y[i] - y[i-1]) / h[i-1])  (indices mod M); the four columns are batch.spline_natural's.  This is the
    specification of a track."""
    P = np.asarray(knots, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 2 or P.shape[0] < MIN_KNOTS:
        raise ValueError(f"a track needs knots [M,2] with M >= {MIN_KNOTS}, got {P.shape}")
    if not np.isfinite(P).all():
        raise ValueError("a track's knots must be finite")
    M = P.shape[0]
    nxt = np.roll(P, -1, axis=0)
    h = np.hypot(*(nxt - P).T)
    if not (h > 0.0).all():
        raise ValueError("a track's consecutive knots must differ (the wrap pair P_{M-1}, P_0 too)")
    sig = np.concatenate([[0.0], np.cumsum(h)])
    A = np.zeros((M, M))
    for i in range(M):
        A[i, (i - 1) % M] += h[i - 1]
        A[i, i] += 2.0 * (h[i - 1] + h[i])
        A[i, (i + 1) % M] += h[i]
    slope = (nxt - P) / h[:, None]
    m = np.linalg.solve(A, 6.0 * (slope - np.roll(slope, 1, axis=0)))      # [M,2]
    mn = np.roll(m, -1, axis=0)
    coef = np.stack([P, slope - h[:, None] * (2.0 * m + mn) / 6.0, m / 2.0, (mn - m) / (6.0 * h[:, None])], axis=2)
    return sig, coef


class TrackSet:
    """Closed tracks shared among trajectories (traj_tracks): nk [n], sig [n,kmax+1], coef [n,kmax,2,4] and track_of
    [B] or None (track 0 for all).  Built on the host; struct() uploads the arrays to the GPU on first use."""

    def __init__(self, nk, sig, coef, track_of=None, device=None):
        self.nk, self.sig, self.coef = nk, sig, coef
        self.track_of = None if track_of is None else np.ascontiguousarray(track_of, dtype=np.int32)
        self.device = device
        self._dev = {}

    @staticmethod
    def build(knots, track_of=None, device=None) -> "TrackSet":
        """knots: a list of [M,2] arrays, one per track (M >= 3, may differ); track_of [B] ints or None."""
        if len(knots) < 1:
            raise ValueError("TrackSet.build needs at least one track")
        pieces = [periodic_spline(k) for k in knots]
        n, kmax = len(pieces), max(len(s) - 1 for s, _ in pieces)
        nk = np.array([len(s) - 1 for s, _ in pieces], dtype=np.int32)
        sig, coef = np.zeros((n, kmax + 1)), np.zeros((n, kmax, 2, 4))
        for i, (s, c) in enumerate(pieces):
            sig[i, :len(s)] = s
            coef[i, :len(c)] = c
        if track_of is not None:
            track_of = np.asarray(track_of)
            if track_of.ndim != 1 or (track_of < 0).any() or (track_of >= n).any():
                raise ValueError(f"track_of must be [B] with entries in 0 .. {n - 1}")
        return TrackSet(nk, sig, coef, track_of, device)

    @property
    def n_tracks(self):
        return int(self.nk.shape[0])

    @property
    def kmax(self):
        return int(self.coef.shape[1])

    @property
    def L(self):
        """The tracks' lengths [n_tracks]."""
        return self.sig[np.arange(self.n_tracks), self.nk]

    def with_track_of(self, track_of) -> "TrackSet":
        """The same tracks for another assignment of trajectories."""
        t = TrackSet(self.nk, self.sig, self.coef, track_of, self.device)
        t._dev = {k: {n: a for n, a in v.items() if n != "track_of"} for k, v in self._dev.items()}
        return t

    def track_index(self, B):
        """track_of as an array [B] (zeros without one)."""
        if self.track_of is None:
            return np.zeros(B, dtype=np.int32)
        if self.track_of.shape[0] != B:
            raise ValueError(f"track_of names {self.track_of.shape[0]} trajectories, the call has {B}")
        return self.track_of

    def _struct(self, arrays, B):
        s = _lib.Tracks()
        s.n_tracks, s.kmax = self.n_tracks, self.kmax
        s.nk, s.sig, s.coef = (_p(a) for a in arrays[:3])
        s.track_of = _p(arrays[3]) if arrays[3] is not None else None
        if arrays[3] is not None and B is not None and arrays[3].shape[0] != B:
            raise ValueError(f"track_of names {arrays[3].shape[0]} trajectories, the call has {B}")
        return s

    def host_struct(self, B=None) -> _lib.Tracks:
        """traj_tracks on host pointers (the _host entry points)."""
        return self._struct((self.nk, self.sig, self.coef, self.track_of), B)

    def struct(self, B=None, device=None) -> _lib.Tracks:
        """traj_tracks on device pointers; the arrays are uploaded once per device and kept."""
        import torch

        from .batch import require_gpu
        dev = require_gpu(device if device is not None else self.device)
        key = str(dev)
        d = self._dev.setdefault(key, {})
        for name in ("nk", "sig", "coef", "track_of"):
            if name not in d:
                a = getattr(self, name)
                d[name] = None if a is None else torch.as_tensor(a, device=dev).contiguous()
        return self._struct((d["nk"], d["sig"], d["coef"], d["track_of"]), B)

    def eval_host(self, i, s):
        """(X, Y, X', Y') of track i at the parameters s (any shape; wrapped): the specification's evaluation."""
        M, L = int(self.nk[i]), float(self.sig[i, self.nk[i]])
        s = np.asarray(s, dtype=np.float64)
        w = s - L * np.floor(s / L)
        w = np.where((w >= L) | (w < 0.0), 0.0, w)
        j = np.clip(np.searchsorted(self.sig[i, :M + 1], w, side="right") - 1, 0, M - 1)
        t = w - self.sig[i, j]
        c = self.coef[i, j]                      # [..., 2, 4]
        val = c[..., 0] + t[..., None] * (c[..., 1] + t[..., None] * (c[..., 2] + t[..., None] * c[..., 3]))
        der = c[..., 1] + t[..., None] * (2.0 * c[..., 2] + t[..., None] * (3.0 * c[..., 3]))
        return val[..., 0], val[..., 1], der[..., 0], der[..., 1]


# ---------------------------------------------------------------- the two geometry calls, on the host

def track_project_host(tracks: TrackSet, xy, s_prev=None, search=None, want_dist2=False):
    """traj_track_project_host: xy [B,>=2] (columns 0, 1), s_prev [B] or None (global) -> s [B] (, dist2 [B])."""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] < 2:
        raise ValueError(f"xy must be [B,2] (or wider rows), got {xy.shape}")
    B = xy.shape[0]
    sp = None if s_prev is None else np.ascontiguousarray(s_prev, dtype=np.float64).reshape(B)
    s, d2 = np.empty(B), (np.empty(B) if want_dist2 else None)
    ts, se = tracks.host_struct(B), search_struct(search)
    _lib.check(_lib.lib().traj_track_project_host(C.byref(ts), C.byref(se), B, _p(xy), xy.shape[1], _p(sp), _p(s),
                                                  _p(d2)), "traj_track_project_host")
    return (s, d2) if want_dist2 else s


def _vref_rows(vref, B, N, xp):
    """vref [N+1] (one shared row) or [B,N+1] -> (array, vref_row)."""
    shape = tuple(np.shape(vref))
    if shape == (N + 1,):
        return xp(vref, (N + 1,)), 0
    if shape == (B, N + 1):
        return xp(vref, (B, N + 1)), N + 1
    raise ValueError(f"vref must be [N+1] or [B,N+1] with B = {B}, N = {N}, got {shape}")


def track_window_host(tracks: TrackSet, s0, vref, N, Ts, phi=None):
    """traj_track_window_host: s0 [B], vref [N+1] or [B,N+1], phi [B] or None -> path_ref [B,N+1,3]."""
    s0 = np.ascontiguousarray(s0, dtype=np.float64).reshape(-1)
    B = s0.shape[0]
    vr, row = _vref_rows(vref, B, N, lambda a, sh: np.ascontiguousarray(a, dtype=np.float64).reshape(sh))
    ph = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64).reshape(B)
    out = np.empty((B, N + 1, 3))
    ts = tracks.host_struct(B)
    _lib.check(_lib.lib().traj_track_window_host(C.byref(ts), B, int(N), float(Ts), _p(s0), _p(ph), _p(vr), row, N + 1,
                                                 0, _p(out)), "traj_track_window_host")
    return out


# ---------------------------------------------------------------- on the device

def track_project_batch(tracks: TrackSet, xy, s_prev=None, search=None, want_dist2=False):
    """traj_track_project_batch: xy [B,>=2] (columns 0, 1: state rows [B,6] pass as they are), s_prev [B] or None
    (global search) -> s [B] (, dist2 [B]) on the device."""
    import torch

    from .batch import dev_f64
    xy = dev_f64(xy, None, xy.device if torch.is_tensor(xy) and xy.is_cuda else tracks.device)
    if xy.dim() != 2 or xy.shape[1] < 2:
        raise ValueError(f"xy must be [B,2] (or wider rows), got {tuple(xy.shape)}")
    B, dev = xy.shape[0], xy.device
    sp = None if s_prev is None else dev_f64(s_prev, (B,), dev)
    s = torch.empty(B, dtype=torch.float64, device=dev)
    d2 = torch.empty(B, dtype=torch.float64, device=dev) if want_dist2 else None
    ts, se = tracks.struct(B, dev), search_struct(search)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_track_project_batch(C.byref(ts), C.byref(se), B, _p(xy), xy.shape[1], _p(sp), _p(s),
                                                       _p(d2), _lib.stream()), "traj_track_project_batch")
    return (s, d2) if want_dist2 else s


def track_window_batch(tracks: TrackSet, s0, vref, N, Ts, phi=None):
    """traj_track_window_batch: s0 [B], vref [N+1] or [B,N+1], phi [B] (the vehicles' headings) or None -> path_ref
    [B,N+1,3] on the device."""
    import torch

    from .batch import dev_f64
    s0 = dev_f64(s0, (-1,), s0.device if torch.is_tensor(s0) and s0.is_cuda else tracks.device)
    B, dev = s0.shape[0], s0.device
    vr, row = _vref_rows(vref, B, N, lambda a, sh: dev_f64(a, sh, dev))
    ph = None if phi is None else dev_f64(phi, (B,), dev)
    out = torch.empty((B, N + 1, 3), dtype=torch.float64, device=dev)
    ts = tracks.struct(B, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().traj_track_window_batch(C.byref(ts), B, int(N), float(Ts), _p(s0), _p(ph), _p(vr), row,
                                                      N + 1, 0, _p(out), _lib.stream()), "traj_track_window_batch")
    return out


def track_plant(x, u_prev, u_cmd, Ts, params=None) -> None:
    """The loop's third launch alone (traj_closed_loop_track_plant): x <- x + Ts f_cont(x, u_cmd), u_prev <- u_cmd, in
    place on contiguous float64 device tensors x [B,6], u_prev [B,2]."""
    import torch

    from .batch import dev_f64, params_struct
    B = x.shape[0]
    uc = dev_f64(u_cmd, (B, 2), x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().traj_closed_loop_track_plant(C.byref(params_struct(params)), float(Ts), B, _p(x),
                                                           _p(u_prev), _p(uc), None, 0, 0, None, None, None,
                                                           _lib.stream()), "traj_closed_loop_track_plant")


_ROLE = "closed_loop_track"     # a workspace of its own: never the cached "closed_loop" or "step" buffer


class _Loop:
    """The buffers of one run on tracks and its two calls into the library."""

    def __init__(self, x0, u0, tracks, vref, T, cfg, params, vref_step, search):
        import torch

        from .batch import dev_f64, params_struct, sized_workspace, speed_reference
        sx = tuple(np.shape(x0))
        if len(sx) != 2 or sx[1] != 6:
            raise ValueError(f"x0 must be [B,6], got {sx}")
        B = sx[0]
        if int(T) < 0:
            raise ValueError(f"T must be >= 0, got {T!r}")
        if tuple(np.shape(u0)) != (B, 2):
            raise ValueError(f"u0 must be [B,2] = [{B},2], got {tuple(np.shape(u0))}")
        tracks.track_index(B)
        # (a bad reference is a ValueError before anything touches the GPU)
        self.vr, self.row, self.L, self.vs = speed_reference(vref, B, cfg.N, tracks.device, vref_step,
                                                             int(T) + cfg.N, "run_closed_loop_track")
        x = dev_f64(x0, (B, 6), tracks.device)
        dev = x.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.B, self.T, self.cfg, self.dev = B, int(T), cfg, dev
        self.x0, self.u0 = x.clone(), dev_f64(u0, (B, 2), dev).clone()
        self.p, self.ts, self.se = params_struct(params), tracks.struct(B, dev), search_struct(search)
        self.x, self.u = torch.empty_like(self.x0), torch.empty_like(self.u0)
        self.s = torch.empty(B, **f64)
        self.X = torch.empty((B, self.T + 1, 6), **f64)
        self.U = torch.empty((B, self.T, 2), **f64)
        self.S = torch.empty((B, self.T + 1), **f64)
        self.hs = torch.empty((B, max(self.T, 1)), **f64)
        self.status = torch.empty((self.T, B), dtype=torch.int32, device=dev)
        self.iters = torch.empty((self.T, B), dtype=torch.int32, device=dev)
        need = int(_lib.lib().traj_closed_loop_track_workspace_bytes(C.byref(cfg), B))
        if need == 0 and B > 0:
            raise ValueError("run_closed_loop_track: invalid MPC configuration")
        self.ws = sized_workspace(need, dev, _ROLE)
        self.tracks = tracks

    def reset(self):
        """The run's initial state (stream-ordered copies into the buffers the launches read)."""
        self.x.copy_(self.x0)
        self.u.copy_(self.u0)
        self.s.fill_(float("nan"))
        self.X[:, 0] = self.x0

    def _common(self):
        return (C.byref(self.p), C.byref(self.cfg), C.byref(self.ts), C.byref(self.se), self.B, _p(self.x), _p(self.u),
                _p(self.s), _p(self.vr), self.row, self.L, self.vs)

    def _tail(self, st, it):
        return (self.T, _p(self.X), _p(self.U), _p(self.hs), _p(st), _p(it), _p(self.ws), self.ws.numel() * 8,
                _lib.stream())

    def run(self, t0, steps):
        _lib.check(_lib.lib().traj_closed_loop_track_run(*self._common(), int(t0), int(steps),
                                                         *self._tail(self.status[t0:], self.iters[t0:])),
                   "traj_closed_loop_track_run")

    def step(self, t):
        _lib.check(_lib.lib().traj_closed_loop_track_step(*self._common(), int(t),
                                                          *self._tail(self.status[t], self.iters[t])),
                   "traj_closed_loop_track_step")

    def finish(self):
        """S from the history rows, and its last column: one more projection, of the final state."""
        if self.T > 0:
            self.S[:, :self.T] = self.hs[:, :self.T]
        _lib.check(_lib.lib().traj_track_project_batch(C.byref(self.ts), C.byref(self.se), self.B, _p(self.x), 6,
                                                       _p(self.s), _p(self.s), None, _lib.stream()),
                   "traj_track_project_batch")
        self.S[:, self.T] = self.s

    def result(self):
        return dict(X=self.X, U=self.U, S=self.S, status=self.status, iters=self.iters, x=self.x, u=self.u)


def run_closed_loop_track(x0, u0, tracks: TrackSet, vref, T, cfg, params=None, vref_step=0, search=None, graph=False,
                          per_step=False) -> dict:
    """T closed-loop steps for B trajectories on closed tracks, all on the device.

    x0 [B,6], u0 [B,2]; tracks: a TrackSet whose track_of names each trajectory's track (None: track 0 for all); vref,
    vref_step as run_closed_loop takes them; search: the projection's settings (search_struct).  Step 0 projects
    globally, every later step locally from the step before.
    graph     capture the whole run once with torch.cuda.graph (a linear chain of launches) and replay it; the result
              then carries "replay": a function that runs the captured loop again from the initial state, into the same
              tensors.
    per_step  one traj_closed_loop_track_step call per step instead of one traj_closed_loop_track_run (the same
              launches).
    Returns X [B,T+1,6] (X[:,0] = x0), U [B,T,2], S [B,T+1] (S[:,t]: the place of X[:,t] on its track; the last column
    is one more projection, of the final state), status / iters [T,B], and the final x, u."""
    import torch
    if graph and per_step:
        raise ValueError("graph=True captures one traj_closed_loop_track_run call: not with per_step")
    loop = _Loop(x0, u0, tracks, vref, T, cfg, params, vref_step, search)
    with torch.cuda.device(loop.dev):
        if not graph:
            loop.reset()
            if per_step:
                for t in range(loop.T):
                    loop.step(t)
            else:
                loop.run(0, loop.T)
            loop.finish()
            return loop.result()
        # every kernel of the sequence loaded before the capture
        loop.reset()
        loop.run(0, min(1, loop.T))
        loop.finish()
        torch.cuda.synchronize(loop.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loop.run(0, loop.T)
            loop.finish()

        def replay():
            loop.reset()
            g.replay()
            return out

        out = loop.result()
        out["replay"] = replay
        return replay()


def tracking_errors(run, tracks: TrackSet) -> dict:
    """Of a finished run (X [B,T+1,6], S [B,T+1]) on its tracks: e_c and e_phi [B,T+1] against the track point and
    heading at S (traj_track_errors_batch, on the GPU; device tensors), progress [B,T+1] -- the unwrapped distance in
    s since step 0: the cumulative sum of the cyclically wrapped differences of S, on the host -- and laps [B] =
    progress[:, -1] / L."""
    import torch

    from .batch import dev_f64
    X = dev_f64(run["X"], None, run["X"].device if torch.is_tensor(run["X"]) and run["X"].is_cuda else tracks.device)
    B, T1 = X.shape[0], X.shape[1]
    S = dev_f64(run["S"], (B, T1), X.device)
    err = torch.empty((B, T1, 2), dtype=torch.float64, device=X.device)
    ts = tracks.struct(B, X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().traj_track_errors_batch(C.byref(ts), B, T1, _p(X), _p(S), _p(err), _lib.stream()),
                   "traj_track_errors_batch")
    progress, laps = progress_host(S.cpu().numpy(), tracks.L[tracks.track_index(B)])
    return dict(e_c=err[:, :, 0], e_phi=err[:, :, 1], progress=progress, laps=laps)


def progress_host(S, L):
    """Unwrapped progress [B,T+1] of the places S [B,T+1] on tracks of lengths L [B], and laps [B]."""
    S, L = np.asarray(S, dtype=np.float64), np.asarray(L, dtype=np.float64).reshape(-1, 1)
    d = np.diff(S, axis=1)
    d = d - L * np.floor(d / L + 0.5)
    progress = np.concatenate([np.zeros((S.shape[0], 1)), np.cumsum(d, axis=1)], axis=1)
    return progress, progress[:, -1] / L[:, 0]

"""Closed tracks on the CPU: TrackSet.build's periodic spline, the projection and the window of csrc/track.h through the
host entry points against the numpy specification (tests/_track_ref.py), the heading's unwinding, the tie rule and the
fallbacks, the argument errors, and csrc/track.h under ASan / UBSan (tests/sanitize/san_track.cpp).  No GPU.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _track_ref as R
from trajectory_generation_amd import _lib
from trajectory_generation_amd import track as TK

HERE = os.path.dirname(os.path.abspath(__file__))
N, TS = 20, 0.02
TWO_PI = R.TWO_PI


def _ccw():
    return TK.TrackSet.build([R.circuit_knots()])


def _spec(ts, i=0):
    M = int(ts.nk[i])
    return ts.sig[i], ts.coef[i], M


# ------------------------------------------------------------------ 1. the spline

@pytest.mark.parametrize("knots", [R.circuit_knots(), R.circuit_knots()[::-1], R.circle_knots(16), R.circle_knots(3),
                                   np.array([[0.0, 0.0], [3.0, 0.2], [2.5, 1.5], [1.0, 1.0], [-0.5, 2.0]])])
def test_spline_is_periodic_c2_and_interpolates(knots):
    """Value, first and second derivative of piece i - 1 at its end equal those of piece i at its start, at every knot,
    the wrap knot included (1e-12 of the coefficients' scale: two Horner evaluations and a dense solve); the pieces
    start on the knots exactly; sig is the cumulative chord length; and the build is the specification's own."""
    ts = TK.TrackSet.build([knots])
    sig, coef, M = _spec(ts)
    assert M == len(knots) and sig[0] == 0.0
    assert np.array_equal(coef[:, :, 0], knots)
    chord = np.hypot(*(np.roll(knots, -1, axis=0) - knots).T)
    assert np.allclose(np.diff(sig[:M + 1]), chord, rtol=0, atol=1e-15 * sig[M])
    scale = np.abs(coef).max()
    for i in range(M):
        prev = (i - 1) % M
        h = sig[prev + 1] - sig[prev]
        end, start = R.eval_piece(coef, prev, float(h)), R.eval_piece(coef, i, 0.0)
        for a, b in zip(end, start):
            assert abs(a - b) <= 1e-12 * max(1.0, scale), (i, a, b)
    rs, rc = R.build(knots)
    assert np.allclose(sig[:M + 1], rs, rtol=0, atol=1e-14) and np.allclose(coef[:M], rc, rtol=0, atol=1e-12 * scale)


def test_spline_on_a_circle_within_the_interpolation_bound():
    """16 knots on a circle of radius 2: per coordinate the spline interpolates R cos / sin(w s), w = (2 pi / M) / chord,
    at uniform spacing h = chord, so |f - s| <= 5/384 h^4 max|f''''| = 5/384 R (2 pi / M)^4 (Hall and Meyer's bound for
    cubic spline interpolation), and the radius errs by at most sqrt(2) of that."""
    Mk, Rad = 16, 2.0
    ts = TK.TrackSet.build([R.circle_knots(Mk, Rad)])
    L = ts.L[0]
    bound = math.sqrt(2.0) * 5.0 / 384.0 * Rad * (2.0 * math.pi / Mk) ** 4
    X, Y, dX, dY = ts.eval_host(0, np.linspace(0.0, L, 4001))
    err = np.abs(np.hypot(X, Y) - Rad).max()
    print(f"circle: radius error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(np.hypot(dX, dY) - 1.0).max() < 0.01      # chord length is close to arc length
    assert abs(L - 2 * Mk * Rad * math.sin(math.pi / Mk)) < 1e-12


def test_track_set_shapes_and_refusals():
    ts = TK.TrackSet.build([R.circle_knots(3), R.circuit_knots(), R.circle_knots(16)], track_of=[0, 1, 2, 1])
    assert ts.n_tracks == 3 and ts.kmax == 16 and ts.nk.tolist() == [3, 12, 16]
    assert ts.sig.shape == (3, 17) and ts.coef.shape == (3, 16, 2, 4) and ts.L.shape == (3,)
    assert (ts.coef[0, 3:] == 0).all() and (ts.sig[0, 4:] == 0).all()
    for bad in ([[0.0, 0.0], [1.0, 0.0]], [[0.0, 0.0], [1.0, 0.0], [1.0, 0.0]], [[0.0, 0.0], [1.0, np.nan], [0.0, 1.0]]):
        with pytest.raises(ValueError):
            TK.TrackSet.build([np.array(bad)])
    with pytest.raises(ValueError):
        TK.TrackSet.build([R.circle_knots(4)], track_of=[0, 1])
    with pytest.raises(ValueError):
        TK.TrackSet.build([])


# ------------------------------------------------------------------ 2. projection and window against the specification

def test_host_projection_and_window_against_the_specification():
    """64 points within 0.3 m of the 12-knot circuit, each projected globally and then locally from the global place;
    the window at N = 20, Ts = 0.02, vref 1.0 from headings on other branches.  s / L and path_ref within rel 1e-12
    (test_ref_window_vs_oracle's bar for the y(x) window), chosen windings equal."""
    ts = _ccw()
    sig, coef, M = _spec(ts)
    L = float(sig[M])
    pts = R.points_near(sig, coef, M, 64, 0.3, seed=11)
    sg = TK.track_project_host(ts, pts)
    sl, d2 = TK.track_project_host(ts, pts, s_prev=sg, want_dist2=True)
    rg = np.array([R.project(sig, coef, M, p)[0] for p in pts])
    rl = np.array([R.project(sig, coef, M, p, s_prev=s)[0] for p, s in zip(pts, rg)])
    eg, el = R.cyc(sg, rg, L).max() / L, R.cyc(sl, rl, L).max() / L
    print(f"projection: global {eg:.3e}, local {el:.3e} of L")
    assert eg <= 1e-12 and el <= 1e-12
    assert ((sg >= 0) & (sg < L)).all() and ((sl >= 0) & (sl < L)).all()
    foot = np.stack(ts.eval_host(0, sl)[:2], axis=1)
    assert np.allclose(d2, ((foot - pts) ** 2).sum(axis=1), rtol=0, atol=1e-15) and (np.sqrt(d2) <= 0.3 + 1e-9).all()
    # the window
    rng = np.random.default_rng(12)
    a0 = np.array([R.window(sig, coef, M, s, None, np.ones(N + 1), 1, TS)[2][0] for s in rl])
    phi = a0 + TWO_PI * rng.integers(-1, 2, 64) + rng.uniform(-0.3, 0.3, 64)
    got = TK.track_window_host(ts, sl, np.ones(N + 1), N, TS, phi=phi)
    worst = 0.0
    for b in range(64):
        pr, wind, raw = R.window(sig, coef, M, sl[b], phi[b], np.ones(N + 1), N, TS)
        worst = max(worst, R.rel(got[b], pr))
        assert np.array_equal(np.rint((got[b, :, 2] - raw) / TWO_PI).astype(int), wind), b
    print(f"window: worst rel {worst:.3e}")
    assert worst <= 1e-12
    # without a heading n_0 = 0: the raw atan2 at stage 0; a per-trajectory vref is read row by row
    vr = np.linspace(0.8, 1.5, 64)[:, None] * np.ones((1, N + 1))
    got = TK.track_window_host(ts, sl, vr, N, TS)
    for b in (0, 17, 63):
        assert R.rel(got[b], R.window(sig, coef, M, sl[b], None, vr[b], N, TS)[0]) <= 1e-12
        assert abs(got[b, 0, 2]) <= math.pi


# ------------------------------------------------------------------ 3. the heading

@pytest.mark.parametrize("m", [-1, 0, 2])
def test_heading_starts_on_the_vehicles_branch(m):
    ts = _ccw()
    s0 = np.linspace(0.0, ts.L[0], 9)[:-1]
    a0 = TK.track_window_host(ts, s0, np.ones(N + 1), N, TS)[:, 0, 2]
    phi = a0 + TWO_PI * m + 0.1
    pr = TK.track_window_host(ts, s0, np.ones(N + 1), N, TS, phi=phi)
    assert (np.abs(pr[:, 0, 2] - phi) <= 0.1 + 1e-12).all()
    assert np.array_equal(np.rint((pr[:, 0, 2] - a0) / TWO_PI), np.full(8, float(m)))


def test_heading_is_continuous_across_the_cut_and_follows_the_direction():
    """A window that crosses the +-pi cut (it starts near the top of the counter-clockwise circuit, where the heading
    is near pi) keeps |phi*_{k+1} - phi*_k| < 0.2; the clockwise track gives a decreasing phi*."""
    ts = TK.TrackSet.build([R.circuit_knots(), R.circuit_knots()[::-1]])
    sig, coef, M = _spec(ts)
    # the raw heading along the counter-clockwise circuit: the last place before it jumps from +pi to -pi
    ss = np.linspace(0.0, sig[M], 2000, endpoint=False)
    X, Y, dX, dY = ts.eval_host(0, ss)
    a = np.arctan2(dY, dX)
    cut = int(np.argmax(np.diff(a) < -math.pi))
    assert Y[cut] > 1.0 and a[cut] > 3.0                      # near the top, heading near +pi
    Nw, vr = 60, np.ones(61)                                  # 60 stages of 0.02 m: 1.2 m along the track
    s0 = np.array([ss[cut] - 0.05])
    pr = TK.track_window_host(ts, s0, vr, Nw, TS)[0]
    d = np.diff(pr[:, 2])
    assert (np.abs(d) < 0.2).all() and pr[-1, 2] > math.pi + 0.3 and (d > 0).sum() > 50
    raw = np.array([R.window(sig, coef, M, s0[0], None, vr, Nw, TS)[2]])[0]
    assert np.abs(np.diff(raw)).max() > 6.0                   # the raw atan2 does jump
    # clockwise: the same curve run the other way
    cw = ts.with_track_of([1])
    pr = TK.track_window_host(cw, np.array([1.0]), vr, Nw, TS)[0]
    d = np.diff(pr[:, 2])
    assert (np.abs(d) < 0.2).all() and (d < 0).sum() > 50 and pr[-1, 2] < pr[0, 2] - 0.3


# ------------------------------------------------------------------ 4. the tie rule and the fallbacks

def test_ties_resolve_to_the_lowest_candidate():
    """Four knots on a circle of radius 2 with one candidate per piece: the centre is equidistant from all four
    candidates (4.0 exactly) and resolves to (0, 0); (-1, 1) is equidistant from candidates 1 and 2 and resolves to
    1.  On the 16-knot circle with 8 candidates per piece the centre resolves as the specification says."""
    ts = TK.TrackSet.build([np.array([[2.0, 0.0], [0.0, 2.0], [-2.0, 0.0], [0.0, -2.0]])])
    sig, coef, M = _spec(ts)
    se = dict(samples=1, newton=0)
    for p, want in (((0.0, 0.0), 0), ((-1.0, 1.0), 1), ((1.0, 1.0), 0), ((-1.0, -1.0), 2), ((1.0, -1.0), 0)):
        s = TK.track_project_host(ts, np.array([p]), search=se)[0]
        rs, (i, j), _ = R.project(sig, coef, M, p, samples=1, newton=0)
        assert (i, j) == (want, 0) and s == sig[want] == rs, (p, s)
    c16 = TK.TrackSet.build([R.circle_knots(16)])
    sig, coef, M = _spec(c16)
    s = TK.track_project_host(c16, np.zeros((1, 2)), search=dict(newton=0))[0]
    assert s == R.project(sig, coef, M, (0.0, 0.0), newton=0)[0]


def test_local_search_with_no_candidate_falls_back_to_global():
    ts = _ccw()
    sig, coef, M = _spec(ts)
    pts = R.points_near(sig, coef, M, 8, 0.2, seed=5)
    sg = TK.track_project_host(ts, pts)
    sp = np.full(8, 0.123)                                    # on no candidate: [-0, 0] holds none
    s0 = TK.track_project_host(ts, pts, s_prev=sp, search=dict(back=0.0, fwd=0.0))
    assert np.array_equal(s0, sg)
    # with the default reach the search is local: far points land near s_prev, not on their global place
    sl = TK.track_project_host(ts, pts, s_prev=sp, search=dict(newton=0))
    far = R.cyc(sg, 0.123, sig[M]) > 2.0
    off = (sl - 0.123 + sig[M] / 2) % sig[M] - sig[M] / 2
    assert far.any() and ((off >= -0.5) & (off <= 1.0)).all()
    assert not np.array_equal(TK.track_project_host(ts, pts, s_prev=sp), sg)
    # a NaN s_prev is the global search
    assert np.array_equal(TK.track_project_host(ts, pts, s_prev=np.full(8, np.nan)), sg)


def test_refinement_stops_where_g_prime_is_not_positive():
    """A point beyond the centre of curvature: on the circle of radius 2 from the place near (0, 2), the point
    (0, -1) has g' = |P'|^2 + (P - p) . P'' ~ 1 - 3/2 < 0, so the candidate is returned as it is; a point inside the
    radius is refined."""
    ts = TK.TrackSet.build([R.circle_knots(16)])
    sig, coef, M = _spec(ts)
    se = dict(back=0.3, fwd=0.3)
    s = TK.track_project_host(ts, np.array([[0.0, -1.0]]), s_prev=np.array([sig[4]]), search=se)[0]
    rs, ij, moved = R.project(sig, coef, M, (0.0, -1.0), s_prev=float(sig[4]), back=0.3, fwd=0.3)
    assert moved == 0 and s == rs
    assert s == TK.track_project_host(ts, np.array([[0.0, -1.0]]), s_prev=np.array([sig[4]]),
                                      search=dict(back=0.3, fwd=0.3, newton=0))[0]
    s = TK.track_project_host(ts, np.array([[0.3, 1.7]]), s_prev=np.array([sig[4]]), search=se)[0]
    rs, ij, moved = R.project(sig, coef, M, (0.3, 1.7), s_prev=float(sig[4]), back=0.3, fwd=0.3)
    assert moved == 8 and abs(s - rs) <= 1e-12 * sig[M]
    assert s != R.project(sig, coef, M, (0.3, 1.7), s_prev=float(sig[4]), back=0.3, fwd=0.3, newton=0)[0]


def test_clamp_never_binds_on_the_test_inputs():
    """The Newton step's clamp to the candidate spacing is a guard: on the 64 test points (global and local) no
    iteration's |g / g'| reaches h."""
    ts = _ccw()
    sig, coef, M = _spec(ts)
    L = float(sig[M])
    pts = R.points_near(sig, coef, M, 64, 0.3, seed=11)
    worst = 0.0
    for p in pts:
        s, (i, j), _ = R.project(sig, coef, M, p, newton=0)
        h = (sig[i + 1] - sig[i]) / 8
        for _ in range(8):
            X, Y, dX, dY, ddX, ddY = R.eval_at(sig, coef, M, s)
            g = (X - p[0]) * dX + (Y - p[1]) * dY
            gp = dX * dX + dY * dY + (X - p[0]) * ddX + (Y - p[1]) * ddY
            assert gp > 0
            worst = max(worst, abs(g / gp) / h)
            s = R.wrap(s - g / gp, L)
    print(f"largest |g / g'| / h over the test points: {worst:.3f}")
    assert worst < 1.0


# ------------------------------------------------------------------ 5. argument errors

def _bad_searches():
    for k, v in (("samples", 0), ("samples", _lib.TRACK_MAX_SAMPLES + 1), ("newton", -1), ("back", -0.1),
                 ("back", float("nan")), ("fwd", -1.0), ("fwd", float("nan"))):
        yield TK.search_struct({k: v})


def test_argument_errors():
    """samples < 1, newton < 0, a negative or NaN back / fwd, kmax < 3 and n_tracks < 1 are TRAJ_E_ARG from every entry
    point that takes them, before any launch (B = 0 calls of the device entry points launch nothing anyway); so are the
    host entry points' own: a knot count below 3, a track_of entry outside the tracks, a short vref row."""
    L = _lib.lib()
    ts = _ccw()
    good, se = ts.host_struct(), TK.search_struct()
    p, c = _lib.default_params(), _lib.default_config(N, TS)
    xy, s, out, vr = np.zeros((2, 2)), np.zeros(2), np.zeros((2, N + 1, 3)), np.ones(N + 1)
    P = _lib.ptr

    def project(t, q, B=2):
        return L.traj_track_project_host(C.byref(t), C.byref(q), B, P(xy), 2, None, P(s), None)

    def window(t, B=2, n=N, ts_=TS, row=0, ln=N + 1, off=0):
        return L.traj_track_window_host(C.byref(t), B, n, ts_, P(s), None, P(vr), row, ln, off, P(out))

    def step(t, q, cfg=c):
        return L.traj_closed_loop_track_step(C.byref(p), C.byref(cfg), C.byref(t), C.byref(q), 0, *([None] * 4), N + 1,
                                             N + 1, 0, 0, 0, *([None] * 6), 0, None)

    def run(t, q, steps=1):
        return L.traj_closed_loop_track_run(C.byref(p), C.byref(c), C.byref(t), C.byref(q), 0, *([None] * 4), N + 1,
                                            N + 1, 0, 0, steps, 0, *([None] * 6), 0, None)

    assert project(good, se) == window(good) == step(good, se) == run(good, se) == _lib.TRAJ_OK
    assert L.traj_track_project_batch(C.byref(good), C.byref(se), 0, None, 2, None, None, None, None) == _lib.TRAJ_OK
    for q in _bad_searches():
        assert project(good, q) == step(good, q) == run(good, q) == _lib.TRAJ_E_ARG
        assert L.traj_track_project_batch(C.byref(good), C.byref(q), 0, None, 2, None, None, None, None) == _lib.TRAJ_E_ARG
    for field, v in (("kmax", 2), ("n_tracks", 0), ("nk", None), ("sig", None), ("coef", None)):
        bad = ts.host_struct()
        setattr(bad, field, v)
        assert project(bad, se) == window(bad) == step(bad, se) == run(bad, se) == _lib.TRAJ_E_ARG, field
        assert L.traj_track_window_batch(C.byref(bad), 0, N, TS, None, None, None, 0, N + 1, 0, None,
                                         None) == _lib.TRAJ_E_ARG
        assert L.traj_track_errors_batch(C.byref(bad), 0, 3, None, None, None, None) == _lib.TRAJ_E_ARG
    # the host's own checks
    two = TK.TrackSet(np.array([2], np.int32), ts.sig, ts.coef)
    assert project(two.host_struct(), se) == window(two.host_struct()) == _lib.TRAJ_E_ARG
    lost = TK.TrackSet(ts.nk, ts.sig, ts.coef, track_of=[0, 1])
    assert project(lost.host_struct(), se) == window(lost.host_struct()) == _lib.TRAJ_E_ARG
    assert project(good, se, B=-1) == window(good, B=-1) == _lib.TRAJ_E_ARG
    assert L.traj_track_project_host(C.byref(good), C.byref(se), 2, P(xy), 1, None, P(s), None) == _lib.TRAJ_E_ARG
    assert L.traj_track_project_host(C.byref(good), C.byref(se), 2, None, 2, None, P(s), None) == _lib.TRAJ_E_ARG
    assert window(good, n=0) == window(good, ts_=0.0) == window(good, ln=N) == window(good, off=1) == _lib.TRAJ_E_ARG
    assert window(good, row=N) == window(good, off=-1) == _lib.TRAJ_E_ARG
    # the loop: an invalid configuration, a schedule too short, negative steps; the workspace query
    badc = _lib.default_config(N, TS)
    badc.rho = -1.0
    assert step(good, se, badc) == _lib.TRAJ_E_ARG and L.traj_closed_loop_track_workspace_bytes(C.byref(badc), 4) == 0
    assert run(good, se, steps=-1) == _lib.TRAJ_E_ARG and run(good, se, steps=0) == _lib.TRAJ_OK
    assert L.traj_closed_loop_track_step(C.byref(p), C.byref(c), C.byref(good), C.byref(se), 0, *([None] * 4), N, N, 0,
                                         0, 0, *([None] * 6), 0, None) == _lib.TRAJ_E_ARG
    assert L.traj_closed_loop_track_run(C.byref(p), C.byref(c), C.byref(good), C.byref(se), 0, *([None] * 4), 0, N + 5,
                                        1, 0, 6, 0, *([None] * 6), 0, None) == _lib.TRAJ_E_ARG   # step 5 reads N + 5
    need = L.traj_closed_loop_track_workspace_bytes(C.byref(c), 4)
    step_need = (L.traj_mpc_step_workspace_bytes(C.byref(c), 4) + 7) // 8 * 8
    assert need == step_need + (4 * (N + 1) * 4 + 4 * 2) * 8 + 16
    assert L.traj_debug_track_lanes(3) == _lib.TRAJ_E_ARG
    assert L.traj_debug_track_lanes(1) == L.traj_debug_track_lanes(16) == _lib.TRAJ_OK
    with pytest.raises(ValueError):
        TK.set_track_lanes(8)
    with pytest.raises(TypeError):
        TK.search_struct(dict(sample=3))


def test_workload_and_dataset_refusals(tmp_path):
    """make_track_workload's shapes and ranges, reproducible per id; dataset.generate(kind="track") refuses what this
    loop does not take, before anything touches a GPU."""
    from trajectory_generation_amd import dataset
    from trajectory_generation_amd.workload import make_track_workload
    w = make_track_workload(12, N, TS, seed=3)
    assert len(w["knots"]) == 8 and all(k.shape == (16, 2) for k in w["knots"])
    assert w["track_of"].tolist() == [b % 8 for b in range(12)]
    assert w["x0"].shape == (12, 6) and w["u0"].shape == (12, 2) and w["vref"].shape == (12, N + 1)
    assert ((w["x0"][:, 3] >= 0.8) & (w["x0"][:, 3] <= 1.5)).all() and (w["vref"] == w["x0"][:, 3:4]).all()
    assert np.ptp(w["x0"][:, 2]) > math.pi                    # headings all round the compass
    ts = TK.TrackSet.build(w["knots"], w["track_of"])
    s, d2 = TK.track_project_host(ts, w["x0"], want_dist2=True)
    assert (np.sqrt(d2) <= 0.1 + 1e-9).all() and R.cyc(s, w["s0"], ts.L[w["track_of"]]).max() < 0.02
    # odd tracks run clockwise: the signed area of their knots is negative
    for i, k in enumerate(w["knots"]):
        area = 0.5 * np.sum(k[:, 0] * np.roll(k[:, 1], -1) - np.roll(k[:, 0], -1) * k[:, 1])
        assert (area < 0) == (i % 2 == 1), i
    w2 = make_track_workload(4, N, TS, seed=3, id_offset=8)
    assert np.array_equal(w2["x0"], w["x0"][8:]) and all(np.array_equal(a, b) for a, b in zip(w["knots"], w2["knots"]))
    for kw in (dict(stats=True), dict(speed_schedule=np.ones((12, 30 + N))), dict(device_workload=True)):
        with pytest.raises(ValueError):
            dataset.generate(12, 30, N=N, Ts=TS, kind="track", seed=3, out_prefix=str(tmp_path / "t"), **kw)


# ------------------------------------------------------------------ csrc/track.h under the sanitizers

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_track_header_under_asan_ubsan(tmp_path):
    """csrc/track.h alone under g++ -fsanitize=address,undefined (tests/sanitize/san_track.cpp, a stand-alone
    program): tracks in heap buffers of exactly their size, project and window at the edge inputs -- s at 0 and at L,
    M = 3, a point on a knot, a NaN s_prev, a point that is not finite."""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = str(tmp_path / "san_track")
    r = subprocess.run(["g++", *san, "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                        os.path.join(HERE, "sanitize", "san_track.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "san_track ok" in r.stdout and "ERROR" not in r.stderr

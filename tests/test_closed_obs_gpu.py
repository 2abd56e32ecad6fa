"""The closed loop on a state estimate on the GPU (include/trajobs.h, trajectory_generation_amd/observed.py).

1. truth      estimator="truth" is run_closed_loop(fused=True), bit for bit, on every solver tier and with a schedule.
2. steps      every step is the step entry point on the estimate; the plant and the measurement are one expression.
3. EKF        the in-loop filter is the offline one (knet.ekf_run) on the recorded signals, bit for bit, in both forms
              of the step, and within ekf_kernel's bar of the float64 oracle; the estimator alone gives the same bits.
4. filters    the estimate beats the measurements (pooled over the measured channels, steps >= 5).
5. callables  a callable returning the truth is truth mode; KalmanNet in the loop is KalmanNet offline on Y, U.
6. graph      the captured run replays the plain stream's bits.
7. arguments  every refusal leaves the buffers untouched; B == 0.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests._knet_weights import LIMITS, knet_weights
from tests._mpc_checks import VCAP
from tests.test_vref_schedule_gpu import _same, schedule
from trajectory_generation_amd import _lib
from trajectory_generation_amd import batch as TB
from trajectory_generation_amd.workload import make_workload

pytestmark = pytest.mark.gpu

TS, T, B = 0.05, 6, 9
HR = [0, 1, 3, 4, 5]
WIDE = dict(LIMITS, omega_min=-20.0, omega_max=20.0)   # the truth reaches |omega| ~ 12.5 on these workloads
KEYS = ("X", "U", "status", "iters")


def _ekf_params(limits):
    """Vehicle parameters and clamp limits as one dict (what knet.ekf_run and the oracle take)."""
    from oracle import knet_oracle as KO
    p = dict(KO.PARAMS)
    p.update(limits)
    return p


def _noise(Bn, Tn, seed=7):
    from trajectory_generation_amd.knet import EKF_R
    return np.random.default_rng(seed).normal(size=(Bn, Tn, 5)) * np.sqrt(np.array(EKF_R))


def _setup(Bn, N, warm=0, kind="spline", seed=6, **cfg_kw):
    w = make_workload(Bn, N, TS, kind=kind, seed=seed)
    return w, TB.PathSet.build(w["kinds"], w["pcs"], w["knots"]), TB.config_struct(N=N, Ts=TS, warm_start=warm, **cfg_kw)


@pytest.fixture
def lanes():
    """Sets the EKF step's form; the library's default is back afterwards."""
    from trajectory_generation_amd import observed as OB
    yield OB.set_obs_lanes
    OB.set_obs_lanes(_lib.OBS_DEFAULT_LANES)


# ------------------------------------------------------------------------------------------------ 1. truth mode

@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("N,cfg_kw,sched", [(8, {}, False), (24, {}, False), (66, {}, False), (20, VCAP, False),
                                            (12, {}, True)],
                         ids=["reg-N8", "split-N24", "long-N66", "general-N20", "sched-N12"])
def test_truth_mode_is_the_closed_loop(gpu, N, cfg_kw, sched, warm):
    from trajectory_generation_amd import observed as OB
    w, paths, cfg = _setup(B, N, warm, **cfg_kw)
    vref, vs = (schedule(B, T + N, TS, jump=(4, N + 3)), 1) if sched else (w["vref"], 0)
    base = TB.run_closed_loop(w["x0"], w["u0"], paths, vref, T, cfg, fused=True, vref_step=vs)
    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, vref, T, cfg, estimator="truth", noise=_noise(B, T),
                                      vref_step=vs)
    for k in KEYS:
        assert _same(run[k], base[k]), k
    assert _same(run["Xhat"], run["X"]) and _same(run["x"], base["x"]) and _same(run["u"], base["u"])
    assert _same(run["Y"], run["X"][:, 1:][:, :, HR] + torch.as_tensor(_noise(B, T), device=gpu))


# ------------------------------------------------------------------------------------------------ 2. the steps

def test_every_step_is_the_step_entry_point_on_the_estimate(gpu):
    from trajectory_generation_amd import observed as OB
    N = 12
    w, paths, cfg = _setup(B, N, 0)
    noise = _noise(B, T)
    xhat0 = w["x0"] + np.random.default_rng(2).normal(size=(B, 6)) * 0.02
    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, params=WIDE, estimator="ekf",
                                      xhat0=xhat0, noise=noise)
    X, Xhat, Y, U = run["X"], run["Xhat"], run["Y"], run["U"]
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
    nz = torch.as_tensor(noise, device=gpu)
    assert _same(Xhat[:, 0], torch.as_tensor(xhat0, device=gpu)) and not _same(Xhat[:, 1:], X[:, 1:])
    for t in range(T):
        up = U[:, t - 1] if t > 0 else torch.as_tensor(w["u0"], device=gpu)
        pr = TB.ref_window_batch(paths, Xhat[:, t, 0].contiguous(), vr, N, TS)
        o = TB.mpc_step_batch(Xhat[:, t].contiguous(), up.contiguous(), pr, vr, cfg)
        assert _same(o["u_cmd"], U[:, t]), t
        assert torch.equal(o["status"], run["status"][t]), t
        f = TB.f_cont_batch(X[:, t].contiguous(), U[:, t].contiguous())
        assert _same(X[:, t + 1], X[:, t] + TS * f), t
        assert _same(Y[:, t], X[:, t + 1][:, HR] + nz[:, t]), t


# ------------------------------------------------------------------------------------------------ 3. the EKF

EKF_B, EKF_T, EKF_N = 70, 12, 12    # B = 70: a partial last block (64 per block) and a partial last wave (4 per wave)


@functools.lru_cache(maxsize=None)
def _ekf_case(variant):
    w = make_workload(EKF_B, EKF_N, TS, kind="spline", seed=6)
    xhat0 = w["x0"] + np.random.default_rng(11).normal(size=(EKF_B, 6)) * 0.02
    noise = _noise(EKF_B, EKF_T)
    for a in (xhat0, noise, w["x0"], w["u0"]):   # shared among the cases: left unchanged
        a.setflags(write=False)
    return w, noise, xhat0, (WIDE if variant == "wide" else dict(LIMITS))


@functools.lru_cache(maxsize=None)
def _ekf_oracle(variant, y_bytes, u_bytes):
    """The float64 oracle on recorded signals (computed once per distinct record and shared)."""
    from oracle import knet_oracle as KO
    from trajectory_generation_amd import knet as K
    _, _, xhat0, limits = _ekf_case(variant)
    Yt = np.frombuffer(y_bytes).reshape(EKF_B, 5, EKF_T)
    Ut = np.frombuffer(u_bytes).reshape(EKF_B, 2, EKF_T)
    ref = KO.ekf_run(_ekf_params(limits), TS, Yt, Ut, xhat0, K.EKF_P0, K.EKF_Q, K.EKF_R)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("form", [1, 16])
@pytest.mark.parametrize("variant", ["wide", "omega6"])
def test_in_loop_ekf_is_the_offline_ekf(gpu, lanes, variant, form):
    """Measured against the oracle: see the printed ratio (DESIGN.md 7i records it)."""
    from trajectory_generation_amd import knet as K
    from trajectory_generation_amd import observed as OB
    w, noise, xhat0, limits = _ekf_case(variant)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=EKF_N, Ts=TS)
    p = _ekf_params(limits)
    lanes(form)
    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], EKF_T, cfg, params=p, estimator="ekf",
                                      xhat0=xhat0, noise=noise)
    Yt, Ut = run["Y"].permute(0, 2, 1).contiguous(), run["U"].permute(0, 2, 1).contiguous()
    got = run["Xhat"][:, 1:].permute(0, 2, 1)                       # [B,6,T]
    off = K.ekf_run(p, TS, Yt, Ut, xhat0)
    assert _same(got, off)
    if variant == "omega6":   # the estimate leaves the model's omega range: clamped rows, zero Jacobian rows
        assert bool((run["Xhat"][:, :-1, 5].abs() > 6.0).any())
    ref = _ekf_oracle(variant, Yt.cpu().numpy().tobytes(), Ut.cpu().numpy().tobytes())
    err, bar = np.abs(got.cpu().numpy() - ref).max(), 1e-8 * (1 + np.abs(ref).max())
    print(f"in-loop EKF ({variant}, lanes {form}) against the oracle: {err:.3e} = {err / bar:.4f} of the bar {bar:.3e}")
    assert err <= bar
    # the estimator alone, T calls on the same signals
    x = torch.as_tensor(xhat0, device=gpu).clone()
    P = torch.diag_embed(torch.as_tensor(K.EKF_P0, dtype=torch.float64, device=gpu).expand(EKF_B, 6)).contiguous()
    for t in range(EKF_T):
        OB.ekf_step(p, TS, x, P, run["U"][:, t], run["Y"][:, t])
        assert _same(x, run["Xhat"][:, t + 1]), t
    assert _same(P, run["P"])


# ------------------------------------------------------------------------------------------------ 4. it filters

def test_the_loop_filters(gpu):
    from trajectory_generation_amd import observed as OB
    Bn, N, Tn = 70, 12, 40
    w, paths, cfg = _setup(Bn, N)
    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], Tn, cfg, params=WIDE, estimator="ekf",
                                      noise=_noise(Bn, Tn))
    X = run["X"].cpu().numpy()
    for i, k in enumerate(("x", "y", "phi", "vx", "vy", "omega")):
        lo, hi = X[..., i].min(), X[..., i].max()
        print(f"truth {k}: {lo:.3f} .. {hi:.3f}")
        assert WIDE[k + "_min"] < lo and hi < WIDE[k + "_max"], k
    assert bool((run["status"] == 0).all())
    e = OB.estimation_errors(run, skip=5)
    print(f"mse_est / mse_meas = {e['ratio']:.3f}; per channel {(e['mse_est_ch'][HR] / e['mse_meas_ch']).round(3).tolist()}")
    assert e["mse_est"] < e["mse_meas"]
    # closed_loop_stats takes the run as it takes run_closed_loop's
    s = TB.closed_loop_stats(run, paths, w["vref"], w["u0"])
    assert s["pooled"].shape == (7, 5) and s["fails_total"] == 0 and s["n"]["e_c"] == Bn * Tn


# ------------------------------------------------------------------------------------------------ 5. callables

def test_a_callable_returning_the_truth_is_truth_mode(gpu):
    from trajectory_generation_amd import observed as OB
    N = 12
    w, paths, cfg = _setup(B, N, 1)
    noise = _noise(B, T)
    ref = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, estimator="truth", noise=noise)
    seen = []

    def est(t, y, u):
        assert _same(y, ref["Y"][:, t]) and _same(u, ref["U"][:, t])
        seen.append(t)
        return ref["X"][:, t + 1]

    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, estimator=est, noise=noise)
    assert seen == list(range(T))
    for k in KEYS + ("Xhat", "Y", "x", "xhat", "u"):
        assert _same(run[k], ref[k]), k
    with pytest.raises(ValueError):
        OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, estimator=lambda t, y, u: y)


def _knet(dev):
    from trajectory_generation_amd import knet as K
    g = np.load("tests/golden/knet.npz")
    sysm = K.VehicleModel(TS, T, T, torch.zeros(6, 1))
    sysm.Params.update(LIMITS)
    model = K.KalmanNetNN(dev)
    model.NNBuild(sysm, in_mult_KNet=5, out_mult_KNet=40, hidden_dim_gru=128)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)   # noqa: E731
    model.set_normalization(f32(g["x_mean"]), f32(g["x_std"]), f32(g["y_mean"]), f32(g["y_std"]))
    model.load_state_dict({k: torch.tensor(v) for k, v in knet_weights(seed=0).items()}, strict=True)
    return model


def test_kalmannet_in_the_loop_is_kalmannet_offline(gpu):
    """Plumbing: an untrained filter may drive the solver's statuses off optimal; the estimates are still the
    module's own on the recorded Y, U."""
    from trajectory_generation_amd import observed as OB
    N = 12
    w, paths, cfg = _setup(B, N)
    run = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg,
                                      estimator=OB.knet_estimator(_knet(gpu), w["x0"]), noise=_noise(B, T))
    off = OB.knet_estimator(_knet(gpu), w["x0"])
    for t in range(T):
        assert _same(off(t, run["Y"][:, t], run["U"][:, t]), run["Xhat"][:, t + 1]), t
    assert _same(run["Xhat"][:, 0], run["X"][:, 0]) and not _same(run["Xhat"][:, 1:], run["X"][:, 1:])
    assert run["Xhat"].dtype == torch.float64


# ------------------------------------------------------------------------------------------------ 6. graph

def test_graph_replays_the_plain_streams_bits(gpu):
    from trajectory_generation_amd import observed as OB
    N = 12
    w, paths, cfg = _setup(B, N, 1)
    kw = dict(params=WIDE, estimator="ekf", noise=_noise(B, T))
    plain = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, **kw)
    keys = KEYS + ("Xhat", "Y", "x", "xhat", "u", "P")
    g = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], T, cfg, graph=True, **kw)
    for rep in range(3):   # the capture's own replay, then two more
        for k in keys:
            assert _same(g[k], plain[k]), (rep, k)
        for k in ("X", "Xhat", "Y", "U", "status", "iters"):
            g[k].zero_()
        if rep < 2:
            g["replay"]()


# ------------------------------------------------------------------------------------------------ 7. arguments

def test_argument_errors_launch_nothing(gpu):
    from trajectory_generation_amd import observed as OB
    N, Tn = 12, 4
    w, paths, cfg = _setup(B, N)
    L = _lib.lib()
    p = _lib.default_params()
    from trajectory_generation_amd.knet import limits_struct
    lim = limits_struct(WIDE)
    f64 = dict(dtype=torch.float64, device=gpu)
    x = torch.as_tensor(w["x0"], device=gpu).clone()
    xh, u = x.clone(), torch.as_tensor(w["u0"], device=gpu).clone()
    P = torch.diag_embed(torch.full((B, 6), 0.1, **f64)).contiguous()
    vr = torch.as_tensor(np.tile(w["vref"], (B, 1)), device=gpu)
    hx, hxh = torch.zeros((B, Tn + 1, 6), **f64), torch.zeros((B, Tn + 1, 6), **f64)
    hu, hy, nz = torch.zeros((B, Tn, 2), **f64), torch.zeros((B, Tn, 5), **f64), torch.zeros((B, Tn, 5), **f64)
    st, it = torch.zeros(B, dtype=torch.int32, device=gpu), torch.zeros(B, dtype=torch.int32, device=gpu)
    need = L.traj_closed_loop_obs_workspace_bytes(C.byref(cfg), B)
    ws = torch.zeros(need // 8, **f64)
    ps = paths.struct()
    ptr, stream = _lib.ptr, _lib.stream
    keep = [t.clone() for t in (x, xh, u, P, hx, hxh, hu, hy, st, it)]

    def step(**kw):
        a = dict(p=C.byref(p), c=C.byref(cfg), paths=C.byref(ps), lim=C.byref(lim), o=C.byref(OB.obs_config("ekf")), B=B,
                 x=ptr(x), xh=ptr(xh), P=ptr(P), u=ptr(u), vref=ptr(vr), row=N + 1, len=N + 1, vs=0, noise=ptr(nz), t=0,
                 hT=Tn, hx=ptr(hx), hxh=ptr(hxh), hu=ptr(hu), hy=ptr(hy), ws=ptr(ws), wb=need)
        a.update(kw)
        return L.traj_closed_loop_obs_step(a["p"], a["c"], a["paths"], a["lim"], a["o"], a["B"], a["x"], a["xh"], a["P"],
                                           a["u"], a["vref"], a["row"], a["len"], a["vs"], a["noise"], a["t"], a["hT"],
                                           a["hx"], a["hxh"], a["hu"], a["hy"], ptr(st), ptr(it), a["ws"], a["wb"],
                                           stream())

    def o_of(est=_lib.OBS_EKF, Q=(1e-6,) * 6, R=(1e-4,) * 5):
        o = _lib.ObsConfig()
        o.estimator = est
        o.Q[:], o.R[:] = list(Q), list(R)
        return C.byref(o)

    nan = float("nan")
    cases = [dict(p=None), dict(c=None), dict(paths=None), dict(o=None), dict(B=-1), dict(o=o_of(est=3)), dict(lim=None),
             dict(P=None), dict(o=o_of(R=(0.0,) + (1.0,) * 4)), dict(o=o_of(R=(nan,) + (1.0,) * 4)),
             dict(o=o_of(Q=(-1.0,) + (0.0,) * 5)), dict(o=o_of(Q=(nan,) + (0.0,) * 5)), dict(x=None), dict(xh=None),
             dict(u=None), dict(vref=None), dict(ws=None), dict(wb=need - 8), dict(t=Tn), dict(t=-1),
             dict(noise=ptr(nz), hx=None, hxh=None, hu=None, hy=None, t=Tn), dict(vs=2), dict(len=N), dict(row=3),
             dict(vs=1, t=1)]
    for kw in cases:
        assert step(**kw) == _lib.TRAJ_E_ARG, sorted(kw)
    assert step(B=0) == _lib.TRAJ_OK
    torch.cuda.synchronize()
    for t_, k_ in zip((x, xh, u, P, hx, hxh, hu, hy, st, it), keep):
        assert _same(t_, k_)
    # the same call, valid: it runs
    assert step() == _lib.TRAJ_OK
    torch.cuda.synchronize()
    assert not _same(x, keep[0]) and _same(hx[:, 1], x) and _same(hxh[:, 1], xh) and _same(hu[:, 0], u)
    # the EKF's limits come from params: a missing key is limits_struct's KeyError
    short = {k: v for k, v in WIDE.items() if k != "vy_max"}
    with pytest.raises(KeyError):
        OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], Tn, cfg, params=short, estimator="ekf")
    with pytest.raises(KeyError):
        OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], Tn, cfg, estimator="ekf")
    # the observed loop's workspace is its own buffer, never the closed loop's
    OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], Tn, cfg, estimator="truth")
    TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], Tn, cfg)
    roles = {k[2]: v.data_ptr() for k, v in TB._WS.items() if k[0] == str(gpu)}
    assert roles["closed_loop_observed"] != roles["closed_loop"]

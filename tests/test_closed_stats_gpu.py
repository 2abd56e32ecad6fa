"""The closed loop's statistics and tracking errors on the GPU (csrc/closed_stats.hip, batch.closed_loop_stats) against
the numpy specification and exact sums.

Histories come from run_closed_loop at N = 10, Ts = 0.02 over parabolas, sinusoids and splines mixed (kinds 0, 1, 2
in turn), built once per (B, T) and left unchanged.  The bars:

  exact fields      n, fails, fails_total, and min / max of d, delta, dd, ddelta (inputs, or one IEEE difference of
                    inputs) equal the specification to the bit.
  mean, M2 / n      of d, delta, dd, ddelta against exact rational moments of the same samples (tests/_stats_cases.py
                    exact_moments), within the forward-error bound of the accumulation used, derived there:
                        |mean - exact| <= 8 L u V,   |M2 / n - exact| <= (16 L^2 + 8 L) u V^2,
                    u = 2^-53, V = max |v|, L the longest chain of Welford updates and Chan merges a sample goes
                    through (per trajectory ceil(T / 64) + 6; pooled over K kept trajectories + ceil(K / 256) + 9;
                    + 1 per merge_stats).  In the issue's form c n u V^k: at T = 130, c = 0.55 and 10.5; pooled over
                    the 67 trajectories (n = 8710) 0.017 and 0.68.  Every bound used is asserted below 1e-12 first.
  e_c, e_phi, e_v   mean, M2 / n, min and max against the specification with the oracle's path and arctangent
                    (orc_ref_window's first point), within 1e-12 max(1, |value|): the device's sine and arctangent are
                    within 2 ulp of libm (test_oracle_golden.py), a few ulp of an O(1..10) quantity are five orders
                    below that.
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests._stats_cases import assert_moments, chain_length, mean_bound, var_bound
from trajectory_generation_amd import _lib
from trajectory_generation_amd import batch as TB
from trajectory_generation_amd.workload import SPLINE_KNOTS_X

pytestmark = pytest.mark.gpu

N, TS = 10, 0.02
CASES = ((1, 1), (5, 37), (67, 130))
U_SERIES, E_SERIES = (0, 1, 2, 3), (4, 5, 6)


def _workload(B, seed):
    """B trajectories over the three path kinds in turn, started near their paths (the ranges of workload.py)."""
    import oracle as O
    rng = np.random.default_rng(seed)
    kinds, pcs, knots, opaths = [], [], [], []
    for b in range(B):
        k = b % 3
        kinds.append(k)
        if k == 0:
            pcs.append([rng.uniform(-0.2, 0.2), 0.0, rng.uniform(0.05, 0.15), 0.0])
            knots.append(None)
            opaths.append(O.Path(0, pcs[-1]))
        elif k == 1:
            pcs.append([0.5 * rng.uniform(0.8, 1.2), 0.5 * rng.uniform(0.8, 1.2), rng.uniform(0, 2 * np.pi), 0.0])
            knots.append(None)
            opaths.append(O.Path(1, pcs[-1]))
        else:
            pcs.append([0.0] * 4)
            knots.append((SPLINE_KNOTS_X.copy(), rng.uniform(-1.0, 1.0, len(SPLINE_KNOTS_X))))
            opaths.append(O.Path(2, xk=knots[-1][0], coef=TB.spline_natural(*knots[-1]).ravel()))
    x0 = np.empty((B, 6))
    for b in range(B):
        X = rng.uniform(-2.0, 2.0)
        y, dy = opaths[b].eval(X)
        x0[b] = [X, y + rng.uniform(-0.5, 0.5), np.arctan(dy) + rng.uniform(-0.2, 0.2), rng.uniform(0.4, 1.5),
                 rng.uniform(-0.05, 0.05), rng.uniform(-1.0, 1.0)]
    u0 = np.stack([[TB.d_steady_state(v), 0.0] for v in x0[:, 3]])
    return kinds, pcs, knots, opaths, x0, u0


def _oracle_path_fn(opaths):
    """path_fn of the specification by the oracle: the first point (Y*, phi*) of orc_ref_window from each abscissa."""
    import oracle as O

    def fn(b, xs):
        pts = np.array([O.ref_window(opaths[b], float(x), 1, TS, [0.0, 0.0])[0] for x in xs])
        return pts[:, 1], pts[:, 2]
    return fn


@functools.lru_cache(maxsize=None)
def case(B, T):
    """One closed loop per (B, T): the run (device), its device statistics, the host copies and the specification."""
    import oracle as O
    O.build()
    kinds, pcs, knots, opaths, x0, u0 = _workload(B, 100 + B)
    paths = TB.PathSet.build(kinds, pcs, knots)
    vref = TB.vref_ramp(N, TS)
    run = TB.run_closed_loop(x0, u0, paths, vref, T, TB.config_struct(N=N, Ts=TS))
    X, U, st = run["X"].cpu().numpy(), run["U"].cpu().numpy(), run["status"].cpu().numpy()
    assert np.isfinite(X).all() and np.isfinite(U).all()
    fn = _oracle_path_fn(opaths)
    spec = TB.closed_loop_stats_host(X, U, u0, fn, vref[0], status=st)
    dev = TB.closed_loop_stats(run, paths, vref, u0)
    return dict(run=run, paths=paths, vref=vref, u0=u0, X=X, U=U, status=st, fn=fn, spec=spec, dev=dev)


def _close_to_spec(got, want, what):
    """Records [..., 5] of the error series against the specification's: n exactly; mean, M2 / n, min, max within
    1e-12 max(1, |value|)."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got[..., 0], want[..., 0]), what
    g = np.stack([got[..., 1], got[..., 2] / got[..., 0], got[..., 3], got[..., 4]], axis=-1)
    w = np.stack([want[..., 1], want[..., 2] / want[..., 0], want[..., 3], want[..., 4]], axis=-1)
    err = np.abs(g - w) / np.maximum(1.0, np.abs(w))
    print(f"{what}: worst scaled difference to the specification {err.max():.3e}")
    assert (err <= 1e-12).all(), (what, err.max())


@pytest.mark.parametrize("B,T", CASES, ids=[f"B{b}-T{t}" for b, t in CASES])
def test_statistics_against_specification_and_exact_sums(gpu, B, T):
    """Checks 1-5 of the module docstring on one closed loop of B trajectories and T steps.  The bound of check 2, for
    a record whose samples pass a chain of L Welford updates and Chan merges (u = 2^-53, V = max |v|):
        |mean - exact| <= 8 L u V,    |M2 / n - exact variance| <= (16 L^2 + 8 L) u V^2,
    L = ceil(T / 64) + 6 per trajectory, + ceil(K / 256) + 9 pooled over K trajectories, + 1 per merge_stats; derived in
    tests/_stats_cases.py, not measured.  At (67, 130) with V <= 1: 8.0e-15 and 1.5e-13 per trajectory, 1.7e-14 and
    6.6e-13 pooled -- below 1e-12, which assert_moments checks before it uses a bound.  Measured on an MI355X:
    worst 2.8e-17 and 6.9e-18; the error series against the specification 1.1e-16 scaled (bar 1e-12)."""
    c = case(B, T)
    spec, dev = c["spec"], c["dev"]
    per = dev["per_traj"].cpu().numpy()
    assert per.shape == (B, 7, 5) and dev["pooled"].shape == (7, 5)
    # 1. exact fields
    assert (per[:, :, 0] == T).all() and (dev["pooled"][:, 0] == B * T).all()
    assert np.array_equal(dev["fails"].cpu().numpy(), spec["fails"]) and dev["fails_total"] == spec["fails_total"]
    assert np.array_equal(per[:, U_SERIES, 3:], spec["per_traj"][:, U_SERIES, 3:])
    assert np.array_equal(dev["pooled"][list(U_SERIES), 3:], spec["pooled"][list(U_SERIES), 3:])
    # 2. mean and M2 / n of the input series against exact moments
    worst = [0.0, 0.0]
    for s in U_SERIES:
        for b in range(B):
            em, ev = assert_moments(per[b, s], spec["series"][b, s], chain_length(T), ("per_traj", b, s))
            worst = [max(worst[0], em), max(worst[1], ev)]
        em, ev = assert_moments(dev["pooled"][s], spec["series"][:, s], chain_length(T, B), ("pooled", s))
        worst = [max(worst[0], em), max(worst[1], ev)]
    print(f"B={B} T={T}: worst |mean - exact| {worst[0]:.3e}, worst |M2/n - exact| {worst[1]:.3e}")
    # 3. the error series against the specification
    _close_to_spec(per[:, E_SERIES], spec["per_traj"][:, E_SERIES], f"per_traj B={B} T={T}")
    _close_to_spec(dev["pooled"][list(E_SERIES)], spec["pooled"][list(E_SERIES)], f"pooled B={B} T={T}")
    # the named views
    assert dev["mean"]["d"] == dev["pooled"][0, 1] and dev["std"]["e_c"] == np.sqrt(dev["pooled"][4, 2] / (B * T))
    assert dev["min"]["delta"] == dev["pooled"][1, 3] and dev["max"]["e_v"] == dev["pooled"][6, 4]
    # 4. pooling: a mask is the kept rows alone, to the bit; halves merged on the host agree with the whole
    keep = np.arange(B) % 3 != 1
    masked = TB.pool_stats(dev["per_traj"], dev["fails"], keep)
    kd = torch.from_numpy(np.nonzero(keep)[0]).to(dev["per_traj"].device)
    alone = TB.pool_stats(dev["per_traj"][kd], dev["fails"][kd])
    assert masked[0].tobytes() == alone[0].tobytes() and masked[1] == alone[1]
    assert masked[0][0, 0] == keep.sum() * T
    none = TB.pool_stats(dev["per_traj"], dev["fails"], np.zeros(B, dtype=bool))
    assert (none[0][:, 0] == 0).all() and np.isnan(none[0][:, 1:]).all() and none[1] == 0
    if B >= 2:
        h = B // 2
        a, fa = TB.pool_stats(dev["per_traj"][:h], dev["fails"][:h])
        b2, fb = TB.pool_stats(dev["per_traj"][h:], dev["fails"][h:])
        merged = TB.merge_stats(a, b2)
        assert fa + fb == dev["fails_total"]
        assert np.array_equal(merged[:, [0, 3, 4]], dev["pooled"][:, [0, 3, 4]])
        for s in U_SERIES:
            assert_moments(merged[s], spec["series"][:, s], chain_length(T, B - h, parts=2), ("halves", s))
        _close_to_spec(merged[list(E_SERIES)], spec["pooled"][list(E_SERIES)], f"halves B={B} T={T}")
    # 5. determinism: a second launch on the same histories gives the same bits
    again = TB.closed_loop_stats(c["run"], c["paths"], c["vref"], c["u0"])
    assert again["per_traj"].cpu().numpy().tobytes() == per.tobytes()
    assert again["pooled"].tobytes() == dev["pooled"].tobytes() and again["fails_total"] == dev["fails_total"]


def test_fewer_steps_than_recorded(gpu):
    c = case(5, 37)
    T = 20
    dev = TB.closed_loop_stats(c["run"], c["paths"], c["vref"], c["u0"], T=T)
    spec = TB.closed_loop_stats_host(c["X"][:, :T + 1], c["U"][:, :T], c["u0"], c["fn"], c["vref"][0],
                                     status=c["status"][:T])
    per = dev["per_traj"].cpu().numpy()
    assert (per[:, :, 0] == T).all() and (dev["pooled"][:, 0] == 5 * T).all()
    assert np.array_equal(per[:, U_SERIES, 3:], spec["per_traj"][:, U_SERIES, 3:])
    for s in U_SERIES:
        for b in range(5):
            assert_moments(per[b, s], spec["series"][b, s], chain_length(T), (b, s))
        assert_moments(dev["pooled"][s], spec["series"][:, s], chain_length(T, 5), ("pooled", s))
    _close_to_spec(per[:, E_SERIES], spec["per_traj"][:, E_SERIES], "per_traj T=20 of 37")
    _close_to_spec(dev["pooled"][list(E_SERIES)], spec["pooled"][list(E_SERIES)], "pooled T=20 of 37")
    assert np.array_equal(dev["fails"].cpu().numpy(), spec["fails"])
    for bad in (0, 38):
        with pytest.raises(ValueError):
            TB.closed_loop_stats(c["run"], c["paths"], c["vref"], c["u0"], T=bad)


def test_status_counting(gpu):
    c = case(5, 37)
    st = torch.zeros((37, 5), dtype=torch.int32, device=c["run"]["X"].device)
    planted = {(0, 0): 2, (36, 0): 6, (5, 3): 6, (6, 3): 2, (7, 3): 3, (8, 1): 1, (9, 4): 1}
    for (t, b), code in planted.items():
        st[t, b] = code
    run = dict(X=c["run"]["X"], U=c["run"]["U"], status=st)
    dev = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"])
    assert dev["fails"].cpu().tolist() == [2, 0, 0, 3, 0] and dev["fails_total"] == 5
    assert dev["per_traj"].cpu().numpy().tobytes() == c["dev"]["per_traj"].cpu().numpy().tobytes()
    part = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"], T=7, mask=[1, 1, 1, 0, 1])
    assert part["fails"].cpu().tolist() == [1, 0, 0, 2, 0] and part["fails_total"] == 1
    run["status"] = None
    dev = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"])
    assert dev["fails"].cpu().tolist() == [0] * 5 and dev["fails_total"] == 0


def test_non_finite_rule(gpu):
    c = case(5, 37)
    X = c["run"]["X"].clone()
    X[2, 11, :] = float("nan")          # the post-step state of step 10 of trajectory 2 (a spline path)
    run = dict(X=X, U=c["run"]["U"], status=c["run"]["status"])
    dev = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"])
    per, ref = dev["per_traj"].cpu().numpy(), c["dev"]["per_traj"].cpu().numpy()
    assert np.isnan(per[2, E_SERIES, 1:]).all() and (per[:, :, 0] == 37).all()
    others = [0, 1, 3, 4]
    assert per[others].tobytes() == ref[others].tobytes() and per[2, U_SERIES].tobytes() == ref[2, U_SERIES].tobytes()
    assert np.isnan(dev["pooled"][list(E_SERIES), 1:]).all() and np.isfinite(dev["pooled"][list(U_SERIES)]).all()
    assert (dev["pooled"][:, 0] == 5 * 37).all()
    out = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"], mask=np.arange(5) != 2)
    assert np.isfinite(out["pooled"]).all() and (out["pooled"][:, 0] == 4 * 37).all()
    X[2, 11, :] = c["run"]["X"][2, 11, :]
    X[0, 3, 3] = float("inf")           # an infinite speed: e_v alone
    dev = TB.closed_loop_stats(run, c["paths"], c["vref"], c["u0"])
    per = dev["per_traj"].cpu().numpy()
    assert np.isnan(per[0, 6, 1:]).all() and np.isfinite(per[0, :6]).all() and np.isfinite(per[1:]).all()


def test_argument_errors_launch_nothing(gpu):
    L = _lib.lib()
    fake, nul = C.c_void_p(16), None
    ps = _lib.Paths()
    ps.kmax, ps.kind, ps.pc = 0, 16, 16                      # never dereferenced: every call below returns first
    ok = dict(paths=C.byref(ps), B=4, N=10, T=5, hist_T=8, hist_x=fake, hist_u=fake, u0=fake, vref=fake, status=nul,
              rec=fake, fails=nul)

    def stats(**kw):
        a = dict(ok, **kw)
        return L.traj_closed_loop_stats(a["paths"], a["B"], a["N"], a["T"], a["hist_T"], a["hist_x"], a["hist_u"],
                                        a["u0"], a["vref"], a["status"], a["rec"], a["fails"], nul)

    for kw in (dict(B=-1), dict(T=0), dict(T=9), dict(N=0), dict(paths=nul), dict(hist_x=nul), dict(hist_u=nul),
               dict(u0=nul), dict(vref=nul), dict(rec=nul)):
        assert stats(**kw) == _lib.TRAJ_E_ARG, kw
    no_kind = _lib.Paths()
    no_kind.kmax, no_kind.pc = 0, 16
    assert stats(paths=C.byref(no_kind)) == _lib.TRAJ_E_ARG
    assert stats(B=0, hist_x=nul, hist_u=nul, u0=nul, vref=nul, rec=nul) == _lib.TRAJ_OK
    assert stats(B=0, T=9) == _lib.TRAJ_E_ARG
    pool = L.traj_closed_loop_stats_pool
    assert pool(-1, fake, nul, nul, fake, nul, nul) == _lib.TRAJ_E_ARG
    assert pool(4, nul, nul, nul, fake, nul, nul) == _lib.TRAJ_E_ARG
    assert pool(4, fake, nul, nul, nul, nul, nul) == _lib.TRAJ_E_ARG
    assert pool(0, nul, nul, nul, nul, nul, nul) == _lib.TRAJ_OK
    torch.cuda.synchronize()


def test_mpc_main_simulate_feeds_the_type1_generator(gpu):
    from trajectory_generation_amd import generation_type1 as G1
    from trajectory_generation_amd import mpc_main as M
    run = M.simulate(B=3, steps=25)
    U = run["U"].cpu().numpy()
    assert U.shape == (3, 25, 2) and run["X"].shape == (3, 26, 6) and np.isfinite(U).all()
    pooled = run["stats"]["pooled"]
    L = chain_length(25, 3)
    for s, name in ((0, "d"), (1, "delta")):
        v = U[:, :, s]
        V = np.abs(v).max()
        assert_moments(pooled[s], v, L, name)
        # numpy's own mean / std of the 75 samples: the same bound plus numpy's few roundings
        assert abs(run["stats"]["mean"][name] - np.mean(v)) <= mean_bound(L, V) + 16 * 2.0 ** -53 * V
        assert abs(run["stats"]["std"][name] ** 2 - np.std(v) ** 2) <= var_bound(L, V) + 64 * 2.0 ** -53 * V * V
    text = M.format_statistics(run["stats"])
    assert f"  - Mean: {np.mean(U[:, :, 0]):.4f}" in text and f"  - Std Dev: {np.std(U[:, :, 1]):.4f}" in text
    ms = TB.mpc_stats(pooled)
    out = G1.generate_steps(4, 50, stats=ms)
    assert tuple(out["X"].shape) == (4, 51, 6) and tuple(out["U"].shape) == (4, 50, 2)
    assert bool(torch.isfinite(out["X"]).all())


def test_dataset_generate_writes_the_statistics_beside_the_sidecar(gpu, tmp_path):
    from trajectory_generation_amd import dataset as D
    from trajectory_generation_amd.workload import make_workload
    B, T = 8, 12
    plain = D.generate(B, T, seed=5, out_prefix=str(tmp_path / "plain"))
    withs = D.generate(B, T, seed=5, out_prefix=str(tmp_path / "stats"), stats=True)
    for suffix in ("_clean.csv", "_noisy.csv", "_status.csv"):
        assert (tmp_path / f"plain{suffix}").read_bytes() == (tmp_path / f"stats{suffix}").read_bytes(), suffix
    assert not (tmp_path / "plain_stats.json").exists()
    for a, b in zip(plain, withs):
        assert torch.equal(a, b)
    doc = json.loads((tmp_path / "stats_stats.json").read_text())
    w = make_workload(B, 20, 0.05, kind="spline", seed=5)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    X, U, st = withs
    want = TB.closed_loop_stats(dict(X=X, U=U, status=st), paths, w["vref"], w["u0"])
    got = np.array([[doc["pooled"][s][f] for f in TB.STATS_FIELDS] for s in TB.STATS_SERIES])
    assert got.tobytes() == want["pooled"].tobytes()
    assert doc["fails_total"] == want["fails_total"] and doc["mpc_stats"] == TB.mpc_stats(want["pooled"])
    assert (got[:, 0] == B * T).all()

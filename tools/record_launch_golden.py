"""Record tests/golden/launch_parent.npz: what every MPC entry point returns on every solver route, from a library
built at the PARENT commit of a change to the host side of the launches (tests/test_launch_parent_gpu.py asserts equal
bit patterns against the file: float64 viewed as int64, NaN bits included).

  git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/trajectory_generation_amd/csrc
  TRAJMPC_LIB=/tmp/parent/trajectory_generation_amd/libtrajmpc.so \
      python tools/record_launch_golden.py --commit <parent commit> [--out tests/golden/launch_parent.npz]

Runs: B = 5, Ts = 0.05, mixed references, seed 5, one per route (ROUTES).  Each records
  the closed loop   run_closed_loop's X, U, status, iters over T = 4 as two launches of two steps (the order kernel and
                    the queue lead run on the second), fused and per step;
  the step entry    mpc_step_batch's seven outputs on the run's first state, traj_debug_step_linearize 1 and 0;
  the QP entry      mpc_qp_batch's outputs on linearize_discretize_batch's matrices.
Once more at N = 20 and N = 24 (EXTRA_HORIZONS): a shared [L] and a [B,L] speed schedule with vref_step = 1,
run_closed_loop_observed with "truth" and "ekf" (3 steps), closed_loop_stats' per_traj / fails / pooled, and a fused run
at B = 9 on a grid of one workgroup (traj_debug_fused_grid(1): the ceil(B / 8) floor), which equals the default grid's.
Every debug switch is back at its default afterwards.  The commit is stored in the file (key "commit")."""
import argparse
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

B, TS, SEED, T, KIND = 5, 0.05, 5, 4, "mixed"
# name: (N, debug switches, configuration keywords)
ROUTES = {
    "cap16": (8, {}, {}),
    "cap40": (20, {}, {}),
    "split40": (24, {}, {}),
    "split48": (44, {}, {}),
    "split64": (60, {}, {}),
    "cap80": (24, {"traj_debug_split_min_n": 41}, {}),
    "long_lds": (60, {"traj_debug_split_max_n": 0}, {}),
    "long256": (70, {}, {}),
    "long512": (130, {}, {}),
    "general": (20, {}, {"x_hi": [1e30, 1e30, 1e30, 2.5, 1e30, 1e30]}),
}
EXTRA_HORIZONS = (20, 24)
DEFAULTS = {"traj_debug_split_min_n": 21, "traj_debug_split_max_n": 64, "traj_debug_step_linearize": 1,
            "traj_debug_fused_grid": 0}
RUN_KEYS = ("X", "U", "status", "iters")
STEP_KEYS = ("u_cmd", "status", "objective", "X_opt", "U_opt", "iters", "polished")
OBS_KEYS = ("X", "Xhat", "Y", "U", "status", "iters")
EKF_LIMITS = {"x_min": -5.0, "x_max": 40.0, "y_min": -6.0, "y_max": 6.0, "phi_min": -3.2, "phi_max": 3.2,
              "vx_min": 0.0, "vx_max": 3.0, "vy_min": -1.0, "vy_max": 1.0, "omega_min": -20.0, "omega_max": 20.0}


@contextlib.contextmanager
def switches(**sw):
    """The given traj_debug_* switches set for the block; every switch of DEFAULTS restored after it."""
    from trajectory_generation_amd import _lib
    try:
        for name, v in sw.items():
            _lib.check(getattr(_lib.lib(), name)(int(v)), name)
        yield
    finally:
        for name, v in DEFAULTS.items():
            getattr(_lib.lib(), name)(v)


def _np(d, keys):
    return {k: d[k].cpu().numpy() for k in keys}


def _setup(N, cfg_kw, batch=B):
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(batch, N, TS, kind=KIND, seed=SEED)
    return TB, w, TB.PathSet.build(w["kinds"], w["pcs"], w["knots"]), TB.config_struct(N=N, Ts=TS, **cfg_kw)


def closed_loop(TB, w, paths, cfg, fused, vref=None, vref_step=0, batch=B):
    """T steps as two launches (fused) or T step calls, on histories of T steps: X, U, status, iters."""
    import torch
    x, u = TB.dev_f64(w["x0"], (batch, 6)).clone(), TB.dev_f64(w["u0"], (batch, 2)).clone()
    dev = x.device
    vr = np.tile(w["vref"], (batch, 1)) if vref is None else vref
    hx = torch.empty((batch, T + 1, 6), dtype=torch.float64, device=dev)
    hu = torch.empty((batch, T, 2), dtype=torch.float64, device=dev)
    hx[:, 0] = x
    st = torch.empty((T, batch), dtype=torch.int32, device=dev)
    it = torch.empty((T, batch), dtype=torch.int32, device=dev)
    if fused:
        for t0 in range(0, T, 2):
            TB.closed_loop_run(x, u, paths, vr, cfg, None, t0, 2, hx, hu, st[t0:], it[t0:], vref_step=vref_step)
    else:
        for t in range(T):
            TB.closed_loop_step(x, u, paths, vr, cfg, None, t, hx, hu, st[t], it[t], vref_step=vref_step)
    return _np(dict(X=hx, U=hu, status=st, iters=it), RUN_KEYS)


def run_route(name):
    """{key: array} of one route's closed loops, steps and QP."""
    N, sw, cfg_kw = ROUTES[name]
    TB, w, paths, cfg = _setup(N, cfg_kw)
    out = {}
    with switches(**sw):
        for fused in (True, False):
            r = closed_loop(TB, w, paths, cfg, fused)
            out.update({f"{'fused' if fused else 'step'}/{k}": v for k, v in r.items()})
    vr = np.tile(w["vref"], (B, 1))
    pr = TB.ref_window_batch(paths, w["x0"][:, 0], vr, N, TS)
    for inlin in (1, 0):
        with switches(traj_debug_step_linearize=inlin, **sw):
            o = _np(TB.mpc_step_batch(w["x0"], w["u0"], pr, vr, cfg), STEP_KEYS)
        out.update({f"mpc_step_inlin{inlin}/{k}": v for k, v in o.items()})
    with switches(**sw):
        # the QP entry on one linearization per instance, the same at every stage (linearize_discretize_batch's)
        A, Bm, g = TB.linearize_discretize_batch(w["x0"], w["u0"], TS)
        rep = lambda m: m[:, None].expand(B, N, *m.shape[1:]).contiguous()   # noqa: E731
        o = _np(TB.mpc_qp_batch(w["x0"], w["u0"], pr, vr, rep(A), rep(Bm), rep(g), cfg), STEP_KEYS)
        out.update({f"mpc_qp/{k}": v for k, v in o.items()})
    return out


def run_extra(N):
    """{key: array} of the schedules, the observed loops, the statistics and the one-workgroup grid at horizon N."""
    from trajectory_generation_amd import observed as OB
    TB, w, paths, cfg = _setup(N, {})
    out = {}
    j = np.arange(T + N)
    S = 1.5 + 0.5 * np.sin(2 * np.pi * (j[None, :] * TS) / 1.5 + np.arange(B)[:, None])
    with switches():
        for tag, sched in (("shared", S[0]), ("rows", S)):
            for fused in (True, False):
                r = closed_loop(TB, w, paths, cfg, fused, vref=sched, vref_step=1)
                out.update({f"sched_{tag}_{'fused' if fused else 'step'}/{k}": v for k, v in r.items()})
        noise = np.random.default_rng(7).normal(size=(B, 3, 5)) * 1e-2
        for est in ("truth", "ekf"):
            r = OB.run_closed_loop_observed(w["x0"], w["u0"], paths, w["vref"], 3, cfg, params=EKF_LIMITS,
                                            estimator=est, noise=noise)
            out.update({f"observed_{est}/{k}": v for k, v in _np(r, OBS_KEYS).items()})
        run = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)
        s = TB.closed_loop_stats(run, paths, w["vref"], w["u0"])
        out["stats/per_traj"], out["stats/fails"] = s["per_traj"].cpu().numpy(), s["fails"].cpu().numpy()
        out["stats/pooled"] = np.asarray(s["pooled"])
    TB9, w9, paths9, cfg9 = _setup(N, {}, batch=9)
    grids = {}
    for grid in (1, 0):
        with switches(traj_debug_fused_grid=grid):
            grids[grid] = closed_loop(TB9, w9, paths9, cfg9, True, batch=9)
    for k in RUN_KEYS:
        if not np.array_equal(bits(grids[1][k]), bits(grids[0][k])):
            raise AssertionError(f"N = {N}: the one-workgroup grid's {k} differs from the default grid's")
    out.update({f"grid1_B9/{k}": v for k, v in grids[1].items()})
    return out


def bits(a):
    """float64 as its int64 bit patterns (NaN payloads compare); everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def cases():
    """(case name, function, argument) of every recorded group."""
    return [(f"route_{n}", run_route, n) for n in ROUTES] + [(f"extra_N{N}", run_extra, N) for N in EXTRA_HORIZONS]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built at (stored in the file)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "launch_parent.npz"))
    args = ap.parse_args()
    from trajectory_generation_amd import _lib
    out = {"commit": np.array(args.commit), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for name, fn, arg in cases():
        out.update({f"{name}/{k}": v for k, v in fn(arg).items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(out) - 2} arrays in {len(cases())} groups from {_lib.LIB_PATH} ({args.commit}), "
          f"{os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

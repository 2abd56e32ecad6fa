"""The closed loop on a state estimate against the plain per-step closed loop -> profiles/closed_obs_bench.json.

  python tools/closed_obs_bench.py [--B 4096] [--T 240] [--N 20] [--Ts 0.05] [--kind mixed] [--reps 5] [--json PATH]

One process.  The workload is workload.make_workload_device's; the measurement noise is seeded (sqrt(EKF_R) sigmas), the
EKF's omega limits are +-20 (the truth leaves +-6 on these paths).  After one warm-up of each, the runs alternate `reps`
times, each timed by the host clock around a call that ends in a device synchronise:
  per_step       batch.run_closed_loop(fused=False): the plain loop, one launch sequence per step -- the baseline;
  obs_truth      observed.run_closed_loop_observed(estimator="truth"): the same steps + the copy and the observe kernel;
  obs_ekf_1      estimator="ekf", the EKF step one thread per trajectory (traj_debug_obs_lanes(1));
  obs_ekf_16     estimator="ekf", sixteen lanes per trajectory (traj_debug_obs_lanes(16));
  graph_ekf_1 / graph_ekf_16   the EKF run captured once as a graph: the replay alone.
Beside them the observe kernel alone (traj_closed_loop_observe, EKF) by device events in both forms: `--kreps` launches
between one event pair, on the state a finished run left.  Per figure: median, min, max.  The two forms' runs are
compared bit for bit.  Needs the GPU; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (wide enough for the truth on every kind: a parabola path reaches |Y| ~ 90 m in 240 steps)
LIMITS = {"x_min": -20.0, "x_max": 100.0, "y_min": -300.0, "y_max": 300.0, "phi_min": -3.2, "phi_max": 3.2,
          "vx_min": 0.0, "vx_max": 3.0, "vy_min": -1.0, "vy_max": 1.0, "omega_min": -20.0, "omega_max": 20.0}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--Ts", type=float, default=0.05)
    ap.add_argument("--kind", default="mixed", choices=("mixed", "spline", "parabola"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "closed_obs_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("closed_obs_bench needs the GPU")
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd import knet as K
    from trajectory_generation_amd import observed as OB
    from trajectory_generation_amd import workload as W
    sync = torch.cuda.synchronize

    w = W.make_workload_device(a.B, a.N, a.Ts, kind=a.kind)
    paths, vref, x0, u0 = w["paths"], w["vref"], w["x0"], w["u0"]
    cfg = TB.config_struct(N=a.N, Ts=a.Ts)
    noise = torch.as_tensor(np.random.default_rng(7).normal(size=(a.B, a.T, 5)) * np.sqrt(np.array(K.EKF_R)),
                            device=x0.device)

    def per_step():
        return TB.run_closed_loop(x0, u0, paths, vref, a.T, cfg, fused=False)

    def observed(est, lanes, graph=False):
        OB.set_obs_lanes(lanes)
        return OB.run_closed_loop_observed(x0, u0, paths, vref, a.T, cfg, params=LIMITS, estimator=est, noise=noise,
                                           graph=graph)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t0, r

    graphs = {lanes: observed("ekf", lanes, graph=True) for lanes in (1, 16)}   # capture + one replay: their warm-up
    runs = {"per_step": per_step, "obs_truth": lambda: observed("truth", 1), "obs_ekf_1": lambda: observed("ekf", 1),
            "obs_ekf_16": lambda: observed("ekf", 16), "graph_ekf_1": graphs[1]["replay"],
            "graph_ekf_16": graphs[16]["replay"]}
    times = {k: [] for k in runs}
    last = {}
    for rep in range(a.reps + 1):          # the first pass is the warm-up of each
        for k, fn in runs.items():
            dt, r = timed(fn)
            if k.startswith("graph"):      # (the replay writes into the capture's tensors: keep what is compared)
                r = {q: r[q].clone() for q in ("X", "Xhat", "U", "status")}
            last[k] = r
            if rep:
                times[k].append(dt)

    def kernel_ms(lanes):
        """the observe kernel alone (EKF), `kreps` launches between one event pair, on copies of a finished state"""
        OB.set_obs_lanes(lanes)
        r = last["obs_ekf_1"]
        x, xh, P, u = (r[k].clone() for k in ("x", "xhat", "P", "u"))
        o, lim, p = OB.obs_config("ekf"), K.limits_struct(LIMITS), TB.params_struct(LIMITS)
        L, ptr = _lib.lib(), _lib.ptr

        def launch():
            _lib.check(L.traj_closed_loop_observe(C.byref(p), a.Ts, C.byref(lim), C.byref(o), a.B, ptr(x), ptr(xh), ptr(P),
                                                  ptr(u), None, 0, 0, None, None, None, None, _lib.stream()), "observe")
        launch()
        sync()
        with _lib.event_pair() as e:
            for _ in range(a.kreps):
                launch()
        sync()
        return e[0].elapsed_time(e[1]) / a.kreps

    kern = {f"observe_kernel_ms_lanes_{lanes}": spread([kernel_ms(lanes) for _ in range(a.reps)]) for lanes in (1, 16)}
    OB.set_obs_lanes(_lib.OBS_DEFAULT_LANES)

    same = lambda p, q, keys: all(bool(((p[k] == q[k]) | ((p[k] != p[k]) & (q[k] != q[k]))).all()) for k in keys)  # noqa: E731
    keys = ("X", "Xhat", "U", "status")
    err = OB.estimation_errors(last["obs_ekf_1"], skip=5)
    out = {"B": a.B, "T": a.T, "N": a.N, "Ts": a.Ts, "kind": a.kind, "reps": a.reps, "kreps": a.kreps,
           "device": torch.cuda.get_device_name(0), "steps": a.B * a.T}
    out.update({k + "_s": spread(v) for k, v in times.items()})
    out.update(kern)
    base = out["per_step_s"]["median"]
    out["over_per_step_at_median"] = {k: out[k + "_s"]["median"] / base for k in runs if k != "per_step"}
    out["lanes_16_faster_beyond_spread"] = bool(out["obs_ekf_16_s"]["max"] < out["obs_ekf_1_s"]["min"])
    out["lanes_1_faster_beyond_spread"] = bool(out["obs_ekf_1_s"]["max"] < out["obs_ekf_16_s"]["min"])
    out["default_lanes"] = _lib.OBS_DEFAULT_LANES
    out["compare"] = {
        "truth_is_per_step": same(last["obs_truth"], last["per_step"], ("X", "U", "status", "iters")),
        "lanes_16_is_lanes_1": same(last["obs_ekf_16"], last["obs_ekf_1"], keys),
        "graph_1_is_stream": same(last["graph_ekf_1"], last["obs_ekf_1"], keys),
        "graph_16_is_stream": same(last["graph_ekf_16"], last["obs_ekf_1"], keys),
        "status_optimal_fraction_ekf": float((last["obs_ekf_1"]["status"] == 0).float().mean()),
        "status_optimal_fraction_truth": float((last["obs_truth"]["status"] == 0).float().mean()),
        "mse_est_over_mse_meas": err["ratio"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    c = out["compare"]
    if not (c["truth_is_per_step"] and c["lanes_16_is_lanes_1"] and c["graph_1_is_stream"] and c["graph_16_is_stream"]):
        raise SystemExit("the runs that must agree bit for bit differ")


if __name__ == "__main__":
    main()

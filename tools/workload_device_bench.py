"""The closed loop's workload built on the host against built on the GPU -> profiles/workload_device_bench.json.

  python tools/workload_device_bench.py [--B 4096] [--N 20] [--T 25] [--reps 5] [--json PATH]

One process; per workload kind (spline, mixed), after one warm-up of each, the builders alternate `reps` times:
  host     workload.make_workload (one numpy Generator per trajectory) and batch.PathSet.build (the stacked solve per
           knot count, then the upload); beside it the per-trajectory spline_natural loop PathSet.build ran before,
           on the same knots;
  device   workload.make_workload_device: wall time of the call to a device synchronise, and the kernel alone by
           device events around traj_gen_workload_batch;
and end to end, the analogue of bench.py's 'host_io': build the workload and its paths, T fused closed-loop steps,
histories X, U, status back in host numpy -- with the host builders and with the device builder.
Per figure: median, min, max over the repeats.  The two workloads are compared as tests/test_workload_gpu.py compares
them (draws equal, the rest to rounding).  Needs the GPU; there is no CPU fallback.
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


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def timed(f, sync):
    sync()
    t0 = time.perf_counter()
    r = f()
    sync()
    return time.perf_counter() - t0, r


def loop_rows(TB, w, kmax):
    """PathSet.build's host arrays by the per-trajectory spline_natural loop (what it ran before the stacked solve)."""
    B = len(w["kinds"])
    xk, coef, nk = np.zeros((B, kmax)), np.zeros((B, kmax - 1, 4)), np.zeros(B, np.int32)
    for b in range(B):
        if w["kinds"][b] == 2:
            kx, ky = w["knots"][b]
            nk[b] = len(kx)
            xk[b, :len(kx)] = kx
            coef[b, :len(kx) - 1] = TB.spline_natural(kx, ky)
    return nk, xk, coef


def kernel_ms(_lib, TB, W, B, kind):
    """traj_gen_workload_batch alone, by device events."""
    import torch
    code, words, kmax = W._workload_args(B, kind, 0, 0)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    outs = [torch.empty(B, **i32), torch.empty((B, 4), **f64), torch.empty(B, **i32), torch.empty((B, kmax), **f64),
            torch.empty((B, kmax), **f64), torch.empty((B, kmax - 1, 4), **f64), torch.empty((B, 6), **f64),
            torch.empty((B, 2), **f64)]
    with _lib.event_pair() as ev:
        _lib.check(_lib.lib().traj_gen_workload_batch(C.byref(TB.params_struct()), code, _lib.ptr(words), len(words), 0,
                                                      B, kmax, *[_lib.ptr(t) for t in outs], _lib.stream()),
                   "traj_gen_workload_batch")
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(a, kind):
    import torch
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd import workload as W
    sync = torch.cuda.synchronize
    cfg = TB.config_struct(N=a.N, Ts=a.Ts)
    host_np = lambda r: [r[k].cpu().numpy() for k in ("X", "U", "status")]   # noqa: E731

    def e2e_host():
        w = W.make_workload(a.B, a.N, a.Ts, kind=kind)
        paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
        return host_np(TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], a.T, cfg))

    def e2e_device():
        w = W.make_workload_device(a.B, a.N, a.Ts, kind=kind)
        return host_np(TB.run_closed_loop(w["x0"], w["u0"], w["paths"], w["vref"], a.T, cfg))

    w = W.make_workload(a.B, a.N, a.Ts, kind=kind)
    kmax = max([2] + [len(k[0]) for k in w["knots"] if k is not None])
    runs = {
        "host_make_workload_s": lambda: W.make_workload(a.B, a.N, a.Ts, kind=kind),
        "host_pathset_build_s": lambda: TB.PathSet.build(w["kinds"], w["pcs"], w["knots"]),
        "host_spline_rows_stacked_s": lambda: TB.spline_rows(w["kinds"], w["knots"], kmax),
        "host_spline_rows_loop_s": lambda: loop_rows(TB, w, kmax),
        "device_make_workload_s": lambda: W.make_workload_device(a.B, a.N, a.Ts, kind=kind),
        "end_to_end_host_build_s": e2e_host,
        "end_to_end_device_build_s": e2e_device,
    }
    res = {k: [] for k in runs}
    kern = []
    for rep in range(a.reps + 1):            # the first pass is the warm-up of each
        for k, f in runs.items():
            dt, _ = timed(f, sync)
            if rep:
                res[k].append(dt)
        ms = kernel_ms(_lib, TB, W, a.B, kind)
        if rep:
            kern.append(ms)
    out = {k: spread(v) for k, v in res.items()}
    out["device_kernel_ms"] = spread(kern)
    med = lambda k: out[k]["median"]   # noqa: E731
    host_build = med("host_make_workload_s") + med("host_pathset_build_s")
    out["host_build_s_at_median"] = host_build
    out["host_over_device_build_at_median"] = host_build / med("device_make_workload_s")
    out["device_build_faster_beyond_spread"] = bool(
        out["device_make_workload_s"]["max"] < out["host_make_workload_s"]["min"] + out["host_pathset_build_s"]["min"])
    out["loop_over_stacked_rows_at_median"] = med("host_spline_rows_loop_s") / med("host_spline_rows_stacked_s")
    out["end_to_end_host_over_device_at_median"] = med("end_to_end_host_build_s") / med("end_to_end_device_build_s")
    out["end_to_end_device_faster_beyond_spread"] = bool(
        out["end_to_end_device_build_s"]["max"] < out["end_to_end_host_build_s"]["min"])
    steps = a.B * a.T
    out["end_to_end_steps_per_s_at_median"] = {"host_build": steps / med("end_to_end_host_build_s"),
                                               "device_build": steps / med("end_to_end_device_build_s")}
    # the two workloads: the draws equal, the rest to rounding; the two end-to-end histories side by side
    d = W.make_workload_device(a.B, a.N, a.Ts, kind=kind)
    x0 = d["x0"].cpu().numpy()
    loop = loop_rows(TB, w, kmax)
    stacked = TB.spline_rows(w["kinds"], w["knots"], kmax)
    Xh, Xd = e2e_host()[0], e2e_device()[0]
    # control for the histories: the host workload again with every Y moved by one ulp -- how far T closed-loop steps
    # carry a last-bit difference of the start, whatever builder it came from
    x0p = w["x0"].copy()
    x0p[:, 1] = np.nextafter(x0p[:, 1], np.inf)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    Xp = TB.run_closed_loop(x0p, w["u0"], paths, w["vref"], a.T, cfg)["X"].cpu().numpy()

    def per_trajectory(A, B_):
        d = np.abs(A - B_).reshape(A.shape[0], -1).max(axis=1)
        return {"median": float(np.median(d)), "p99": float(np.quantile(d, 0.99)), "max": float(d.max()),
                "above_1e-6": int((d > 1e-6).sum())}

    out["compare"] = {
        "history_diff_per_trajectory_device_vs_host_build": per_trajectory(Xd, Xh),
        "history_diff_per_trajectory_host_Y_plus_1ulp_vs_host": per_trajectory(Xp, Xh),
        "draws_identical": bool((x0[:, [0, 3, 4, 5]] == w["x0"][:, [0, 3, 4, 5]]).all()
                                and (d["pcs"].cpu().numpy() == w["pcs"]).all()
                                and (d["kinds"].cpu().numpy() == w["kinds"]).all()),
        "x0_max_abs_diff": float(np.abs(x0 - w["x0"]).max()),
        "coef_max_abs_diff": float(np.abs(d["paths"].coef.cpu().numpy() - stacked[2]).max()),
        "stacked_rows_equal_loop_bits": bool(all((p == q).all() for p, q in zip(loop, stacked))),
        "history_max_abs_diff_after_T_steps": float(np.abs(Xh - Xd).max()),
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--Ts", type=float, default=0.05)
    ap.add_argument("--T", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "workload_device_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("workload_device_bench needs the GPU")
    out = {"B": a.B, "N": a.N, "Ts": a.Ts, "T": a.T, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "spline": measure(a, "spline"), "mixed": measure(a, "mixed")}
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    ok = all(out[k]["compare"]["draws_identical"] and out[k]["compare"]["stacked_rows_equal_loop_bits"]
             for k in ("spline", "mixed"))
    if not ok:
        raise SystemExit("the device workload's draws or the stacked rows differ from the host's")


if __name__ == "__main__":
    main()

"""The closed loop on closed tracks against the plain per-step closed loop -> profiles/track_loop_bench.json.

  python tools/track_loop_bench.py [--B 4096] [--T 240] [--N 20] [--Ts 0.02] [--reps 5] [--kreps 50] [--json PATH]

One process.  The track loop runs workload.make_track_workload (eight 16-knot circuits shared by the B trajectories);
the yardstick is the existing per-step loop on the spline workload, batch.run_closed_loop(fused=False) with the warm
start off -- like the track loop it starts every step's rho cold.  After one warm-up of each, the runs alternate `reps`
times, each timed by the host clock around a call that ends in a device synchronise:
  per_step          the yardstick (its own workload: other QPs, the same shapes and launch structure)
  track_1 / _16     track.run_closed_loop_track, stream-ordered, the track kernel one thread / sixteen lanes per trajectory
  graph_1 / _16     the same run captured once as a graph: the replay alone
Beside them the track kernel alone (traj_closed_loop_track_window: the loop's first launch) in both lane forms and the
plant kernel alone (traj_closed_loop_track_plant), by device events: `--kreps` launches between one event pair, on the
state a finished run left.  Per figure: median, min, max.  The two forms' runs are compared bit for bit.  Needs the GPU;
there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--Ts", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "track_loop_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_loop_bench needs the GPU")
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd import track as TK
    from trajectory_generation_amd import workload as W
    sync = torch.cuda.synchronize

    w = W.make_track_workload(a.B, a.N, a.Ts, seed=0)
    tracks = TK.TrackSet.build(w["knots"], w["track_of"])
    cfg = TB.config_struct(N=a.N, Ts=a.Ts)
    x0, u0, vref = (TB.dev_f64(w[k]) for k in ("x0", "u0", "vref"))
    ws = W.make_workload_device(a.B, a.N, a.Ts, kind="spline")
    cfg0 = TB.config_struct(N=a.N, Ts=a.Ts, warm_start=0)

    def per_step():
        return TB.run_closed_loop(ws["x0"], ws["u0"], ws["paths"], ws["vref"], a.T, cfg0, fused=False)

    def on_track(lanes, graph=False):
        TK.set_track_lanes(lanes)
        return TK.run_closed_loop_track(x0, u0, tracks, vref, a.T, cfg, graph=graph)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t0, r

    graphs = {lanes: on_track(lanes, graph=True) for lanes in (1, 16)}   # capture + one replay: their warm-up
    runs = {"per_step": per_step, "track_1": lambda: on_track(1), "track_16": lambda: on_track(16),
            "graph_1": graphs[1]["replay"], "graph_16": graphs[16]["replay"]}
    keys = ("X", "U", "S", "status", "iters")
    times = {k: [] for k in runs}
    last = {}
    for rep in range(a.reps + 1):          # the first pass is the warm-up of each
        for k, fn in runs.items():
            dt, r = timed(fn)
            if k.startswith("graph"):      # (the replay writes into the capture's tensors: keep what is compared)
                r = {q: r[q].clone() for q in keys}
            last[k] = r
            if rep:
                times[k].append(dt)

    L, ptr = _lib.lib(), _lib.ptr
    fin = last["track_16"]
    se, p = TK.search_struct(), TB.params_struct(None)
    ts = tracks.struct(a.B, x0.device)

    def events(launch):
        launch()
        sync()
        with _lib.event_pair() as e:
            for _ in range(a.kreps):
                launch()
        sync()
        return e[0].elapsed_time(e[1]) / a.kreps

    def track_kernel_ms(lanes):
        """the loop's first launch alone on the final state (local search from the final place)"""
        TK.set_track_lanes(lanes)
        x, s = fin["x"].clone(), fin["S"][:, -1].clone()
        pref = torch.empty((a.B, a.N + 1, 3), dtype=torch.float64, device=x.device)
        vr = torch.empty((a.B, a.N + 1), dtype=torch.float64, device=x.device)
        return events(lambda: _lib.check(L.traj_closed_loop_track_window(
            C.byref(ts), C.byref(se), a.B, a.N, a.Ts, ptr(x), ptr(s), ptr(vref), a.N + 1, a.N + 1, 0, ptr(pref), ptr(vr),
            _lib.stream()), "traj_closed_loop_track_window"))

    def plant_kernel_ms():
        x, u, uc = fin["x"].clone(), fin["u"].clone(), fin["u"].clone()
        return events(lambda: _lib.check(L.traj_closed_loop_track_plant(
            C.byref(p), a.Ts, a.B, ptr(x), ptr(u), ptr(uc), None, 0, 0, None, None, None, _lib.stream()),
            "traj_closed_loop_track_plant"))

    kern = {f"track_kernel_ms_lanes_{lanes}": spread([track_kernel_ms(lanes) for _ in range(a.reps)]) for lanes in (1, 16)}
    kern["plant_kernel_ms"] = spread([plant_kernel_ms() for _ in range(a.reps)])
    TK.set_track_lanes(_lib.TRACK_DEFAULT_LANES)

    same = lambda p_, q_: all(bool(((p_[k] == q_[k]) | ((p_[k] != p_[k]) & (q_[k] != q_[k]))).all()) for k in keys)  # noqa: E731
    err = TK.tracking_errors(fin, tracks)
    out = {"B": a.B, "T": a.T, "N": a.N, "Ts": a.Ts, "reps": a.reps, "kreps": a.kreps,
           "device": torch.cuda.get_device_name(0), "steps": a.B * a.T}
    out.update({k + "_s": spread(v) for k, v in times.items()})
    out.update({k + "_ms_per_step": out[k + "_s"]["median"] / a.T * 1e3 for k in runs})
    out.update(kern)
    base = out["per_step_s"]["median"]
    out["over_per_step_at_median"] = {k: out[k + "_s"]["median"] / base for k in runs if k != "per_step"}
    k1, k16 = out["track_kernel_ms_lanes_1"], out["track_kernel_ms_lanes_16"]
    out["lanes_16_kernel_faster_beyond_spread"] = bool(k16["max"] < k1["min"])
    out["lanes_1_kernel_faster_beyond_spread"] = bool(k1["max"] < k16["min"])
    out["lanes_16_loop_faster_beyond_spread"] = bool(out["track_16_s"]["max"] < out["track_1_s"]["min"])
    out["lanes_1_loop_faster_beyond_spread"] = bool(out["track_1_s"]["max"] < out["track_16_s"]["min"])
    out["default_lanes"] = _lib.TRACK_DEFAULT_LANES
    out["compare"] = {
        "lanes_16_is_lanes_1": same(last["track_16"], last["track_1"]),
        "graph_1_is_stream": same(last["graph_1"], last["track_1"]),
        "graph_16_is_stream": same(last["graph_16"], last["track_1"]),
        "status_optimal_fraction_track": float((fin["status"] == 0).float().mean()),
        "status_optimal_fraction_per_step": float((last["per_step"]["status"] == 0).float().mean()),
        "max_abs_e_c_after_100_steps": float(err["e_c"][:, min(100, a.T):].abs().max()) if a.T > 0 else 0.0,
        "laps_min_max": [float(err["laps"].min()), float(err["laps"].max())],
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    c = out["compare"]
    if not (c["lanes_16_is_lanes_1"] and c["graph_1_is_stream"] and c["graph_16_is_stream"]):
        raise SystemExit("the runs that must agree bit for bit differ")


if __name__ == "__main__":
    main()

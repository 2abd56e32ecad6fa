"""Where the time of the open-loop dataset generation goes, at the reference's own size (B = 5,000 trajectories of
T = 1,200 steps, Ts = 0.01): host draw of the profiles, upload, the kernel in both forms (LDS-staged and direct
stores, traj_gen_debug_store_form), download, CSV write.  Writes / updates profiles/openloop_probe.json.

  python tools/openloop_probe.py --gpu [--out FILE]             the GPU legs (needs the MI355X)
  python tools/openloop_probe.py --cpu [--reference-dir DIR]    the CPU figure: the per-trajectory numpy loop
        (limiter + Euler loop) on 16 trajectories -- the reference's own generation_type1.py when DIR (its
        generation_traj folder) is given, otherwise this package's host port of it

Kernel times are HIP events around single launches, after warm-up, the two forms alternating within one process;
the other legs are a host clock around work that ends in a device synchronize.  No pass bar: the figures are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "openloop_probe.json")


def cpu_leg(args):
    from trajectory_generation_amd import generation_type1 as G
    n, T, Ts = 16, args.T, 0.01
    if args.reference_dir:
        import matplotlib
        matplotlib.use("Agg")
        sys.path.insert(0, args.reference_dir)
        import generation_type1 as R
        source = "reference generation_type1.py"
    else:
        R, source = G, "trajectory_generation_amd.generation_type1 (host port)"
    x0, u_raw, _ = G.draw_controls(n, T, Ts, seed=42)
    t_slew = t_sim = 0.0
    for b in range(n):
        t0 = time.perf_counter()
        U = np.stack([np.clip(R.apply_du_bounds(u_raw[b, :, c], *G.DU_BOUNDS[c]), *G.U_BOUNDS[c]) for c in range(2)], 1)
        t1 = time.perf_counter()
        R.simulate_trajectory(x0[b], U, Ts, R.Params)
        t2 = time.perf_counter()
        t_slew += t1 - t0
        t_sim += t2 - t1
    return {"source": source, "trajectories": n, "T": T, "slew_limiter_ms_per_trajectory": 1e3 * t_slew / n,
            "euler_loop_ms_per_trajectory": 1e3 * t_sim / n,
            "extrapolated_s_for_B": (t_slew + t_sim) / n * args.B, "B": args.B}


def gpu_leg(args):
    import torch
    from trajectory_generation_amd import _lib, batch as TB, dataset as DS
    from trajectory_generation_amd import generation_type1 as G
    B, T, Ts = args.B, args.T, 0.01
    dev = TB.require_gpu()
    res = {"B": B, "T": T, "Ts": Ts, "device": torch.cuda.get_device_name(dev)}

    t0 = time.perf_counter()
    x0, u_raw, _ = G.draw_controls(B, T, Ts, seed=42)
    res["host_draw_s"] = time.perf_counter() - t0

    torch.cuda.synchronize()
    ups = []
    for _ in range(5):
        t0 = time.perf_counter()
        dx0, du = torch.as_tensor(x0, device=dev), torch.as_tensor(u_raw, device=dev)
        torch.cuda.synchronize()
        ups.append(time.perf_counter() - t0)
    res["upload_ms"] = 1e3 * statistics.median(ups[1:])

    cfg = TB.gen_config_struct(_lib.GEN_MODEL_TYPE1, Ts)
    forms = {"staged": _lib.GEN_FORM_STAGED, "direct": _lib.GEN_FORM_DIRECT}
    outs, times = {}, {k: [] for k in forms}
    for rep in range(args.warmup + args.reps):
        for name, form in forms.items():
            TB.set_gen_store_form(form)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = TB.simulate_open_loop(dx0, du, cfg)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    TB.set_gen_store_form(_lib.GEN_FORM_DEFAULT)
    bytes_moved = B * T * 2 * 8 * 2 + B * (T + 1) * 6 * 8
    for name, ts in times.items():
        med = statistics.median(ts)
        res[f"kernel_{name}_ms"] = {"median": med, "min": min(ts), "max": max(ts), "reps": len(ts),
                                    "GB_per_s_at_median": bytes_moved / med / 1e6,
                                    "trajectory_steps_per_s_at_median": B * T / med * 1e3}
    res["forms_bit_identical"] = bool(torch.equal(outs["staged"]["X"], outs["direct"]["X"])
                                      and torch.equal(outs["staged"]["U"], outs["direct"]["U"]))
    out = TB.simulate_open_loop(dx0, du, cfg)
    torch.cuda.synchronize()
    res["default_equals_both"] = bool(torch.equal(out["X"], outs["staged"]["X"]) and res["forms_bit_identical"])

    downs = []
    for _ in range(3):
        t0 = time.perf_counter()
        Xh, Uh = out["X"].cpu().numpy(), out["U"].cpu().numpy()
        downs.append(time.perf_counter() - t0)
    res["download_ms"] = 1e3 * statistics.median(downs)

    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        DS.write_csv(os.path.join(d, "probe"), Xh, Uh, np.arange(B), Ts)
        res["csv_write_s"] = time.perf_counter() - t0
        res["csv_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))

    default = {v: k for k, v in forms.items()}[_lib.GEN_DEFAULT_FORM]   # TRAJ_GEN_DEFAULT_FORM
    k = res[f"kernel_{default}_ms"]["median"] * 1e-3
    total = res["host_draw_s"] + res["upload_ms"] * 1e-3 + k + res["download_ms"] * 1e-3 + res["csv_write_s"]
    res["end_to_end_s"] = total
    res["share_of_end_to_end"] = {"host_draw": res["host_draw_s"] / total, "upload": res["upload_ms"] * 1e-3 / total,
                                  "kernel": k / total, "download": res["download_ms"] * 1e-3 / total,
                                  "csv_write": res["csv_write_s"] / total}
    res["default_form"] = default
    res["faster_form"] = min(forms, key=lambda n: res[f"kernel_{n}_ms"]["median"])
    res["default_form_note"] = (f"the library's default (TRAJ_GEN_DEFAULT_FORM) is the form measured faster at B = 5,000, "
                                f"T = 1,200.  Reading of the figures, not measured further: {(B + 63) // 64} one-wave "
                                "workgroups leave most CUs with one wave, whose serial instruction stream is the kernel "
                                "time, at a small fraction of the HBM rate; the staged form's LDS round trip, barriers and "
                                "index arithmetic lengthen that stream, while the direct form's strided stores are issued "
                                "and retire behind the arithmetic")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reference-dir", default=None)
    ap.add_argument("--B", type=int, default=5000)
    ap.add_argument("--T", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.cpu:
        doc["cpu_numpy_loop"] = cpu_leg(args)
    if args.gpu:
        doc["gpu"] = gpu_leg(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()

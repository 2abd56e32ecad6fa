"""Where the time of the type-2 (piecewise state machine) dataset generation goes, at the reference's own size
(B = 5,000 trajectories of T = 1,200 steps, Ts = 0.01): host seeding (x0 and the 5,000 PCG64 states), upload, the FSM
kernel (traj_gen_piecewise_batch), download, CSV write -- and, as the yardstick, the type-2 replay kernel
(traj_gen_simulate_batch, model 2) on the controls the FSM kernel produced, alternating with it in the same run.
Writes / updates profiles/piecewise_probe.json.

  python tools/piecewise_probe.py --gpu [--out FILE]             the GPU legs (needs the MI355X)
  python tools/piecewise_probe.py --cpu [--reference-dir DIR]    the CPU figure: sample_controls_piecewise plus the
        Euler loop on 4 trajectories -- the reference's own generation_type2.py when DIR (its generation_traj folder)
        is given, otherwise this package's host port of it

Kernel times are HIP events around the library call alone (buffers allocated before), after warm-up, the two kernels
alternating; the other legs are a host clock around work that ends in a device synchronize.  The GPU leg also records
the worst errors against tests/golden/generation2.npz (the figures the GPU tests hold to their bars).  No pass bar:
the figures are recorded.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "piecewise_probe.json")


def cpu_leg(args):
    from trajectory_generation_amd import generation_type2 as G
    n, T, Ts = 4, args.T, 0.01
    if args.reference_dir:
        import matplotlib
        matplotlib.use("Agg")
        sys.path.insert(0, args.reference_dir)
        import generation_type2 as R
        source = "reference generation_type2.py"
    else:
        R, source = G, "trajectory_generation_amd.generation_type2 (host port)"
    x0 = G.draw_x0(n, seed=42)
    rules = R.ControlRules()
    t_ctl = t_sim = 0.0
    for b in range(n):
        t0 = time.perf_counter()
        U, _ = R.sample_controls_piecewise(T, Ts, x0[b], R.Params, rules, seed=42 + b)
        t1 = time.perf_counter()
        X = np.empty((T + 1, 6))
        X[0] = x0[b]
        for k in range(T):                                   # generation_type2.py:182-187
            X[k + 1] = X[k] + Ts * R.f_cont(X[k], U[k], R.Params)
            X[k + 1, 3] = max(X[k + 1, 3], 0.0)
            X[k + 1, 5] = float(np.clip(X[k + 1, 5], -6, 6))
        t2 = time.perf_counter()
        t_ctl += t1 - t0
        t_sim += t2 - t1
    return {"source": source, "trajectories": n, "T": T, "controller_s_per_trajectory": t_ctl / n,
            "euler_loop_s_per_trajectory": t_sim / n, "s_per_trajectory": (t_ctl + t_sim) / n,
            "extrapolated_s_for_B": (t_ctl + t_sim) / n * args.B, "B": args.B}


def fixture_errors(TB, G, _lib):
    """Worst errors of the kernel on the three fixture cases (the quantities tests/test_generation2_gpu.py bounds)."""
    import torch
    gold = np.load(os.path.join(ROOT, "tests", "golden", "generation2.npz"))
    res = {}
    for pre in ("a", "b", "c"):
        rules = G.ControlRules(v_turn_max=0.6, v_high=1.0) if pre == "b" else G.ControlRules()
        Uref, Xref = gold[f"{pre}_U"], gold[f"{pre}_X"]
        T, Ts = Uref.shape[1], float(gold[f"{pre}_Ts"])
        out = TB.simulate_piecewise(gold[f"{pre}_x0"], G.pcg64_states(gold[f"{pre}_seeds"]), T, Ts, rules)
        torch.cuda.synchronize()
        X, U, M = (out[k].cpu().numpy() for k in ("X", "U", "mode"))
        bar = T * Ts * 1e-12 * (1.0 + gold[f"{pre}_Fmax"])
        res[pre] = {"modes_identical": bool(np.array_equal(M, gold[f"{pre}_mode"])),
                    "d_samples_differing": int((U[:, :, 0].view(np.int64) != Uref[:, :, 0].view(np.int64)).sum()),
                    "delta_samples_differing": int((U[:, :, 1].view(np.int64) != Uref[:, :, 1].view(np.int64)).sum()),
                    "worst_abs_delta_error": float(np.abs(U[:, :, 1] - Uref[:, :, 1]).max()),
                    "worst_abs_X_error": float(np.abs(X - Xref).max()),
                    "worst_X_error_over_bar": float((np.abs(X - Xref).max(axis=1) / bar[:, None]).max())}
    seeds = np.arange(1000, 1065)
    got, _ = TB.rng_draw_batch(G.pcg64_states(seeds), 4096, _lib.RNG_NORMAL)
    want = np.stack([np.random.default_rng(int(s)).standard_normal(4096) for s in seeds])
    ulps = np.abs(got.view(np.int64) - want.view(np.int64))
    tail = np.abs(want) > 3.6541528853610087963519472518
    res["normals_65x4096"] = {"tail_draws": int(tail.sum()), "worst_tail_ulps": int(ulps[tail].max()),
                              "body_draws_differing": int((ulps[~tail] != 0).sum())}
    return res


def gpu_leg(args):
    import torch
    from trajectory_generation_amd import _lib, batch as TB, dataset as DS
    from trajectory_generation_amd import generation_type2 as G
    B, T, Ts = args.B, args.T, 0.01
    dev = TB.require_gpu()
    res = {"B": B, "T": T, "Ts": Ts, "device": torch.cuda.get_device_name(dev)}

    t0 = time.perf_counter()
    x0 = G.draw_x0(B, seed=42)
    t1 = time.perf_counter()
    states = G.pcg64_states(42 + np.arange(B))
    res["host_seeding_s"] = {"x0": t1 - t0, "pcg64_states": time.perf_counter() - t1}
    host_s = time.perf_counter() - t0

    torch.cuda.synchronize()
    ups = []
    for _ in range(5):
        t0 = time.perf_counter()
        dx0 = torch.as_tensor(x0, device=dev)
        dst = torch.from_numpy(states.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        ups.append(time.perf_counter() - t0)
    res["upload_ms"] = 1e3 * statistics.median(ups[1:])

    f64 = dict(dtype=torch.float64, device=dev)
    X, U = torch.empty((B, T + 1, 6), **f64), torch.empty((B, T, 2), **f64)
    Xr, Ur = torch.empty_like(X), torch.empty_like(U)
    M = torch.empty((B, T), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    p, cfg, rules = _lib.default_params(), TB.gen_config_struct(_lib.GEN_MODEL_TYPE2, Ts), TB.fsm_rules_struct(None)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fsm():
        _lib.check(L.traj_gen_piecewise_batch(C.byref(p), C.byref(cfg), C.byref(rules), B, T, ptr(dx0), ptr(dst),
                                              ptr(X), ptr(U), ptr(M), None, st), "traj_gen_piecewise_batch")

    def replay():
        _lib.check(L.traj_gen_simulate_batch(C.byref(p), C.byref(cfg), B, T, ptr(dx0), ptr(U), ptr(Xr), ptr(Ur), st),
                   "traj_gen_simulate_batch")

    times = {"fsm": [], "replay": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("fsm", fsm), ("replay", replay)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    for name, ts in times.items():
        med = statistics.median(ts)
        res[f"kernel_{name}_ms"] = {"median": med, "min": min(ts), "max": max(ts), "reps": len(ts),
                                    "trajectory_steps_per_s_at_median": B * T / med * 1e3}
    res["fsm_over_replay"] = res["kernel_fsm_ms"]["median"] / res["kernel_replay_ms"]["median"]
    res["replay_of_fsm_controls_bit_identical"] = bool(torch.equal(X, Xr) and torch.equal(U, Ur))
    Mh = M.cpu().numpy()
    res["mode_share"] = {n: float((Mh == i).mean()) for i, n in enumerate(_lib.FSM_MODES)}
    res["segments_per_trajectory"] = float(1 + (Mh[:, 1:] != Mh[:, :-1]).sum() / B)   # lower bound: label changes

    downs = []
    for _ in range(3):
        t0 = time.perf_counter()
        Xh, Uh = X.cpu().numpy(), U.cpu().numpy()
        downs.append(time.perf_counter() - t0)
    res["download_ms"] = 1e3 * statistics.median(downs)

    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        DS.write_csv(os.path.join(d, "probe"), Xh, Uh, np.arange(B), Ts)
        res["csv_write_s"] = time.perf_counter() - t0
        res["csv_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))

    k = res["kernel_fsm_ms"]["median"] * 1e-3
    total = host_s + res["upload_ms"] * 1e-3 + k + res["download_ms"] * 1e-3 + res["csv_write_s"]
    res["end_to_end_s"] = total
    res["share_of_end_to_end"] = {"host_seeding": host_s / total, "upload": res["upload_ms"] * 1e-3 / total,
                                  "kernel": k / total, "download": res["download_ms"] * 1e-3 / total,
                                  "csv_write": res["csv_write_s"] / total}
    res["fixture_errors"] = fixture_errors(TB, G, _lib)
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
    if "cpu_numpy_loop" in doc and "gpu" in doc:
        doc["cpu_loop_over_fsm_kernel"] = (doc["cpu_numpy_loop"]["s_per_trajectory"] * doc["gpu"]["B"]
                                           / (doc["gpu"]["kernel_fsm_ms"]["median"] * 1e-3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()

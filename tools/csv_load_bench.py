"""The three dataset loaders at the reference's dataset size -> profiles/csv_load_bench.json.

  python tools/csv_load_bench.py [--B 5000] [--T 1200] [--T-steps 600] [--reps 5] [--out-dir DIR] [--json PATH]

One process.  The two files are written once by generate_open_loop(B, T, device_csv=True) and read once by every loader
before anything is timed, so the page cache is warm throughout: file_read_s below is a copy out of the page cache, not
a disk read.  Then the three loaders alternate `reps` times, every call ending on a device synchronisation:
  pandas  load_vehicle_dataset(device="cuda"): pd.read_csv, pandas grouping, copy up (the default);
  native  load_vehicle_dataset(native=True, device="cuda"): traj_dataset_read_csv in 16 threads, numpy grouping, copy up;
  device  load_vehicle_dataset(device_csv=True): read_csv_device (text parsed on the GPU), grouping as device ops, one
          gather / cast / transpose kernel per block.
Per path the wall time of the whole call (median, min, max over the repeats); for the device path also each stage per
file -- file read, H2D (device events), each kernel (device events), host fallback -- and the grouping.  The last
repeat's device tensors must equal the native path's bit for bit (elements that differ from the pandas path's are
counted: pandas' default float parser is not correctly rounded).  Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=5000)
    ap.add_argument("--T", type=int, default=1200)
    ap.add_argument("--Ts", type=float, default=0.01)
    ap.add_argument("--T-steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "csv_load_bench.json"))
    a = ap.parse_args()
    import torch
    from trajectory_generation_amd import dataset as D
    if not torch.cuda.is_available():
        raise SystemExit("csv_load_bench needs the GPU")
    tmp = a.out_dir or tempfile.mkdtemp(prefix="csvload_")
    os.makedirs(tmp, exist_ok=True)
    prefix = os.path.join(tmp, "ds")
    D.generate_open_loop(a.B, a.T, Ts=a.Ts, out_prefix=prefix, device_csv=True)
    noisy, clean = f"{prefix}_noisy.csv", f"{prefix}_clean.csv"
    nbytes = os.path.getsize(noisy) + os.path.getsize(clean)
    args = (noisy, clean, a.T_steps, 0.7, 0.15, 42)

    def pandas_path():
        return D.load_vehicle_dataset(*args, device="cuda")

    def native_path():
        return D.load_vehicle_dataset(*args, device="cuda", native=True)

    stages = []

    def device_path():
        tm = {}
        out = D._load_device(*args, "cuda", timings=tm)
        stages.append(tm)
        return out

    paths = {"pandas": pandas_path, "native": native_path, "device": device_path}
    wall = {k: [] for k in paths}
    last = {}
    for rep in range(a.reps + 1):          # rep 0 warms up: code objects, pinned allocations, page cache
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"rep {rep} {name} {dt:.3f} s" + ("" if rep else " (warm-up)"), file=sys.stderr, flush=True)
            if rep:
                wall[name].append(dt)
    stages = stages[1:]

    def differing(a, b):
        """elements that differ between two loaders' tensors, NaN equal to NaN"""
        return sum(int(((x.isnan() != y.isnan()) | (x.nan_to_num().view(torch.int32) != y.nan_to_num().view(torch.int32)))
                       .sum()) for pa, pb in zip(a, b) for x, y in zip(pa, pb))

    elements = sum(x.numel() for part in last["device"] for x in part)
    diff = {"device_vs_native": differing(last["device"], last["native"]),
            "device_vs_pandas": differing(last["device"], last["pandas"]),
            "native_vs_pandas": differing(last["native"], last["pandas"])}
    for p in (noisy, clean):
        os.remove(p)

    def file_stages(key):
        out = {k: spread([s[key][k] for s in stages]) for k in ("file_read_s", "h2d_s", "kernels_s", "fallback_s",
                                                                 "total_s")}
        out["kernel_ms"] = {k: spread([s[key]["kernel_ms"][k] for s in stages]) for k in stages[0][key]["kernel_ms"]}
        out["fallback_fields"] = stages[-1][key]["fallback_fields"]
        out["rows"], out["bytes"] = stages[-1][key]["rows"], stages[-1][key]["bytes"]
        return out

    out = {
        "B": a.B, "T": a.T, "Ts": a.Ts, "T_steps": a.T_steps, "reps": a.reps, "device": torch.cuda.get_device_name(0),
        "csv_bytes": nbytes, "page_cache": "warm: the files were written and read by every loader once before timing",
        "pandas_path": {"total_s": spread(wall["pandas"])},
        "native_path": {"total_s": spread(wall["native"])},
        "device_path": {"total_s": spread(wall["device"]), "noisy_file": file_stages("noisy"),
                        "clean_file": file_stages("clean"), "grouping_s": spread([s["grouping_s"] for s in stages]),
                        "gather_ms": spread([s["gather_ms"] for s in stages])},
        "device_equals_native": diff["device_vs_native"] == 0, "elements": elements, "differing_elements": diff,
        "pandas_note": "pd.read_csv's default float parser is not correctly rounded (float_precision='round_trip' is): "
                       "its float64 values can be one ulp off, which moves a float32 only when it crosses a rounding "
                       "boundary; the native and device readers are both correctly rounded",
    }
    n, d, p = (out[k]["total_s"] for k in ("native_path", "device_path", "pandas_path"))
    out["native_over_device_total_at_median"] = n["median"] / d["median"]
    out["pandas_over_device_total_at_median"] = p["median"] / d["median"]
    out["device_faster_than_native_beyond_spread"] = bool(d["max"] < n["min"])
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    if diff["device_vs_native"]:
        raise SystemExit("the device loader's tensors differ from the native loader's")


if __name__ == "__main__":
    main()

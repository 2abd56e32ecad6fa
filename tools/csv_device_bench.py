"""Host CSV writer against the device CSV path at the reference's dataset size -> profiles/csv_device_bench.json
(with --device-noise: the three writers -> profiles/csv_device_noise_bench.json).

  python tools/csv_device_bench.py [--B 5000] [--T 1200] [--reps 3] [--out-dir DIR] [--json PATH] [--device-noise]

One process, one type-2 dataset (generation_type2.generate_steps) left on the GPU.  After one warm-up of each, the two
writers alternate `reps` times:
  host    what generate_piecewise does by default: X / U copied to the host, the measurement noise drawn
          (measurement_noise per trajectory), traj_dataset_write_csv in 16 threads (format + one file write per file);
  device  dataset.write_csv_device: the text formatted on the GPU in slabs, copied down through two pinned buffers and
          written, the noise drawn in a background thread meanwhile (also timed with 16 drawing threads).
With --device-noise a third writer alternates with the two in the same process:
  device_noise  write_csv_device(device_noise=True): the noise drawn on the GPU before the clean file starts
          (measurement_noise_device), no drawing thread and no upload;
the 16-thread variant and the /dev/null run are left out, the three files pairs are compared, and
generation_type2.pcg64_states at B seeds is timed on the host and on the device.
Per path: each stage and the wall time of the whole call (median, min, max over the repeats).  The host writer also
runs once per repeat into /dev/null, which separates its formatting from its file write.  The last repeat's files are
compared byte for byte (SHA-256).  Needs the GPU; there is no CPU fallback.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def host_path(D, _lib, prefix, X, U, ids, Ts, nthreads, to_null=False):
    """write_csv(native=True) on device tensors, stage by stage (the same calls in the same order)."""
    import torch
    tm = {}
    t_all = time.perf_counter()
    t0 = time.perf_counter()
    Xh, Uh = X.cpu().numpy(), U.cpu().numpy()
    torch.cuda.synchronize()
    tm["d2h_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    noise = np.ascontiguousarray(np.stack([D.measurement_noise(i, Xh.shape[1]) for i in ids]))
    tm["noise_draw_s"] = time.perf_counter() - t0
    ids64 = np.ascontiguousarray(ids, dtype=np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    clean, noisy = (b"/dev/null", b"/dev/null") if to_null else (f"{prefix}_clean.csv".encode(),
                                                                 f"{prefix}_noisy.csv".encode())
    t0 = time.perf_counter()
    _lib.check(_lib.lib().traj_dataset_write_csv(clean, noisy, Xh.shape[0], Xh.shape[1] - 1, float(Ts), p(Xh), p(Uh),
                                                 p(noise), p(ids64), nthreads), "traj_dataset_write_csv")
    tm["format_and_write_s"] = time.perf_counter() - t0
    tm["total_s"] = time.perf_counter() - t_all
    return tm


def device_path(D, prefix, X, U, ids, Ts, nthreads, slab_bytes, device_noise=False):
    import torch
    tm = {}
    torch.cuda.synchronize()
    D.write_csv_device(prefix, X, U, ids, Ts, slab_bytes=slab_bytes, nthreads=nthreads, timings=tm,
                       **({"device_noise": True} if device_noise else {}))
    return tm


def seed_bench(n, reps):
    """generation_type2.pcg64_states at n seeds: numpy's SeedSequence on the host against traj_gen_seed_pcg64_batch
    (wall time to the states being on the device in both cases; the kernel alone by device events)."""
    import torch
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import generation_type2 as G2
    seeds = [2025 + i for i in range(n)]
    host, dev, kern = [], [], []
    same = True
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        h = torch.from_numpy(G2.pcg64_states(seeds).view(np.int64)).cuda()
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        d = G2.pcg64_states(seeds, device="cuda:0")
        torch.cuda.synchronize()
        dev.append(time.perf_counter() - t0)
        same = same and bool(torch.equal(h, d))
        ent = torch.from_numpy(G2.seed_entropy_words(seeds).view(np.int32)).cuda()
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
        with _lib.event_pair() as ev:
            _lib.check(_lib.lib().traj_gen_seed_pcg64_batch(_lib.ptr(ent), n, ent.shape[1], _lib.ptr(out),
                                                            _lib.stream()), "traj_gen_seed_pcg64_batch")
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]))
    return {"seeds": n, "identical": same, "host_s": spread(host[1:]), "device_s": spread(dev[1:]),
            "device_kernel_ms": spread(kern[1:])}


def three_writers(a, D, _lib, X, U, ids, slab, tmp):
    """--device-noise: host writer, device path (host draw: the parent's path) and device path with the device draw,
    alternating in one process."""
    import torch
    pfx = {k: os.path.join(tmp, k) for k in ("host", "device", "device_noise")}
    run = {"host": lambda: host_path(D, _lib, pfx["host"], X, U, ids, a.Ts, a.nthreads),
           "device": lambda: device_path(D, pfx["device"], X, U, ids, a.Ts, a.noise_threads, slab),
           "device_noise": lambda: device_path(D, pfx["device_noise"], X, U, ids, a.Ts, a.noise_threads, slab, True)}
    for f in run.values():      # warm-up of each
        f()
    res = {k: [] for k in run}
    for _ in range(a.reps):
        for k, f in run.items():
            res[k].append(f())
    digests = {k: [sha(f"{p}_{kind}.csv") for kind in ("clean", "noisy")] for k, p in pfx.items()}
    same = digests["host"] == digests["device"] == digests["device_noise"]
    nbytes = sum(os.path.getsize(f"{pfx['host']}_{kind}.csv") for kind in ("clean", "noisy"))
    for p in pfx.values():
        for kind in ("clean", "noisy"):
            os.remove(f"{p}_{kind}.csv")
    fold = lambda runs: {k: spread([r[k] for r in runs]) for k in runs[0] if k not in ("bytes", "slabs")}   # noqa: E731
    out = {"B": a.B, "T": a.T, "Ts": a.Ts, "reps": a.reps, "nthreads": a.nthreads,
           "device": torch.cuda.get_device_name(0), "csv_bytes": nbytes, "files_identical": bool(same),
           "host_writer": fold(res["host"]),
           "device_path_host_noise": dict(fold(res["device"]), slab_bytes=slab, noise_threads=a.noise_threads),
           "device_path_device_noise": dict(fold(res["device_noise"]), slab_bytes=slab)}
    h, d = out["device_path_host_noise"], out["device_path_device_noise"]
    out["host_noise_over_device_noise_total_at_median"] = h["total_s"]["median"] / d["total_s"]["median"]
    out["device_noise_faster_at_median"] = bool(d["total_s"]["median"] < h["total_s"]["median"])
    out["device_noise_faster_beyond_spread"] = bool(d["total_s"]["max"] < h["total_s"]["min"])
    out["noise_draw_s_host_over_device_at_median"] = h["noise_draw_s"]["median"] / d["noise_draw_s"]["median"]
    out["pcg64_states"] = seed_bench(a.B, a.reps)
    return out, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=5000)
    ap.add_argument("--T", type=int, default=1200)
    ap.add_argument("--Ts", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nthreads", type=int, default=16)
    ap.add_argument("--noise-threads", type=int, default=1)
    ap.add_argument("--slab-bytes", type=int, default=None)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--device-noise", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    a.json = a.json or os.path.join(ROOT, "profiles", "csv_device_noise_bench.json" if a.device_noise
                                    else "csv_device_bench.json")
    import torch
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import dataset as D
    from trajectory_generation_amd.generation_type2 import generate_steps
    if not torch.cuda.is_available():
        raise SystemExit("csv_device_bench needs the GPU")
    slab = a.slab_bytes or D.DEVICE_CSV_SLAB_BYTES
    res = generate_steps(a.B, a.T, a.Ts, seed=42)
    X, U, ids = res["X"].contiguous(), res["U"].contiguous(), np.asarray(res["ids"], dtype=np.int64)
    torch.cuda.synchronize()
    tmp = a.out_dir or tempfile.mkdtemp(prefix="csvbench_")
    os.makedirs(tmp, exist_ok=True)
    if a.device_noise:
        out, same = three_writers(a, D, _lib, X, U, ids, slab, tmp)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out, indent=1))
        if not same or not out["pcg64_states"]["identical"]:
            raise SystemExit("the writers' files or the seeded states differ")
        return
    hp, dp = os.path.join(tmp, "host"), os.path.join(tmp, "device")
    # warm-up of each (code objects, pinned allocations, page cache of the target files)
    host_path(D, _lib, hp, X, U, ids, a.Ts, a.nthreads)
    device_path(D, dp, X, U, ids, a.Ts, a.noise_threads, slab)
    host, null, dev, dev16 = [], [], [], []
    for _ in range(a.reps):
        host.append(host_path(D, _lib, hp, X, U, ids, a.Ts, a.nthreads))
        dev.append(device_path(D, dp, X, U, ids, a.Ts, a.noise_threads, slab))
        null.append(host_path(D, _lib, hp, X, U, ids, a.Ts, a.nthreads, to_null=True))
        dev16.append(device_path(D, dp, X, U, ids, a.Ts, 16, slab))
    device_path(D, dp, X, U, ids, a.Ts, a.noise_threads, slab)      # the files compared below: the default's
    same = all(sha(f"{hp}_{k}.csv") == sha(f"{dp}_{k}.csv") for k in ("clean", "noisy"))
    nbytes = sum(os.path.getsize(f"{hp}_{k}.csv") for k in ("clean", "noisy"))
    for k in ("clean", "noisy"):
        for pfx in (hp, dp):
            os.remove(f"{pfx}_{k}.csv")
    fold = lambda runs: {k: spread([r[k] for r in runs]) for k in runs[0] if k not in ("bytes", "slabs")}   # noqa: E731
    out = {
        "B": a.B, "T": a.T, "Ts": a.Ts, "reps": a.reps, "nthreads": a.nthreads, "device": torch.cuda.get_device_name(0),
        "csv_bytes": nbytes, "files_identical": bool(same),
        "host_writer": fold(host),
        "host_writer_to_dev_null": fold(null),
        "device_path": dict(fold(dev), slab_bytes=slab, slabs=dev[-1]["slabs"], noise_threads=a.noise_threads),
        "device_path_16_noise_threads": {k: v for k, v in fold(dev16).items() if k in ("noise_draw_s", "total_s")},
    }
    h, d = out["host_writer"]["total_s"], out["device_path"]["total_s"]
    out["host_over_device_total_at_median"] = h["median"] / d["median"]
    out["device_faster_beyond_spread"] = bool(d["max"] < h["min"])
    out["host_file_write_share_at_median"] = 1.0 - (out["host_writer_to_dev_null"]["format_and_write_s"]["median"]
                                                    / out["host_writer"]["format_and_write_s"]["median"])
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    if not same:
        raise SystemExit("the two writers' files differ")


if __name__ == "__main__":
    main()

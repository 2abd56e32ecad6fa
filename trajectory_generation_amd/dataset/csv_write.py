"""The two CSV writers: write_csv on host arrays (the library's multi-threaded writer, or pandas) and write_csv_device
on CUDA tensors (csrc/dataset_fmt.hip, the same bytes), with the per-float and per-row entry points the tests drive."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .._lib import event_pair, ptr, stream
from .schema import CLEAN_COLUMNS, NOISY_COLUMNS, frames, measurement_noise


def write_csv(out_prefix, X, U, ids, Ts, native=True, nthreads=None, noise_ids=None):
    """``{out_prefix}_clean.csv`` / ``{out_prefix}_noisy.csv`` in the reference schema (see frames).
    native: the library's multi-threaded writer (traj_dataset_write_csv), byte-identical to the pandas
    writer (native=False, frames + DataFrame.to_csv).  noise_ids: see frames."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    U = np.ascontiguousarray(U, dtype=np.float64)
    nids = ids if noise_ids is None else noise_ids
    if not native:
        clean, noisy = frames(X, U, ids, Ts, noise_ids=noise_ids)
        clean.to_csv(f"{out_prefix}_clean.csv", index=False)
        noisy.to_csv(f"{out_prefix}_noisy.csv", index=False)
        return
    import os
    B, n_rows = X.shape[0], X.shape[1]
    noise = np.ascontiguousarray(np.stack([measurement_noise(i, n_rows) for i in nids]) if B else
                                 np.zeros((0, n_rows, 6)))
    ids64 = np.ascontiguousarray(ids, dtype=np.int64)
    nt = int(nthreads or min(16, os.cpu_count() or 1))
    _lib.check(_lib.lib().traj_dataset_write_csv(f"{out_prefix}_clean.csv".encode(), f"{out_prefix}_noisy.csv".encode(),
                                                 B, n_rows - 1, float(Ts), ptr(X), ptr(U), ptr(noise), ptr(ids64), nt),
               "traj_dataset_write_csv")


DEVICE_CSV_SLAB_BYTES = 256 << 20   # write_csv_device: device text held at once (two half-size slabs)
DEVICE_CSV_ROW_MAX = 256            # no row is longer (csrc/dataset_fmt.hip CSV_ROW_MAX)
FMT_F64_MAX = 24                    # characters of the longest float (csrc/fmt_f64.h)
_CSV_HEADERS = (",".join(CLEAN_COLUMNS) + "\n", ",".join(NOISY_COLUMNS) + "\n")


def format_f64_host(v):
    """repr(float) of every element of v through csrc/fmt_f64.h on the CPU (traj_dataset_format_f64_host): a list of
    bytes, NaN as b''."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    out = np.zeros((v.size, FMT_F64_MAX), dtype=np.uint8)
    ln = np.zeros(v.size, dtype=np.int32)
    _lib.check(_lib.lib().traj_dataset_format_f64_host(ptr(v), v.size, ptr(out), ptr(ln)),
               "traj_dataset_format_f64_host")
    return [out[i, :ln[i]].tobytes() for i in range(v.size)]


def format_f64_batch(v):
    """The same header on the GPU (traj_dataset_format_f64_batch): v a CUDA float64 tensor -> list of bytes."""
    import torch
    v = v.to(torch.float64).contiguous().reshape(-1)
    out = torch.zeros((v.numel(), FMT_F64_MAX), dtype=torch.uint8, device=v.device)
    ln = torch.zeros(v.numel(), dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(_lib.lib().traj_dataset_format_f64_batch(ptr(v), v.numel(), ptr(out), ptr(ln), stream()),
                   "traj_dataset_format_f64_batch")
        oh, lh = out.cpu().numpy(), ln.cpu().numpy()
    return [oh[i, :max(lh[i], 0)].tobytes() if lh[i] >= 0 else None for i in range(v.numel())]


def csv_device_rows(which, X, U, noise, ids_d, Ts, row0, nrows, out_len, total=None):
    """traj_dataset_csv_device_rows on the current stream: the byte lengths of file rows row0 .. row0 + nrows - 1 of the
    clean (which = 0) or noisy (1) file into the int32 CUDA tensor out_len."""
    _lib.check(_lib.lib().traj_dataset_csv_device_rows(int(which), X.shape[0], X.shape[1] - 1, float(Ts), ptr(X),
                                                       ptr(U), ptr(noise), ptr(ids_d), int(row0), int(nrows),
                                                       ptr(out_len), ptr(total), stream()),
               "traj_dataset_csv_device_rows")


def csv_device_format(which, X, U, noise, ids_d, Ts, row0, nrows, off, row_len, base, out, out_bytes, err):
    """traj_dataset_csv_device_format on the current stream: rows row0 .. row0 + nrows - 1 at their offsets off - base
    in the uint8 CUDA tensor out, of which out_bytes bytes may be written; err is the device error flag."""
    _lib.check(_lib.lib().traj_dataset_csv_device_format(int(which), X.shape[0], X.shape[1] - 1, float(Ts), ptr(X),
                                                         ptr(U), ptr(noise), ptr(ids_d), int(row0), int(nrows),
                                                         ptr(off), ptr(row_len), int(base), ptr(out), int(out_bytes),
                                                         ptr(err), stream()), "traj_dataset_csv_device_format")


def csv_device_check(err):
    """traj_dataset_csv_device_check: waits for the current stream and returns the library's code for the error flag
    (TRAJ_OK, or TRAJ_E_LAUNCH if a write pass refused a row)."""
    return _lib.lib().traj_dataset_csv_device_check(ptr(err), stream())


def _device_csv_file(path, which, X, U, noise, ids_d, Ts, half, dbuf, hbuf, tm):
    """One file of write_csv_device: header, then the body slab by slab (at most `half` bytes of whole rows each)
    through the two device buffers dbuf and the two pinned host buffers hbuf."""
    import queue
    import threading
    import time
    import torch
    n_rows = X.shape[0] * X.shape[1]
    dev = X.device
    with open(path, "wb", buffering=0) as f:
        f.write(_CSV_HEADERS[which].encode())
        if n_rows == 0:
            return
        # length pass, 64-bit scan, slab cuts at row boundaries
        row_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
        kernel_events, copy_events = [], []
        with event_pair(kernel_events):
            for r0 in range(0, n_rows, 1 << 30):
                n = min(1 << 30, n_rows - r0)
                csv_device_rows(which, X, U, noise, ids_d, Ts, r0, n, row_len[r0:r0 + n])
        cum = torch.cumsum(row_len, 0, dtype=torch.int64)
        off = cum - row_len
        cum_h = cum.cpu().numpy()
        cuts = [0]
        while cuts[-1] < n_rows:
            start = int(cum_h[cuts[-1] - 1]) if cuts[-1] else 0
            j = int(np.searchsorted(cum_h, start + half, side="right"))
            if j <= cuts[-1]:
                raise RuntimeError(f"write_csv_device: row {cuts[-1]} is longer than a slab of {half} bytes")
            cuts.append(j)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        copy_stream = torch.cuda.Stream(device=dev)
        free = [threading.Semaphore(1), threading.Semaphore(1)]
        todo = queue.Queue()
        failed = []
        hnp = [h.numpy() for h in hbuf]

        def writer():
            while True:
                item = todo.get()
                if item is None:
                    return
                i, nb, done = item
                try:
                    if not failed:
                        done.synchronize()
                        t0 = time.perf_counter()
                        mv = memoryview(hnp[i])[:nb]
                        while len(mv):
                            mv = mv[f.write(mv):]
                        tm["file_write_s"] += time.perf_counter() - t0
                except BaseException as e:   # noqa: BLE001  (reported by the caller's thread)
                    failed.append(e)
                finally:
                    free[i].release()

        th = threading.Thread(target=writer, daemon=True)
        th.start()
        try:
            for k in range(len(cuts) - 1):
                i = k & 1
                free[i].acquire()      # slab k - 2 has left both of this slot's buffers
                if failed:
                    free[i].release()
                    break
                r0, r1 = cuts[k], cuts[k + 1]
                base = int(cum_h[r0 - 1]) if r0 else 0
                nb = int(cum_h[r1 - 1]) - base
                with event_pair(kernel_events) as (_, k1):
                    csv_device_format(which, X, U, noise, ids_d, Ts, r0, r1 - r0, off[r0:r1], row_len[r0:r1], base,
                                      dbuf[i], nb, err)
                copy_stream.wait_event(k1)
                with torch.cuda.stream(copy_stream), event_pair(copy_events) as (_, c1):
                    hbuf[i][:nb].copy_(dbuf[i][:nb], non_blocking=True)
                todo.put((i, nb, c1))
        finally:
            todo.put(None)
            th.join()
        if failed:
            raise failed[0]
        _lib.check(csv_device_check(err), "traj_dataset_csv_device_format (a row outside its buffer)")
        copy_stream.synchronize()
        tm["kernel_ms"] += sum(a.elapsed_time(b) for a, b in kernel_events)
        tm["d2h_ms"] += sum(a.elapsed_time(b) for a, b in copy_events)
        tm["bytes"] += int(cum_h[-1]) + len(_CSV_HEADERS[which])
        tm["slabs"] += len(cuts) - 1


def write_csv_device(out_prefix, X, U, ids, Ts, noise_ids=None, slab_bytes=DEVICE_CSV_SLAB_BYTES, nthreads=None,
                     timings=None, device_noise=False):
    """write_csv for X [B,T+1,6], U [B,T,2] that are CUDA tensors: the same two files, byte for byte, with the text
    formatted on the GPU (csrc/dataset_fmt.hip: one file row per thread, a length pass, a 64-bit scan of the lengths,
    a write pass) so the host only copies bytes down and writes them.  Opt-in; write_csv(native=True) stays the
    default writer and is the check of this one.

    slab_bytes bounds the text held on the device: it is formatted in slabs of whole rows of at most slab_bytes // 2
    bytes, alternating between two device buffers and two pinned host buffers, so slab k + 1 is formatted while slab k
    is copied down and slab k - 1 is written (one write call per slab).  The measurement noise is still drawn on the
    host by measurement_noise (numpy's stream; noise_ids as in frames) in a background thread while the clean file is
    formatted and written, then uploaded for the noisy file (x + noise is added on the device, one IEEE add as on the
    host).  nthreads: threads of that draw (default 1: seeding 5,000 generators is interpreter-bound, and 16 threads
    measured slower than one).  timings: a dict that receives noise_draw_s, h2d_s, kernel_ms and d2h_ms (device events, summed),
    file_write_s, clean_file_s and noisy_file_s (wall time of each file's pipeline), bytes, slabs and total_s.

    device_noise: opt-in (default False: the host draw above) -- the noise is drawn on the GPU before the clean file
    starts (measurement_noise_device: the same bits, csrc/dataset_noise.hip), so there is no drawing thread, no pinned
    noise buffer and no upload.  timings then also gets noise_kernel_ms, noise_tails and noise_declined; noise_draw_s is
    the wall time of the device draw with its host patch, and h2d_s is 0."""
    import threading
    import time
    import torch
    t_start = time.perf_counter()
    if not (torch.is_tensor(X) and torch.is_tensor(U) and X.is_cuda and U.is_cuda):
        raise TypeError("write_csv_device takes CUDA tensors (write_csv writes host arrays)")
    if X.dim() != 3 or X.shape[2] != 6 or X.shape[1] < 1 or tuple(U.shape) != (X.shape[0], X.shape[1] - 1, 2):
        raise ValueError(f"write_csv_device: X [B,T+1,6] and U [B,T,2] expected, got {tuple(X.shape)}, {tuple(U.shape)}")
    half = int(slab_bytes) // 2
    if half < DEVICE_CSV_ROW_MAX:
        raise ValueError(f"write_csv_device: slab_bytes must be at least {2 * DEVICE_CSV_ROW_MAX}")
    B, n_rows = X.shape[0], X.shape[1]
    ids_h = np.ascontiguousarray(ids.cpu().numpy() if torch.is_tensor(ids) else ids, dtype=np.int64)
    nids = ids_h if noise_ids is None else np.asarray(noise_ids.cpu() if torch.is_tensor(noise_ids) else noise_ids)
    if ids_h.shape != (B,) or nids.shape != (B,):
        raise ValueError("write_csv_device: one id (and one noise id) per trajectory")
    nt = int(nthreads or 1)
    tm = {"noise_draw_s": 0.0, "h2d_s": 0.0, "kernel_ms": 0.0, "d2h_ms": 0.0, "file_write_s": 0.0, "bytes": 0,
          "slabs": 0}
    if device_noise:
        _write_csv_device_noise(out_prefix, X, U, ids_h, nids, Ts, half, tm)
        tm["total_s"] = time.perf_counter() - t_start
        if timings is not None:
            timings.update(tm)
        return
    noise_h = torch.empty((B, n_rows, 6), dtype=torch.float64, pin_memory=B > 0)
    nh = noise_h.numpy()
    drawn = []

    def draw(j0, j1):      # one contiguous share of the trajectories per thread
        try:
            for j in range(j0, j1):
                nh[j] = measurement_noise(nids[j], n_rows)
        except BaseException as e:   # noqa: BLE001  (reported by the caller's thread)
            drawn.append(e)
        ends.append(time.perf_counter())

    ends = []
    nt = max(1, min(nt, B))
    threads = [threading.Thread(target=draw, args=(B * k // nt, B * (k + 1) // nt), daemon=True) for k in range(nt)]
    t_draw = time.perf_counter()
    for th in threads:
        th.start()      # drawn while the clean file is formatted and written
    with torch.cuda.device(X.device):
        try:
            X = X.to(torch.float64).contiguous()
            U = U.to(torch.float64).contiguous()
            ids_d = torch.from_numpy(ids_h).to(X.device)
            dbuf = [torch.empty(half, dtype=torch.uint8, device=X.device) for _ in range(2)]
            hbuf = [torch.empty(half, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            t0 = time.perf_counter()
            _device_csv_file(f"{out_prefix}_clean.csv", 0, X, U, None, ids_d, Ts, half, dbuf, hbuf, tm)
            tm["clean_file_s"] = time.perf_counter() - t0
        finally:
            for th in threads:
                th.join()
        tm["noise_draw_s"] = max(ends) - t_draw
        if drawn:
            raise drawn[0]
        t0 = time.perf_counter()
        noise_d = noise_h.to(X.device, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        tm["h2d_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        _device_csv_file(f"{out_prefix}_noisy.csv", 1, X, U, noise_d, ids_d, Ts, half, dbuf, hbuf, tm)
        tm["noisy_file_s"] = time.perf_counter() - t0
    tm["total_s"] = time.perf_counter() - t_start
    if timings is not None:
        timings.update(tm)


def _write_csv_device_noise(out_prefix, X, U, ids_h, nids, Ts, half, tm):
    """write_csv_device(device_noise=True) after its argument checks: the noise drawn on the device, then the two
    files one after the other."""
    import time
    import torch
    from .noise import measurement_noise_device
    with torch.cuda.device(X.device):
        t0 = time.perf_counter()
        st = {}
        noise_d = measurement_noise_device(nids, X.shape[1], X.device, stats=st)
        torch.cuda.current_stream().synchronize()
        tm["noise_draw_s"] = time.perf_counter() - t0
        tm.update(noise_kernel_ms=st["kernel_ms"], noise_tails=st["tails"], noise_declined=st["declined"])
        X = X.to(torch.float64).contiguous()
        U = U.to(torch.float64).contiguous()
        ids_d = torch.from_numpy(ids_h).to(X.device)
        dbuf = [torch.empty(half, dtype=torch.uint8, device=X.device) for _ in range(2)]
        hbuf = [torch.empty(half, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        for which, name, noise in ((0, "clean", None), (1, "noisy", noise_d)):
            t0 = time.perf_counter()
            _device_csv_file(f"{out_prefix}_{name}.csv", which, X, U, noise, ids_d, Ts, half, dbuf, hbuf, tm)
            tm[f"{name}_file_s"] = time.perf_counter() - t0

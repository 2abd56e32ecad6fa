"""Closed-loop trajectory dataset emitter and its multi-GPU gather (8(e)).

B trajectories per rank run the device-resident closed loop (batch.run_closed_loop: MPC/main.py:85-101
for every trajectory), then the histories are written in the reference's dataset schema
(generation_traj/generation_type1.py:139-158, :295-339):

  clean CSV  t, X, Y, phi, vx, vy, omega, d, delta, trajectory_id
  noisy CSV  t, X, Y, vx, vy, omega, d, delta, trajectory_id        (phi not measured)

one row per time step (T+1 rows per trajectory, the last row's d / delta = NaN), measurement noise
drawn exactly as the reference draws it: ``numpy.random.default_rng(12345 + trajectory_id)``, one
``normal(0, std, T+1)`` vector per channel in the order X, Y, phi, vx, vy, omega (ControlRules,
generation_type1.py:19-33, :312-322).  These files feed merge_datasets.py / data_loader.py unchanged.

Sharding: rank r owns trajectory ids [r B, (r+1) B) (ids and per-trajectory seeds are global, so the
result does not depend on the rank count); the only collective is the final gather of the histories
to rank 0 over RCCL (dist.gather of one fixed-size [B,T+1,9] block per rank; the other ranks receive
nothing), after which rank 0 writes the CSVs.

generate_open_loop is the same flow for the reference's own open-loop generator (generation_type1.py:240-339,
one kernel launch per rank), and merge_datasets is generation_traj/merge_datasets.py on the files' text.
"""
from __future__ import annotations

import numpy as np

MEAS_NOISE_STD = {"X": 0.05, "Y": 0.05, "phi": 0.003, "vx": 0.010, "vy": 0.003, "omega": 0.030}
NOISE_SEED_BASE = 12345
CLEAN_COLUMNS = ["t", "X", "Y", "phi", "vx", "vy", "omega", "d", "delta", "trajectory_id"]
NOISY_COLUMNS = ["t", "X", "Y", "vx", "vy", "omega", "d", "delta", "trajectory_id"]


def measurement_noise(traj_id: int, n_rows: int, stds=None, seed_base=NOISE_SEED_BASE) -> np.ndarray:
    """[n_rows, 6] noise of one trajectory, generation_type1.py:312-320."""
    s = MEAS_NOISE_STD if stds is None else stds
    rng = np.random.default_rng(seed_base + int(traj_id))
    return np.column_stack([rng.normal(0, s[k], n_rows) for k in ("X", "Y", "phi", "vx", "vy", "omega")])


def frames(X, U, ids, Ts, noise_ids=None):
    """X [B,T+1,6], U [B,T,2] (numpy), ids [B] -> (clean, noisy) pandas DataFrames in the reference
    column order, trajectories stacked in id order.  noise_ids: the ids whose noise draws are added
    (default ids; differs when a filtered dataset is re-indexed)."""
    import pandas as pd
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    B, n_rows = X.shape[0], X.shape[1]
    t = np.arange(n_rows) * Ts
    Xn = X + np.stack([measurement_noise(i, n_rows) for i in (ids if noise_ids is None else noise_ids)])
    dU = np.concatenate([U, np.full((B, 1, 2), np.nan)], axis=1)
    tid = np.repeat(np.asarray(ids, dtype=np.int64), n_rows)
    tt = np.tile(t, B)

    def cols(S, with_phi):
        d = {"t": tt, "X": S[:, :, 0].ravel(), "Y": S[:, :, 1].ravel()}
        if with_phi:
            d["phi"] = S[:, :, 2].ravel()
        d.update({"vx": S[:, :, 3].ravel(), "vy": S[:, :, 4].ravel(), "omega": S[:, :, 5].ravel(),
                  "d": dU[:, :, 0].ravel(), "delta": dU[:, :, 1].ravel(), "trajectory_id": tid})
        return pd.DataFrame(d)

    return cols(X, True)[CLEAN_COLUMNS], cols(Xn, False)[NOISY_COLUMNS]


HIST_CHANNELS = 9   # per row: X, Y, phi, vx, vy, omega, d, delta (NaN on the last row), status (-1 on the last row)


def pack_history(X, U, status):
    """X [B,T+1,6], U [B,T,2], status [T,B] -> one [B,T+1,9] float64 block (the unit of the gather)."""
    import torch
    B, T1 = X.shape[0], X.shape[1]
    blk = torch.empty((B, T1, HIST_CHANNELS), dtype=torch.float64, device=X.device)
    blk[:, :, 0:6] = X
    blk[:, :T1 - 1, 6:8] = U
    blk[:, T1 - 1, 6:8] = float("nan")
    blk[:, :T1 - 1, 8] = status.t().to(torch.float64)
    blk[:, T1 - 1, 8] = -1.0
    return blk


def unpack_history(blk):
    """Inverse of pack_history: (X [B,T+1,6], U [B,T,2], status [T,B] int32)."""
    import torch
    return blk[:, :, 0:6], blk[:, :-1, 6:8], blk[:, :-1, 8].t().to(torch.int32)


def gather_to_root(blk, dist=None, dst=0):
    """The dataset's one collective: every rank's fixed-size [B,T+1,9] block goes to
    rank `dst` only (dist.gather -- RCCL over xGMI with the nccl backend, gloo on CPU).  Returns the
    concatenation in rank order (= global trajectory-id order, ids are rank * B + i) on `dst`, None on
    the other ranks; the block itself without a process group.  With a process group the gather runs at
    every world size, 1 included (the same collective path as on 8 GPUs)."""
    if dist is None or not dist.is_initialized():
        return blk
    import torch
    blk = blk.contiguous()
    if dist.get_rank() == dst:
        parts = [torch.empty_like(blk) for _ in range(dist.get_world_size())]
        dist.gather(blk, gather_list=parts, dst=dst)
        return torch.cat(parts, 0)
    dist.gather(blk, dst=dst)
    return None


FAILED_STATUS = 2   # statuses >= 2 (solver error, infeasible, iteration limit, ...): the step kept u_prev


def status_summary(status, ids):
    """status [T,B] (the closed loop's per-step solver status) -> per trajectory (ids [B]): the worst
    status, the number of failed steps (status >= 2) and the first failed step (-1 if none)."""
    st = np.asarray(status)
    T = st.shape[0]
    failed = st >= FAILED_STATUS
    n_failed = failed.sum(axis=0)
    first = np.where(n_failed > 0, np.argmax(failed, axis=0), -1) if T else np.full(st.shape[1], -1)
    worst = st.max(axis=0) if T else np.zeros(st.shape[1], dtype=st.dtype)
    return {"trajectory_id": np.asarray(ids, dtype=np.int64), "worst_status": worst.astype(np.int64),
            "n_failed_steps": n_failed.astype(np.int64), "first_failed_step": first.astype(np.int64)}


def write_status_csv(out_prefix, status, ids, source_ids=None):
    """``{out_prefix}_status.csv`` beside the dataset CSVs (whose reference schema stays unchanged): one row
    per written trajectory -- trajectory_id, source_id (the generation id; differs after filtering),
    worst_status, n_failed_steps, first_failed_step."""
    sm = status_summary(status, source_ids if source_ids is not None else ids)
    with open(f"{out_prefix}_status.csv", "w") as f:
        f.write("trajectory_id,source_id,worst_status,n_failed_steps,first_failed_step\n")
        for i, src, w, n, fs in zip(np.asarray(ids, np.int64), sm["trajectory_id"], sm["worst_status"],
                                    sm["n_failed_steps"], sm["first_failed_step"]):
            f.write(f"{i},{src},{w},{n},{fs}\n")
    return sm


def _closed_loop_gpu(w, T, cfg):
    """This rank's closed loop on the GPU (batch.run_closed_loop, fused launch)."""
    from . import batch as TB
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    return TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg)


def generate(B, T, N=20, Ts=0.05, kind="spline", seed=0, out_prefix=None, dist=None, polish_mode=0,
             closed_loop=None, drop_failed=False, shards=False, device_csv=False):
    """Run the closed loop for this rank's B trajectories (ids rank * B .. rank * B + B - 1), gather the
    histories to rank 0 and (rank 0) write ``{out_prefix}_clean.csv`` / ``{out_prefix}_noisy.csv`` and the
    status sidecar ``{out_prefix}_status.csv`` (write_status_csv).

    drop_failed: opt-in (default False, the reference generators' behaviour: generation_type1.py:295-339 writes
      every trajectory, a failed step having kept u_prev as mpc_6stati.py:257-262 returns it; merge_datasets.py
      only offsets the ids of its second file, :41-47, and filters nothing).  True leaves out every trajectory
      with a failed step (status >= 2) and re-indexes the rest 0..n-1 (the contiguous ids data_loader.py reads) --
      each keeps the noise of its generation id, which the sidecar's source_id column records; a warning names
      how many were dropped.  Either way the status sidecar flags the failed trajectories.
    shards: no gather -- every rank writes its own ``{out_prefix}_rank{r}_*.csv`` (global ids; the shards'
      bodies concatenated in rank order are the single file's body) and its sidecar (SURVEY.md 8(e)'s
      per-rank alternative); returns this rank's share on every rank.
    closed_loop(workload, T, cfg) -> dict(X, U, status) runs one rank's share (default: the fused GPU
    closed loop); tests inject a CPU stand-in to exercise the id offsets and the gather.
    device_csv: opt-in (default False: the host writer, write_csv) -- the CSVs' text is formatted on the GPU from the
      device tensors (write_csv_device, the same bytes).
    Returns (X [W B,T+1,6], U [W B,T,2], status [T,W B]) on rank 0 and None on the other ranks (shards:
    this rank's (X, U, status) everywhere)."""
    from .workload import make_workload
    rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
    w = make_workload(B, N, Ts, kind=kind, seed=seed, id_offset=rank * B)
    cfg = None
    if closed_loop is None:
        from . import batch as TB
        cfg = TB.config_struct(N=N, Ts=Ts, polish_mode=polish_mode)
        closed_loop = _closed_loop_gpu
    if shards and drop_failed:
        raise ValueError("drop_failed re-indexes the whole dataset: it needs the gather (shards=False)")
    res = closed_loop(w, T, cfg)
    if shards:
        X, U, st = res["X"], res["U"], res["status"]
        if out_prefix is not None:
            _write_with_sidecar(f"{out_prefix}_rank{rank}", X, U, st, np.arange(rank * B, rank * B + B), Ts,
                                drop_failed, device_csv)
        return X, U, st
    blk = gather_to_root(pack_history(res["X"], res["U"], res["status"]), dist)
    if blk is None:
        return None
    X, U, st = unpack_history(blk)
    if out_prefix is not None:
        _write_with_sidecar(out_prefix, X, U, st, np.arange(X.shape[0]), Ts, drop_failed, device_csv)
    return X, U, st


def generate_open_loop(B, T, Ts=0.01, seed=42, out_prefix=None, dist=None, shards=False, device_csv=False):
    """The reference's own dataset (generation_traj/generation_type1.py:240-339), B trajectories of T steps per rank:
    this rank's ids rank * B .. rank * B + B - 1 of the dataset seeded with `seed` (generation_type1.generate_steps:
    host draw, one kernel launch), gathered to rank 0, which writes ``{out_prefix}_clean.csv`` /
    ``{out_prefix}_noisy.csv`` (write_csv).  No status sidecar: the reference has none and no step can fail.
    shards: no gather, every rank writes ``{out_prefix}_rank{r}_*.csv`` with its global ids.
    device_csv: opt-in (default False) -- the files' text is formatted on the GPU (write_csv_device, the same bytes).
    Returns (X [W B,T+1,6], U [W B,T,2]) on rank 0 and None on the other ranks (shards: this rank's share)."""
    import torch
    from .generation_type1 import generate_steps
    rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
    res = generate_steps(B, T, Ts, seed=seed, id_offset=rank * B)
    X, U = res["X"], res["U"]
    if shards:
        if out_prefix is not None:
            _write_xu(f"{out_prefix}_rank{rank}", X, U, res["ids"], Ts, device_csv)
        return X, U
    status = torch.zeros((T, B), dtype=torch.int32, device=X.device)
    blk = gather_to_root(pack_history(X, U, status), dist)
    if blk is None:
        return None
    X, U, _ = unpack_history(blk)
    if out_prefix is not None:
        _write_xu(out_prefix, X, U, np.arange(X.shape[0]), Ts, device_csv)
    return X, U


def generate_piecewise(B, T, Ts=0.01, seed=42, out_prefix=None, dist=None, shards=False, device_csv=False):
    """The reference's second dataset (generation_traj/generation_type2.py:162-220, :290-322), B trajectories of T
    steps per rank: this rank's ids rank * B .. rank * B + B - 1 of the dataset seeded with `seed`
    (generation_type2.generate_steps: the controller, its random streams and the simulation in one kernel launch),
    gathered to rank 0, which writes ``{out_prefix}_clean.csv`` / ``{out_prefix}_noisy.csv`` (write_csv: the
    reference's noise seeds 12345 + id, sigmas and columns; mode strings are not written, the reference drops them).
    shards: no gather, every rank writes ``{out_prefix}_rank{r}_*.csv`` with its global ids.
    device_csv: opt-in (default False) -- the files' text is formatted on the GPU (write_csv_device, the same bytes).
    Returns (X [W B,T+1,6], U [W B,T,2]) on rank 0 and None on the other ranks (shards: this rank's share)."""
    import torch
    from .generation_type2 import generate_steps
    rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
    res = generate_steps(B, T, Ts, seed=seed, id_offset=rank * B)
    X, U = res["X"], res["U"]
    if shards:
        if out_prefix is not None:
            _write_xu(f"{out_prefix}_rank{rank}", X, U, res["ids"], Ts, device_csv)
        return X, U
    status = torch.zeros((T, B), dtype=torch.int32, device=X.device)
    blk = gather_to_root(pack_history(X, U, status), dist)
    if blk is None:
        return None
    X, U, _ = unpack_history(blk)
    if out_prefix is not None:
        _write_xu(out_prefix, X, U, np.arange(X.shape[0]), Ts, device_csv)
    return X, U


def merge_datasets(first_prefix, second_prefix, out_prefix):
    """generation_traj/merge_datasets.py:33-70 for ``{prefix}_clean.csv`` / ``{prefix}_noisy.csv`` pairs: the second
    pair's trajectory ids are shifted by id_offset = max(trajectory_id of the first clean file) + 1 and appended to
    the first pair's rows, into ``{out_prefix}_clean.csv`` / ``{out_prefix}_noisy.csv``.

    The merge works on the text: the first file's lines are copied verbatim and the second file's lines with only
    their last field (trajectory_id) rewritten, so no float passes through a parse / print round trip (the
    reference's read_csv -> to_csv can move last digits).  Raises ValueError if a file is missing, the two headers of
    a pair differ, or the last column is not trajectory_id.  Returns id_offset."""
    import os

    def read(path):
        if not os.path.exists(path):
            raise ValueError(f"merge_datasets: file not found: {path}")
        with open(path, newline="") as f:
            lines = f.read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        if not lines or lines[0].rstrip("\r").split(",")[-1] != "trajectory_id":
            raise ValueError(f"merge_datasets: {path}: the last column must be trajectory_id")
        return lines[0], lines[1:]

    def last_id(line):
        return int(float(line.rstrip("\r").rpartition(",")[2]))

    pairs = {}
    for kind in ("clean", "noisy"):
        h1, b1 = read(f"{first_prefix}_{kind}.csv")
        h2, b2 = read(f"{second_prefix}_{kind}.csv")
        if h1 != h2:
            raise ValueError(f"merge_datasets: the {kind} files' headers differ: {h1!r} / {h2!r}")
        pairs[kind] = (h1, b1, b2)
    id_offset = max((last_id(ln) for ln in pairs["clean"][1]), default=-1) + 1
    for kind, (header, b1, b2) in pairs.items():
        eol = "\r" if header.endswith("\r") else ""
        with open(f"{out_prefix}_{kind}.csv", "w", newline="") as f:
            f.write(header + "\n")
            f.writelines(ln + "\n" for ln in b1)
            for ln in b2:
                head, _, _ = ln.rstrip("\r").rpartition(",")
                f.write(f"{head},{last_id(ln) + id_offset}{eol}\n")
    return id_offset


def _write_xu(prefix, X, U, ids, Ts, device_csv):
    """The two CSVs of device tensors X, U: through the host writer (the default) or formatted on the GPU."""
    if device_csv:
        write_csv_device(prefix, X, U, ids, Ts)
    else:
        write_csv(prefix, X.cpu().numpy(), U.cpu().numpy(), ids, Ts)


def _write_with_sidecar(prefix, X, U, st, ids, Ts, drop_failed, device_csv=False):
    """CSVs + status sidecar of trajectories `ids` (generation ids); drop_failed re-indexes the kept ones."""
    sth = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    ids = np.asarray(ids, dtype=np.int64)
    if device_csv:
        import torch
        if drop_failed:
            keep = np.nonzero((sth >= FAILED_STATUS).sum(axis=0) == 0)[0]
            if keep.size < ids.size:
                import warnings
                warnings.warn(f"{prefix}: drop_failed left out {ids.size - keep.size} of {ids.size} trajectories with "
                              "a failed step and re-indexed the rest (their generation ids: the _status.csv source_id)")
            out_ids = np.arange(keep.size, dtype=np.int64)
            kd = torch.from_numpy(keep).to(X.device)
            write_csv_device(prefix, X[kd], U[kd], out_ids, Ts, noise_ids=ids[keep])
            write_status_csv(prefix, sth[:, keep], out_ids, source_ids=ids[keep])
        else:
            write_csv_device(prefix, X, U, ids, Ts)
            write_status_csv(prefix, sth, ids)
        return
    Xh, Uh = X.cpu().numpy() if hasattr(X, "cpu") else X, U.cpu().numpy() if hasattr(U, "cpu") else U
    if drop_failed:
        keep = np.nonzero((sth >= FAILED_STATUS).sum(axis=0) == 0)[0]
        if keep.size < ids.size:
            import warnings
            warnings.warn(f"{prefix}: drop_failed left out {ids.size - keep.size} of {ids.size} trajectories with a "
                          "failed step and re-indexed the rest (their generation ids: the _status.csv source_id)")
        out_ids = np.arange(keep.size, dtype=np.int64)
        write_csv(prefix, Xh[keep], Uh[keep], out_ids, Ts, noise_ids=ids[keep])
        write_status_csv(prefix, sth[:, keep], out_ids, source_ids=ids[keep])
    else:
        write_csv(prefix, Xh, Uh, ids, Ts)
        write_status_csv(prefix, sth, ids)


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
    import ctypes as C
    import os
    from . import _lib
    B, n_rows = X.shape[0], X.shape[1]
    noise = np.ascontiguousarray(np.stack([measurement_noise(i, n_rows) for i in nids]) if B else
                                 np.zeros((0, n_rows, 6)))
    ids64 = np.ascontiguousarray(ids, dtype=np.int64)
    nt = int(nthreads or min(16, os.cpu_count() or 1))
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(_lib.lib().traj_dataset_write_csv(f"{out_prefix}_clean.csv".encode(), f"{out_prefix}_noisy.csv".encode(),
                                                 B, n_rows - 1, float(Ts), p(X), p(U), p(noise), p(ids64), nt),
               "traj_dataset_write_csv")


DEVICE_CSV_SLAB_BYTES = 256 << 20   # write_csv_device: device text held at once (two half-size slabs)
DEVICE_CSV_ROW_MAX = 256            # no row is longer (csrc/dataset_fmt.hip CSV_ROW_MAX)
FMT_F64_MAX = 24                    # characters of the longest float (csrc/fmt_f64.h)
_CSV_HEADERS = (",".join(CLEAN_COLUMNS) + "\n", ",".join(NOISY_COLUMNS) + "\n")


def format_f64_host(v):
    """repr(float) of every element of v through csrc/fmt_f64.h on the CPU (traj_dataset_format_f64_host): a list of
    bytes, NaN as b''."""
    import ctypes as C
    from . import _lib
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    out = np.zeros((v.size, FMT_F64_MAX), dtype=np.uint8)
    ln = np.zeros(v.size, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(_lib.lib().traj_dataset_format_f64_host(p(v), v.size, p(out), p(ln)), "traj_dataset_format_f64_host")
    return [out[i, :ln[i]].tobytes() for i in range(v.size)]


def format_f64_batch(v):
    """The same header on the GPU (traj_dataset_format_f64_batch): v a CUDA float64 tensor -> list of bytes."""
    import ctypes as C
    import torch
    from . import _lib
    v = v.to(torch.float64).contiguous().reshape(-1)
    out = torch.zeros((v.numel(), FMT_F64_MAX), dtype=torch.uint8, device=v.device)
    ln = torch.zeros(v.numel(), dtype=torch.int32, device=v.device)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with torch.cuda.device(v.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().traj_dataset_format_f64_batch(p(v), v.numel(), p(out), p(ln), st),
                   "traj_dataset_format_f64_batch")
        oh, lh = out.cpu().numpy(), ln.cpu().numpy()
    return [oh[i, :max(lh[i], 0)].tobytes() if lh[i] >= 0 else None for i in range(v.numel())]


def csv_device_rows(which, X, U, noise, ids_d, Ts, row0, nrows, out_len, total=None):
    """traj_dataset_csv_device_rows on the current stream: the byte lengths of file rows row0 .. row0 + nrows - 1 of the
    clean (which = 0) or noisy (1) file into the int32 CUDA tensor out_len."""
    import ctypes as C
    import torch
    from . import _lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().traj_dataset_csv_device_rows(int(which), X.shape[0], X.shape[1] - 1, float(Ts), p(X), p(U),
                                                       p(noise), p(ids_d), int(row0), int(nrows), p(out_len), p(total),
                                                       st), "traj_dataset_csv_device_rows")


def csv_device_format(which, X, U, noise, ids_d, Ts, row0, nrows, off, row_len, base, out, out_bytes, err):
    """traj_dataset_csv_device_format on the current stream: rows row0 .. row0 + nrows - 1 at their offsets off - base
    in the uint8 CUDA tensor out, of which out_bytes bytes may be written; err is the device error flag."""
    import ctypes as C
    import torch
    from . import _lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().traj_dataset_csv_device_format(int(which), X.shape[0], X.shape[1] - 1, float(Ts), p(X), p(U),
                                                         p(noise), p(ids_d), int(row0), int(nrows), p(off), p(row_len),
                                                         int(base), p(out), int(out_bytes), p(err), st),
               "traj_dataset_csv_device_format")


def csv_device_check(err):
    """traj_dataset_csv_device_check: waits for the current stream and returns the library's code for the error flag
    (TRAJ_OK, or TRAJ_E_LAUNCH if a write pass refused a row)."""
    import ctypes as C
    import torch
    from . import _lib
    return _lib.lib().traj_dataset_csv_device_check(C.c_void_p(err.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _device_csv_file(path, which, X, U, noise, ids_d, Ts, half, dbuf, hbuf, tm):
    """One file of write_csv_device: header, then the body slab by slab (at most `half` bytes of whole rows each)
    through the two device buffers dbuf and the two pinned host buffers hbuf."""
    import queue
    import threading
    import time
    import torch
    from . import _lib
    n_rows = X.shape[0] * X.shape[1]
    dev = X.device
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    with open(path, "wb", buffering=0) as f:
        f.write(_CSV_HEADERS[which].encode())
        if n_rows == 0:
            return
        # length pass, 64-bit scan, slab cuts at row boundaries
        row_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
        k0, k1 = ev(), ev()
        k0.record()
        for r0 in range(0, n_rows, 1 << 30):
            n = min(1 << 30, n_rows - r0)
            csv_device_rows(which, X, U, noise, ids_d, Ts, r0, n, row_len[r0:r0 + n])
        k1.record()
        kernel_events = [(k0, k1)]
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
        copy_events = []
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
                k0, k1, c0, c1 = ev(), ev(), ev(), ev()
                k0.record()
                csv_device_format(which, X, U, noise, ids_d, Ts, r0, r1 - r0, off[r0:r1], row_len[r0:r1], base,
                                  dbuf[i], nb, err)
                k1.record()
                kernel_events.append((k0, k1))
                copy_stream.wait_event(k1)
                with torch.cuda.stream(copy_stream):
                    c0.record()
                    hbuf[i][:nb].copy_(dbuf[i][:nb], non_blocking=True)
                    c1.record()
                copy_events.append((c0, c1))
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
                     timings=None):
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
    file_write_s, clean_file_s and noisy_file_s (wall time of each file's pipeline), bytes, slabs and total_s."""
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


def read_csv_native(path, nthreads=None, pin=False):
    """All columns of a dataset CSV as {name: float64 array} through the library's parallel parser
    (traj_dataset_read_csv) into one [rows, C] buffer -- pinned host memory with pin=True."""
    import ctypes as C
    import os
    import torch
    from . import _lib
    with open(path) as f:
        names = f.readline().strip().split(",")
    nc = C.c_int(0)
    rows = int(_lib.lib().traj_dataset_csv_rows(str(path).encode(), C.byref(nc)))
    if rows < 0 or nc.value != len(names):
        raise ValueError(f"{path}: not a dataset CSV ({rows}, {nc.value} columns)")
    buf = torch.empty((rows, len(names)), dtype=torch.float64, pin_memory=pin)
    nt = int(nthreads or min(16, os.cpu_count() or 1))
    _lib.check(_lib.lib().traj_dataset_read_csv(str(path).encode(), rows, len(names), C.c_void_p(buf.data_ptr()), nt),
               "traj_dataset_read_csv")
    return names, buf


DEVICE_CSV_READ_SLAB_BYTES = 64 << 20   # read_csv_device: pinned staging, two slabs of this size
DEVICE_CSV_FALLBACK_CAP = 4096          # read_csv_device: declined fields settled one by one; more: the host reader


def _tokens_block(tokens):
    """A list of bytes as (one uint8 array, int64 offsets, int32 lengths)."""
    ln = np.array([len(t) for t in tokens], dtype=np.int32)
    off = np.zeros(len(tokens), dtype=np.int64)
    if len(tokens):
        off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
    text = np.frombuffer(b"".join(tokens) + b"\0", dtype=np.uint8).copy()   # never empty; the last byte is no field's
    return text, off, ln


def parse_f64_host(tokens, fill=0.0):
    """csrc/parse_f64.h on the CPU (traj_dataset_parse_f64_host) on a list of bytes: (float64 array, int32 statuses);
    a declined token (status _lib.PARSE_FALLBACK) leaves `fill`."""
    import ctypes as C
    from . import _lib
    text, off, ln = _tokens_block(tokens)
    out = np.full(len(tokens), fill, dtype=np.float64)
    st = np.full(len(tokens), -7, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(_lib.lib().traj_dataset_parse_f64_host(p(text), p(off), p(ln), len(tokens), p(out), p(st)),
               "traj_dataset_parse_f64_host")
    return out, st


def parse_f64_batch(tokens, fill=0.0, device=None):
    """The same header on the GPU (traj_dataset_parse_f64_batch), one field per thread: a list of bytes ->
    (float64 CUDA tensor, int32 statuses); a declined token leaves `fill`."""
    import ctypes as C
    import torch
    from . import _lib
    dev = torch.device("cuda" if device is None else device)
    text, off, ln = _tokens_block(tokens)
    n = len(tokens)
    with torch.cuda.device(dev):
        td, od, ld = (torch.from_numpy(a).to(dev) for a in (text, off, ln))
        out = torch.full((n,), fill, dtype=torch.float64, device=dev)
        st = torch.full((n,), -7, dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        _lib.check(_lib.lib().traj_dataset_parse_f64_batch(p(td), p(od), p(ld), n, p(out), p(st),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "traj_dataset_parse_f64_batch")
        torch.cuda.current_stream().synchronize()
    return out, st


def csv_tokens_host(tokens):
    """The host reader's own token code (traj_dataset_csv_token_host: std::from_chars, strtod past the double range,
    the nan / inf spellings) on a list of non-empty bytes: (float64 array, True if every token is a number)."""
    import ctypes as C
    from . import _lib
    text, off, ln = _tokens_block(tokens)
    out = np.zeros(len(tokens), dtype=np.float64)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = _lib.lib().traj_dataset_csv_token_host(p(text), p(off), p(ln), len(tokens), p(out))
    return out, rc == _lib.TRAJ_OK


def csv_parse_index(text, nbytes, events=None):
    """The line index of a file body on the device (uint8 CUDA tensor `text`, its first nbytes bytes), on the current
    stream: (rows, starts) with starts the int64 CUDA tensor of every row's first byte.  events: a dict that receives
    (start, end) CUDA event pairs named count, scan and starts."""
    import ctypes as C
    import torch
    from . import _lib
    L = _lib.lib()
    dev = text.device
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def timed(name, fn):
        if events is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        events[name] = (a, b)
        return r

    chunks = int(L.traj_dataset_csv_parse_chunks(int(nbytes)))
    if chunks < 0:
        raise ValueError(f"csv_parse_index: {nbytes} bytes")
    if chunks == 0:
        return 0, torch.empty(0, dtype=torch.int64, device=dev)
    counts = torch.empty(chunks, dtype=torch.int64, device=dev)
    timed("count", lambda: _lib.check(L.traj_dataset_csv_parse_count(p(text), int(nbytes), p(counts), st),
                                      "traj_dataset_csv_parse_count"))
    cum = timed("scan", lambda: torch.cumsum(counts, 0))
    chunk_off = cum - counts
    # a last line without its newline is a row; a trailing newline starts none
    rows = int(cum[-1]) + (0 if int(text[nbytes - 1]) == 0x0A else 1)
    starts = torch.empty(rows, dtype=torch.int64, device=dev)
    timed("starts", lambda: _lib.check(L.traj_dataset_csv_parse_starts(p(text), int(nbytes), p(chunk_off), p(starts), rows,
                                                                       st), "traj_dataset_csv_parse_starts"))
    return rows, starts


def csv_parse_rows(text, nbytes, starts, rows, ncols, out, err, fb_count, fb_rec):
    """traj_dataset_csv_parse_rows on the current stream: the rows at `starts` of the body `text` (its first nbytes
    bytes) into the float64 CUDA tensor out [rows, ncols]; err (int32), fb_count (int64) and fb_rec ([cap, 4] int64)
    are the device error word, the declined fields' counter and their records."""
    import ctypes as C
    import torch
    from . import _lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(_lib.lib().traj_dataset_csv_parse_rows(p(text), int(nbytes), p(starts), int(rows), int(ncols), p(out),
                                                      p(err), p(fb_count), p(fb_rec), int(fb_rec.shape[0]),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "traj_dataset_csv_parse_rows")


def csv_gather_f32(src, rowidx, n, T_steps, cols):
    """traj_dataset_csv_gather_f32 on the current stream: src [rows, C] float64 (CUDA), rowidx [n * T_steps] int64 row
    numbers, cols a list of column numbers -> [n, len(cols), T_steps] float32, cast with round to nearest even."""
    import ctypes as C
    import torch
    from . import _lib
    dev = src.device
    out = torch.empty((n, len(cols), T_steps), dtype=torch.float32, device=dev)
    cd = torch.tensor(list(cols), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(_lib.lib().traj_dataset_csv_gather_f32(p(src), src.shape[0], src.shape[1], p(rowidx), int(n), int(T_steps),
                                                      p(cd), len(cols), p(out), p(err),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "traj_dataset_csv_gather_f32")
    if int(err[0]):
        raise RuntimeError("traj_dataset_csv_gather_f32: a row or column index outside the parsed block")
    return out


def _upload_body(f, nbytes, dev, slab_bytes, tm):
    """nbytes bytes of the open file f into a new uint8 CUDA tensor through two pinned slabs: a thread reads slab k + 1
    from the file while slab k is copied up."""
    import threading
    import queue
    import time
    import torch
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)     # the tail is never read
    slab = max(1, min(int(slab_bytes), nbytes))
    hbuf = [torch.empty(slab, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    hnp = [h.numpy() for h in hbuf]
    free = [threading.Semaphore(1), threading.Semaphore(1)]
    filled = queue.Queue()
    failed = []

    def reader():
        try:
            done, k = 0, 0
            while done < nbytes:
                i = k & 1
                free[i].acquire()
                t0 = time.perf_counter()
                want = min(slab, nbytes - done)
                mv, got = memoryview(hnp[i])[:want], 0
                while got < want:
                    r = f.readinto(mv[got:])
                    if not r:
                        raise ValueError("read_csv_device: the file shrank while it was read")
                    got += r
                tm["file_read_s"] += time.perf_counter() - t0
                filled.put((i, done, want))
                done += want
                k += 1
        except BaseException as e:   # noqa: BLE001  (reported by the caller's thread)
            failed.append(e)
        filled.put(None)

    th = threading.Thread(target=reader, daemon=True)
    th.start()
    copy_stream = torch.cuda.Stream(device=dev)
    copies, prev = [], None
    while True:
        item = filled.get()
        if item is None:
            break
        i, o, nb = item
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(copy_stream):
            c0.record()
            text[o:o + nb].copy_(hbuf[i][:nb], non_blocking=True)
            c1.record()
        copies.append((c0, c1))
        if prev is not None:           # the copy before this one has left its slab: the reader may fill it again
            prev[1].synchronize()
            free[prev[0]].release()
        prev = (i, c1)
    th.join()
    copy_stream.synchronize()
    if failed:
        raise failed[0]
    torch.cuda.current_stream().wait_stream(copy_stream)
    tm["h2d_s"] += sum(a.elapsed_time(b) for a, b in copies) * 1e-3
    return text


def read_csv_device(path, device=None, timings=None, fallback_cap=None, slab_bytes=DEVICE_CSV_READ_SLAB_BYTES):
    """read_csv_native with the text parsed on the GPU (csrc/dataset_parse.hip): (names, [rows, C] float64 CUDA tensor),
    the tensor equal to read_csv_native's bit for bit.  Opt-in; read_csv_native stays the check of this one.

    The header line is parsed on the host; the body goes through two pinned slabs of slab_bytes to the device whole
    (read and copy overlapped), where a count pass, a 64-bit scan and a starts pass index its lines and a parse pass
    takes one row per thread (csrc/parse_f64.h: Eisel-Lemire on at most 19 significant digits).  A field the device
    declines (more digits, a '+' sign, any other spelling) is recorded; the host reader's own token code
    (traj_dataset_csv_token_host) settles up to fallback_cap (default DEVICE_CSV_FALLBACK_CAP) of them from the file's
    bytes and the values are scattered into the tensor; with more, the whole file goes through read_csv_native and is
    copied up.  So the two readers agree by construction on everything the device declines.  Raises what read_csv_native
    raises: RuntimeError for a field that is no number or a row with too few fields.
    timings: a dict that receives file_read_s, h2d_s, kernels_s, kernel_ms (count, scan, starts, parse), fallback_s,
    fallback_fields, rows, bytes and total_s."""
    import os
    import time
    import torch
    from . import _lib
    t_start = time.perf_counter()
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("read_csv_device parses on a CUDA device (read_csv_native reads into host memory)")
    cap = DEVICE_CSV_FALLBACK_CAP if fallback_cap is None else int(fallback_cap)
    tm = {"file_read_s": 0.0, "h2d_s": 0.0, "kernels_s": 0.0, "kernel_ms": {}, "fallback_s": 0.0, "fallback_fields": 0,
          "rows": 0, "bytes": 0}

    def finish(names, t):
        tm["total_s"] = time.perf_counter() - t_start
        if timings is not None:
            timings.update(tm)
        return names, t

    with open(path, "rb") as f:
        header = f.readline()
    names = header.decode().strip().split(",")
    if header.count(b",") + 1 != len(names):
        raise ValueError(f"{path}: not a dataset CSV ({header.count(b',') + 1} columns)")
    ncols = len(names)
    with torch.cuda.device(dev):
        with open(path, "rb", buffering=0) as f:
            nbytes = os.fstat(f.fileno()).st_size - len(header)
            tm["bytes"] = nbytes + len(header)
            if nbytes <= 0 or not header.endswith(b"\n"):
                return finish(names, torch.empty((0, ncols), dtype=torch.float64, device=dev))
            f.seek(len(header))
            text = _upload_body(f, nbytes, dev, slab_bytes, tm)
        ev = {}
        rows, starts = csv_parse_index(text, nbytes, ev)
        out = torch.empty((rows, ncols), dtype=torch.float64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        fb_count = torch.zeros(1, dtype=torch.int64, device=dev)
        fb_rec = torch.zeros((max(cap, 1), 4), dtype=torch.int64, device=dev)
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0.record()
        csv_parse_rows(text, nbytes, starts, rows, ncols, out, err, fb_count, fb_rec[:cap])
        k1.record()
        ev["parse"] = (k0, k1)
        n_fb, flag = int(fb_count[0]), int(err[0])      # waits for the stream
        tm["kernel_ms"] = {k: a.elapsed_time(b) for k, (a, b) in ev.items()}
        tm["kernels_s"] = sum(tm["kernel_ms"].values()) * 1e-3
        tm["fallback_fields"], tm["rows"] = n_fb, rows
        if flag & 2:
            raise RuntimeError("traj_dataset_csv_parse_rows: the line index does not describe the text")
        if flag & 1:
            _lib.check(_lib.TRAJ_E_ARG, "read_csv_device (a row with too few fields)")
        if n_fb > cap:
            del text, out, starts
            t0 = time.perf_counter()
            names, buf = read_csv_native(path, pin=True)
            out = buf.to(dev)
            tm["fallback_s"] = time.perf_counter() - t0
            return finish(names, out)
        if n_fb:
            t0 = time.perf_counter()
            rec = fb_rec[:n_fb].cpu().numpy()
            tokens = []
            with open(path, "rb") as f:
                for _, _, off, ln in rec:
                    f.seek(len(header) + int(off))
                    tokens.append(f.read(int(ln)))
            vals, ok = csv_tokens_host(tokens)
            if not ok:
                _lib.check(_lib.TRAJ_E_ARG, "read_csv_device (a field that is no number)")
            flat = torch.from_numpy(rec[:, 0] * ncols + rec[:, 1]).to(dev)
            out.view(-1)[flat] = torch.from_numpy(vals).to(dev)
            tm["fallback_s"] = time.perf_counter() - t0
    return finish(names, out)


def load_vehicle_dataset(noisy_csv_path, clean_csv_path, T_steps=600, train_split=0.7, val_split=0.15, seed=42,
                         device=None, native=False, device_csv=False):
    """KalmanNet/data_loader.py:5-109 (load_vehicle_dataset), vectorized: the first T_steps rows of every
    trajectory (ids 0..n-1), y = noisy [X, Y, vx, vy, omega], u = [d, delta], x = clean
    [X, Y, phi, vx, vy, omega] as float32 [n, C, T]; trajectories shuffled by default_rng(seed) and split
    70 / 15 / 15.  Returns ((y, u, x) train, val, test) torch tensors (on ``device`` if given), or None
    when a file or a trajectory is missing, as the reference does.
    native: opt-in -- the library's host parser instead of pandas (_load_native), the same tensors.
    device_csv: opt-in -- the files' text is parsed and grouped on the GPU (_load_device: read_csv_device, device ops,
      one gather / cast / transpose kernel per block); the same tensors, on ``device`` (default: the current GPU)."""
    import pandas as pd
    import torch
    if device_csv:
        return _load_device(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, device)
    if native:
        return _load_native(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, device)
    try:
        dn = pd.read_csv(noisy_csv_path)
        dc = pd.read_csv(clean_csv_path)
    except FileNotFoundError:
        return None
    n = dn["trajectory_id"].nunique()

    def block(df, cols):
        df = df[df["trajectory_id"] < n]
        df = df.assign(_r=df.groupby("trajectory_id").cumcount())
        df = df[df["_r"] < T_steps]
        counts = df.groupby("trajectory_id").size()
        if len(counts) != n or (counts < T_steps).any():
            raise KeyError("trajectory missing or shorter than T_steps")
        df = df.sort_values(["trajectory_id", "_r"], kind="stable")
        return df[cols].to_numpy(dtype=np.float32).reshape(n, T_steps, len(cols)).transpose(0, 2, 1)

    try:
        y = block(dn, ["X", "Y", "vx", "vy", "omega"])
        u = block(dn, ["d", "delta"])
        x = block(dc, ["X", "Y", "phi", "vx", "vy", "omega"])
    except KeyError:
        return None
    idx = np.arange(n)
    np.random.default_rng(seed).shuffle(idx)
    y, u, x = y[idx], u[idx], x[idx]
    n_tr, n_va = int(n * train_split), int(n * val_split)
    cut = lambda a: (a[:n_tr], a[n_tr:n_tr + n_va], a[n_tr + n_va:])   # noqa: E731
    out = []
    for part in zip(cut(y), cut(u), cut(x)):
        out.append(tuple(torch.tensor(np.ascontiguousarray(p), dtype=torch.float32, device=device) for p in part))
    return tuple(out)


def _load_native(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, device):
    """load_vehicle_dataset with the library's parser: both files parsed in parallel into pinned host
    buffers, grouped per trajectory with numpy (first T_steps rows of ids 0..n-1, data_loader.py:14-53),
    the three [n, C, T] float32 blocks copied to `device` from pinned memory."""
    import os
    import torch
    if not (os.path.exists(noisy_csv_path) and os.path.exists(clean_csv_path)):
        return None
    pin = device is not None and torch.device(device).type == "cuda"
    blocks = []
    n = None
    for path, cols in ((noisy_csv_path, (["X", "Y", "vx", "vy", "omega"], ["d", "delta"])),
                       (clean_csv_path, (["X", "Y", "phi", "vx", "vy", "omega"],))):
        names, buf = read_csv_native(path, pin=False)
        a = buf.numpy()
        tid = a[:, names.index("trajectory_id")].astype(np.int64)
        if n is None:
            n = int(np.unique(tid).size)
        keep = np.nonzero(tid < n)[0]
        order = keep[np.argsort(tid[keep], kind="stable")]
        counts = np.bincount(tid[keep], minlength=n)
        if counts.size != n or (counts < T_steps).any():
            return None
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        rows = order[(first[:, None] + np.arange(T_steps)[None, :]).reshape(-1)]
        for cl in cols:
            idx = [names.index(c) for c in cl]
            blk = a[rows][:, idx].astype(np.float32).reshape(n, T_steps, len(cl)).transpose(0, 2, 1)
            blocks.append(np.ascontiguousarray(blk))
    y, u, x = blocks
    idx = np.arange(n)
    np.random.default_rng(seed).shuffle(idx)
    y, u, x = y[idx], u[idx], x[idx]
    n_tr, n_va = int(n * train_split), int(n * val_split)
    cut = lambda a: (a[:n_tr], a[n_tr:n_tr + n_va], a[n_tr + n_va:])   # noqa: E731

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if pin:
            return t.pin_memory().to(device, non_blocking=True)
        return t.to(device) if device is not None else t

    return tuple(tuple(dev(p) for p in part) for part in zip(cut(y), cut(u), cut(x)))


def _load_device(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, device, timings=None):
    """load_vehicle_dataset with the text parsed on the GPU: read_csv_device per file, _load_native's grouping as
    device ops (n = the noisy file's distinct ids; rows with id < n, stably sorted by id; every id needs T_steps rows;
    the first T_steps of each), then traj_dataset_csv_gather_f32 with the shuffled trajectory order
    (default_rng(seed).shuffle, drawn on the host) folded into its row index.  An id column with anything but
    non-negative integers hands the whole call to _load_native.  timings: a dict that receives each file's
    read_csv_device timings (noisy, clean), grouping_s (the device ops and the gather kernels, wall time) and gather_ms
    (the gather kernels alone, device events)."""
    import os
    import time
    import torch
    if not (os.path.exists(noisy_csv_path) and os.path.exists(clean_csv_path)):
        return None
    dev = torch.device("cuda" if device is None else device)
    tm = {"grouping_s": 0.0, "gather_ms": 0.0}
    blocks = []
    n = perm = None
    with torch.cuda.device(dev):
        for key, path, cols in (("noisy", noisy_csv_path, (["X", "Y", "vx", "vy", "omega"], ["d", "delta"])),
                                ("clean", clean_csv_path, (["X", "Y", "phi", "vx", "vy", "omega"],))):
            tm[key] = {}
            names, a = read_csv_device(path, device=dev, timings=tm[key])
            t0 = time.perf_counter()
            tf = a[:, names.index("trajectory_id")]
            if not bool(((tf >= 0) & (tf < 2.0 ** 62) & (tf == tf.floor())).all()):
                return _load_native(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, dev)
            tid = tf.to(torch.int64)
            if n is None:
                n = int(torch.unique(tid).numel())
                idx = np.arange(n)
                np.random.default_rng(seed).shuffle(idx)
                perm = torch.from_numpy(idx).to(dev)
            keep = torch.nonzero(tid < n).reshape(-1)
            kept = tid[keep]
            order = keep[torch.argsort(kept, stable=True)]
            counts = torch.bincount(kept, minlength=n)
            if counts.numel() != n or n == 0 or bool((counts < T_steps).any()):
                return None
            first = torch.cumsum(counts, 0) - counts
            rowidx = order[(first[perm][:, None] + torch.arange(T_steps, device=dev)[None, :]).reshape(-1)].contiguous()
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            for cl in cols:
                blocks.append(csv_gather_f32(a, rowidx, n, T_steps, [names.index(c) for c in cl]))
            g1.record()
            torch.cuda.current_stream().synchronize()
            tm["grouping_s"] += time.perf_counter() - t0
            tm["gather_ms"] += g0.elapsed_time(g1)
    y, u, x = blocks
    n_tr, n_va = int(n * train_split), int(n * val_split)
    cut = lambda t: (t[:n_tr], t[n_tr:n_tr + n_va], t[n_tr + n_va:])   # noqa: E731
    if timings is not None:
        timings.update(tm)
    return tuple(tuple(part) for part in zip(cut(y), cut(u), cut(x)))

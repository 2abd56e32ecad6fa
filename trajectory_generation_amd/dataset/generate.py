"""The three generators (closed loop, open loop, piecewise), their one collective and what rank 0 writes: the two
CSVs through either writer, the status sidecar of the closed loop, and merge_datasets on the files' text."""
from __future__ import annotations

import numpy as np

from .csv_write import write_csv, write_csv_device
from .schema import FAILED_STATUS, HIST_CHANNELS


def pack_history(X, U, status=None):
    """X [B,T+1,6], U [B,T,2], status [T,B] (None: all zero, the open-loop generators' steps cannot fail) -> one
    [B,T+1,9] float64 block (the unit of the gather)."""
    import torch
    B, T1 = X.shape[0], X.shape[1]
    blk = torch.empty((B, T1, HIST_CHANNELS), dtype=torch.float64, device=X.device)
    blk[:, :, 0:6] = X
    blk[:, :T1 - 1, 6:8] = U
    blk[:, T1 - 1, 6:8] = float("nan")
    blk[:, :T1 - 1, 8] = 0.0 if status is None else status.t().to(torch.float64)
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
    from .. import batch as TB
    paths = w.get("paths")      # make_workload_device built them with the workload
    if paths is None:
        paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    return TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, vref_step=w.get("vref_step", 0))


def _closed_loop_track_gpu(w, T, cfg):
    """This rank's closed loop on closed tracks on the GPU (track.run_closed_loop_track)."""
    from .. import track as TK
    tracks = TK.TrackSet.build(w["knots"], w["track_of"])
    return TK.run_closed_loop_track(w["x0"], w["u0"], tracks, w["vref"], T, cfg)


def _run_rank(run, B, out_prefix, dist, shards, write):
    """What every generator does around its own computation.  run(id_offset) -> this rank's (X, U, status) for the
    ids rank * B .. rank * B + B - 1; write(prefix, X, U, status, ids) writes one set of files.  shards: this rank
    writes ``{out_prefix}_rank{r}`` and gets its share back.  Otherwise the packed histories are gathered to rank 0,
    which writes ``out_prefix`` and gets the whole (X, U, status); the other ranks get None."""
    rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
    X, U, st = run(rank * B)
    if shards:
        if out_prefix is not None:
            write(f"{out_prefix}_rank{rank}", X, U, st, np.arange(rank * B, rank * B + B))
        return X, U, st
    blk = gather_to_root(pack_history(X, U, st), dist)
    if blk is None:
        return None
    X, U, st = unpack_history(blk)
    if out_prefix is not None:
        write(out_prefix, X, U, st, np.arange(X.shape[0]))
    return X, U, st


def generate(B, T, N=20, Ts=0.05, kind="spline", seed=0, out_prefix=None, dist=None, polish_mode=0,
             closed_loop=None, drop_failed=False, shards=False, device_csv=False, device_noise=False,
             device_workload=False, stats=False, speed_schedule=None):
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
    device_noise: opt-in, with device_csv only (ValueError otherwise) -- the noisy file's measurement noise is drawn on
      the GPU too (measurement_noise_device, the same bits).
    device_workload: opt-in (default False: workload.make_workload, the specification) -- this rank's workload and its
      PathSet are built on the GPU in one launch (workload.make_workload_device: the same draws; Y, phi and the spline
      coefficients to rounding, so the trajectories are not the host-built workload's bit for bit).  closed_loop gets
      that dict: device tensors, knots=None, the PathSet under "paths".
    stats: opt-in (default False: every output as without it, byte for byte) -- ``{out_prefix}_stats.json`` beside the
      status sidecar (write_stats_json): the closed loop's statistics and tracking errors pooled over the written
      trajectories (batch.closed_loop_stats on this rank's histories, on the GPU; drop_failed leaves the dropped ones
      out), the four numbers generation_type1 takes as `stats`, and the failed steps.  With a process group every
      rank's pooled record goes to rank 0 and is merged there in rank order (batch.merge_stats); shards: every rank
      writes ``{out_prefix}_rank{r}_stats.json`` of its own share.
    speed_schedule: None (default: every output as without it, byte for byte -- the workload's vref [B,N+1], the same
      window at every step), or a speed reference over the whole run, one sample per Ts: an array [W B,T+N] (row i:
      trajectory id i) or a callable (ids, T, N, Ts) -> [len(ids),T+N].  Each rank takes the rows of its ids; its
      workload then carries vref [B,T+N] and vref_step = 1, step t reads vref[b, t : t + N + 1]
      (batch.run_closed_loop(vref_step=1)), and the statistics' e_v is taken against the schedule.
    kind="track": the trajectories drive on shared closed circuits (workload.make_track_workload, eight 16-knot tracks;
      track.run_closed_loop_track, one launch sequence per step), so phi covers every heading and winds past +-pi.  The
      CSV schema, the sidecar, the sharding and the gather are the other kinds'.  stats=True, speed_schedule and
      device_workload raise ValueError with it, and there is no fused single-launch loop on tracks yet.
    Returns (X [W B,T+1,6], U [W B,T,2], status [T,W B]) on rank 0 and None on the other ranks (shards:
    this rank's (X, U, status) everywhere)."""
    from ..workload import make_track_workload, make_workload, make_workload_device
    _check_device_noise(device_csv, device_noise)
    track = kind == "track"
    if track and (stats or speed_schedule is not None or device_workload):
        raise ValueError('kind="track" takes no stats, speed_schedule or device_workload yet')
    if speed_schedule is not None and not callable(speed_schedule):
        speed_schedule = np.asarray(speed_schedule, dtype=np.float64)
        if speed_schedule.ndim != 2 or speed_schedule.shape[1] != T + N:
            raise ValueError(f"speed_schedule must be [W*B,T+N] = [*,{T + N}] (or a callable), got "
                             f"{speed_schedule.shape}")
    build = make_workload_device if device_workload else make_workload
    cfg = None
    if closed_loop is None:
        from .. import batch as TB
        cfg = TB.config_struct(N=N, Ts=Ts, polish_mode=polish_mode)
        closed_loop = _closed_loop_track_gpu if track else _closed_loop_gpu
    if shards and drop_failed:
        raise ValueError("drop_failed re-indexes the whole dataset: it needs the gather (shards=False)")

    pooled = []     # stats: this rank's (pooled record, failed steps)

    def run(id_offset):
        w = (make_track_workload(B, N, Ts, seed=seed, id_offset=id_offset) if track
             else build(B, N, Ts, kind=kind, seed=seed, id_offset=id_offset))
        if speed_schedule is not None:
            w["vref"], w["vref_step"] = _rank_schedule(speed_schedule, id_offset, B, T, N, Ts), 1
        if stats and w.get("paths") is None:
            from .. import batch as TB
            w["paths"] = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
        res = closed_loop(w, T, cfg)
        if stats:
            pooled.append(_rank_stats(res, w, drop_failed))
        return res["X"], res["U"], res["status"]

    out = _run_rank(run, B, out_prefix, dist, shards, lambda prefix, X, U, st, ids: _write_with_sidecar(
        prefix, X, U, st, ids, Ts, drop_failed, device_csv, device_noise))
    if stats:
        _write_rank_stats(pooled[0], out_prefix, dist, shards)
    return out


def _rank_schedule(speed_schedule, id_offset, B, T, N, Ts):
    """The rows of generate's speed_schedule for the ids id_offset .. id_offset + B - 1, as float64 [B,T+N]."""
    ids = np.arange(id_offset, id_offset + B)
    if callable(speed_schedule):
        rows = np.asarray(speed_schedule(ids, T, N, Ts), dtype=np.float64)
    else:
        if id_offset + B > speed_schedule.shape[0]:
            raise ValueError(f"speed_schedule holds {speed_schedule.shape[0]} rows, this rank's ids reach "
                             f"{id_offset + B - 1}")
        rows = speed_schedule[ids]
    if rows.shape != (B, T + N):
        raise ValueError(f"speed_schedule: the rows of {B} ids must be [{B},{T + N}], got {rows.shape}")
    return np.ascontiguousarray(rows)


def _rank_stats(res, w, drop_failed):
    """(pooled [7,5], fails_total) of one rank's closed loop res on its workload w; drop_failed: over the trajectories
    without a failed step, the ones that are written."""
    import torch

    from .. import batch as TB
    st = res["status"]
    mask = None
    if drop_failed:
        mask = (torch.as_tensor(st) >= FAILED_STATUS).sum(dim=0) == 0
    s = TB.closed_loop_stats(dict(X=res["X"], U=res["U"], status=st), w["paths"], w["vref"], w["u0"], mask=mask,
                             vref_step=w.get("vref_step", 0))
    return s["pooled"], s["fails_total"]


def _write_rank_stats(mine, out_prefix, dist, shards):
    """The statistics' one collective: every rank's 36 numbers (the pooled record, the failed steps) gathered to rank
    0 like the histories, merged there in rank order; shards: no gather, every rank writes its own."""
    import torch

    from .. import batch as TB
    pooled, fails_total = mine
    grouped = dist is not None and dist.is_initialized()
    rank = dist.get_rank() if grouped else 0
    if shards:
        if out_prefix is not None:
            write_stats_json(f"{out_prefix}_rank{rank}", pooled, fails_total)
        return
    if grouped:
        dev = TB.require_gpu() if dist.get_backend() == "nccl" else torch.device("cpu")
        row = torch.as_tensor(np.append(pooled.ravel(), float(fails_total)), dtype=torch.float64, device=dev)[None]
        rows = gather_to_root(row, dist)
        if rows is None:
            return
        rows = rows.cpu().numpy()
        pooled, fails_total = rows[0, :-1].reshape(pooled.shape), int(rows[:, -1].sum())
        for r in rows[1:]:
            pooled = TB.merge_stats(pooled, r[:-1].reshape(pooled.shape))
    if out_prefix is not None:
        write_stats_json(out_prefix, pooled, fails_total)


def write_stats_json(out_prefix, pooled, fails_total):
    """``{out_prefix}_stats.json``: the pooled record by series name (n, mean, M2, min, max; floats as repr writes
    them, so they read back to the bit), mpc_stats (batch.mpc_stats: generation_type1's `stats`) and fails_total."""
    import json

    from .. import batch as TB
    pooled = np.asarray(pooled, dtype=np.float64)
    doc = {"pooled": {s: {f: float(pooled[i, j]) for j, f in enumerate(TB.STATS_FIELDS)}
                      for i, s in enumerate(TB.STATS_SERIES)},
           "mpc_stats": TB.mpc_stats(pooled), "fails_total": int(fails_total)}
    with open(f"{out_prefix}_stats.json", "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def _check_device_noise(device_csv, device_noise):
    if device_noise and not device_csv:
        raise ValueError("device_noise=True draws the noise for write_csv_device: it needs device_csv=True")


def _generate_xu(generate_steps, B, T, Ts, seed, out_prefix, dist, shards, device_csv, device_noise=False, **gen_kw):
    """generate_open_loop / generate_piecewise around their module's generate_steps: no step can fail, so the gather
    carries no status and no sidecar is written.  gen_kw: further keywords of generate_steps."""
    _check_device_noise(device_csv, device_noise)

    def run(id_offset):
        res = generate_steps(B, T, Ts, seed=seed, id_offset=id_offset, **gen_kw)
        return res["X"], res["U"], None

    r = _run_rank(run, B, out_prefix, dist, shards, lambda prefix, X, U, st, ids: _write_xu(
        prefix, X, U, ids, Ts, device_csv, device_noise=device_noise))
    return None if r is None else r[:2]


def generate_open_loop(B, T, Ts=0.01, seed=42, out_prefix=None, dist=None, shards=False, device_csv=False,
                       device_noise=False):
    """The reference's own dataset (generation_traj/generation_type1.py:240-339), B trajectories of T steps per rank:
    this rank's ids rank * B .. rank * B + B - 1 of the dataset seeded with `seed` (generation_type1.generate_steps:
    host draw, one kernel launch), gathered to rank 0, which writes ``{out_prefix}_clean.csv`` /
    ``{out_prefix}_noisy.csv`` (write_csv).  No status sidecar: the reference has none and no step can fail.
    shards: no gather, every rank writes ``{out_prefix}_rank{r}_*.csv`` with its global ids.
    device_csv: opt-in (default False) -- the files' text is formatted on the GPU (write_csv_device, the same bytes).
    device_noise: opt-in, with device_csv only (ValueError otherwise) -- the measurement noise is drawn on the GPU too.
    Returns (X [W B,T+1,6], U [W B,T,2]) on rank 0 and None on the other ranks (shards: this rank's share)."""
    from ..generation_type1 import generate_steps
    return _generate_xu(generate_steps, B, T, Ts, seed, out_prefix, dist, shards, device_csv, device_noise)


def generate_piecewise(B, T, Ts=0.01, seed=42, out_prefix=None, dist=None, shards=False, device_csv=False,
                       device_noise=False, device_seed=False):
    """The reference's second dataset (generation_traj/generation_type2.py:162-220, :290-322), B trajectories of T
    steps per rank: this rank's ids rank * B .. rank * B + B - 1 of the dataset seeded with `seed`
    (generation_type2.generate_steps: the controller, its random streams and the simulation in one kernel launch),
    gathered to rank 0, which writes ``{out_prefix}_clean.csv`` / ``{out_prefix}_noisy.csv`` (write_csv: the
    reference's noise seeds 12345 + id, sigmas and columns; mode strings are not written, the reference drops them).
    shards: no gather, every rank writes ``{out_prefix}_rank{r}_*.csv`` with its global ids.
    device_csv: opt-in (default False) -- the files' text is formatted on the GPU (write_csv_device, the same bytes).
    device_noise: opt-in, with device_csv only (ValueError otherwise) -- the measurement noise is drawn on the GPU too.
    device_seed: opt-in -- the trajectories' generator states are seeded on the GPU (generation_type2.pcg64_states).
    Returns (X [W B,T+1,6], U [W B,T,2]) on rank 0 and None on the other ranks (shards: this rank's share)."""
    from ..generation_type2 import generate_steps
    return _generate_xu(generate_steps, B, T, Ts, seed, out_prefix, dist, shards, device_csv, device_noise,
                        device_seed=device_seed)


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


def _write_xu(prefix, X, U, ids, Ts, device_csv, noise_ids=None, device_noise=False):
    """The two CSVs of X, U (device tensors, or host arrays with device_csv=False): through the host writer (the
    default) or formatted on the GPU (device_noise: with the noise drawn there too)."""
    _check_device_noise(device_csv, device_noise)
    if device_csv:
        write_csv_device(prefix, X, U, ids, Ts, noise_ids=noise_ids, device_noise=device_noise)
    else:
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a   # noqa: E731
        write_csv(prefix, host(X), host(U), ids, Ts, noise_ids=noise_ids)


def _write_with_sidecar(prefix, X, U, st, ids, Ts, drop_failed, device_csv=False, device_noise=False):
    """CSVs + status sidecar of trajectories `ids` (generation ids); drop_failed re-indexes the kept ones."""
    sth = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    ids = np.asarray(ids, dtype=np.int64)
    source_ids = None
    if drop_failed:
        keep = np.nonzero((sth >= FAILED_STATUS).sum(axis=0) == 0)[0]
        if keep.size < ids.size:
            import warnings
            warnings.warn(f"{prefix}: drop_failed left out {ids.size - keep.size} of {ids.size} trajectories with a "
                          "failed step and re-indexed the rest (their generation ids: the _status.csv source_id)")
        if hasattr(X, "cpu"):
            import torch
            kd = torch.from_numpy(keep).to(X.device)
            X, U = X[kd], U[kd]
        else:
            X, U = X[keep], U[keep]
        sth, source_ids, ids = sth[:, keep], ids[keep], np.arange(keep.size, dtype=np.int64)
    _write_xu(prefix, X, U, ids, Ts, device_csv, noise_ids=source_ids, device_noise=device_noise)
    write_status_csv(prefix, sth, ids, source_ids=source_ids)

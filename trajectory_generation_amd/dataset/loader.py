"""load_vehicle_dataset (KalmanNet/data_loader.py) three ways -- pandas, the library's host parser, the device parser --
over one block specification (schema.LOADER_BLOCKS), one shuffled trajectory order and one train / val / test cut."""
from __future__ import annotations

import numpy as np

from .._lib import event_pair
from .csv_read import csv_gather_f32, read_csv_device, read_csv_native
from .schema import LOADER_BLOCKS


def _shuffled_order(n, seed):
    """The trajectories' order after data_loader.py's shuffle: default_rng(seed).shuffle of 0..n-1, on the host."""
    idx = np.arange(n)
    np.random.default_rng(seed).shuffle(idx)
    return idx


def _split(blocks, n, train_split, val_split, to_tensor=lambda a: a):
    """The (y, u, x) blocks of n shuffled trajectories cut into ((y, u, x) train, val, test), each part through
    to_tensor."""
    n_tr, n_va = int(n * train_split), int(n * val_split)
    cut = lambda a: (a[:n_tr], a[n_tr:n_tr + n_va], a[n_tr + n_va:])   # noqa: E731
    return tuple(tuple(to_tensor(p) for p in part) for part in zip(*(cut(b) for b in blocks)))


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
        dfs = {"noisy": pd.read_csv(noisy_csv_path), "clean": pd.read_csv(clean_csv_path)}
    except FileNotFoundError:
        return None
    n = dfs["noisy"]["trajectory_id"].nunique()

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
        blocks = [block(dfs[key], cl) for key, cols in LOADER_BLOCKS for cl in cols]
    except KeyError:
        return None
    idx = _shuffled_order(n, seed)
    return _split([b[idx] for b in blocks], n, train_split, val_split,
                  lambda p: torch.tensor(np.ascontiguousarray(p), dtype=torch.float32, device=device))


def _load_native(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, device):
    """load_vehicle_dataset with the library's parser: both files parsed in parallel into pinned host
    buffers, grouped per trajectory with numpy (first T_steps rows of ids 0..n-1, data_loader.py:14-53),
    the three [n, C, T] float32 blocks copied to `device` from pinned memory."""
    import os
    import torch
    paths = {"noisy": noisy_csv_path, "clean": clean_csv_path}
    if not all(os.path.exists(p) for p in paths.values()):
        return None
    pin = device is not None and torch.device(device).type == "cuda"
    blocks = []
    n = None
    for key, cols in LOADER_BLOCKS:
        names, buf = read_csv_native(paths[key], pin=False)
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
    idx = _shuffled_order(n, seed)

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if pin:
            return t.pin_memory().to(device, non_blocking=True)
        return t.to(device) if device is not None else t

    return _split([b[idx] for b in blocks], n, train_split, val_split, dev)


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
    paths = {"noisy": noisy_csv_path, "clean": clean_csv_path}
    if not all(os.path.exists(p) for p in paths.values()):
        return None
    dev = torch.device("cuda" if device is None else device)
    tm = {"grouping_s": 0.0, "gather_ms": 0.0}
    blocks = []
    n = perm = None
    with torch.cuda.device(dev):
        for key, cols in LOADER_BLOCKS:
            tm[key] = {}
            names, a = read_csv_device(paths[key], device=dev, timings=tm[key])
            t0 = time.perf_counter()
            tf = a[:, names.index("trajectory_id")]
            if not bool(((tf >= 0) & (tf < 2.0 ** 62) & (tf == tf.floor())).all()):
                return _load_native(noisy_csv_path, clean_csv_path, T_steps, train_split, val_split, seed, dev)
            tid = tf.to(torch.int64)
            if n is None:
                n = int(torch.unique(tid).numel())
                perm = torch.from_numpy(_shuffled_order(n, seed)).to(dev)
            keep = torch.nonzero(tid < n).reshape(-1)
            kept = tid[keep]
            order = keep[torch.argsort(kept, stable=True)]
            counts = torch.bincount(kept, minlength=n)
            if counts.numel() != n or n == 0 or bool((counts < T_steps).any()):
                return None
            first = torch.cumsum(counts, 0) - counts
            rowidx = order[(first[perm][:, None] + torch.arange(T_steps, device=dev)[None, :]).reshape(-1)].contiguous()
            with event_pair() as (g0, g1):
                for cl in cols:
                    blocks.append(csv_gather_f32(a, rowidx, n, T_steps, [names.index(c) for c in cl]))
            torch.cuda.current_stream().synchronize()
            tm["grouping_s"] += time.perf_counter() - t0
            tm["gather_ms"] += g0.elapsed_time(g1)
    if timings is not None:
        timings.update(tm)
    return _split(blocks, n, train_split, val_split)

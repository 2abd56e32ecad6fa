"""The noisy file's measurement noise drawn on the GPU (csrc/dataset_noise.hip) with the bits of schema.measurement_noise:
the launch, the host's recomputation of the tail draws, the host redraw of what the kernel declines and the relaunch
when the tail list overflows.  Opt-in; schema.measurement_noise stays the default and is the check of this one."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .._lib import event_pair, ptr, stream
from .schema import MEAS_NOISE_STD, NOISE_SEED_BASE, measurement_noise

NOISE_CHANNELS = ("X", "Y", "phi", "vx", "vy", "omega")
NOISE_TIE_MARGIN = 2.0 ** -40     # thousands of ulp: far above the error of either library's exp / log1p
NOISE_TAIL_RATE = 2.58e-4         # tail draws per draw (the normal's mass beyond the ziggurat's r = 3.654...)


def noise_sigma(stds=None):
    """The six sigmas in channel order, float64 (stds: a dict like MEAS_NOISE_STD)."""
    s = MEAS_NOISE_STD if stds is None else stds
    return np.array([float(s[k]) for k in NOISE_CHANNELS], dtype=np.float64)


def _noise_ids(noise_ids, seed_base):
    """noise_ids as int64 [B]; ValueError, before anything is launched, for a seed numpy refuses (negative) or one past
    int64 (which numpy takes and this path does not)."""
    a = np.asarray(noise_ids.cpu() if hasattr(noise_ids, "cpu") else noise_ids).reshape(-1)
    base = int(seed_base)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.dtype.kind not in "iu":
        a = np.array([int(i) for i in a], dtype=object)
    lo, hi = int(a.min()), int(a.max())
    if base + lo < 0:
        raise ValueError(f"measurement noise: seed {base} + {lo} is negative (numpy refuses it too)")
    if not -(1 << 63) <= base < (1 << 63) or not -(1 << 63) <= lo or max(hi, base + hi) >= (1 << 63):
        raise ValueError(f"measurement noise: seed {base} + {hi} does not fit in int64; draw it with measurement_noise")
    return np.ascontiguousarray(a.astype(np.int64))


def measurement_noise_host(noise_ids, n_rows, stds=None, seed_base=NOISE_SEED_BASE, tie_margin=None, declined=None):
    """np.stack([measurement_noise(i, n_rows, stds, seed_base) for i in noise_ids]) through the library's own headers on
    the CPU (traj_dataset_noise_host): float64 [B, n_rows, 6].  declined: an int32 [B] array that receives what the
    kernel's margin test says of each trajectory (the values are numpy's either way: the host libm is numpy's)."""
    ids = _noise_ids(noise_ids, seed_base)
    out = np.empty((ids.size, int(n_rows), 6), dtype=np.float64)
    m = NOISE_TIE_MARGIN if tie_margin is None else float(tie_margin)
    _lib.check(_lib.lib().traj_dataset_noise_host(ids.size, int(n_rows), int(seed_base), ptr(ids), ptr(noise_sigma(stds)),
                                                  m, ptr(out), ptr(declined)), "traj_dataset_noise_host")
    return out


def noise_device_raw(noise_ids, n_rows, device, stds=None, seed_base=NOISE_SEED_BASE, tie_margin=None,
                     tail_capacity=None):
    """One launch of traj_dataset_noise_batch on the current stream of `device`, nothing patched: (noise [B,n_rows,6]
    float64, declined [B] int32, tail_count [1] int64, tail_rec [capacity,4] int64), all CUDA tensors.  tail_rec rows:
    flat index into noise, bits of u1, bits of u2, 1 for a negative draw; rows past min(count, capacity) are unset."""
    import torch
    ids = _noise_ids(noise_ids, seed_base)
    B, n_rows = ids.size, int(n_rows)
    cap = max(1024, B * n_rows * 6 // 1000) if tail_capacity is None else int(tail_capacity)
    m = NOISE_TIE_MARGIN if tie_margin is None else float(tie_margin)
    with torch.cuda.device(device):
        ids_d = torch.from_numpy(ids).to(device)
        noise = torch.empty((B, n_rows, 6), dtype=torch.float64, device=device)
        declined = torch.zeros(B, dtype=torch.int32, device=device)
        count = torch.zeros(1, dtype=torch.int64, device=device)
        rec = torch.empty((max(cap, 1), 4), dtype=torch.int64, device=device)
        _lib.check(_lib.lib().traj_dataset_noise_batch(B, n_rows, int(seed_base), ptr(ids_d), ptr(noise_sigma(stds)), m,
                                                       ptr(noise), ptr(declined), ptr(count), ptr(rec), cap, stream()),
                   "traj_dataset_noise_batch")
    return noise, declined, count, rec[:cap]


def noise_tails_host(rec, stds=None):
    """traj_dataset_noise_tails_host on the records rec [n,4] int64 (host): (values float64 [n], accepted int32 [n])."""
    rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 4)
    val = np.empty(rec.shape[0], dtype=np.float64)
    acc = np.empty(rec.shape[0], dtype=np.int32)
    _lib.check(_lib.lib().traj_dataset_noise_tails_host(rec.shape[0], ptr(rec), ptr(noise_sigma(stds)), ptr(val),
                                                        ptr(acc)), "traj_dataset_noise_tails_host")
    return val, acc


def measurement_noise_device(noise_ids, n_rows, device, stds=None, seed_base=NOISE_SEED_BASE, tie_margin=None,
                             tail_capacity=None, stats=None):
    """np.stack([measurement_noise(i, n_rows, stds, seed_base) for i in noise_ids]) as a CUDA float64 tensor
    [B, n_rows, 6] on `device`, bit for bit, drawn by one lane per trajectory (csrc/dataset_noise.hip).

    The device library's exp and log1p are not the host libm's, which is numpy's, so two things come back to the host:
    the tail draws (about one in 3,900), whose values the host recomputes from the kernel's tail list and this function
    stores over the device's, and the trajectories the kernel declines because a wedge or tail test came within the
    relative tie_margin (default 2^-40) of a tie -- those are drawn by measurement_noise and uploaded.  tail_capacity:
    entries of the tail list (default max(1024, draws // 1000), about four times the expectation); when the kernel
    counts more, it is launched once more with that count.  stats: a dict that receives tails, declined, relaunched and
    kernel_ms (device events, both launches summed).  A negative seed raises ValueError before anything is launched."""
    import torch
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError("measurement_noise_device: n_rows must be at least 1")
    ids = _noise_ids(noise_ids, seed_base)
    B = ids.size
    st = {"tails": 0, "declined": 0, "relaunched": False, "kernel_ms": 0.0}
    if B == 0:
        if stats is not None:
            stats.update(st)
        return torch.empty((0, n_rows, 6), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        events = []
        cap = tail_capacity
        for attempt in range(2):
            with event_pair(events):
                noise, declined, count, rec = noise_device_raw(ids, n_rows, device, stds, seed_base, tie_margin, cap)
            n_tails = int(count.item())
            if n_tails <= rec.shape[0]:
                break
            if attempt:
                raise RuntimeError("measurement_noise_device: the tail list overflowed at its own count")
            cap, st["relaunched"] = n_tails, True
        st["kernel_ms"] = sum(a.elapsed_time(b) for a, b in events)
        redo = set(np.nonzero(declined.cpu().numpy())[0].tolist())
        if n_tails:
            rec_h = rec[:n_tails].cpu().numpy()
            val, acc = noise_tails_host(rec_h, stds)
            redo |= set((rec_h[acc == 0, 0] // (n_rows * 6)).tolist())
            noise.view(-1)[torch.from_numpy(rec_h[:, 0].copy()).to(device)] = torch.from_numpy(val).to(device)
        if redo:
            redo = sorted(redo)
            blocks = np.stack([measurement_noise(ids[b], n_rows, stds, seed_base) for b in redo])
            noise[torch.tensor(redo, device=device)] = torch.from_numpy(np.ascontiguousarray(blocks)).to(device)
        st["tails"], st["declined"] = n_tails, len(redo)
    if stats is not None:
        stats.update(st)
    return noise

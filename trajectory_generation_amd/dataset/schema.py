"""The dataset's schema: the two files' columns, the measurement noise of the noisy file, the solver-status threshold
and the columns the loader takes from each file.  numpy only: the generators and knet_eval import their constants
from here without loading torch or the library."""
from __future__ import annotations

import numpy as np

MEAS_NOISE_STD = {"X": 0.05, "Y": 0.05, "phi": 0.003, "vx": 0.010, "vy": 0.003, "omega": 0.030}
NOISE_SEED_BASE = 12345
CLEAN_COLUMNS = ["t", "X", "Y", "phi", "vx", "vy", "omega", "d", "delta", "trajectory_id"]
NOISY_COLUMNS = ["t", "X", "Y", "vx", "vy", "omega", "d", "delta", "trajectory_id"]
HIST_CHANNELS = 9   # per row: X, Y, phi, vx, vy, omega, d, delta (NaN on the last row), status (-1 on the last row)
FAILED_STATUS = 2   # statuses >= 2 (solver error, infeasible, iteration limit, ...): the step kept u_prev

# load_vehicle_dataset's blocks in the order y, u, x (KalmanNet/data_loader.py:14-53): file -> column lists
LOADER_BLOCKS = (("noisy", (["X", "Y", "vx", "vy", "omega"], ["d", "delta"])),
                 ("clean", (["X", "Y", "phi", "vx", "vy", "omega"],)))


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

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
from .csv_read import (DEVICE_CSV_FALLBACK_CAP, DEVICE_CSV_READ_SLAB_BYTES, _upload_body, csv_gather_f32,  # noqa: F401
                       csv_parse_index, csv_parse_rows, csv_tokens_host, parse_f64_batch, parse_f64_host,
                       read_csv_device, read_csv_native)
from .csv_write import (DEVICE_CSV_ROW_MAX, DEVICE_CSV_SLAB_BYTES, FMT_F64_MAX, _device_csv_file,  # noqa: F401
                        csv_device_check, csv_device_format, csv_device_rows, format_f64_batch, format_f64_host,
                        write_csv, write_csv_device)
from .generate import (_write_with_sidecar, _write_xu, gather_to_root, generate, generate_open_loop,  # noqa: F401
                       generate_piecewise, merge_datasets, pack_history, status_summary, unpack_history,
                       write_stats_json, write_status_csv)
from .loader import _load_device, _load_native, load_vehicle_dataset  # noqa: F401
from .noise import (NOISE_TIE_MARGIN, measurement_noise_device, measurement_noise_host, noise_device_raw,  # noqa: F401
                    noise_sigma, noise_tails_host)
from .schema import (CLEAN_COLUMNS, FAILED_STATUS, HIST_CHANNELS, MEAS_NOISE_STD, NOISE_SEED_BASE,  # noqa: F401
                     NOISY_COLUMNS, frames, measurement_noise)

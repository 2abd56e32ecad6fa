"""MPC/main.py of the reference without its import-time side effects: the script's functions and constants, its loop
for B trajectories on the GPU, and the statistics it prints.

Reference correspondence (DorianaG01/trajectory_generation, MPC/main.py):
  d_steady_state                  :9-18
  vref_profile_ramp_cruise / _trapezoid / _sine   :28-47 (the same numpy expressions)
  ref_window_from_x_with_vref     :51-68, in numpy: the specification of batch.ref_window_batch on the script's parabola
  Ts, sim_steps, N, x0, v0_target :21, :72-77
  simulate                        the loop :85-101 through batch.run_closed_loop, then the evaluation :107-121 through
                                  batch.closed_loop_stats
  format_statistics               the text of :113-121
The plots and the GIF (:123-200) are out of scope, as everywhere in the package.  Like the script, simulate evaluates
the speed profile at simulation time 0 on every step (:87 calls it with no time argument); simulate(scheduled=True)
samples it once over the whole run instead and slides the horizon's window along it, one sample per step.
"""
from __future__ import annotations

import numpy as np

from .batch import d_steady_state, vref_ramp   # main.py:9-18 (with the reference's Params) and :28-32, already there

vref_profile_ramp_cruise = vref_ramp             # main.py:28-32 under the script's name


def vref_profile_trapezoid(N, Ts, v0=0.8, vmax=2.0, t_acc=2.0, t_flat=3.0, t_dec=2.0):
    """main.py:34-42: rise over t_acc seconds, vmax for t_flat, fall over t_dec, held inside [v0, vmax]."""
    t = np.arange(N + 1) * Ts
    rise = v0 + (vmax - v0) * (t / t_acc)
    fall = vmax - (vmax - v0) * ((t - (t_acc + t_flat)) / t_dec)
    return np.clip(np.where(t > t_acc + t_flat, fall, np.where(t <= t_acc, rise, vmax)), v0, vmax)


def vref_profile_sine(N, Ts, v_mean=1.5, v_amp=0.5, period_s=6.0):
    """main.py:44-47: a sinusoid of amplitude v_amp and period period_s around v_mean."""
    return v_mean + v_amp * np.sin(2 * np.pi * (np.arange(N + 1) * Ts) / period_s)


def ref_window_from_x_with_vref(x_start, N, Ts, vref_seq):
    """main.py:51-68: the window (X*, Y*, phi*) [N+1,3] from x_start on the script's parabola y = 0.1 x^2, X advancing
    by vref_seq[k] Ts per stage (a running sum, in the script's order)."""
    v = np.asarray(vref_seq).reshape(N + 1)
    X = np.zeros(N + 1)
    X[0] = x_start
    for k in range(N):
        X[k + 1] = X[k] + v[k] * Ts
    return np.stack([X, 0.1 * X**2, np.arctan(0.2 * X)], axis=1)


# the script's constants (main.py:21, :72-77)
v0_target = 1.0
Ts = 0.02
sim_steps = 600
N = 40
x0 = np.array([0.0, 0.5, 0.0, v0_target, 0.0, 0.0])
_SCRIPT_X0 = x0


def simulate(B=1, steps=sim_steps, N=N, Ts=Ts, profile=vref_profile_ramp_cruise, x0=None, path=(0, [0, 0, 0.1, 0]),
             device=None, scheduled=False) -> dict:
    """The script's loop (main.py:85-101) for B trajectories in one fused launch, and its evaluation (:107-121).

    profile(N, Ts) -> vref [N+1] (one of the three above, or any callable of that form); x0 [6] or [B,6] (default: the
    script's, for every trajectory); path = (kind, [c0, c1, c2, c3]) as batch.PathSet takes it (default: the script's
    parabola y = 0.1 x^2) or a batch.PathSet of B paths.  u_prev starts at [d_steady_state(v0_target), 0] (:22).
    scheduled=False (default): the script's loop, the profile's first N + 1 samples at every step.  True: the profile in
    the run's own time -- profile(steps + N - 1, Ts), its steps + N samples one per Ts -- and step t reads samples
    t .. t + N (run_closed_loop(vref_step=1)); e_v is then taken against the schedule (closed_loop_stats(vref_step=1)).
    Returns run_closed_loop's dict (X [B,steps+1,6], U [B,steps,2], status, iters, ...) with "stats": what
    batch.closed_loop_stats returns for it, and "vref", "vref_step", "u0", "paths"."""
    from . import batch as TB
    dev = TB.require_gpu(device)
    B = int(B)
    xs = np.broadcast_to(np.asarray(_SCRIPT_X0 if x0 is None else x0, dtype=np.float64), (B, 6)).copy()
    u0 = np.tile(np.array([d_steady_state(v0_target), 0.0]), (B, 1))
    vref_step = 1 if scheduled else 0
    L = int(steps) + N if scheduled else N + 1
    vref = np.asarray(profile(L - 1, Ts), dtype=np.float64).reshape(L)
    if isinstance(path, TB.PathSet):
        paths = path
    else:
        kind, pc = path
        paths = TB.PathSet.build([int(kind)] * B, np.tile(np.asarray(pc, dtype=np.float64), (B, 1)), device=dev)
    run = TB.run_closed_loop(TB.dev_f64(xs, None, dev), TB.dev_f64(u0, None, dev), paths, vref, int(steps),
                             TB.config_struct(N=N, Ts=Ts), vref_step=vref_step)
    run.update(stats=TB.closed_loop_stats(run, paths, vref, u0, vref_step=vref_step), vref=vref, vref_step=vref_step,
               u0=u0, paths=paths)
    return run


def format_statistics(stats) -> str:
    """The text main.py:113-121 prints, from a pooled record [7,5] or from what batch.closed_loop_stats returns."""
    from .batch import stats_views
    v = stats_views(stats["pooled"] if isinstance(stats, dict) else stats)
    lines = []
    for title, s in (("Accelerator 'd_seq'", "d"), ("Steering 'delta_seq'", "delta")):
        lines += [f"\n{title} Statistics:",
                  f"  - Mean: {v['mean'][s]:.4f}",
                  f"  - Std Dev: {v['std'][s]:.4f}",
                  f"  - Range: [{v['min'][s]:.4f}, {v['max'][s]:.4f}]"]
    return "\n".join(lines)

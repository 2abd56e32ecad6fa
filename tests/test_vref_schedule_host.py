"""The speed schedule's host side (no GPU, no launch): the argument checks of traj_closed_loop_step_sched / _run_sched /
_stats_sched, the ValueErrors of the Python layer, the numpy specification with a per-step vref0, and
dataset.generate(speed_schedule=...) handing each rank the schedule rows of its ids (gloo, world size 2)."""
import ctypes as C
import glob
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from trajectory_generation_amd import _lib
from trajectory_generation_amd import batch as TB

NEW = ("traj_closed_loop_step_sched", "traj_closed_loop_run_sched", "traj_closed_loop_stats_sched")
N = 20


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_declared_exported_and_bound(L):
    """The three names by test_abi's rule -- declared in include/*.h, exported by the library, bound in _lib._SIGS --
    and the ABI version is still 4."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set()
    for h in glob.glob(os.path.join(root, "include", "*.h")):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        declared |= set(re.findall(r"\b(traj_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NEW:
        assert n in declared and n in exported and n in _lib.exported_symbols() and hasattr(L, n), n
    assert L.traj_abi_version() == 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _calls(L):
    """f(vref_row, vref_len, vref_step, t, steps) -> return code of each new entry point at B = 0 (nothing is
    dereferenced and nothing launched): TRAJ_OK for a schedule the call accepts."""
    p, c = _lib.default_params(), _lib.default_config(N, 0.05)
    ps = _lib.Paths()
    ps.kmax, ps.kind, ps.pc = 0, 16, 16
    nul = C.c_void_p(0)

    def step(row, ln, vs, t):
        return L.traj_closed_loop_step_sched(C.byref(p), C.byref(c), C.byref(ps), 0, nul, nul, nul, row, ln, vs, t, 0,
                                             nul, nul, nul, nul, nul, 0, nul)

    def run(row, ln, vs, t0, steps):
        return L.traj_closed_loop_run_sched(C.byref(p), C.byref(c), C.byref(ps), 0, nul, nul, nul, row, ln, vs, t0,
                                            steps, 0, nul, nul, nul, nul, nul, 0, nul)

    def stats(row, ln, vs, T, n=N):
        return L.traj_closed_loop_stats_sched(C.byref(ps), 0, n, T, T, nul, nul, nul, nul, row, ln, vs, nul, nul, nul,
                                              nul)
    return step, run, stats


def test_schedule_argument_errors(L):
    """TRAJ_E_ARG before any launch: vref_step not 0 or 1; vref_len < N + 1; vref_row neither 0 nor >= vref_len; the
    last element read at or past vref_len -- t vref_step + N (step), (t0 + steps - 1) vref_step + N (run),
    T vref_step (stats).  Each beside the nearest accepted call."""
    step, run, stats = _calls(L)
    OK, E = _lib.TRAJ_OK, _lib.TRAJ_E_ARG
    Ln = 100
    # accepted: the plain reference, a schedule per trajectory, a shared row
    for row, ln, vs in ((N + 1, N + 1, 0), (Ln, Ln, 1), (Ln + 7, Ln, 1), (0, Ln, 1), (0, N + 1, 0), (Ln, Ln, 0)):
        assert step(row, ln, vs, 0) == OK and run(row, ln, vs, 0, 1) == OK and stats(row, ln, vs, 1) == OK
    # vref_step
    for vs in (-1, 2, 3):
        assert step(Ln, Ln, vs, 0) == E and run(Ln, Ln, vs, 0, 1) == E and stats(Ln, Ln, vs, 1) == E
    # vref_len < N + 1
    assert step(N, N, 0, 0) == E and run(N, N, 0, 0, 1) == E and stats(N, N, 0, 1) == E
    assert step(0, N, 1, 0) == E and run(0, N, 1, 0, 1) == E and stats(0, N, 1, 1) == E
    # vref_row
    for row in (1, Ln - 1, -Ln):
        assert step(row, Ln, 1, 0) == E and run(row, Ln, 1, 0, 1) == E and stats(row, Ln, 1, 1) == E
    # the last element read: t + N <= Ln - 1
    assert step(Ln, Ln, 1, Ln - 1 - N) == OK and step(Ln, Ln, 1, Ln - N) == E
    assert step(Ln, Ln, 0, 10 ** 6) == OK                      # vref_step = 0: every step reads 0 .. N
    assert run(Ln, Ln, 1, 0, Ln - N) == OK and run(Ln, Ln, 1, 0, Ln - N + 1) == E
    assert run(Ln, Ln, 1, 30, Ln - N - 30) == OK and run(Ln, Ln, 1, 31, Ln - N - 30) == E
    assert run(Ln, Ln, 0, 0, 10 ** 6) == OK
    assert run(Ln, Ln, 1, Ln, 0) == OK                         # no step: nothing is read
    assert stats(Ln, Ln, 1, Ln - 1) == OK and stats(Ln, Ln, 1, Ln) == E
    assert stats(N + 1, N + 1, 0, 10 ** 6) == OK
    # the functions they extend still refuse what they refused
    assert stats(Ln, Ln, 1, 0) == E and stats(Ln, Ln, 1, 1, n=0) == E


class _FakePaths:
    B = 3


def test_python_layer_value_errors():
    """vref_step other than 0 / 1, a schedule that is not [L] or [B,L], or one too short for the call: ValueError
    before anything touches the GPU."""
    cfg = TB.config_struct(N=N, Ts=0.05)
    Bn, T = 3, 5
    x, u = np.zeros((Bn, 6)), np.zeros((Bn, 2))
    ok = np.ones((Bn, T + N))
    for bad_step in (2, -1, 1.5):
        with pytest.raises(ValueError, match="vref_step"):
            TB.run_closed_loop(x, u, None, ok, T, cfg, vref_step=bad_step)
        with pytest.raises(ValueError, match="vref_step"):
            TB.closed_loop_run(x, u, None, ok, cfg, steps=T, vref_step=bad_step)
        with pytest.raises(ValueError, match="vref_step"):
            TB.closed_loop_step(x, u, None, ok, cfg, vref_step=bad_step)
        with pytest.raises(ValueError, match="vref_step"):
            TB.closed_loop_stats(dict(X=np.zeros((Bn, T + 1, 6)), U=np.zeros((Bn, T, 2))), _FakePaths(), ok, u,
                                 vref_step=bad_step)
    for bad in (np.ones((Bn, T + N - 1)), np.ones(T + N - 1), np.ones((Bn + 1, T + N)), np.ones((1, Bn, T + N)),
                np.float64(1.0)):
        with pytest.raises(ValueError, match="schedule"):
            TB.run_closed_loop(x, u, None, bad, T, cfg, vref_step=1)
        with pytest.raises(ValueError, match="schedule"):
            TB.closed_loop_run(x, u, None, bad, cfg, t0=0, steps=T, vref_step=1)
    # the step at t reads t .. t + N; a run from t0 reads up to t0 + steps - 1 + N
    with pytest.raises(ValueError, match="schedule"):
        TB.closed_loop_step(x, u, None, ok, cfg, t=T, vref_step=1)
    with pytest.raises(ValueError, match="schedule"):
        TB.closed_loop_run(x, u, None, ok, cfg, t0=1, steps=T, vref_step=1)
    # the statistics read S[:, 1 .. T]
    run = dict(X=np.zeros((Bn, T + 1, 6)), U=np.zeros((Bn, T, 2)))
    for bad in (np.ones((Bn, T)), np.ones(T), np.ones((Bn + 1, T + 1))):
        with pytest.raises(ValueError, match="schedule"):
            TB.closed_loop_stats(run, _FakePaths(), bad, u, vref_step=1)


def test_specification_takes_a_speed_per_step():
    """closed_loop_series_host / closed_loop_stats_host with vref0 [B,T]: e_v at step t is vx(X[b,t+1]) - vref0[b,t];
    [B] and a scalar stay what they were; another shape is a ValueError."""
    rng = np.random.default_rng(5)
    Bn, T = 4, 9
    X, U, u0 = rng.normal(size=(Bn, T + 1, 6)), rng.normal(size=(Bn, T, 2)), rng.normal(size=(Bn, 2))
    fn = lambda b, xs: (0.1 * xs ** 2, np.arctan(0.2 * xs))   # noqa: E731
    v = rng.uniform(0.5, 2.0, size=(Bn, T))
    ser = TB.closed_loop_series_host(X, U, u0, fn, v)
    assert np.array_equal(ser[:, 6], X[:, 1:, 3] - v)
    const = TB.closed_loop_series_host(X, U, u0, fn, v[:, 0])
    assert np.array_equal(const[:, 6], X[:, 1:, 3] - v[:, :1]) and np.array_equal(const[:, :6], ser[:, :6])
    assert np.array_equal(TB.closed_loop_series_host(X, U, u0, fn, 1.25)[:, 6], X[:, 1:, 3] - 1.25)
    assert np.array_equal(TB.closed_loop_series_host(X, U, u0, fn, np.tile(v[:, :1], (1, T))), const)
    st = TB.closed_loop_stats_host(X, U, u0, fn, v)
    assert st["pooled"][6, 0] == Bn * T and abs(st["pooled"][6, 1] - np.mean(X[:, 1:, 3] - v)) <= 1e-15
    with pytest.raises(ValueError):
        TB.closed_loop_series_host(X, U, u0, fn, v[:, :-1])


def test_profiles_sample_once_per_ts_over_a_run():
    """What simulate(scheduled=True) relies on: profile(steps + N - 1, Ts) is steps + N samples, one per Ts, and its
    first N + 1 are profile(N, Ts)."""
    from trajectory_generation_amd import mpc_main as M
    for prof in (M.vref_profile_ramp_cruise, M.vref_profile_trapezoid, M.vref_profile_sine):
        long = prof(60 + N - 1, 0.05)
        assert long.shape == (60 + N,) and np.array_equal(long[:N + 1], prof(N, 0.05))


# ------------------------------------------------------------------ dataset.generate: each rank's rows

B_RANK, T_DS, N_DS = 4, 5, 8


def _schedule_rows(ids, T, Nh, Ts):
    ids = np.asarray(ids)
    return 1.0 + ids[:, None] + 0.001 * np.arange(T + Nh)[None, :] + Ts


def _echo_closed_loop(w, T, cfg):
    """CPU stand-in for one rank's closed loop: the histories carry the workload's schedule (X, flattened), its
    vref_step and the ids (U)."""
    ids = np.asarray(w["ids"], dtype=np.float64)
    Bn = len(ids)
    v = np.broadcast_to(np.asarray(w["vref"], dtype=np.float64), (Bn, np.shape(w["vref"])[-1]))
    X = np.zeros((Bn, (T + 1) * 6))
    X[:, :v.shape[1]] = v
    X[:, -1] = v.shape[1]
    U = np.zeros((Bn, T, 2))
    U[:, 0, 0], U[:, 0, 1] = w.get("vref_step", 0), ids
    return dict(X=torch.tensor(X.reshape(Bn, T + 1, 6)), U=torch.tensor(U),
                status=torch.zeros((T, Bn), dtype=torch.int32))


def _worker(rank, world, port, q, as_callable):
    from trajectory_generation_amd import dataset as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sched = _schedule_rows if as_callable else _schedule_rows(np.arange(world * B_RANK), T_DS, N_DS, 0.05)
    r = D.generate(B_RANK, T_DS, N=N_DS, Ts=0.05, kind="spline", seed=3, dist=dist, closed_loop=_echo_closed_loop,
                   speed_schedule=sched)
    q.put(None if r is None else (r[0].numpy(), r[1].numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("as_callable", [False, True], ids=["array", "callable"])
def test_generate_hands_each_rank_its_schedule_rows(as_callable):
    """World size 2 (gloo): rank r's workload holds exactly rows r B .. r B + B - 1 of the schedule, [B,T+N], with
    vref_step = 1 -- from an array [W B,T+N] and from a callable (ids, T, N, Ts)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, as_callable)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sum(g is None for g in got) == 1
    X, U = next(g for g in got if g is not None)
    Ln = T_DS + N_DS
    flat = X.reshape(2 * B_RANK, -1)
    assert np.array_equal(flat[:, -1], np.full(2 * B_RANK, Ln))                  # every rank's vref is [B,T+N]
    assert np.array_equal(U[:, 0, 1], np.arange(2 * B_RANK))                     # rank order = id order
    assert np.array_equal(U[:, 0, 0], np.ones(2 * B_RANK))                       # vref_step = 1
    assert np.array_equal(flat[:, :Ln], _schedule_rows(np.arange(2 * B_RANK), T_DS, N_DS, 0.05))


def test_generate_schedule_errors_and_default():
    """An array of the wrong width, too few rows for the ids, a callable returning the wrong shape: ValueError.  With
    the default None the workload is untouched (vref [N+1], no vref_step)."""
    from trajectory_generation_amd import dataset as D
    seen = {}

    def spy(w, T, cfg):
        seen.update(vref=np.asarray(w["vref"]), step=w.get("vref_step"))
        return _echo_closed_loop(w, T, cfg)
    D.generate(B_RANK, T_DS, N=N_DS, Ts=0.05, seed=3, closed_loop=spy)
    assert seen["vref"].shape == (N_DS + 1,) and seen["step"] is None
    with pytest.raises(ValueError, match="speed_schedule"):
        D.generate(B_RANK, T_DS, N=N_DS, closed_loop=spy, speed_schedule=np.ones((B_RANK, T_DS + N_DS - 1)))
    with pytest.raises(ValueError, match="speed_schedule"):
        D.generate(B_RANK, T_DS, N=N_DS, closed_loop=spy, speed_schedule=np.ones((B_RANK - 1, T_DS + N_DS)))
    with pytest.raises(ValueError, match="speed_schedule"):
        D.generate(B_RANK, T_DS, N=N_DS, closed_loop=spy, speed_schedule=lambda ids, T, Nh, Ts: np.ones((len(ids), T)))

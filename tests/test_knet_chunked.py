"""Chunk-and-shuffle KalmanNet training (trajectory_generation_amd/pipeline_indipendent_chunking.py, csrc/knet_opt.h),
the part that needs no GPU: ``create_chunks`` against the reference's (tests/golden/knet_chunked.npz, written by
tests/golden/gen_knet_chunked_golden.py), the golden configuration's distance from the kinks of the vehicle step, and
the argument checks of traj_knet_chunk_gather_f32 / traj_knet_clip_adamw_f32: every call made here has a bad argument
and returns TRAJ_E_ARG before any launch (no call with only valid arguments is made with the placeholder pointers)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _knet_bptt_ref as BR
from tests import _knet_ref as R
from tests._knet_weights import LIMITS, knet_weights
from trajectory_generation_amd import _lib

CG = np.load("tests/golden/knet_chunked.npz")
G = np.load("tests/golden/knet.npz")
KINK_MIN = 1e-3   # the exclusion the training comparisons on the GPU apply (tests/test_knet_train_fused_gpu.py)


def real_data():
    """The golden configuration's data in real units: y [4,5,20], u [4,2,20], x [4,6,20] and the four statistics."""
    f = lambda k: torch.tensor(G[k], dtype=torch.float32)   # noqa: E731
    stats = {k: f(k) for k in ("x_mean", "x_std", "y_mean", "y_std")}
    return f("y_norm") * stats["y_std"] + stats["y_mean"], f("u"), f("x_true"), stats


def test_create_chunks_equals_reference():
    from trajectory_generation_amd import pipeline_chunk_shuffle as PS
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    assert PS.create_chunks is PC.create_chunks and PS.Pipeline_Vehicle_KNet is PC.Pipeline_Vehicle_KNet
    ramp = torch.arange(3 * 5 * 20, dtype=torch.float32).reshape(3, 5, 20)
    c5, c6 = PC.create_chunks(ramp, 5), PC.create_chunks(ramp, 6)
    assert c5.shape == (12, 5, 5) and c6.shape == (9, 5, 6)   # 6 drops the tail of 2
    assert np.array_equal(c5.numpy(), CG["ramp_chunks5"]) and np.array_equal(c6.numpy(), CG["ramp_chunks6"])
    # chunk c is trajectory c // cpt, steps [(c % cpt) size, + size): what the gather kernel's ids mean
    assert torch.equal(c6[4], ramp[1, :, 6:12])


def test_golden_chunks_stay_clear_of_kinks():
    """At the initial weights, every chunk of the recorded epochs (with its recorded start noise) stays >= 1e-3 (real
    units) from every kink of the vehicle step over its five steps: the comparisons against the reference on the GPU
    leave no chunk out."""
    from trajectory_generation_amd.pipeline_indipendent_chunking import INIT_NOISE_STD, create_chunks
    y, u, x, st = real_data()
    Tc = int(CG["T_train"])
    yc, uc, xc = (create_chunks(t, Tc) for t in (y, u, x))
    assert yc.shape[0] == 16 and CG["perm"].shape == (2, 16) and CG["noise"].shape == (2, 16, 6)
    p = dict(R.PARAMS)
    p.update(LIMITS)
    w = BR._w({k: torch.tensor(v) for k, v in knet_weights(seed=0).items()}, torch.float64)
    norm = (st["x_mean"], st["x_std"], st["y_mean"], st["y_std"], None, None)
    for e in range(2):
        perm = torch.tensor(CG["perm"][e])
        assert sorted(perm.tolist()) == list(range(16))
        y_norm, x_norm = (yc[perm] - st["y_mean"]) / st["y_std"], (xc[perm] - st["x_mean"]) / st["x_std"]
        m1x0 = x_norm[:, :, 0] + torch.tensor(CG["noise"][e]) * INIT_NOISE_STD
        tape = BR.forward_tape(w, p, float(G["Ts"]), y_norm, uc[perm], m1x0, norm)
        d = BR.chunk_kink_distance(p, float(G["Ts"]), tape, norm)
        print(f"[knet-chunked] epoch {e}: smallest kink distance {d.min().item():.3g}")
        assert (d >= KINK_MIN).all(), d.tolist()


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


FK = C.c_void_p(16)   # a placeholder: every call that takes it is refused before a launch


def test_chunk_gather_arguments(L):
    def f(n_traj=5, T_full=23, Tc=5, B=3, ptrs=None, noise=FK, y_tgt=FK):
        a = [FK] * 8 if ptrs is None else ptrs   # y, u, x, chunk_ids, four statistics
        return L.traj_knet_chunk_gather_f32(n_traj, T_full, Tc, B, *a, noise, 0.3, FK, FK, FK, y_tgt, FK, None)

    for bad in (dict(B=0), dict(B=-1), dict(n_traj=0), dict(Tc=0), dict(Tc=24), dict(Tc=-5), dict(T_full=0),
                dict(B=1 << 20, Tc=1 << 10, T_full=1 << 10), dict(n_traj=1 << 20, T_full=1 << 10)):
        assert f(**bad) == _lib.TRAJ_E_ARG, bad
    for missing in range(8):
        a = [FK] * 8
        a[missing] = None
        assert f(ptrs=a) == _lib.TRAJ_E_ARG, missing
    for out in (0, 1, 2, 4):   # Y, U, x_tgt, m1x0 are required (y_tgt, index 3, is optional: checked on the GPU)
        o = [FK] * 5
        o[out] = None
        assert L.traj_knet_chunk_gather_f32(5, 23, 5, 3, *([FK] * 8), FK, 0.3, *o, None) == _lib.TRAJ_E_ARG, out


def test_clip_adamw_arguments(L):
    need = L.traj_knet_clip_adamw_workspace_bytes()
    assert need >= 8 and need % 8 == 0

    def f(table=FK, n_tensors=3, n_total=100, lr=FK, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, max_norm=5.0, step=FK,
          total=FK, ws=FK, ws_bytes=need):
        return L.traj_knet_clip_adamw_f32(table, n_tensors, n_total, lr, b1, b2, eps, wd, max_norm, step, total, ws,
                                          ws_bytes, None)

    for bad in (dict(table=None), dict(n_tensors=0), dict(n_tensors=-1), dict(n_total=2), dict(lr=None),
                dict(step=None), dict(ws=None), dict(ws_bytes=need - 8), dict(ws_bytes=0), dict(ws=C.c_void_p(20)),
                dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(eps=-1.0), dict(wd=-1.0),
                dict(max_norm=float("nan"))):
        assert f(**bad) == _lib.TRAJ_E_ARG, bad
    assert C.sizeof(_lib.KnetOptEntry) == 40 and _lib.KnetOptEntry.n.offset == 32

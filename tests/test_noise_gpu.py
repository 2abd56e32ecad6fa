"""The device noise draw on the MI355X (csrc/dataset_noise.hip, csrc/seed_seq.h) against numpy and the host writer: the
seeded states, the noise block, the two files -- bit for bit and byte for byte, no tolerance.  The shapes are the
smallest that reach every path: B = 64 at 129 rows (one full wave, 14 tail draws with numpy 2.2.6), 65 and 1 (a partial
wave), one row, no trajectory; a margin that declines some trajectories and not others; a tail list of one entry."""
import functools

import numpy as np
import pytest

import torch

from tests._noise_cases import DECLINE_MARGIN, ENTROPIES, ZIG_R, coerce, numpy_noise
from trajectory_generation_amd import _lib
from trajectory_generation_amd import dataset as D
from trajectory_generation_amd import generation_type2 as G2

pytestmark = pytest.mark.gpu

TS = 0.01
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def reference(B, n):
    """numpy's noise of ids 0 .. B - 1: computed once, shared, never written to."""
    ref = numpy_noise(np.arange(B), n)
    ref.setflags(write=False)
    return ref


def bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).view(np.uint64)


def assert_bits(got, want):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape
    bad = np.argwhere(g != w)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("B", [1, 37, 64, 65])
def test_seed_batch_equals_the_host_entry(B):
    L, p = _lib.lib(), _lib.ptr
    for entropy in ENTROPIES:
        w = coerce(entropy)
        # stream b: the listed entropy with b added to its first word (mod 2^32), so the lanes differ
        ent = np.tile(w, (B, 1))
        ent[:, 0] += np.arange(B, dtype=np.uint32)
        ent = np.ascontiguousarray(ent)
        want = np.zeros((B, 4), dtype=np.uint64)
        assert L.traj_gen_seed_pcg64_host(p(ent), B, w.size, p(want)) == _lib.TRAJ_OK
        ent_d = torch.from_numpy(ent.view(np.int32)).to(DEV)
        got = torch.zeros((B, 4), dtype=torch.int64, device=DEV)
        assert L.traj_gen_seed_pcg64_batch(p(ent_d), B, w.size, p(got), _lib.stream()) == _lib.TRAJ_OK
        assert got.cpu().numpy().view(np.uint64).tolist() == want.tolist(), entropy
    assert want[0].tolist() == G2.pcg64_state_words(np.random.PCG64(ENTROPIES[-1])).tolist()


def test_pcg64_states_on_the_device():
    seeds = [0, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 64 + 9] + list(range(2025, 2025 + 70))
    got = G2.pcg64_states(seeds, device=DEV)
    assert got.is_cuda and got.dtype == torch.int64
    assert got.cpu().numpy().view(np.uint64).tolist() == G2.pcg64_states(seeds).tolist()
    with pytest.raises(ValueError):
        G2.pcg64_states([3, -1], device=DEV)


def test_noise_equals_numpy_and_only_tails_differ_before_the_patch():
    want = reference(64, 129)
    st = {}
    got = D.measurement_noise_device(np.arange(64), 129, DEV, stats=st)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (64, 129, 6)
    assert_bits(got, want)
    assert st["tails"] >= 10 and st["declined"] == 0 and st["relaunched"] is False and st["kernel_ms"] > 0.0
    # the kernel's own output: everything outside the tail list is numpy's already, and the list is the tail draws
    raw, declined, count, rec = D.noise_device_raw(np.arange(64), 129, DEV)
    n = int(count.item())
    assert n == st["tails"] and declined.cpu().numpy().tolist() == [0] * 64
    rec = rec[:n].cpu().numpy()
    idx = np.sort(rec[:, 0])
    z = want.reshape(-1) / np.tile(D.noise_sigma(), 64 * 129)
    assert idx.tolist() == np.nonzero(np.abs(z) > ZIG_R)[0].tolist()
    differ = np.nonzero(bits(raw).reshape(-1) != bits(want).reshape(-1))[0]
    assert set(differ.tolist()) <= set(idx.tolist())
    val, acc = D.noise_tails_host(rec)
    assert acc.tolist() == [1] * n
    assert bits(val).tolist() == bits(want).reshape(-1)[rec[:, 0]].tolist()


@pytest.mark.parametrize("B,n", [(65, 129), (1, 129), (65, 1), (1, 1)])
def test_partial_waves_and_one_row(B, n):
    assert_bits(D.measurement_noise_device(np.arange(B), n, DEV), reference(B, n))


def test_no_trajectory():
    st = {}
    got = D.measurement_noise_device(np.zeros(0, dtype=np.int64), 7, DEV, stats=st)
    assert tuple(got.shape) == (0, 7, 6) and got.is_cuda and st["tails"] == 0 and st["declined"] == 0


def test_noise_ids_unsorted_with_repeats_other_sigmas_and_base():
    ids = np.array([40, 3, 3, 2 ** 32 - D.NOISE_SEED_BASE, 17, 2 ** 32 - D.NOISE_SEED_BASE - 1, 0, 40, 2 ** 40])
    assert_bits(D.measurement_noise_device(ids, 33, DEV), numpy_noise(ids, 33))
    assert_bits(D.measurement_noise_device(torch.from_numpy(ids).to(DEV), 33, DEV), numpy_noise(ids, 33))
    stds = {"X": 0.5, "Y": 1e-3, "phi": 0.0, "vx": 7.0, "vy": 1.0, "omega": 3e-300}
    assert_bits(D.measurement_noise_device(ids[:5], 129, DEV, stds=stds, seed_base=7), numpy_noise(ids[:5], 129, stds, 7))


def test_declined_trajectories_are_drawn_on_the_host():
    """tests/test_noise_host.py checks on the CPU that DECLINE_MARGIN declines some of these trajectories, not all."""
    st = {}
    got = D.measurement_noise_device(np.arange(64), 129, DEV, tie_margin=DECLINE_MARGIN, stats=st)
    assert 0 < st["declined"] < 64, st
    assert_bits(got, reference(64, 129))


def test_tail_list_overflow_relaunches():
    st = {}
    got = D.measurement_noise_device(np.arange(64), 129, DEV, tail_capacity=1, stats=st)
    assert st["relaunched"] is True and st["tails"] >= 10
    assert_bits(got, reference(64, 129))
    # capacity 0: the counter still counts, nothing is recorded
    _, _, count, rec = D.noise_device_raw(np.arange(64), 129, DEV, tail_capacity=0)
    assert int(count.item()) == st["tails"] and rec.shape[0] == 0


@functools.lru_cache(maxsize=None)
def csv_case(B, T):
    rng = np.random.default_rng(77 * B + T)
    X = rng.standard_normal((B, T + 1, 6)) * 10.0 ** rng.uniform(-3, 2, (B, T + 1, 6))
    U = rng.uniform(-1, 1, (B, T, 2))
    ids = np.arange(B, dtype=np.int64) * 5 + 2
    return X, U, ids


def read_pair(prefix):
    return open(prefix + "_clean.csv", "rb").read(), open(prefix + "_noisy.csv", "rb").read()


@pytest.mark.parametrize("B,T", [(37, 60), (3, 1)])
def test_files_equal_the_host_writers(B, T, tmp_path):
    X, U, ids = csv_case(B, T)
    Xd, Ud = torch.from_numpy(X).to(DEV), torch.from_numpy(U).to(DEV)
    nids = np.arange(B, dtype=np.int64)[::-1] * 3 + 100
    for tag, noise_ids, kw in (("a", None, {}), ("b", None, {"slab_bytes": 4096}), ("c", nids, {})):
        host, dev = str(tmp_path / f"host_{tag}"), str(tmp_path / f"dev_{tag}")
        D.write_csv(host, X, U, ids, TS, native=True, noise_ids=noise_ids)
        tm = {}
        D.write_csv_device(dev, Xd, Ud, ids, TS, noise_ids=noise_ids, device_noise=True, timings=tm, **kw)
        assert read_pair(dev) == read_pair(host), tag
        assert tm["noise_kernel_ms"] > 0.0 and tm["noise_draw_s"] > 0.0 and tm["h2d_s"] == 0.0
        assert tm["noise_tails"] >= 0 and tm["noise_declined"] == 0 and tm["total_s"] >= tm["noise_draw_s"]


@pytest.mark.parametrize("gen", ["generate_open_loop", "generate_piecewise"])
def test_generators_write_the_same_files(gen, tmp_path):
    f = getattr(D, gen)
    a, b = str(tmp_path / "default"), str(tmp_path / "device")
    Xa, Ua = f(8, 50, out_prefix=a)
    Xb, Ub = f(8, 50, out_prefix=b, device_csv=True, device_noise=True)
    assert torch.equal(Xa, Xb) and torch.equal(Ua, Ub)
    assert read_pair(a) == read_pair(b)


def test_device_seed_gives_the_same_trajectories():
    Xa, Ua = D.generate_piecewise(8, 50)
    Xb, Ub = D.generate_piecewise(8, 50, device_seed=True)
    assert torch.equal(Xa, Xb) and torch.equal(Ua, Ub)
    ra = G2.generate_steps(70, 20, seed=2 ** 32 - 30, want_rng_state=True)
    rb = G2.generate_steps(70, 20, seed=2 ** 32 - 30, want_rng_state=True, device_seed=True)
    for k in ("X", "U", "modes", "rng_state"):
        assert torch.equal(ra[k], rb[k]), k


def test_device_noise_without_device_csv_raises(tmp_path):
    with pytest.raises(ValueError):
        D.generate_piecewise(2, 5, out_prefix=str(tmp_path / "x"), device_noise=True)
    with pytest.raises(ValueError):
        D.generate_open_loop(2, 5, out_prefix=str(tmp_path / "y"), device_csv=False, device_noise=True)

"""The measurement-noise draw of csrc/noise_draw.h on the CPU (traj_dataset_noise_host) against numpy's
(dataset.measurement_noise): ids 0..63 at 129 rows (14 tail draws with numpy 2.2.6, at least 10 asserted, so the tail
path is compared), one row, ids on both sides of the one-word / two-word seed boundary, other sigmas and seed base;
the host's recomputation of tail records; the margin test's decline counts that tests/test_noise_gpu.py relies on;
argument errors; the headers under ASan / UBSan (tests/sanitize/san_noise.cpp, a host program).  No tolerance: the bits
are equal or the test fails."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests._noise_cases import DECLINE_MARGIN, ZIG_R, numpy_noise
from trajectory_generation_amd import _lib
from trajectory_generation_amd import dataset as D

HERE = os.path.dirname(os.path.abspath(__file__))


def assert_bits(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(got[tuple(i)].hex(), want[tuple(i)].hex()) for i in bad[:5]])


def test_equals_numpy_with_tails():
    ids = np.arange(64)
    want = numpy_noise(ids, 129)
    tails = int((np.abs(want / D.noise_sigma()) > ZIG_R).sum())
    assert tails >= 10, tails
    assert_bits(D.measurement_noise_host(ids, 129), want)


def test_one_row():
    assert_bits(D.measurement_noise_host(np.arange(70), 1), numpy_noise(np.arange(70), 1))


def test_ids_around_the_word_boundary():
    """seed_base + id = 2^32 - 1 is one uint32 word to numpy, 2^32 two."""
    edge = 2 ** 32 - D.NOISE_SEED_BASE
    ids = np.array([edge - 2, edge - 1, edge, edge + 1, 2 ** 40, 2 ** 62], dtype=np.int64)
    assert_bits(D.measurement_noise_host(ids, 17), numpy_noise(ids, 17))
    assert_bits(D.measurement_noise_host([5, 6], 9, seed_base=2 ** 32 - 6), numpy_noise([5, 6], 9, seed_base=2 ** 32 - 6))


def test_other_sigmas_and_seed_base():
    stds = {"X": 0.5, "Y": 1e-3, "phi": 0.0, "vx": 7.0, "vy": 1.0, "omega": 3e-300}
    ids = [9, 3, 3, 40]
    assert_bits(D.measurement_noise_host(ids, 33, stds=stds, seed_base=7), numpy_noise(ids, 33, stds, 7))
    assert_bits(D.measurement_noise_host([0], 5, seed_base=0), numpy_noise([0], 5, seed_base=0))


def test_margin_declines_some_of_the_gpu_tests_trajectories():
    """The margin test restated on the host: at the default 2^-40 nothing among ids 0..63 x 129 rows is declined, at
    DECLINE_MARGIN some trajectories are and some are not (22 of 64 here), and the values do not depend on it."""
    ids = np.arange(64)
    want = numpy_noise(ids, 129)
    dec = np.full(64, -1, dtype=np.int32)
    assert_bits(D.measurement_noise_host(ids, 129, declined=dec), want)
    assert dec.tolist() == [0] * 64
    assert_bits(D.measurement_noise_host(ids, 129, tie_margin=DECLINE_MARGIN, declined=dec), want)
    assert set(dec.tolist()) == {0, 1} and 8 <= int(dec.sum()) <= 56, dec.sum()


def test_tail_records_recomputed_on_the_host():
    """traj_dataset_noise_tails_host gives numpy's value for the uniforms of a tail draw: the draws of a stream are
    replayed in Python up to its first tail draw, whose two uniforms are read from the raw stream."""
    r, inv_r = ZIG_R, 0.27366123732975827203338247596
    found = 0
    for seed in range(400):
        n = 400
        z = np.random.default_rng(seed).standard_normal(n)
        hit = np.nonzero(np.abs(z) > r)[0]
        if not hit.size:
            continue
        k = int(hit[0])
        # candidates for (u1, u2): consecutive doubles of the raw stream; the record that reproduces z[k] is the one
        raw = np.random.PCG64(seed).random_raw(4 * n)
        u = (raw >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        rec = np.zeros((u.size - 1, 4), dtype=np.int64)
        rec[:, 0] = 3                                   # channel 3: sigma = vx's
        rec[:, 1], rec[:, 2] = u[:-1].view(np.int64), u[1:].view(np.int64)
        rec[:, 3] = 1 if z[k] < 0 else 0
        val, acc = D.noise_tails_host(rec)
        want = 0.0 + D.noise_sigma()[3] * z[k]
        match = np.nonzero((val.view(np.uint64) == np.float64(want).view(np.uint64)) & (acc == 1))[0]
        assert match.size >= 1, seed
        j = int(match[0])
        xx = -inv_r * np.log1p(-u[j])
        assert (r + xx) == abs(z[k])
        found += 1
        if found == 5:
            break
    assert found == 5


def test_argument_errors():
    L, p, E = _lib.lib(), _lib.ptr, _lib.TRAJ_E_ARG
    ids = np.zeros(2, dtype=np.int64)
    sg = D.noise_sigma()
    out = np.zeros((2, 3, 6))
    assert L.traj_dataset_noise_host(2, 3, 12345, None, p(sg), 0.0, p(out), None) == E
    assert L.traj_dataset_noise_host(2, 3, 12345, p(ids), None, 0.0, p(out), None) == E
    assert L.traj_dataset_noise_host(2, 3, 12345, p(ids), p(sg), 0.0, None, None) == E
    assert L.traj_dataset_noise_host(-1, 3, 12345, p(ids), p(sg), 0.0, p(out), None) == E
    assert L.traj_dataset_noise_host(2, 0, 12345, p(ids), p(sg), 0.0, p(out), None) == E
    assert L.traj_dataset_noise_host(2, 3, 12345, p(ids), p(sg), -1.0, p(out), None) == E
    assert L.traj_dataset_noise_host(2, 3, -1, p(ids), p(sg), 0.0, p(out), None) == E         # a negative seed
    assert L.traj_dataset_noise_host(0, 3, 12345, None, p(sg), 0.0, None, None) == _lib.TRAJ_OK
    # the device entry refuses the same before any launch
    fk = p(out)
    assert L.traj_dataset_noise_batch(2, 3, 12345, None, p(sg), 0.0, fk, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, None, 0.0, fk, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), 0.0, None, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), 0.0, fk, None, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), 0.0, fk, fk, None, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), 0.0, fk, fk, fk, None, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), 0.0, fk, fk, fk, fk, -1, None) == E
    assert L.traj_dataset_noise_batch(-1, 3, 12345, fk, p(sg), 0.0, fk, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 0, 12345, fk, p(sg), 0.0, fk, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(2, 3, 12345, fk, p(sg), float("nan"), fk, fk, fk, fk, 4, None) == E
    assert L.traj_dataset_noise_batch(0, 3, 12345, None, p(sg), 0.0, None, None, None, None, 0, None) == _lib.TRAJ_OK
    assert L.traj_dataset_noise_tails_host(-1, fk, p(sg), fk, fk) == E
    assert L.traj_dataset_noise_tails_host(1, None, p(sg), fk, fk) == E
    assert L.traj_dataset_noise_tails_host(0, None, p(sg), None, None) == _lib.TRAJ_OK


def test_negative_seed_raises_before_anything_runs():
    with pytest.raises(ValueError):
        D.measurement_noise_host([0, -12346], 4)
    with pytest.raises(ValueError):
        D.measurement_noise_device([0, -12346], 4, "cuda:0")      # raised by the id check: no GPU is touched
    with pytest.raises(ValueError):
        D.measurement_noise_host([2 ** 63 - 12345], 4)
    with pytest.raises(ValueError):
        D.measurement_noise(-12346, 4)                              # numpy's own refusal


def test_device_noise_needs_device_csv():
    X, U = np.zeros((1, 2, 6)), np.zeros((1, 1, 2))
    with pytest.raises(ValueError):
        D._write_xu("unused", X, U, [0], 0.01, device_csv=False, device_noise=True)
    for gen in (D.generate_open_loop, D.generate_piecewise, D.generate):
        with pytest.raises(ValueError):
            gen(1, 2, device_noise=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_noise_headers_under_asan_ubsan(tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:strict_string_checks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = str(tmp_path / "san_noise")
    r = subprocess.run(["g++", *san, "-std=c++17", "-Wall", "-Werror", "-o", exe,
                        os.path.join(HERE, "sanitize", "san_noise.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "san_noise ok" in r.stdout and "ERROR" not in r.stderr

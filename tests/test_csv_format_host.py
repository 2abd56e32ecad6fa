"""csrc/fmt_f64.h on the CPU (traj_dataset_format_f64_host) against Python's repr(float), NaN as the empty field: the
edge list, every power of two, the neighbours of the powers of ten, 10^6 random bit patterns and 10^6 values of
dataset magnitude; the committed power-of-ten table against its generator; the header alone under ASan / UBSan
(tests/sanitize/san_fmt.cpp, a host program).  No tolerance anywhere: the strings are equal or the test fails."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests._csv_fmt_cases import edge_values, py_fields
from trajectory_generation_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "trajectory_generation_amd", "csrc")


def host_fields(v):
    """traj_dataset_format_f64_host on v: (the [n,24] character block, the lengths)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.zeros((v.size, 24), dtype=np.uint8)
    ln = np.full(v.size, -7, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    assert _lib.lib().traj_dataset_format_f64_host(p(v), v.size, p(out), p(ln)) == _lib.TRAJ_OK
    return out, ln


def assert_equals_repr(v):
    out, ln = host_fields(v)
    want = py_fields(v)
    wl = np.array([len(w) for w in want], dtype=np.int32)
    bad = np.nonzero(ln != wl)[0]
    assert bad.size == 0, [(v[i].hex(), int(ln[i]), want[i]) for i in bad[:5]]
    assert ln.max() <= 24
    # one comparison of the whole block: the expected characters padded with the zeros the block was filled with
    exp = np.zeros((v.size, 24), dtype=np.uint8)
    flat = np.frombuffer(b"".join(w.ljust(24, b"\0") for w in want), dtype=np.uint8).reshape(v.size, 24)
    exp[:] = flat
    rows = np.nonzero((out != exp).any(axis=1))[0]
    assert rows.size == 0, [(v[i].hex(), out[i, :ln[i]].tobytes(), want[i]) for i in rows[:5]]


def test_edge_list_equals_repr():
    v = edge_values()
    assert v.size > 4400
    assert_equals_repr(v)


def test_random_bit_patterns_equal_repr():
    bits = np.random.default_rng(20240607).integers(0, 2 ** 64, size=1_000_000, dtype=np.uint64)
    assert_equals_repr(bits.view(np.float64))


def test_dataset_magnitudes_equal_repr():
    rng = np.random.default_rng(77)
    v = rng.standard_normal(1_000_000) * 10.0 ** rng.uniform(-6, 3, 1_000_000)
    assert_equals_repr(v)


def test_wrapper_and_argument_errors():
    from trajectory_generation_amd import dataset as D
    assert D.format_f64_host([0.5, float("nan"), -1e-7, 1e16]) == [b"0.5", b"", b"-1e-07", b"1e+16"]
    L = _lib.lib()
    a = (C.c_double * 1)(1.0)
    assert L.traj_dataset_format_f64_host(None, 0, None, None) == _lib.TRAJ_OK
    assert L.traj_dataset_format_f64_host(a, -1, None, None) == _lib.TRAJ_E_ARG
    assert L.traj_dataset_format_f64_host(a, 1, None, None) == _lib.TRAJ_E_ARG
    # the device entry points report argument errors before any launch (no GPU is touched here)
    fk = C.c_void_p(16)
    assert L.traj_dataset_format_f64_batch(None, 3, fk, fk, None) == _lib.TRAJ_E_ARG
    assert L.traj_dataset_format_f64_batch(None, 0, None, None, None) == _lib.TRAJ_OK
    rows, fmt = L.traj_dataset_csv_device_rows, L.traj_dataset_csv_device_format
    assert rows(0, 2, 3, 0.01, fk, fk, None, fk, 0, 0, None, None, None) == _lib.TRAJ_OK
    assert rows(2, 2, 3, 0.01, fk, fk, None, fk, 0, 8, fk, None, None) == _lib.TRAJ_E_ARG      # which
    assert rows(0, 2, 3, 0.01, fk, fk, None, fk, 1, 8, fk, None, None) == _lib.TRAJ_E_ARG      # past the last row
    assert rows(0, 2, 3, 0.01, fk, fk, None, fk, -1, 2, fk, None, None) == _lib.TRAJ_E_ARG
    assert rows(1, 2, 3, 0.01, fk, fk, None, fk, 0, 8, fk, None, None) == _lib.TRAJ_E_ARG      # noisy without noise
    assert rows(0, 2, 3, 0.01, fk, None, None, fk, 0, 8, fk, None, None) == _lib.TRAJ_E_ARG
    assert rows(0, 2, 3, 0.01, fk, fk, None, fk, 0, 8, None, None, None) == _lib.TRAJ_E_ARG
    assert fmt(0, 2, 3, 0.01, fk, fk, None, fk, 0, 0, None, None, 0, None, 0, fk, None) == _lib.TRAJ_OK
    assert fmt(0, 2, 3, 0.01, fk, fk, None, fk, 0, 8, fk, fk, 0, fk, 64, None, None) == _lib.TRAJ_E_ARG   # no flag
    assert fmt(0, 2, 3, 0.01, fk, fk, None, fk, 0, 8, fk, fk, 0, fk, -1, fk, None) == _lib.TRAJ_E_ARG
    assert fmt(0, 2, 3, 0.01, fk, fk, None, fk, 0, 9, fk, fk, 0, fk, 64, fk, None) == _lib.TRAJ_E_ARG
    assert fmt(0, 2, 3, 0.01, fk, fk, None, fk, 0, 8, None, fk, 0, fk, 64, fk, None) == _lib.TRAJ_E_ARG
    assert L.traj_dataset_csv_device_check(None, None) == _lib.TRAJ_E_ARG


def test_committed_table_is_the_generators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_pow10_tables as G
    finally:
        sys.path.pop(0)
    G.check_logs()
    assert open(os.path.join(CSRC, "fmt_pow10_tables.h")).read() == G.text()
    # spot values: 10^0 = 2^127 / 2^127 exactly, 10^27 is exact in 128 bits, 10^-1 rounds up
    assert G.g(0) == 1 << 127
    assert G.g(27) == 10 ** 27 << (127 - (10 ** 27).bit_length() + 1)
    assert G.g(-1) == (1 << 131) // 10 + 1


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """The digits stay in a 64-bit integer and go straight to their destination: the compiler's resource report for
    the three kernels of dataset_fmt.hip (device code only, the library's flags) shows no scratch."""
    import re
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "dataset_fmt.co"),
                        os.path.join(CSRC, "dataset_fmt.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == 3, r.stderr[-3000:]
    assert scratch == [0, 0, 0], list(zip(names, scratch))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fmt_header_under_asan_ubsan(tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:strict_string_checks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = str(tmp_path / "san_fmt")
    r = subprocess.run(["g++", *san, "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize", "san_fmt.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "san_fmt ok" in r.stdout and "ERROR" not in r.stderr

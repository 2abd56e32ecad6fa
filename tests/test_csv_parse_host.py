"""csrc/parse_f64.h on the CPU (traj_dataset_parse_f64_host) against Python's float(), the correctly rounded double:
repr / %.17e / %.18e spellings of the formatter tests' edge list, 199,891 random bit patterns, exact halfway integers and
dataset magnitudes; zeros, range edges, what must be declined (with the output untouched) and the literals; the
committed power-of-five table against its generator; argument errors of the new entry points; the kernels' scratch;
the header and the host token function under ASan / UBSan (tests/sanitize/san_parse.cpp, a host program).  No
tolerance anywhere: the bits are equal or the test fails."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import _csv_parse_cases as K
from trajectory_generation_amd import _lib
from trajectory_generation_amd import dataset as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "trajectory_generation_amd", "csrc")
FILL = -7.25          # what a declined token must leave in the output


def parse(tokens):
    """(bits, statuses) of traj_dataset_parse_f64_host; the output starts as FILL."""
    out, st = D.parse_f64_host(tokens, fill=FILL)
    return out.view(np.uint64), st


def assert_exact(tokens):
    bits, st = parse(tokens)
    bad = np.nonzero(st != _lib.PARSE_OK)[0]
    assert bad.size == 0, [tokens[i] for i in bad[:5]]
    want = K.float_bits(tokens)
    bad = np.nonzero(bits != want)[0]
    assert bad.size == 0, [(tokens[i], hex(bits[i]), hex(want[i])) for i in bad[:5]]


def test_edge_spellings_equal_float():
    t = K.edge_spellings()
    assert len(t) > 3 * 4400
    assert_exact(t)


def test_random_reprs_equal_float():
    t = K.random_reprs()
    assert len(t) == 199_891
    assert_exact(t)


def test_random_19_digit_spellings_equal_float():
    assert_exact(K.random_19_digits())


def test_halfway_integers_round_to_even():
    t = K.halfway_integers()
    assert len(t) > 1200 and max(len(x) for x in t) == 19
    assert_exact(t)
    bits, _ = parse([b"9007199254740993", b"9007199254740995"])
    assert [float(x) for x in bits.view(np.float64)] == [9007199254740992.0, 9007199254740996.0]


def test_dataset_magnitudes_equal_float():
    assert_exact(K.dataset_magnitudes())


def test_zeros_keep_their_sign():
    t = [b"-0.0", b"0.0", b"-0", b"0", b"-0e5", b"-0.000", b"000.000e-5", b"-1e-999"]
    bits, st = parse(t)
    assert (st == _lib.PARSE_OK).all()
    assert bits.tolist() == [1 << 63, 0, 1 << 63, 0, 1 << 63, 1 << 63, 0, 1 << 63]


def test_range_edges():
    t = K.RANGE_EDGES
    bits, st = parse(t)
    want = K.float_bits(t)
    assert (st[:5] == _lib.PARSE_OK).all(), st
    fill = np.array([FILL]).view(np.uint64)[0]
    for i, tok in enumerate(t):
        assert (st[i] == _lib.PARSE_OK and bits[i] == want[i]) or (st[i] == _lib.PARSE_FALLBACK and bits[i] == fill), \
            (tok[:40], int(st[i]), hex(bits[i]), hex(want[i]))
    assert [float(x) for x in bits[:5].view(np.float64)] == [float("inf"), -0.0, float("inf"), 0.0, 5e-324]


def test_fallbacks_leave_the_output_untouched():
    bits, st = parse(K.FALLBACKS)
    assert (st == _lib.PARSE_FALLBACK).all(), [K.FALLBACKS[i] for i in np.nonzero(st != _lib.PARSE_FALLBACK)[0]]
    assert (bits.view(np.float64) == FILL).all()
    # 20 digits, one of them a trailing zero: 19 significant digits
    assert_exact([b"12345678901234567890e-5", b"12345678901234567890", b"0.00012345678901234567890"])
    bits, st = parse([b"12345678901234567891"])
    assert st[0] == _lib.PARSE_FALLBACK


def test_literals():
    bits, st = parse([b"", b"nan", b"NaN", b"inf", b"-inf"])
    assert (st == _lib.PARSE_OK).all()
    assert bits.tolist() == [K.NAN_BITS, K.NAN_BITS, K.NAN_BITS, 0x7FF0000000000000, 0xFFF0000000000000]
    # the empty field has the host reader's NaN bits
    hv, ok = D.csv_tokens_host([b"nan", b"NaN"])
    assert ok and hv.view(np.uint64).tolist() == [K.NAN_BITS, K.NAN_BITS]


def test_host_token_function():
    """traj_dataset_csv_token_host is the reader's token code: float()'s value for what the device declines."""
    t = [b"1234567890123456789012345", b"1e999", b"-1e-999", b"infinity", b"1.5", b"2.4703282292062328e-324"]
    v, ok = D.csv_tokens_host(t)
    assert ok and v.view(np.uint64).tolist() == K.float_bits(t).tolist()
    for bad in (b"+1.5", b" 1.0", b"1e", b"zz", b"1.2.3"):
        assert not D.csv_tokens_host([b"1.0", bad])[1], bad


def test_committed_table_is_the_generators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_pow5_tables as G
    finally:
        sys.path.pop(0)
    G.check_logs()
    assert open(os.path.join(CSRC, "parse_pow5_tables.h")).read() == G.text()
    # spot values: 5^0, 5^27 and 5^55 are exact (5^55 < 2^128), 5^-1 is the reciprocal rounded up
    assert G.t(0) == 1 << 127
    assert G.t(27) == 5 ** 27 << (128 - (5 ** 27).bit_length())
    assert G.t(55) == 5 ** 55 << (128 - (5 ** 55).bit_length()) and (5 ** 55).bit_length() == 128
    assert G.t(-1) == (1 << 130) // 5 + 1 == 0xCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCD
    assert G.t(56) == 5 ** 56 >> ((5 ** 56).bit_length() - 128)          # a floor from here on


def test_argument_errors():
    L = _lib.lib()
    OK, E = _lib.TRAJ_OK, _lib.TRAJ_E_ARG
    fk = C.c_void_p(16)
    assert L.traj_dataset_parse_f64_host(None, None, None, 0, None, None) == OK
    assert L.traj_dataset_parse_f64_host(fk, fk, fk, -1, fk, fk) == E
    assert L.traj_dataset_parse_f64_host(fk, fk, fk, 1, None, fk) == E
    assert L.traj_dataset_parse_f64_host(fk, fk, fk, 1, fk, None) == E
    assert L.traj_dataset_csv_token_host(None, None, None, 0, None) == OK
    assert L.traj_dataset_csv_token_host(fk, fk, fk, -1, fk) == E
    assert L.traj_dataset_csv_token_host(fk, None, fk, 1, fk) == E
    # the device entry points report argument errors before any launch (no GPU is touched here)
    assert L.traj_dataset_parse_f64_batch(None, None, None, 0, None, None, None) == OK
    assert L.traj_dataset_parse_f64_batch(None, fk, fk, 3, fk, fk, None) == E
    assert L.traj_dataset_parse_f64_batch(fk, fk, fk, -3, fk, fk, None) == E
    chunk = _lib.CSV_PARSE_CHUNK
    assert L.traj_dataset_csv_parse_chunks(0) == 0 and L.traj_dataset_csv_parse_chunks(-1) == E
    assert L.traj_dataset_csv_parse_chunks(chunk) == 1 and L.traj_dataset_csv_parse_chunks(chunk + 1) == 2
    assert L.traj_dataset_csv_parse_count(None, 0, None, None) == OK
    assert L.traj_dataset_csv_parse_count(None, 5, fk, None) == E
    assert L.traj_dataset_csv_parse_count(fk, 5, None, None) == E
    assert L.traj_dataset_csv_parse_count(fk, -5, fk, None) == E
    assert L.traj_dataset_csv_parse_starts(None, 0, None, None, 0, None) == OK
    assert L.traj_dataset_csv_parse_starts(fk, 5, fk, None, 1, None) == E
    assert L.traj_dataset_csv_parse_starts(fk, 5, None, fk, 1, None) == E
    assert L.traj_dataset_csv_parse_starts(fk, 5, fk, fk, -1, None) == E
    assert L.traj_dataset_csv_parse_starts(fk, 0, fk, fk, 1, None) == E          # rows without text
    rows = L.traj_dataset_csv_parse_rows
    assert rows(None, 0, None, 0, 3, None, fk, fk, None, 0, None) == OK
    assert rows(fk, 5, fk, 1, 3, fk, None, fk, fk, 4, None) == E                # no error word
    assert rows(fk, 5, fk, 1, 3, fk, fk, None, fk, 4, None) == E                # no counter
    assert rows(fk, 5, fk, 1, 3, fk, fk, fk, None, 4, None) == E                # cap without records
    assert rows(fk, 5, fk, 1, 0, fk, fk, fk, fk, 4, None) == E                  # no columns
    assert rows(fk, 5, None, 1, 3, fk, fk, fk, fk, 4, None) == E
    assert rows(fk, 5, fk, 1, 3, None, fk, fk, fk, 4, None) == E
    assert rows(fk, -5, fk, 1, 3, fk, fk, fk, fk, 4, None) == E
    assert rows(fk, 0, fk, 1, 3, fk, fk, fk, fk, 4, None) == E                  # rows without text
    assert rows(fk, 5, fk, 1, 3, fk, fk, fk, fk, -1, None) == E
    gat = L.traj_dataset_csv_gather_f32
    assert gat(None, 0, 9, None, 0, 25, None, 5, None, fk, None) == OK
    assert gat(fk, 10, 9, fk, 2, 5, fk, 5, fk, None, None) == E                 # no error word
    assert gat(None, 10, 9, fk, 2, 5, fk, 5, fk, fk, None) == E
    assert gat(fk, 10, 9, None, 2, 5, fk, 5, fk, fk, None) == E
    assert gat(fk, 10, 9, fk, 2, 5, None, 5, fk, fk, None) == E
    assert gat(fk, 10, 9, fk, 2, 5, fk, 5, None, fk, None) == E
    assert gat(fk, 10, 0, fk, 2, 5, fk, 5, fk, fk, None) == E
    assert gat(fk, -1, 9, fk, 2, 5, fk, 5, fk, fk, None) == E
    assert gat(fk, 10, 9, fk, -2, 5, fk, 5, fk, fk, None) == E


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """The digits stay in a 64-bit integer and the field is read where it lies: the compiler's resource report for the
    five kernels of dataset_parse.hip (device code only, the library's flags) shows no scratch."""
    import re
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "dataset_parse.co"),
                        os.path.join(CSRC, "dataset_parse.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 5 and len(scratch) == 5, r.stderr[-3000:]
    assert scratch == [0] * 5, list(zip(names, scratch))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_parse_header_under_asan_ubsan(tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:strict_string_checks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = str(tmp_path / "san_parse")
    r = subprocess.run(["g++", *san, "-std=c++17", "-Wall", "-Werror", "-o", exe,
                        os.path.join(HERE, "sanitize", "san_parse.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "san_parse ok" in r.stdout and "ERROR" not in r.stderr

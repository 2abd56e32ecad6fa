"""csrc/spline.h and csrc/workload.hip on the CPU (traj_gen_spline_coef_host, traj_gen_workload_host) against an exact
rational spline solve, batch.spline_natural and workload.make_workload; and the vectorised PathSet.build arrays against
the spline_natural loop, bit for bit; the header under ASan / UBSan (tests/sanitize/san_spline.cpp, a host program).
No GPU: the same text runs in the kernels (tests/test_workload_gpu.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests._workload_cases import (CASE_IDS, CASES, KINDS, exact_spline, host_workload, irregular_knot_sets, pack_knots,
                                   scaled_error, ulp_distance, workload_knot_sets)
from trajectory_generation_amd import _lib
from trajectory_generation_amd.batch import (REFERENCE_PARAMS, spline_coef_host, spline_natural, spline_natural_stacked,
                                             spline_rows)
from trajectory_generation_amd.workload import SPLINE_KNOTS_X, workload_rows_host

HERE = os.path.dirname(os.path.abspath(__file__))

# Y, phi and the spline coefficients of traj_gen_workload_host against make_workload: 4 x the worst absolute
# difference measured over the nine (kind, case) workloads below (1.1e-16, in a coefficient and in Y of the two-word
# spline case; the mixed and parabola rows were equal), capped at 1e-13
ROUNDING_BAR = min(4 * 1.1102230246251565e-16, 1e-13)


@pytest.mark.parametrize("sets", [workload_knot_sets, irregular_knot_sets], ids=["workload-knots", "irregular"])
def test_coefficients_against_the_exact_solve(sets):
    """The header's Thomas solve is as accurate as spline_natural's LAPACK solve: over each input set its worst error
    against the exact rational spline, scaled by max(1, max |coef|) of the trajectory, is at most twice
    spline_natural's worst on the same set (a different but equally long rounding chain), and the two agree within
    1e-15 scaled.  Measured: 1.3e-16 against 1.6e-16 on the workload's knots (64 sets), 3.9e-16 against 5.1e-16 on
    the 200 irregular sets; worst difference between the two 1.7e-16 and 3.9e-16."""
    sets = sets()
    kinds, nk, xk, yk = pack_knots(sets, 12)
    coef, flag = spline_coef_host(kinds, nk, xk, yk)
    assert not flag.any()
    err_header = err_numpy = diff = 0.0
    for b, (x, y) in enumerate(sets):
        n = len(x)
        exact = exact_spline(x, y)
        ref = spline_natural(x, y)
        err_header = max(err_header, scaled_error(coef[b, :n - 1], exact))
        err_numpy = max(err_numpy, scaled_error(ref, exact))
        diff = max(diff, np.abs(coef[b, :n - 1] - ref).max() / max(1.0, np.abs(ref).max()))
        assert (coef[b, n - 1:] == 0.0).all(), b
    print(f"scaled error: header {err_header:.3e}, spline_natural {err_numpy:.3e}, between them {diff:.3e}")
    assert err_header <= 2.0 * err_numpy
    assert diff <= 1e-15


def test_edge_rows_flags_and_padding():
    kmax = 5
    rows = [
        (2, 2, [1.0, 3.5], [0.25, -1.0]),                          # 0: nk = 2, one piece, the chord
        (2, 3, [0.0, 1.0, 2.5], [0.5, -0.5, 2.0]),                 # 1: nk = 3
        (2, 4, [-1.0, 0.0, 0.7, 4.0], [1.0, 2.0, -3.0, 0.1]),      # 2: nk = 4
        (2, 1, [0.0], [1.0]),                                      # 3: nk = 1                    -> flag
        (2, 6, [0.0, 1.0, 2.0, 3.0, 4.0], [0.0] * 5),              # 4: nk > kmax                 -> flag
        (2, 3, [0.0, 1.0, 1.0], [0.0, 1.0, 2.0]),                  # 5: equal knots               -> flag
        (2, 3, [0.0, 2.0, 1.0], [0.0, 1.0, 2.0]),                  # 6: descending knots          -> flag
        (2, 3, [0.0, 1.0, 2.0], [0.0, float("nan"), 2.0]),         # 7: a NaN ordinate            -> flag
        (2, 3, [0.0, 1.0, float("inf")], [0.0, 1.0, 2.0]),         # 8: an infinite knot          -> flag
        (0, 3, [0.0, 0.0, 0.0], [5.0, 5.0, 5.0]),                  # 9: kind 0: zeros, no flag, whatever the knots
        (1, 0, [], []),                                            # 10: kind 1
        (2, 5, [0.0, 1.0, 2.0, 3.0, 4.0], [1.0, -1.0, 1.0, -1.0, 1.0]),   # 11: nk = kmax
    ]
    B = len(rows)
    kinds = np.array([r[0] for r in rows], dtype=np.int32)
    nk = np.array([r[1] for r in rows], dtype=np.int32)
    xk, yk = np.zeros((B, kmax)), np.zeros((B, kmax))
    for b, (_, _, x, y) in enumerate(rows):
        xk[b, :len(x)] = x
        yk[b, :len(y)] = y
    coef, flag = spline_coef_host(kinds, nk, xk, yk)
    assert flag.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert coef[0, 0].tolist() == [0.25, (-1.0 - 0.25) / (3.5 - 1.0), 0.0, 0.0]
    assert (coef[0, 1:] == 0.0).all()
    # against the exact solve: the longest chain to a coefficient of these short rows is about nine rounded operations
    # (two slopes, the right-hand side, the pivot, d', M, then 2 M + M', the product with h, the division by 6 and the
    # difference), each within 2^-53 relative on values no larger than the row's largest coefficient: 9 x 2^-53 = 1e-15
    for b in (1, 2, 11):
        n = nk[b]
        assert scaled_error(coef[b, :n - 1], exact_spline(xk[b, :n], yk[b, :n])) <= 9 * 2.0 ** -53, b
        assert (coef[b, n - 1:] == 0.0).all()
    for b in (3, 4, 5, 6, 7, 8, 9, 10):
        assert (coef[b] == 0.0).all(), b


@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_workload_host_against_make_workload(kind, case):
    """traj_gen_workload_host is make_workload: kinds, pcs, the knot ordinates and x0's X, vx, vy, omega bit for bit
    (integer arithmetic and one written order of float64 operations); u0[:, 0] within 2 ulp (the host's scalar v ** 2 is
    libm pow, the library forms v * v); Y, phi and the spline coefficients within ROUNDING_BAR = 4.4e-16 (4 x the
    measured worst, 1.1e-16: Thomas against LAPACK and what follows from it) -- a wrong spline piece, derivative or draw
    order misses by 1e-3 or more."""
    seed, off, B = CASES[case]
    w = host_workload(kind, case)
    h = workload_rows_host(B, kind, seed, off)
    assert h["kinds"].tolist() == w["kinds"].tolist()
    assert h["pcs"].view(np.int64).tolist() == w["pcs"].view(np.int64).tolist()
    for col in (0, 3, 4, 5):
        assert h["x0"][:, col].view(np.int64).tolist() == w["x0"][:, col].view(np.int64).tolist(), col
    assert (h["u0"][:, 1] == 0.0).all() and not np.signbit(h["u0"][:, 1]).any()
    assert ulp_distance(h["u0"][:, 0], w["u0"][:, 0]).max() <= 2.0
    dY = np.abs(h["x0"][:, 1] - w["x0"][:, 1]).max()
    dphi = np.abs(h["x0"][:, 2] - w["x0"][:, 2]).max()
    print(f"{kind} {CASE_IDS[case]}: |dY| {dY:.3e} |dphi| {dphi:.3e}")
    assert dY <= ROUNDING_BAR and dphi <= ROUNDING_BAR
    if kind == "spline":
        n = len(SPLINE_KNOTS_X)
        assert h["xk"].shape == (B, n) and (h["xk"] == SPLINE_KNOTS_X).all() and (h["nk"] == n).all()
        assert h["yk"].view(np.int64).tolist() == w["yk"].view(np.int64).tolist()
        dcoef = np.abs(h["coef"] - w["coef"]).max()
        print(f"  |dcoef| {dcoef:.3e}")
        assert dcoef <= ROUNDING_BAR
    else:
        assert (h["nk"] == 0).all()
        assert not h["xk"].any() and not h["yk"].any() and not h["coef"].any()


def test_workload_host_takes_vehicle_params():
    """u0 is d_steady_state with the caller's parameters; the draws do not depend on them."""
    p = dict(REFERENCE_PARAMS, Cr0=0.07, Cm2=0.04)
    a = workload_rows_host(5, "mixed", 3, 0)
    b = workload_rows_host(5, "mixed", 3, 0, params=p)
    assert (a["x0"] == b["x0"]).all()
    v = b["x0"][:, 3]
    want = (p["Cr0"] + p["Cr2"] * (v * v)) / (p["Cm1"] - p["Cm2"] * v)
    assert b["u0"][:, 0].tolist() == want.tolist() and (a["u0"][:, 0] != b["u0"][:, 0]).all()


def test_vectorised_rows_equal_the_spline_natural_loop():
    """batch.spline_rows (PathSet.build's arrays: one stacked np.linalg.solve per knot count) against the per-trajectory
    spline_natural loop it replaces, bit for bit: knot counts 2, 3, 4 and 11 mixed with kind-0 / kind-1 rows."""
    rng = np.random.default_rng(5)
    kinds, knots = [], []
    for i in range(72):
        if i % 6 == 4:
            kinds.append(i % 2); knots.append(None)
            continue
        n = (2, 3, 4, 11)[i % 4]
        kinds.append(2)
        knots.append((np.cumsum(rng.uniform(0.2, 5.0, n)) - 6.0, rng.uniform(-3.0, 3.0, n)))
    nk, xk, coef = spline_rows(kinds, knots, 11)
    want_nk, want_xk, want = np.zeros(72, np.int32), np.zeros((72, 11)), np.zeros((72, 10, 4))
    for b, k in enumerate(knots):
        if kinds[b] == 2:
            want_nk[b] = len(k[0])
            want_xk[b, :len(k[0])] = k[0]
            want[b, :len(k[0]) - 1] = spline_natural(*k)
    assert nk.tolist() == want_nk.tolist() and (xk == want_xk).all()
    assert coef.view(np.int64).tolist() == want.view(np.int64).tolist()
    one = spline_natural_stacked(knots[3][0][None], knots[3][1][None])[0]
    assert one.view(np.int64).tolist() == spline_natural(*knots[3]).view(np.int64).tolist()


def test_argument_errors():
    L, p = _lib.lib(), _lib.ptr
    E = _lib.TRAJ_E_ARG
    B, kmax = 3, 11
    kind, nk = np.full(B, 2, np.int32), np.full(B, 2, np.int32)
    xk, yk = np.tile(np.arange(kmax, dtype=np.float64), (B, 1)), np.zeros((B, kmax))
    coef, flag = np.zeros((B, kmax - 1, 4)), np.zeros(B, np.int32)
    good = [p(kind), p(nk), p(xk), p(yk), p(coef), p(flag)]
    for host in (True, False):      # no launch happens for any of these: the device entries refuse them on the host
        f = L.traj_gen_spline_coef_host if host else (lambda *a: L.traj_gen_spline_coef_batch(*a, None))
        assert f(0, kmax, *good) == E and f(-1, kmax, *good) == E and f(B, 1, *good) == E
        for i in range(len(good)):
            assert f(B, kmax, *[None if j == i else a for j, a in enumerate(good)]) == E, i
    assert L.traj_gen_spline_coef_host(B, kmax, *good) == _lib.TRAJ_OK

    vp = _lib.default_params()
    words = np.zeros(8, dtype=np.uint32)
    outs = [np.zeros(B, np.int32), np.zeros((B, 4)), np.zeros(B, np.int32), np.zeros((B, kmax)), np.zeros((B, kmax)),
            np.zeros((B, kmax - 1, 4)), np.zeros((B, 6)), np.zeros((B, 2))]
    po = [p(a) for a in outs]
    for host in (True, False):
        f = L.traj_gen_workload_host if host else (lambda *a: L.traj_gen_workload_batch(*a, None))
        assert f(None, 0, p(words), 1, 0, B, kmax, *po) == E
        assert f(C.byref(vp), 0, None, 1, 0, B, kmax, *po) == E
        assert f(C.byref(vp), 3, p(words), 1, 0, B, kmax, *po) == E
        assert f(C.byref(vp), -1, p(words), 1, 0, B, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), 0, 0, B, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), _lib.WORKLOAD_MAX_SEED_WORDS + 1, 0, B, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), 1, 0, 0, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), 1, -1, B, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), 1, 2 ** 63 - 2, B, kmax, *po) == E
        assert f(C.byref(vp), 0, p(words), 1, 0, B, 10, *po) == E      # spline needs its 11 knots
        assert f(C.byref(vp), 1, p(words), 1, 0, B, 1, *po) == E
        for i in range(len(po)):
            holed = [None if j == i else a for j, a in enumerate(po)]
            assert f(C.byref(vp), 0, p(words), 1, 0, B, kmax, *holed) == E, i
    ns = _lib.WORKLOAD_MAX_SEED_WORDS
    assert L.traj_gen_workload_host(C.byref(vp), 1, p(words), ns, 0, B, 2, *po) == _lib.TRAJ_OK
    for bad in (dict(seed=-1), dict(seed=2 ** 192), dict(id_offset=-1), dict(kind="circle")):
        with pytest.raises(ValueError):
            workload_rows_host(**{"B": 2, **bad})
    with pytest.raises(ValueError):
        np.random.default_rng([-1, 0])
    assert L.traj_gen_abi_version() == 1 and L.traj_abi_version() == 4


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_spline_header_under_asan_ubsan(tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = str(tmp_path / "san_spline")
    r = subprocess.run(["g++", *san, "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                        os.path.join(HERE, "sanitize", "san_spline.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "san_spline ok" in r.stdout and "ERROR" not in r.stderr

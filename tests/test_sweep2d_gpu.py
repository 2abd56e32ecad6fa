"""The factorization sweep of the fused capacity-40 instance (8 x 8 blocks, TGMPC_SWEEP_2D) leaves every result where
the parent commit had it: the closed loop's histories, statuses and iteration counts equal the parent's recorded ones
(tests/golden/sweep_parent.npz, written by tools/record_sweep_golden.py from a library built at the commit the file
names) as float64 bit patterns, for every case of the recorder -- the other capacities and the per-step kernels, which
keep the row-per-lane sweep, included.  And the default fused run equals the 3-waves-per-SIMD instance, which keeps the
row-per-lane sweep, on the same inputs."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_parent.npz")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_sweep_golden",
                                                  os.path.join(ROOT, "tools", "record_sweep_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("kind", REC.KINDS)
@pytest.mark.parametrize("N", REC.HORIZONS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "step"])
def test_closed_loop_equals_parent_bits(gpu, golden, kind, N, fused):
    for warm in (0, 1):
        for mode in (0, 1):
            name = REC.case_name(kind, N, warm, mode, fused)
            r = REC.run_case(kind, N, warm, mode, fused)
            for k in REC.KEYS:
                want = golden[f"{name}/{k}"]
                assert r[k].dtype == want.dtype and r[k].shape == want.shape, (name, k)
                assert np.array_equal(_bits(r[k]), _bits(want)), (name, k, str(golden["commit"]))


def test_golden_covers_every_case(golden):
    assert len(str(golden["commit"])) >= 7
    assert sorted(k for k in golden if "/" in k) == sorted(f"{REC.case_name(*c)}/{k}" for c in REC.cases()
                                                           for k in REC.KEYS)


@pytest.mark.parametrize("kind,N,warm,mode", [("spline", 20, 1, 0), ("mixed", 20, 0, 1), ("spline", 17, 0, 0),
                                              ("mixed", 17, 1, 1)])
def test_default_fused_equals_three_wave_instance(gpu, kind, N, warm, mode):
    from trajectory_generation_amd import _lib
    runs = {}
    try:
        for wv in (0, 3):   # the default (2 waves per SIMD: the 8 x 8 sweep), the 3-wave instance (row per lane)
            _lib.check(_lib.lib().traj_debug_fused_waves(wv), "traj_debug_fused_waves")
            runs[wv] = REC.run_case(kind, N, warm, mode, True)
    finally:
        _lib.lib().traj_debug_fused_waves(0)
    for k in REC.KEYS:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[3][k])), k

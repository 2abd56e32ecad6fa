"""The host side of the MPC launches (csrc/mpc_host.h, the workspace layout of csrc/mpc_route.h, the one Python call
path of the closed loop) leaves every result where the parent commit had it: on every solver route the closed loop
(fused and per step, two launches), the step entry (linearization inside and before the solve) and the QP entry, and at
N = 20 and 24 the speed schedules, the observed loops, the statistics and a one-workgroup fused grid, all equal the
parent's recorded ones (tests/golden/launch_parent.npz, written by tools/record_launch_golden.py from a library built
at the commit the file names) as bit patterns: float64 viewed as int64, NaN bits included."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_parent.npz")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_launch_golden",
                                                  os.path.join(ROOT, "tools", "record_launch_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,fn,arg", REC.cases(), ids=[c[0] for c in REC.cases()])
def test_entry_points_equal_parent_bits(gpu, golden, name, fn, arg):
    got = fn(arg)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want), name
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape, (name, k)
        assert np.array_equal(REC.bits(v), REC.bits(want[k])), (name, k, str(golden["commit"]))


def test_golden_names_its_commit_and_every_group(golden):
    assert len(str(golden["commit"])) >= 7
    assert sorted({k.split("/")[0] for k in golden if "/" in k}) == sorted(c[0] for c in REC.cases())


def test_debug_switches_are_back_at_their_defaults(gpu):
    """After the recorder's runs (whatever their order): the default routes' sizes, read through the library."""
    import ctypes as C
    from trajectory_generation_amd import _lib, batch as TB
    L = _lib.lib()
    with REC.switches():
        pass
    cfg = TB.config_struct(N=24, Ts=REC.TS)
    split = int(L.traj_mpc_step_workspace_bytes(C.byref(cfg), REC.B))
    with REC.switches(traj_debug_split_min_n=41):
        assert int(L.traj_mpc_step_workspace_bytes(C.byref(cfg), REC.B)) < split   # capacity 80: no P scratch
    assert int(L.traj_mpc_step_workspace_bytes(C.byref(cfg), REC.B)) == split

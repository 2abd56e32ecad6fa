"""Record tests/golden/sweep_parent.npz: the closed loop's results for the factorization-sweep regression cases,
from a library built at the PARENT commit of the change under test (tests/test_sweep2d_gpu.py asserts equal float64
bit patterns against the file).

  git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/trajectory_generation_amd/csrc
  TRAJMPC_LIB=/tmp/parent/trajectory_generation_amd/libtrajmpc.so \
      python tools/record_sweep_golden.py --commit <parent commit> [--out tests/golden/sweep_parent.npz]

Cases: run_closed_loop X, U, status, iters for B = 8, T = 6, dt 0.05; spline and mixed references; N in {20, 17, 13, 8,
5} (capacity 40 full, capacity 40 with a block of the 8 x 8 sweep straddling the padding, capacities 32 and 16);
warm_start 0 and 1 (cold first steps refactor on rho; every optimal step factors the polish K with inactive rows);
polish_mode 0 and 1; the fused launch and the per-step launches.  The commit is stored in the file (key "commit")."""
import argparse
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

B, T, TS, SEED = 8, 6, 0.05, 5
KINDS = ("spline", "mixed")
HORIZONS = (20, 17, 13, 8, 5)
KEYS = ("X", "U", "status", "iters")


def cases():
    """(kind, N, warm_start, polish_mode, fused) of every recorded run."""
    return list(itertools.product(KINDS, HORIZONS, (0, 1), (0, 1), (True, False)))


def case_name(kind, N, warm, mode, fused):
    return f"{kind}_N{N}_w{warm}_p{mode}_{'fused' if fused else 'step'}"


def run_case(kind, N, warm, mode, fused):
    """The run's X, U, status, iters as numpy arrays."""
    from trajectory_generation_amd import batch as TB
    from trajectory_generation_amd.workload import make_workload
    w = make_workload(B, N, TS, kind=kind, seed=SEED)
    paths = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"])
    cfg = TB.config_struct(N=N, Ts=TS, warm_start=warm, polish_mode=mode)
    r = TB.run_closed_loop(w["x0"], w["u0"], paths, w["vref"], T, cfg, fused=fused)
    return {k: r[k].cpu().numpy() for k in KEYS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built at (stored in the file)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "sweep_parent.npz"))
    args = ap.parse_args()
    from trajectory_generation_amd import _lib
    out = {"commit": np.array(args.commit), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for c in cases():
        r = run_case(*c)
        for k in KEYS:
            out[f"{case_name(*c)}/{k}"] = r[k]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(cases())} runs from {_lib.LIB_PATH} ({args.commit}), {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

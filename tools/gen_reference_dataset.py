"""The reference's own training set in one call: generation_type1 (open-loop profiles), generation_type2 (piecewise
state machine) and merge_datasets, at the reference's sizes by default (5,000 trajectories of 1,200 steps each,
Ts = 0.01, seed 42).  Both generators run as one kernel launch each on the GPU; the merge works on the CSV text.

  python tools/gen_reference_dataset.py --out-dir data                         all three steps
  python tools/gen_reference_dataset.py --out-dir data --only type2            vehicle_piecewise_{clean,noisy}.csv alone
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
      tools/gen_reference_dataset.py --out-dir data --trajectories 625         625 per GPU, gathered into rank 0

Files (the reference's names): vehicle_mpc_like_{clean,noisy}.csv (type 1), vehicle_piecewise_{clean,noisy}.csv
(type 2), vehicle_merged_{clean,noisy}.csv (type 2's ids shifted past type 1's).  Prints the timings as JSON on rank 0.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--trajectories", type=int, default=5000, help="per generator and per GPU")
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--only", choices=("type1", "type2"), default=None)
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from trajectory_generation_amd import dataset as D
    os.makedirs(a.out_dir, exist_ok=True)
    pre = {k: os.path.join(a.out_dir, v) for k, v in (("type1", "vehicle_mpc_like"), ("type2", "vehicle_piecewise"),
                                                       ("merged", "vehicle_merged"))}
    res = {"trajectories_per_generator": a.trajectories * world, "steps": a.steps, "n_gpus": world}
    root = True
    for kind, fn in (("type1", D.generate_open_loop), ("type2", D.generate_piecewise)):
        if a.only not in (None, kind):
            continue
        t0 = time.perf_counter()
        r = fn(a.trajectories, a.steps, Ts=a.dt, seed=a.seed, out_prefix=pre[kind], dist=dist)
        torch.cuda.synchronize()
        res[f"{kind}_s"] = time.perf_counter() - t0        # draw / seeding, kernel, gather, CSV write
        root = r is not None
    if root and a.only is None:
        t0 = time.perf_counter()
        res["id_offset"] = D.merge_datasets(pre["type1"], pre["type2"], pre["merged"])
        res["merge_s"] = time.perf_counter() - t0
    if root:
        print(json.dumps(res))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

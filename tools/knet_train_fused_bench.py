"""KalmanNet training step: the module path under autograd (knet_train.tbptt_sequence) against the fused graph path
(knet_train_fused.py), timed alternately in one process at the training.py configuration of tools/knet_train_bench.py:
in_mult 10, out_mult 40, hidden 128, batch 64, K = T = 200, AdamW(lr 1e-4, wd 1e-5), composite loss (alpha 0.8),
strategy 'standard'; synthetic data, random-init weights; three epochs each after a warm-up epoch of each path (the
fused path's includes the graph capture, reported on its own).  A second line: the same with the open-loop prediction
loss (pipeline_prediction.train_epoch, lambda_pred 0.5, H = 20).  One JSON line each, both written to
profiles/knet_train_fused_bench.json.   python tools/knet_train_fused_bench.py [B] [T]"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from trajectory_generation_amd import knet as K  # noqa: E402
from trajectory_generation_amd import knet_train as KT  # noqa: E402
from trajectory_generation_amd import knet_train_fused as KF  # noqa: E402
from trajectory_generation_amd import pipeline_prediction as PP  # noqa: E402

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = int(sys.argv[2]) if len(sys.argv) > 2 else 200
REPS = 3


def setup():
    torch.manual_seed(0)
    random.seed(0)
    sysm = K.VehicleModel(0.01, T, T, torch.zeros(6, 1))
    sysm.Params.update(bench.KNET_LIMITS)
    model = K.KalmanNetNN(dev)
    model.NNBuild(sysm, in_mult_KNet=10, out_mult_KNet=40, hidden_dim_gru=128)
    norm = {"x_mean": torch.zeros(1, 6, 1), "x_std": torch.ones(1, 6, 1), "y_mean": torch.zeros(1, 5, 1),
            "y_std": torch.ones(1, 5, 1)}
    model.set_normalization(norm["x_mean"], norm["x_std"], norm["y_mean"], norm["y_std"])
    x = 0.5 * torch.randn((B, 6, T), device=dev)
    y = x[:, [0, 1, 3, 4, 5], :] + 0.05 * torch.randn((B, 5, T), device=dev)
    u = 0.2 * torch.randn((B, 2, T), device=dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    return model, opt, norm, x, y, u


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(name, epoch, p):
    model, opt, norm, x, y, u = setup()
    run = {False: lambda: epoch(model, opt, y, u, x, norm, dict(p, fused=False)),
           True: lambda: epoch(model, opt, y, u, x, norm, dict(p, fused=True))}
    run[False]()                      # warm-up (GEMM heuristics, allocator)
    warm_fused, _ = timed(run[True])  # warm-up: two eager chunks, the capture, one replay
    dt, losses = {False: [], True: []}, {False: [], True: []}
    for _ in range(REPS):
        for fused in (False, True):   # alternately, in one process
            d, out = timed(run[fused])
            dt[fused].append(d)
            losses[fused].append(float(out[0]))
    runner = KF.runner_for(model, B, min(p["K_TBPTT"], T))
    ms = {k: 1e3 * min(v) / T for k, v in dt.items()}
    lp = KF.LAUNCHES_PER_STEP
    return {"metric": f"KalmanNet training ms per time step, module path vs fused graph path ({name})",
            "ms_per_step_parent": ms[False], "ms_per_step_fused": ms[True], "ratio": ms[False] / ms[True],
            "ms_per_step_all": {"parent": [1e3 * d / T for d in dt[False]], "fused": [1e3 * d / T for d in dt[True]]},
            "sequence_steps_per_s_fused": B * T / min(dt[True]),
            "graph_instantiate_s": runner.graph_instantiate_s, "fused_first_epoch_s": warm_fused,
            "tape_bytes": runner.tape_bytes, "graphs": len(runner.graphs),
            "launches_per_step_train_mode": lp["forward"][1] + lp["backward"][1],
            "config": dict({k: v for k, v in p.items() if k != "device"}, batch=B, in_mult=10, out_mult=40, hidden=128,
                           optimizer="AdamW(lr 1e-4, wd 1e-5)", reps=REPS, statistic="min of reps"),
            "losses": {"parent": losses[False], "fused": losses[True]}}


if __name__ == "__main__":
    base = dict(K_TBPTT=200, T=T, m=6, n=5, N_E=B, N_batch=B, device=dev)
    res = [measure("composite loss", KT.train_epoch,
                   dict(base, strategy="standard", CompositionLoss=True, alpha=0.8)),
           measure("state loss + 0.5 x prediction loss, H = 20", PP.train_epoch,
                   dict(base, lambda_pred=0.5, pred_horizon=20))]
    for r in res:
        print(json.dumps(r))
    out = os.path.join(ROOT, "profiles", "knet_train_fused_bench.json")
    with open(out, "w") as f:
        for r in res:
            f.write(json.dumps(r) + "\n")

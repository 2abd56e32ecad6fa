"""KalmanNet training with the open-loop prediction loss at the reference's training.py
configuration: in_mult 10, out_mult 40, hidden 128, batch 64, TBPTT chunk 200, AdamW(lr 1e-4, wd 1e-5), lambda_pred
0.5, H = 20; synthetic data, random-init weights, T = 200 steps per measured epoch (one chunk; the reference's T = 1200
is six).  Reports the time of one filter step of the epoch (forward + backward + AdamW, per time step)
  * without the prediction loss (lambda_pred = 0: the same filter path as tools/knet_train_bench.py, whose figure on
    the parent commit is the baseline),
  * with it on the fused path (one traj_knet_pred_loss_f32 launch per chunk),
  * with it on the step-wise path (H model.f launches per time step under autograd, as the reference evaluates it),
and the kernel's own time for batch x chunk = 12,800 windows at H = 20 and 50 (values + gradients).
python tools/knet_pred_train_bench.py [B] [T] [H] [--no-stepwise]"""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from trajectory_generation_amd import knet as K  # noqa: E402
from trajectory_generation_amd import pipeline_prediction as PP  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dev = torch.device("cuda:0")
B = int(args[0]) if len(args) > 0 else 64
T = int(args[1]) if len(args) > 1 else 200
H = int(args[2]) if len(args) > 2 else 20
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
base = dict(K_TBPTT=200, T=T, m=6, n=5, N_E=B, N_batch=B, device=dev, pred_horizon=H)


def epoch_ms(p, reps):
    PP.train_epoch(model, opt, y, u, x, norm, dict(p, T=min(T, 20)))   # warm-up (GEMM heuristics, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [PP.train_epoch(model, opt, y, u, x, norm, p) for _ in range(reps)]
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps / T, out[-1]


res = {"filter_only_ms_per_step": epoch_ms(dict(base, lambda_pred=0.0), 3)[0]}
res["fused_ms_per_step"], last = epoch_ms(dict(base, lambda_pred=0.5), 3)
res["fused_losses"] = [last[0], last[1]]
if "--no-stepwise" not in sys.argv:
    res["stepwise_ms_per_step"], last = epoch_ms(dict(base, lambda_pred=0.5, stepwise=True), 1)
    res["stepwise_losses"] = [last[0], last[1]]

# the kernel alone: batch x chunk windows, values + gradients
Kc = 200
xe = 0.5 * torch.randn((B, 6, Kc), device=dev)
uu, xg = 0.2 * torch.randn((B, 2, Kc + 64), device=dev), 0.5 * torch.randn((B, 6, Kc + 64), device=dev)
xm, xs = torch.zeros(6, device=dev), torch.ones(6, device=dev)
for h in (20, 50):
    call = lambda: K.knet_pred_loss(sysm.Params, sysm.Ts, xe, 0, 1, uu, xg, h, xm, xs)   # noqa: E731
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    torch.cuda.synchronize()
    res[f"kernel_us_{B * Kc}_windows_H{h}"] = 1e3 * e0.elapsed_time(e1) / 20   # (launch + two output allocations)
print(json.dumps({"metric": "KalmanNet training step with the open-loop prediction loss (ms per time step)", **res,
                  "config": {"batch": B, "T": T, "K_TBPTT": 200, "H": H, "lambda_pred": 0.5, "in_mult": 10,
                             "out_mult": 40, "hidden": 128, "optimizer": "AdamW(lr 1e-4, wd 1e-5)"}}))

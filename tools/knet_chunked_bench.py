"""Chunk-and-shuffle KalmanNet training (pipeline_indipendent_chunking.py): milliseconds per optimizer update of
  (a) the module path under autograd, torch's clip_grad_norm_ and AdamW;
  (b) the fused chunk of knet_train_fused.py with the update outside the graph, as the other fused pipelines run it:
      torch gather + normalisation, add_grads, clip_grad_norm_, the foreach AdamW, zero_grad and a loss read per batch;
  (c) the whole update in the graph (chunked_batches' fused path): gather, chunk, clip + AdamW replayed, the losses
      read once per epoch.
The reference's configuration (training_indipendent_chunking.py:36-62): in_mult 5, out_mult 40, hidden 128, batch 64,
AdamW(lr 1e-4, wd 1e-5), composite loss (alpha 0.8), train mode; synthetic data as tools/knet_train_fused_bench.py,
64 trajectories of 4 T_train steps = 4 batches per epoch; T_train = 200 and 25.  The variants run alternately in one
process after a warm-up epoch each (the fused ones' includes the capture); the figure is the min of 3 epochs / 4.
Every epoch's shuffle and start noise are drawn once (seeded) and shared by the three variants, so their recorded
epoch losses are comparable: equal weights at the start, equal batches, only the dropout streams differ.
One JSON line per T_train, both written to profiles/knet_chunked_bench.json.   python tools/knet_chunked_bench.py"""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.nn.utils import clip_grad_norm_  # noqa: E402

import bench  # noqa: E402
from trajectory_generation_amd import knet as K  # noqa: E402
from trajectory_generation_amd import knet_train_fused as KF  # noqa: E402
from trajectory_generation_amd import pipeline_indipendent_chunking as PC  # noqa: E402

dev = torch.device("cuda:0")
B, N_TRAJ, BATCHES, REPS = 64, 64, 4, 3
NORM = {"x_mean": torch.zeros(1, 6, 1), "x_std": torch.ones(1, 6, 1), "y_mean": torch.zeros(1, 5, 1),
        "y_std": torch.ones(1, 5, 1)}


def setup(Tc):
    torch.manual_seed(0)
    sysm = K.VehicleModel(0.01, Tc, Tc, torch.zeros(6, 1))
    sysm.Params.update(bench.KNET_LIMITS)
    model = K.KalmanNetNN(dev)
    model.NNBuild(sysm, in_mult_KNet=5, out_mult_KNet=40, hidden_dim_gru=128)
    model.set_normalization(NORM["x_mean"], NORM["x_std"], NORM["y_mean"], NORM["y_std"])
    model.train()
    return model, torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)


def data(Tc):
    torch.manual_seed(1)
    T = BATCHES * Tc * B // N_TRAJ
    x = 0.5 * torch.randn((N_TRAJ, 6, T), device=dev)
    y = x[:, [0, 1, 3, 4, 5], :] + 0.05 * torch.randn((N_TRAJ, 5, T), device=dev)
    return y, 0.2 * torch.randn((N_TRAJ, 2, T), device=dev), x


def epoch_b(model, opt, y, u, x, p, perm, noise):
    """Variant (b): what the fused pipelines did before the update moved into the graph, batch by batch."""
    Tc = p["T_train"]
    xm, xs, ym, ys = (NORM[k].to(dev) for k in ("x_mean", "x_std", "y_mean", "y_std"))
    chunks = [PC.create_chunks(t, Tc) for t in (y, u, x)]
    R = KF.runner_for(model, B, Tc)
    losses = []
    for i in range(0, perm.shape[0], B):
        pick = perm[i:i + B].to(dev)
        y_b, u_b, x_b = (c[pick] for c in chunks)
        y_norm, x_norm = (y_b - ym) / ys, (x_b - xm) / xs
        R.reset(x_norm[:, :, 0] + noise[i:i + B].to(dev) * PC.INIT_NOISE_STD)
        loss = R.run_chunk(y_norm, u_b, x_norm, composite=True, alpha=p["alpha"])
        R.add_grads()
        clip_grad_norm_(model.parameters(), max_norm=PC.CLIP_NORM)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.item()))
    return losses


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(Tc):
    y, u, x = data(Tc)
    p = dict(N_batch=B, T_train=Tc, m=6, n=5, device=dev, CompositionLoss=True, alpha=0.8)
    ma, mb, mc = setup(Tc), setup(Tc), setup(Tc)
    run = {"a": lambda pm, nz: PC.chunked_batches(*ma, y, u, x, NORM, dict(p, fused=False), perm=pm, noise=nz),
           "b": lambda pm, nz: epoch_b(*mb, y, u, x, p, pm, nz),
           "c": lambda pm, nz: PC.chunked_batches(*mc, y, u, x, NORM, dict(p, fused=True), perm=pm, noise=nz)}
    gen = torch.Generator().manual_seed(2)

    def draw():   # an epoch's shuffle and start noise, the same for the three variants (their dropout masks differ)
        return torch.randperm(BATCHES * B, generator=gen), torch.randn(BATCHES * B, 6, generator=gen)

    e0 = draw()
    warm = {k: timed(lambda: run[k](*e0))[0] for k in "abc"}   # warm-up epochs: GEMM heuristics, allocator, captures
    dt, losses = {k: [] for k in "abc"}, {k: [] for k in "abc"}
    for _ in range(REPS):
        e = draw()
        for k in "abc":   # alternately, in one process
            d, out = timed(lambda: run[k](*e))
            dt[k].append(d)
            losses[k].append(sum(out) / len(out))
    ms = {k: 1e3 * min(v) / BATCHES for k, v in dt.items()}
    every = {k: [1e3 * d / BATCHES for d in v] for k, v in dt.items()}
    spread_b = max(every["b"]) - min(every["b"])
    st, rb = PC.fused_state(mc[0]), KF.runner_for(mb[0], B, Tc)
    return {"metric": f"KalmanNet chunk-and-shuffle training, ms per optimizer update, T_train = {Tc}",
            "ms_per_update": {"module": ms["a"], "fused_chunk_torch_update": ms["b"], "update_in_graph": ms["c"]},
            "ms_per_update_all": {"module": every["a"], "fused_chunk_torch_update": every["b"],
                                  "update_in_graph": every["c"]},
            "module_over_in_graph": ms["a"] / ms["c"], "torch_update_over_in_graph": ms["b"] / ms["c"],
            "in_graph_minus_torch_update_ms": ms["c"] - ms["b"], "torch_update_spread_ms": spread_b,
            "in_graph_not_slower_than_torch_update": ms["c"] <= ms["b"] + spread_b,
            "in_graph_faster_than_torch_update_beyond_spread": ms["c"] < ms["b"] - spread_b,
            "first_epoch_s": warm, "graph_instantiate_s": {"fused_chunk_torch_update": rb.graph_instantiate_s,
                                                           "update_in_graph": st.batch[B].R.graph_instantiate_s},
            "graphs": {"fused_chunk_torch_update": len(rb.graphs), "update_in_graph": st.graphs},
            "tape_bytes": {"fused_chunk_torch_update": rb.tape_bytes, "update_in_graph": st.tape_bytes},
            "config": dict(T_train=Tc, batch=B, batches_per_epoch=BATCHES, trajectories=N_TRAJ, in_mult=5, out_mult=40,
                           hidden=128, optimizer="AdamW(lr 1e-4, wd 1e-5)", loss="composite, alpha 0.8", mode="train",
                           reps=REPS, statistic="min of reps"),
            "epoch_mean_losses": losses}


if __name__ == "__main__":
    res = []
    for Tc in (200, 25):
        res.append(measure(Tc))
        print(json.dumps(res[-1]), flush=True)
        gc.collect()   # the runners and their models refer to each other
        torch.cuda.empty_cache()
    with open(os.path.join(ROOT, "profiles", "knet_chunked_bench.json"), "w") as f:
        for r in res:
            f.write(json.dumps(r) + "\n")

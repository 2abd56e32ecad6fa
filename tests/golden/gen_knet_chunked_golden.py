"""Generate tests/golden/knet_chunked.npz (KalmanNet training by independent chunks) from the REFERENCE's own code.

Run in the build container only (reads /root/reference):  python tests/golden/gen_knet_chunked_golden.py

Imported read-only from /root/reference/KalmanNet: kalman_net.KalmanNetNN, vehicle_model.VehicleModel,
pipeline_indipendent_chunking.train_epoch_chunked and training_indipendent_chunking.create_chunks (a stub `wandb`
module stands in for the logging import, and `pipeline_chunk_shuffle`, the module the entry script asks for and the
reference does not have, is aliased to its pipeline_indipendent_chunking).  The weights are tests/_knet_weights.py's
seeded set (seed 0, in_mult 5), the data the B=4 x T=20 sequences of tests/golden/knet.npz in real units
(y = y_norm y_std + y_mean), T_train = 5 (16 chunks), N_batch = 6 (batches of 6, 6 and 4), AdamW(1e-4, 1e-5),
composite loss with alpha 0.8.  train_epoch_chunked forces train mode, so every nn.Dropout.p is set to 0: the run is
deterministic.  torch.manual_seed(0), two epochs.  Recorded:
  * create_chunks of a [3,5,20] ramp at chunk sizes 5 and 6 (6 drops a tail of 2);
  * per epoch the permutation (torch.randperm) and the start noise (the torch.randn_like draws of the batches,
    concatenated in the epoch's order), taken from the calls train_epoch_chunked itself makes;
  * the two epoch losses;
  * for three parameters, per epoch: the first 8 entries and the norm of p_after - p_before.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests._knet_weights import LIMITS, knet_weights  # noqa: E402

REF = "/root/reference/KalmanNet"
T_TRAIN, N_BATCH, EPOCHS = 5, 6, 2
DELTA_NAMES = ["FC2.0.weight", "GRU_Q.weight_hh_l0", "FC7.0.bias"]


def main():
    sys.modules["wandb"] = types.ModuleType("wandb")
    sys.path.insert(0, REF)
    import kalman_net as KN
    import pipeline_indipendent_chunking as PC
    import vehicle_model as VM
    sys.modules["pipeline_chunk_shuffle"] = PC
    import training_indipendent_chunking as TC
    torch.set_num_threads(4)
    g = dict(np.load(os.path.join(HERE, "knet.npz")))
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731

    ramp = torch.arange(3 * 5 * 20, dtype=torch.float32).reshape(3, 5, 20)
    ramp5, ramp6 = TC.create_chunks(ramp, 5), TC.create_chunks(ramp, 6)

    params = dict(VM.Params)
    params.update(LIMITS)
    sysm = VM.VehicleModel(float(g["Ts"]), 20, 20, torch.zeros(6, 1), None, None, None)
    sysm.Params = params
    model = KN.KalmanNetNN()
    model.NNBuild(sysm, in_mult_KNet=5, out_mult_KNet=40, hidden_dim_gru=128)
    stats = {k: f32(g[k]) for k in ("x_mean", "x_std", "y_mean", "y_std")}
    model.set_normalization(stats["x_mean"], stats["x_std"], stats["y_mean"], stats["y_std"])
    model.load_state_dict({k: torch.tensor(v) for k, v in knet_weights(seed=0).items()})
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    y = f32(g["y_norm"]) * stats["y_std"] + stats["y_mean"]
    u, x = f32(g["u"]), f32(g["x_true"])
    chunks = [TC.create_chunks(t, T_TRAIN) for t in (y, u, x)]
    assert chunks[0].shape == (16, 5, T_TRAIN)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    tp = {"N_batch": N_BATCH, "T_train": T_TRAIN, "m": 6, "n": 5, "device": "cpu", "CompositionLoss": True,
          "alpha": 0.8}

    # record what train_epoch_chunked draws
    drawn = {"perm": [], "noise": []}
    randperm, randn_like = torch.randperm, torch.randn_like

    def rec_perm(*a, **k):
        out = randperm(*a, **k)
        drawn["perm"].append(out.clone())
        return out

    def rec_noise(*a, **k):
        out = randn_like(*a, **k)
        drawn["noise"].append(out.clone())
        return out

    torch.randperm, torch.randn_like = rec_perm, rec_noise
    torch.manual_seed(0)
    named = dict(model.named_parameters())
    losses, perms, noises, heads, norms = [], [], [], [], []
    try:
        for _ in range(EPOCHS):
            drawn["perm"], drawn["noise"] = [], []
            before = {k: named[k].detach().clone() for k in DELTA_NAMES}
            avg, _ = PC.train_epoch_chunked(model, opt, *chunks, stats, tp)
            assert len(drawn["perm"]) == 1 and [n.shape[0] for n in drawn["noise"]] == [6, 6, 4]
            losses.append(avg)
            perms.append(drawn["perm"][0].numpy())
            noises.append(torch.cat(drawn["noise"], 0).numpy())
            d = [named[k].detach() - before[k] for k in DELTA_NAMES]
            heads.append(np.stack([np.pad(t.reshape(-1)[:8].numpy(), (0, max(0, 8 - t.numel()))) for t in d]))
            norms.append(np.array([float(t.norm()) for t in d]))
    finally:
        torch.randperm, torch.randn_like = randperm, randn_like
    np.savez_compressed(
        os.path.join(HERE, "knet_chunked.npz"), ramp_chunks5=ramp5.numpy(), ramp_chunks6=ramp6.numpy(),
        perm=np.stack(perms).astype(np.int64), noise=np.stack(noises).astype(np.float32),
        epoch_loss=np.array(losses, dtype=np.float64), delta_names=np.array(DELTA_NAMES),
        delta_head=np.stack(heads).astype(np.float32), delta_norm=np.stack(norms).astype(np.float64),
        T_train=T_TRAIN, N_batch=N_BATCH)
    print("wrote knet_chunked.npz", losses, [p.tolist() for p in perms], norms)


if __name__ == "__main__":
    main()

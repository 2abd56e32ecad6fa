"""Generate tests/golden/knet_pred.npz (KalmanNet training with the open-loop prediction loss)
from the REFERENCE's own code.

Run in the build container only (reads /root/reference):  python tests/golden/gen_knet_pred_golden.py

Imported read-only from /root/reference/KalmanNet: kalman_net.KalmanNetNN, vehicle_model.VehicleModel and
pipeline_prediction.py's _compute_step_loss_real, compute_prediction_loss and loss_x_with_angular (a stub `wandb`
module stands in for the logging import).  The weights are tests/_knet_weights.py's seeded set, the data the
B=4 x T=20 sequences of tests/golden/knet.npz (its x_post are the posteriors the windows start from), eval mode
(dropout off) so the run is deterministic.  Recorded:
  * _compute_step_loss_real on seeded tensors whose phi difference spans more than 2 pi;
  * compute_prediction_loss and its autograd gradient w.r.t. x_est at every t < T for H in {1, 5, 8} (truncated
    windows t + H > T - 1 and the zero-step window t = T - 1 included), with real controls and with normalized
    controls (the u statistics of tests/golden/knet_b9_t12_unorm.npz);
  * one train_epoch-style run written out like gen_knet_train_golden.py's run_chunks (pipeline_prediction.py:125-206
    with the batch, initial posterior and normalization of knet.npz): K=10, lambda_pred 0.5, H 5, AdamW(lr 1e-4,
    wd 1e-5), clipping at 1.0 -- the filter and prediction losses per chunk and, of the first chunk's gradient, the
    L2 norm and first 8 entries per parameter.
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
HORIZONS = (1, 5, 8)
f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731


def build(KN, sysm, g, u_stats=None):
    model = KN.KalmanNetNN()
    model.NNBuild(sysm, in_mult_KNet=5, out_mult_KNet=40, hidden_dim_gru=128)
    model.set_normalization(f32(g["x_mean"]), f32(g["x_std"]), f32(g["y_mean"]), f32(g["y_std"]),
                            *([] if u_stats is None else [f32(s) for s in u_stats]))
    model.load_state_dict({k: torch.tensor(v) for k, v in knet_weights(seed=0).items()})
    model.eval()
    return model


def window_table(PP, model, x_est, u, x_norm):
    """compute_prediction_loss and d loss / d x_est for every (H, t): losses [nH, T], gradients [nH, B, 6, T]."""
    B, _, T = x_est.shape
    loss = np.zeros((len(HORIZONS), T), np.float32)
    grad = np.zeros((len(HORIZONS), B, 6, T), np.float32)
    for i, H in enumerate(HORIZONS):
        for t in range(T):
            x = x_est[:, :, t:t + 1].clone().requires_grad_(True)
            v = PP.compute_prediction_loss(model, x, t, u, x_norm, H)
            loss[i, t] = float(v.detach())
            if v.requires_grad:
                grad[i, :, :, t] = torch.autograd.grad(v, x)[0].squeeze(2).numpy()
    return loss, grad


def run_chunks(PP, model, g, K=10, lambda_pred=0.5, H=5):
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    x_mean, x_std = f32(g["x_mean"]), f32(g["x_std"])
    y_norm, u = f32(g["y_norm"]), f32(g["u"])
    x_norm = (f32(g["x_true"]) - x_mean) / x_std
    B, T = y_norm.shape[0], y_norm.shape[2]
    model.batch_size = B
    model.init_hidden_KNet()
    model.InitSequence(f32(g["m1x0"]), T)
    opt.zero_grad()
    outs, xt, pl, lf, lp, grads = [], [], [], [], [], None
    for t in range(T):
        x_out = model(y_norm[:, :, t].unsqueeze(2), u[:, :, t].unsqueeze(2))
        outs.append(x_out.squeeze(2))
        xt.append(x_norm[:, :, t])
        pl.append(PP.compute_prediction_loss(model, x_out, t, u, x_norm, H))
        if (t + 1) % K == 0 or t + 1 == T:
            loss_f = PP.loss_x_with_angular(torch.stack(outs, 2), torch.stack(xt, 2), x_mean, x_std, 6, PP.PHI_IDX)
            loss_p = torch.stack(pl).mean()
            (loss_f + lambda_pred * loss_p).backward()
            if grads is None:
                grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
            opt.zero_grad()
            lf.append(float(loss_f.item()))
            lp.append(float(loss_p.item()))
            outs, xt, pl = [], [], []
            model.h_Q.detach_()
            model.h_Sigma.detach_()
            model.h_S.detach_()
            model.m1x_posterior = model.m1x_posterior.detach()
            model.m1x_prior = model.m1x_prior.detach()
    return lf, lp, grads


def main():
    sys.modules["wandb"] = types.ModuleType("wandb")
    sys.path.insert(0, REF)
    import matplotlib
    matplotlib.use("Agg")
    import kalman_net as KN
    import pipeline_prediction as PP
    import vehicle_model as VM
    torch.set_num_threads(4)
    g = dict(np.load(os.path.join(HERE, "knet.npz")))
    gu = np.load(os.path.join(HERE, "knet_b9_t12_unorm.npz"))
    params = dict(VM.Params)
    params.update(LIMITS)
    sysm = VM.VehicleModel(float(g["Ts"]), 20, 20, torch.zeros(6, 1), None, None, None)
    sysm.Params = params

    # the step loss on seeded tensors: phi differences up to +- 10 rad
    rng = np.random.default_rng(17)
    sl_x = rng.normal(size=(5, 6, 1)).astype(np.float32)
    sl_g = rng.normal(size=(5, 6, 1)).astype(np.float32)
    sl_x[:, 2, 0] = rng.uniform(-5, 5, 5)
    sl_g[:, 2, 0] = rng.uniform(-5, 5, 5)
    assert np.abs(sl_x[:, 2] - sl_g[:, 2]).max() > np.pi
    step_loss = float(PP._compute_step_loss_real(torch.tensor(sl_x), torch.tensor(sl_g)))

    x_mean, x_std = f32(g["x_mean"]), f32(g["x_std"])
    x_est, u = f32(g["x_post"]), f32(g["u"])
    x_norm = (f32(g["x_true"]) - x_mean) / x_std
    loss, grad = window_table(PP, build(KN, sysm, g), x_est, u, x_norm)
    u_mean, u_std = f32(gu["u_mean"]), f32(gu["u_std"])
    u_norm = (u - u_mean) / u_std
    loss_un, grad_un = window_table(PP, build(KN, sysm, g, (gu["u_mean"], gu["u_std"])), x_est, u_norm, x_norm)

    lf, lp, grads = run_chunks(PP, build(KN, sysm, g), g)
    names = sorted(grads)
    np.savez_compressed(
        os.path.join(HERE, "knet_pred.npz"),
        step_in_x=sl_x, step_in_gt=sl_g, step_loss=step_loss,
        horizons=np.array(HORIZONS), x_est=x_est.numpy(), x_norm=x_norm.numpy(), loss=loss, grad=grad,
        u_mean=u_mean.numpy(), u_std=u_std.numpy(), u_norm=u_norm.numpy(), loss_unorm=loss_un, grad_unorm=grad_un,
        grad_names=np.array(names), grad_norm=np.array([float(grads[k].norm()) for k in names]),
        grad_head=np.stack([np.pad(grads[k].reshape(-1)[:8].numpy(), (0, max(0, 8 - grads[k].numel())))
                            for k in names]),
        losses_filter=np.array(lf), losses_pred=np.array(lp))
    print("wrote knet_pred.npz", lf, lp, loss[:, :3], step_loss)


if __name__ == "__main__":
    main()

"""KalmanNet training with the open-loop prediction loss on MI355X: the import swap for
KalmanNet/pipeline_prediction.py (same names and call signatures: the loss functions, ``compute_prediction_loss``,
``train_epoch``, ``validate_epoch``, ``Pipeline_Vehicle_KNet``).

The reference adds to the filter loss ``lambda_pred`` x the error of an H-step physics rollout started from every
posterior, differentiated through the rollout, as H x some dozens of small torch ops per time step.  Here the
rollouts of a whole TBPTT chunk -- every (sequence, step) pair an independent window -- are one launch of
``traj_knet_pred_loss_f32`` (include/trajknet.h), which returns each window's loss and its gradient w.r.t. the
window's posterior (the exact derivative of the clamped Euler step, carried forward with the rollout); autograd
continues from there into the filter steps (``knet.KalmanNetNN`` under autograd, as ``knet_train.py``).

``compute_prediction_loss_stepwise`` evaluates the same loss one ``model.f`` call per step (differentiable: the HIP
prior kernel under ``knet._KnetPriorFn``), as the reference does: the on-device cross-check of the fused launch and
what it is timed against.  Logging is a plain per-epoch callback; W&B and plotting are out of scope (DESIGN.md
section 9).
"""
from __future__ import annotations

import os
import random

import torch
from torch.autograd.function import once_differentiable
from torch.nn.utils import clip_grad_norm_

from .knet import KNetSequenceRunner, knet_pred_loss
from .knet_train import EPS_DB, PHI_IDX, _angular_mse_from_real, loss_x_with_angular  # noqa: F401  (re-exported)

INIT_NOISE_STD = 0.2   # spread of the initial posterior around the true first state (training and validation)
VAL_EVERY = 10         # validation scores the prediction loss at every 10th step
VAL_HORIZON = 50       # ... over this horizon unless params carries pred_horizon
CLIP_NORM = 1.0


def _wrap_channel(err, phi_idx):
    """err [B,m,...] with channel phi_idx replaced by its wrapped value atan2(sin, cos)."""
    phi = err[:, phi_idx:phi_idx + 1]
    return torch.cat((err[:, :phi_idx], torch.atan2(torch.sin(phi), torch.cos(phi)), err[:, phi_idx + 1:]), 1)


def _compute_step_loss_real(x_next_real, x_gt_next_real, phi_idx=PHI_IDX):
    """Mean squared error of a predicted state against the ground truth, both [B,m,1] in real units, with the heading
    error taken modulo 2 pi."""
    return (_wrap_channel(x_next_real - x_gt_next_real, phi_idx) ** 2).mean()


class _PredLossFn(torch.autograd.Function):
    """traj_knet_pred_loss_f32: per-window losses [B,nwin] of x_est [B,6,nwin]; backward = grad_out x the kernel's
    gradient."""

    @staticmethod
    def forward(ctx, x_est, model, t0, step, u_full, x_norm_full, horizon):
        want = ctx.needs_input_grad[0]
        xm, xs = model._norm_tensors()[:2]
        part, grad = knet_pred_loss(model.sys.Params, model.sys.Ts, x_est, t0, step, u_full, x_norm_full, horizon,
                                    xm, xs, model.u_mean, model.u_std, want_grad=want)
        if want:
            ctx.save_for_backward(grad)
        return part

    @staticmethod
    @once_differentiable
    def backward(ctx, g_part):
        grad, = ctx.saved_tensors
        return (g_part.unsqueeze(1) * grad,) + (None,) * 6


def _batch_mean(part):
    """Mean over dim 0 by pairwise elementwise adds: a fixed order, so a window's loss has the same bits whether it is
    launched alone or inside a chunk (a library reduction picks its order from the whole shape)."""
    B = part.shape[0]
    while part.shape[0] > 1:
        h = part.shape[0] // 2
        part = torch.cat((part[:h] + part[h:2 * h], part[2 * h:]), 0)
    return part[0] / B


def prediction_loss_windows(model, x_est, t0, step, nwin, u_full, x_norm_full, horizon):
    """compute_prediction_loss for nwin windows in one launch: window w starts at t = t0 + w * step from
    x_est[:, :, w] (normalized posteriors indexed by window: a stacked TBPTT chunk [B,6,K] with t0 = its first step
    and step = 1, or a strided slice of a [B,6,T] estimate tensor).  Returns the per-window losses [nwin] (the
    reference's loss at each t), differentiable w.r.t. x_est."""
    if x_est.dim() != 3 or x_est.shape[2] != nwin:
        raise ValueError("prediction_loss_windows: x_est [B,6,nwin]")
    if horizon < 1:
        return torch.zeros(nwin, device=x_est.device)
    return _batch_mean(_PredLossFn.apply(x_est, model, t0, step, u_full, x_norm_full, horizon))


def _valid_steps(t, horizon, T):
    return max(0, min(horizon, T - 1 - t))


def compute_prediction_loss(model, x_est_norm_t, t, u_train_full, x_train_norm_full, horizon):
    """The open-loop prediction loss at time t: the physics rolled `horizon` steps (fewer at the end of the sequence)
    from the posterior x_est_norm_t [B,m,1] with the logged controls, scored against x_train_norm_full.  One fused
    launch (nwin = 1)."""
    if _valid_steps(t, horizon, x_train_norm_full.shape[2]) == 0:
        return torch.tensor(0.0, device=x_est_norm_t.device)
    B = x_est_norm_t.shape[0]
    return prediction_loss_windows(model, x_est_norm_t.reshape(B, 6, 1), t, 1, 1, u_train_full, x_train_norm_full,
                                   horizon)[0]


def compute_prediction_loss_stepwise(model, x_est_norm_t, t, u_train_full, x_train_norm_full, horizon):
    """The same loss one ``model.f`` launch per step, the step losses in torch ops, autograd through every step (how
    the reference evaluates it).  The cross-check of the fused launch, and what it is timed against."""
    n = _valid_steps(t, horizon, x_train_norm_full.shape[2])
    if n == 0:
        return torch.tensor(0.0, device=x_est_norm_t.device)
    x = model._denorm_x(x_est_norm_t)
    acc = 0.0
    for j in range(t, t + n):   # x(j) -> x(j + 1) with u(j)
        x = model.f(x, model._denorm_u(u_train_full[:, :, j:j + 1]))
        acc = acc + _compute_step_loss_real(x, model._denorm_x(x_train_norm_full[:, :, j + 1:j + 2]), PHI_IDX)
    return acc / n


def tbptt_prediction_sequence(model, optimizer, y_norm, u, x_norm, m1x0, params, x_mean, x_std, stepwise=False,
                              on_chunk=None):
    """One TBPTT pass over a batch already on the device: normalized observations y_norm [B,n,T], controls u [B,2,T],
    normalized targets x_norm [B,m,T], initial posterior m1x0 [B,m,1].  Per chunk of K_TBPTT steps: the filter steps,
    one prediction_loss_windows call on the stacked chunk (stepwise=True: one stepwise loss per step instead),
    loss_filter + lambda_pred * mean, backward, clip at 1.0, optimizer step, detach.  on_chunk(model) runs after each
    backward, before clipping.  Returns (filter losses, prediction losses) per chunk."""
    K, T, m = params["K_TBPTT"], params["T"], params["m"]
    lambda_pred, H = params.get("lambda_pred", 0.0), params.get("pred_horizon", 0)
    use_pred = lambda_pred > 0 and H > 0
    model.batch_size = y_norm.shape[0]
    model.init_hidden_KNet()
    model.InitSequence(m1x0, T)
    optimizer.zero_grad()
    lf, lp = [], []
    for c0 in range(0, T, K):
        c1 = min(c0 + K, T)
        outs, step_losses = [], []
        for t in range(c0, c1):
            outs.append(model(y_norm[:, :, t:t + 1], u[:, :, t:t + 1]).squeeze(2))
            if use_pred and stepwise:
                step_losses.append(compute_prediction_loss_stepwise(model, outs[-1].unsqueeze(2), t, u, x_norm, H))
        xo = torch.stack(outs, dim=2)
        loss_filter = loss_x_with_angular(xo, x_norm[:, :, c0:c1], x_mean, x_std, m, PHI_IDX)
        if not use_pred:
            loss_pred = torch.zeros((), device=xo.device)
        elif stepwise:
            loss_pred = torch.stack(step_losses).mean()
        else:
            loss_pred = prediction_loss_windows(model, xo, c0, 1, c1 - c0, u, x_norm, H).mean()
        (loss_filter + lambda_pred * loss_pred).backward()
        if on_chunk is not None:
            on_chunk(model)
        clip_grad_norm_(model.parameters(), max_norm=CLIP_NORM)
        optimizer.step()
        optimizer.zero_grad()
        lf.append(float(loss_filter.item()))
        lp.append(float(loss_pred.item()))
        for name in ("h_Q", "h_Sigma", "h_S", "m1x_posterior", "m1x_prior"):
            setattr(model, name, getattr(model, name).detach())
    return lf, lp


class _PredExtra:
    """The prediction loss inside a fused chunk (knet_train_fused.FusedTBPTT.run_chunk's ``extra`` hook): one
    knet_pred_loss launch on the tape's posteriors, its gradient x lambda_pred / (B Kc) -- the mean over sequences and
    windows -- written to the loss kernel's g_extra.  The launch's t0 and T are fixed in the captured graph, so it
    reads a window [c0, c0 + Tw) of u / x_norm copied into static buffers (t0 = 0, T = Tw = min(Kc + H, T - c0))."""

    def __init__(self, model, B, Kc, Tw, H, lambda_pred):
        self.model, self.Kc, self.Tw, self.H, self.lam = model, Kc, Tw, H, lambda_pred
        dev = model.device
        self.u = torch.zeros((B, 2, Tw), dtype=torch.float32, device=dev)
        self.x = torch.zeros((B, 6, Tw), dtype=torch.float32, device=dev)
        self.part = None

    def load(self, u, x_norm, c0):
        self.u.copy_(u[:, :, c0:c0 + self.Tw])
        self.x.copy_(x_norm[:, :, c0:c0 + self.Tw])

    def __call__(self, runner, Kc):
        md = self.model
        xm, xs = md._norm_tensors()[:2]
        self.part, grad = knet_pred_loss(md.sys.Params, md.sys.Ts, runner.posteriors(Kc), 0, 1, self.u, self.x, self.H,
                                         xm, xs, md.u_mean, md.u_std)
        torch.mul(grad, self.lam / (grad.shape[0] * Kc), out=runner.g_extra(Kc))


def tbptt_prediction_sequence_fused(model, optimizer, y_norm, u, x_norm, m1x0, params, x_mean, x_std, on_chunk=None):
    """tbptt_prediction_sequence on the fused path (knet_train_fused.FusedTBPTT): the chunk -- filter steps, prediction
    loss, state loss, backward sweep, weight-gradient products -- replayed as one HIP graph; clipping and the optimizer
    as there.  Returns (filter losses, prediction losses) per chunk."""
    from .knet_train_fused import _publish_state, runner_for
    K, T = params["K_TBPTT"], params["T"]
    lambda_pred, H = params.get("lambda_pred", 0.0), params.get("pred_horizon", 0)
    use_pred = lambda_pred > 0 and H > 0
    B = y_norm.shape[0]
    model.batch_size = B
    model.T = T
    R = runner_for(model, B, min(K, T))
    hooks = R.__dict__.setdefault("_pred_hooks", {})
    R.reset(m1x0)
    optimizer.zero_grad()
    lf, lp, Kc = [], [], 0
    for c0 in range(0, T, K):
        c1 = min(c0 + K, T)
        Kc = c1 - c0
        hook, key = None, None
        if use_pred:
            key = (Kc, min(Kc + H, T - c0), H, float(lambda_pred))
            if key not in hooks:
                hooks[key] = _PredExtra(model, B, *key)
            hook = hooks[key]
            hook.load(u, x_norm, c0)
        loss = R.run_chunk(y_norm[:, :, c0:c1], u[:, :, c0:c1], x_norm[:, :, c0:c1], composite=False, extra=hook,
                           extra_key=key)
        R.add_grads()
        if on_chunk is not None:
            on_chunk(model)
        clip_grad_norm_(model.parameters(), max_norm=CLIP_NORM)
        optimizer.step()
        optimizer.zero_grad()
        lf.append(float(loss.item()))
        lp.append(float(_batch_mean(hook.part).mean().item()) if use_pred else 0.0)
        R.carry_over(Kc)
    _publish_state(model, R, Kc)
    return lf, lp


def _noisy_start(x_norm):
    x0 = x_norm[:, :, 0]
    return (x0 + INIT_NOISE_STD * torch.randn_like(x0)).unsqueeze(2)


def train_epoch(model, optimizer, y_train, u_train, x_train, norm_stats, params):
    """One TBPTT pass (train mode) over a random batch of N_batch of the N_E trajectories (y / u / x [N_E, c, T] in
    real units) from a noisy normalized first state.  params: N_E, N_batch, K_TBPTT, T, m, device, lambda_pred,
    pred_horizon (and stepwise=True for the per-step loss path, fused=True for the graph path of knet_train_fused.py).
    Returns (average filter loss, average prediction loss, filter loss in dB)."""
    device = params["device"]
    x_mean, x_std = norm_stats["x_mean"].to(device), norm_stats["x_std"].to(device)
    model.train()
    pick = random.sample(range(params["N_E"]), k=params["N_batch"])
    y_b, u_b, x_b = (t[pick].to(device) for t in (y_train, u_train, x_train))
    y_norm = (y_b - norm_stats["y_mean"].to(device)) / norm_stats["y_std"].to(device)
    x_norm = (x_b - x_mean) / x_std
    if params.get("fused", False):   # opt-in: the autograd-free chunk replayed as a HIP graph
        lf, lp = tbptt_prediction_sequence_fused(model, optimizer, y_norm, u_b, x_norm, _noisy_start(x_norm), params,
                                                 x_mean, x_std)
    else:
        lf, lp = tbptt_prediction_sequence(model, optimizer, y_norm, u_b, x_norm, _noisy_start(x_norm), params, x_mean,
                                           x_std, stepwise=params.get("stepwise", False))
    avg_filter = sum(lf) / max(1, len(lf))
    avg_pred = sum(lp) / max(1, len(lp)) if params.get("lambda_pred", 0.0) > 0 else 0.0
    return avg_filter, avg_pred, 10 * torch.log10(torch.tensor(avg_filter).clamp_min(EPS_DB))


def validation_windows(T, horizon, every=VAL_EVERY):
    """How many window starts validate_epoch scores: t % every == 0 with t + horizon < T."""
    return len(range(0, max(0, T - horizon), every)) if horizon > 0 else 0


def validate_epoch(model, y_val_norm, u_val, x_val_norm, norm_stats, params, runner=None):
    """The filter over the whole validation set (the fused sequence runner: eval mode, no gradient) from a noisy
    first state, its state loss, and the prediction loss of every 10th step with t + H < T in one launch.
    params: N_CV, T, m (and pred_horizon, default 50).  Returns (state loss, its dB value, mean prediction loss)."""
    N_CV, T, m = params["N_CV"], params["T"], params["m"]
    H = params.get("pred_horizon", VAL_HORIZON)
    dev = y_val_norm.device
    x_mean, x_std = norm_stats["x_mean"].to(dev), norm_stats["x_std"].to(dev)
    model.eval()
    with torch.no_grad():
        if runner is None or runner.B != N_CV:
            runner = KNetSequenceRunner(model, N_CV)
        y, u, xg = (a[:, :, :T].float().contiguous() for a in (y_val_norm, u_val, x_val_norm))
        x_out = runner.run(y, u, _noisy_start(xg), fused=True)
        val = loss_x_with_angular(x_out, xg, x_mean, x_std, m, PHI_IDX).item()
        avg_pred = 0.0
        nwin = validation_windows(T, H)
        if nwin > 0:
            starts = x_out[:, :, ::VAL_EVERY][:, :, :nwin]   # a strided view: no gather
            avg_pred = prediction_loss_windows(model, starts, 0, VAL_EVERY, nwin, u, xg, H).mean().item()
    return val, 10 * torch.log10(torch.tensor(val).clamp_min(EPS_DB)), avg_pred


class Pipeline_Vehicle_KNet:
    """The reference's training driver by name and method signatures (set_models / set_data / set_training_params /
    train / test), AdamW + ReduceLROnPlateau, the best validation state_dict saved under folderName.  ``log`` (a
    callable taking a dict) is called once per epoch and once after the test with the figures the reference sends
    to its experiment tracker."""

    def __init__(self, folderName, modelName, log=None):
        self.folderName, self.modelName, self.log = folderName, modelName, log
        self.best_model_path = os.path.join(folderName, f"best_model_{modelName}.pt")
        os.makedirs(folderName, exist_ok=True)

    def set_models(self, sys_model, model):
        self.sys_model, self.model = sys_model, model

    def set_data(self, train_data, val_data, test_data, norm_stats, device):
        """Each data set is a (y, u, x) triple of [N, c, T] tensors in real units."""
        (self.y_train, self.u_train, self.x_train), (self.y_val, self.u_val, self.x_val) = train_data, val_data
        self.y_test, self.u_test, self.x_test = test_data
        self.norm_stats, self.device = norm_stats, device
        self.N_E, self.N_CV, self.N_T = len(self.y_train), len(self.y_val), len(self.y_test)

    def set_training_params(self, n_steps, n_batch, lr, wd, K_TBPTT, T, lambda_pred=0.0, pred_horizon=0, fused=False):
        """fused=True: train on the autograd-free graph path (knet_train_fused.py)."""
        self.N_steps, self.N_batch, self.lr, self.wd, self.fused = n_steps, n_batch, lr, wd, fused
        self.K_TBPTT, self.T = K_TBPTT, T
        self.m, self.n = self.sys_model.m, self.sys_model.n
        self.lambda_pred, self.pred_horizon = lambda_pred, pred_horizon
        self.optimizer = torch.optim.AdamW(self.model.parameters(), lr=lr, weight_decay=wd)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode="min", factor=0.5,
                                                                    patience=10, min_lr=1e-7)
        self.train_loss_history_db, self.val_loss_history_db = [], []

    def _normalized(self, y, u, x):
        ns, dev = self.norm_stats, self.device
        y, u, x = y.to(dev), u.to(dev), x.to(dev)
        return (y - ns["y_mean"].to(dev)) / ns["y_std"].to(dev), u, (x - ns["x_mean"].to(dev)) / ns["x_std"].to(dev)

    def _eval_params(self, N):
        return {"N_CV": N, "T": self.T, "m": self.m, "n": self.n, "device": self.device}

    def train(self):
        best = float("inf")
        val_set = self._normalized(self.y_val, self.u_val, self.x_val)
        train_params = dict(self._eval_params(self.N_CV), N_E=self.N_E, N_batch=self.N_batch, K_TBPTT=self.K_TBPTT,
                            lambda_pred=self.lambda_pred, pred_horizon=self.pred_horizon, fused=self.fused)
        for epoch in range(self.N_steps):
            avg_filt, avg_pred, train_db = train_epoch(self.model, self.optimizer, self.y_train, self.u_train,
                                                       self.x_train, self.norm_stats, train_params)
            val_lin, val_db, val_pred = validate_epoch(self.model, *val_set, self.norm_stats,
                                                       self._eval_params(self.N_CV))
            self.train_loss_history_db.append(train_db)
            self.val_loss_history_db.append(val_db)
            self.scheduler.step(val_lin)
            if self.log is not None:
                self.log({"epoch": epoch, "lr": self.optimizer.param_groups[0]["lr"], "train_loss_filter": avg_filt,
                          "train_loss_pred": avg_pred, "train_loss_dB": float(train_db), "val_loss_linear": val_lin,
                          "val_loss_dB": float(val_db), "val_pred_loss": val_pred})
            if val_lin < best:
                best = val_lin
                torch.save(self.model.state_dict(), self.best_model_path)

    def test(self):
        """Scores the test set with the best saved state_dict: (state loss, its dB value, prediction loss); None when
        no model was saved."""
        if not os.path.exists(self.best_model_path):
            return None
        self.model.load_state_dict(torch.load(self.best_model_path, map_location=self.device))
        self.model.to(self.device)
        lin, db, pred = validate_epoch(self.model, *self._normalized(self.y_test, self.u_test, self.x_test),
                                       self.norm_stats, self._eval_params(self.N_T))
        if self.log is not None:
            self.log({"test_loss_linear": lin, "test_loss_dB": float(db), "test_pred_loss": pred})
        return lin, db, pred

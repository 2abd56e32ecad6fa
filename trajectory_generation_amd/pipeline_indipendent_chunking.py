"""KalmanNet training by independent chunks on MI355X: the import swap for KalmanNet/pipeline_indipendent_chunking.py
(same spelling, names and call signatures: the loss functions, ``train_epoch_chunked``, ``validate_epoch``,
``Pipeline_Vehicle_KNet``) and for ``create_chunks`` of training_indipendent_chunking.py.  ``pipeline_chunk_shuffle``,
the module name the reference's entry script imports, re-exports this one.

The strategy: every trajectory is cut into ``T_train``-step chunks, all chunks are shuffled each epoch and batched,
every batch starts from a noisy ground-truth state with zero hidden states and ends in one clipped AdamW step.  No
state is carried between batches, so nothing between two updates needs the host.

``chunked_batches`` has two paths (``params["fused"]``, default False):

* the module path: ``knet.KalmanNetNN`` under autograd, torch's ``clip_grad_norm_`` and AdamW -- the comparison;
* the fused path: one update is one replay of a HIP graph that holds the batch gather (``traj_knet_chunk_gather_f32``:
  chunk ids -> normalised tape inputs and the noisy start), the zeroing of the hidden states, the K forward steps,
  the loss, the K backward steps, the weight gradients (``knet_train_fused.FusedTBPTT``) and clipping + AdamW
  (``traj_knet_clip_adamw_f32``, reading the runner's gradient buffers: no ``.grad``).  Per batch the host copies the
  batch's ids and noise rows into the graph's static buffers (device to device), draws the dropout masks in train
  mode, replays, and copies the loss into a device vector; the losses are read once after the last batch.  The
  kernel updates the torch optimizer's own state (``exp_avg``, ``exp_avg_sq``) in place and ``state[p]["step"]`` is
  advanced after the epoch, so ``state_dict()``, a scheduler and a later ``optimizer.step()`` see what torch's AdamW
  would have left.

Logging is a plain per-epoch callback; W&B and plotting are out of scope.
"""
from __future__ import annotations

import os

import torch
from torch.nn.utils import clip_grad_norm_

from .knet import KNetSequenceRunner
from .knet_train import (EPS_DB, PHI_IDX, _angular_mse_from_real, compute_composite_loss,  # noqa: F401  (re-exported)
                         loss_x_with_angular)

INIT_NOISE_STD = 0.3   # spread of a training batch's initial posterior around the chunk's true first state
VAL_NOISE_STD = 0.2    # ... of validation's around the trajectory's
CLIP_NORM = 5.0


def create_chunks(data_tensor, chunk_size):
    """[N_traj, features, T_full] -> [N_traj * (T_full // chunk_size), features, chunk_size]: chunk c is trajectory
    c // cpt, steps [(c % cpt) chunk_size, + chunk_size); the tail T_full % chunk_size is dropped."""
    n_traj, n_feats, T_full = data_tensor.shape
    cpt = T_full // chunk_size
    view = data_tensor[:, :, :cpt * chunk_size].reshape(n_traj, n_feats, cpt, chunk_size)
    return view.permute(0, 2, 1, 3).reshape(-1, n_feats, chunk_size)


def _stats(norm_stats, dev):
    return tuple(norm_stats[k].to(dev) for k in ("x_mean", "x_std", "y_mean", "y_std"))


# ---------------------------------------------------------------------- the fused path

class _BatchGraph:
    """What one batch size needs: its FusedTBPTT, the static id / noise buffers the gather reads, and the two hooks."""

    def __init__(self, owner, B):
        from .knet_train_fused import ClipAdamW, FusedTBPTT
        self.owner, self.B = owner, B
        R = self.R = FusedTBPTT(owner.model, B, owner.Tc)
        dev = R.dev
        self.ids = torch.zeros(B, dtype=torch.int32, device=dev)
        self.noise = torch.zeros((B, 6), dtype=torch.float32, device=dev)
        p, m, v = owner.p, owner.m, owner.v
        self.opt = ClipAdamW(p, [R.grads[k] for k in owner.names], m, v, owner.lr, owner.hyper[:2], owner.hyper[2],
                             owner.hyper[3], CLIP_NORM, owner.t)

    def pre(self, R, Kc):
        from .knet_train_fused import chunk_gather
        o, T, B = self.owner, R.T, R.B
        yt = R.yt[:B * 5 * Kc].view(B, 5, Kc) if o.composite else None
        chunk_gather(o.y, o.u, o.x, self.ids, Kc, *o.stats, noise=self.noise, noise_std=INIT_NOISE_STD,
                     out=(T["Y"][:Kc], T["U"][:Kc], R.xt[:B * 6 * Kc].view(B, 6, Kc), yt, T["P"][0]))
        for k in ("HQ", "HSig", "HS"):
            T[k][0].zero_()

    def post(self, R, Kc):
        self.opt.step()


class _FusedChunked:
    """The fused path's state for one (model, optimizer, data shape, chunk length, mode): device-resident data, one
    _BatchGraph per batch size, the shared learning-rate scalar and step counter.  It is rebuilt (``matches``) when any
    of these changes, a parameter's or a moment's storage included: the kernels' tables hold their addresses."""

    def __init__(self, model, optimizer, shapes, Tc, composite):
        self.model, self.optimizer, self.shapes, self.Tc, self.composite = model, optimizer, shapes, Tc, composite
        self.train = bool(model.training)
        dev = self.dev = model.device
        group = _adamw_group(optimizer)
        self.hyper = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                      float(group["weight_decay"]))
        by_id = {id(p): k for k, p in model.named_parameters()}
        self.p = list(group["params"])
        self.pptrs = tuple(p.data_ptr() for p in self.p)   # what the kernels' device tables hold
        if any(id(p) not in by_id for p in self.p):
            raise ValueError("chunked_batches: the optimizer holds a tensor that is not a parameter of the model")
        self.names = [by_id[id(p)] for p in self.p]
        for p in self.p:   # the state torch.optim.AdamW creates on its first step
            st = optimizer.state[p]
            if len(st) == 0:
                on_dev = group.get("capturable", False) or group.get("fused", False)
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if on_dev else \
                    torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self.m = [optimizer.state[p]["exp_avg"] for p in self.p]
        self.v = [optimizer.state[p]["exp_avg_sq"] for p in self.p]
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.y, self.u, self.x = (torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes)
        self.stats = tuple(torch.zeros(n, dtype=torch.float32, device=dev) for n in (6, 6, 5, 5))
        self.batch = {}
        # the optimizer kernels' first launch happens here, not inside a capture (post is left out of the warm-up runs)
        from .knet_train_fused import ClipAdamW
        d = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(4)]
        ClipAdamW(d[:1], d[1:2], d[2:3], d[3:], 0.0).step()

    def matches(self, model, optimizer, shapes, Tc, composite):
        group = optimizer.param_groups[0]
        return (self.model is model and self.optimizer is optimizer and self.shapes == shapes and self.Tc == Tc
                and self.composite == composite and self.train == bool(model.training)
                and self.hyper == (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                   float(group["weight_decay"]))
                and self.pptrs == tuple(p.data_ptr() for p in self.p)
                and all(optimizer.state[p].get("exp_avg") is m and optimizer.state[p].get("exp_avg_sq") is v
                        for p, m, v in zip(self.p, self.m, self.v)))

    @property
    def graphs(self):
        return sum(len(b.R.graphs) for b in self.batch.values())

    @property
    def tape_bytes(self):
        return sum(b.R.tape_bytes for b in self.batch.values())

    def run(self, y, u, x, norm_stats, perm, noise, N_batch, alpha):
        dev = self.dev
        for dst, src in zip((self.y, self.u, self.x), (y, u, x)):
            dst.copy_(src)
        for dst, src in zip(self.stats, _stats(norm_stats, dev)):
            dst.copy_(src.reshape(-1))
        # the gather normalises with norm_stats, the filter steps and the loss with the model's own statistics
        if any(not torch.equal(a, b.reshape(-1).float()) for a, b in zip(self.stats, self.model._norm_tensors())):
            raise ValueError("chunked_batches: norm_stats differ from the model's normalization")
        group = self.optimizer.param_groups[0]
        steps = {float(self.optimizer.state[p]["step"]) for p in self.p}
        if len(steps) != 1:
            raise ValueError("chunked_batches: the optimizer's parameters are at different step counts")
        self.lr.fill_(float(group["lr"]))
        self.t.fill_(int(steps.pop()))
        ids = perm.to(dev, torch.int32)
        nz = noise.to(dev, torch.float32)
        n = ids.shape[0]
        losses = torch.zeros((n + N_batch - 1) // N_batch, dtype=torch.float32, device=dev)
        for j, i in enumerate(range(0, n, N_batch)):
            B = min(N_batch, n - i)
            if B not in self.batch:
                self.batch[B] = _BatchGraph(self, B)
            bg = self.batch[B]
            bg.ids.copy_(ids[i:i + B])
            bg.noise.copy_(nz[i:i + B])
            loss = bg.R.run_chunk(None, None, None, composite=self.composite, alpha=alpha, pre=bg.pre, post=bg.post,
                                  Kc=self.Tc)
            losses[j:j + 1].copy_(loss)
        out = losses.tolist()   # the epoch's one read-back
        for p in self.p:
            self.optimizer.state[p]["step"] += len(out)
        return out


def _adamw_group(optimizer):
    if not isinstance(optimizer, torch.optim.AdamW) or len(optimizer.param_groups) != 1:
        raise NotImplementedError("chunked_batches (fused): one parameter group of torch.optim.AdamW")
    group = optimizer.param_groups[0]
    if group.get("amsgrad", False) or group.get("maximize", False):
        raise NotImplementedError("chunked_batches (fused): AdamW with amsgrad=False and maximize=False")
    return group


def fused_state(model):
    """The fused path's state of the model's last ``chunked_batches`` call (None before the first): ``graphs`` (how
    many HIP graphs it holds), ``tape_bytes``, ``batch`` (batch size -> runner and buffers)."""
    return model.__dict__.get("_chunked_fused")


# ---------------------------------------------------------------------- the epoch

def chunked_batches(model, optimizer, y, u, x, norm_stats, params, perm=None, noise=None):
    """The body of train_epoch_chunked in the model's current mode: y / u / x are the full trajectories
    [N_traj, c, T_full] in real units (already chunked tensors [N_chunks, c, T_train] are the case T_full == T_train).
    Chunk ids are those of create_chunks; ``perm`` [n] lists the chunks to visit in order (default: torch.randperm of
    all N_chunks, an epoch), ``noise`` [n, 6] the start noise in that order, row j for the j-th chunk visited
    (default: standard normal draws); batch i takes entries [i N_batch, (i + 1) N_batch) of both.  params: N_batch,
    T_train, m, n, CompositionLoss, alpha (and fused).  Returns the per-batch losses."""
    Tc, N_batch = int(params["T_train"]), int(params["N_batch"])
    composite, alpha = bool(params["CompositionLoss"]), params["alpha"]
    n_traj, _, T_full = y.shape
    if not (1 <= Tc <= T_full) or N_batch < 1:
        raise ValueError("chunked_batches: 1 <= T_train <= T_full and N_batch >= 1")
    n_chunks = n_traj * (T_full // Tc)
    perm = torch.randperm(n_chunks) if perm is None else perm
    noise = torch.randn(perm.shape[0], 6) if noise is None else noise
    if perm.dim() != 1 or perm.shape[0] < 1 or noise.shape != (perm.shape[0], 6):
        raise ValueError("chunked_batches: perm [n], noise [n, 6]")
    if int(perm.min()) < 0 or int(perm.max()) >= n_chunks:
        raise ValueError("chunked_batches: a chunk id outside [0, N_chunks)")
    if params.get("fused", False):
        shapes = (tuple(y.shape), tuple(u.shape), tuple(x.shape))
        st = fused_state(model)
        if st is None or not st.matches(model, optimizer, shapes, Tc, composite):
            del st
            model.__dict__.pop("_chunked_fused", None)   # the old tapes go before the new ones are allocated
            st = model.__dict__["_chunked_fused"] = _FusedChunked(model, optimizer, shapes, Tc, composite)
        with torch.no_grad():
            return st.run(y, u, x, norm_stats, perm, noise, N_batch, alpha)
    dev = model.device
    x_mean, x_std, y_mean, y_std = _stats(norm_stats, dev)
    chunks = [create_chunks(t, Tc) for t in (y, u, x)]
    losses = []
    for i in range(0, perm.shape[0], N_batch):
        pick = perm[i:i + N_batch].to(chunks[0].device)
        y_b, u_b, x_b = (c[pick].to(dev) for c in chunks)
        y_norm, x_norm = (y_b - y_mean) / y_std, (x_b - x_mean) / x_std
        model.batch_size = pick.shape[0]
        model.init_hidden_KNet()
        m1x0 = (x_norm[:, :, 0] + noise[i:i + N_batch].to(dev) * INIT_NOISE_STD).unsqueeze(2)
        model.InitSequence(m1x0, Tc)
        optimizer.zero_grad()
        outs = [model(y_norm[:, :, t:t + 1], u_b[:, :, t:t + 1]).squeeze(2) for t in range(Tc)]
        xo = torch.stack(outs, dim=2)
        if composite:
            loss = compute_composite_loss(xo, x_norm, y_norm, x_mean, x_std, params["m"], params["n"], alpha, PHI_IDX)
        else:
            loss = loss_x_with_angular(xo, x_norm, x_mean, x_std, params["m"], PHI_IDX)
        loss.backward()
        clip_grad_norm_(model.parameters(), max_norm=CLIP_NORM)
        optimizer.step()
        losses.append(float(loss.item()))
        for name in ("h_Q", "h_Sigma", "h_S", "m1x_posterior"):
            setattr(model, name, getattr(model, name).detach())
    return losses


def train_epoch_chunked(model, optimizer, y_chunks, u_chunks, x_chunks, norm_stats, params):
    """One epoch over all chunks, shuffled, in train mode (pipeline_indipendent_chunking.py:65-158).  The three data
    tensors are chunks [N_chunks, c, T_train] or full trajectories [N_traj, c, T_full] (real units).  Returns (average
    batch loss, its dB value)."""
    model.train()
    losses = chunked_batches(model, optimizer, y_chunks, u_chunks, x_chunks, norm_stats, params)
    avg = sum(losses) / max(1, len(losses))
    return avg, 10 * torch.log10(torch.tensor(avg).clamp_min(EPS_DB))


def validate_epoch(model, y_val_norm, u_val, x_val_norm, norm_stats, params, runner=None):
    """The filter over the full validation trajectories (the fused sequence runner: eval mode, no gradient) from a
    noisy first state, scored with the composite or the plain state loss (traj_knet_train_loss_f32).  params: N_CV,
    T_val, CompositionLoss, alpha.  Returns (loss, its dB value)."""
    from .knet_train_fused import train_loss
    N_CV, T = params["N_CV"], params["T_val"]
    dev = y_val_norm.device
    x_mean, x_std = norm_stats["x_mean"].to(dev), norm_stats["x_std"].to(dev)
    model.eval()
    with torch.no_grad():
        if runner is None or runner.B != N_CV:
            runner = KNetSequenceRunner(model, N_CV)
        y, u, xg = (a[:, :, :T].float().contiguous() for a in (y_val_norm, u_val, x_val_norm))
        x0 = xg[:, :, 0]
        x_out = runner.run(y, u, (x0 + VAL_NOISE_STD * torch.randn_like(x0)).unsqueeze(2), fused=True)
        if params["CompositionLoss"]:
            loss, _ = train_loss(x_out, xg, x_mean, x_std, y_tgt=y, alpha=params["alpha"])
        else:
            loss, _ = train_loss(x_out, xg, x_mean, x_std)
        val = float(loss.item())
    return val, 10 * torch.log10(torch.tensor(val).clamp_min(EPS_DB))


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

    def set_data(self, train_data_chunks, val_data_full, test_data_full, norm_stats, device):
        """Each data set is a (y, u, x) triple in real units: the training set as chunks [N_chunks, c, T_chunk] (or
        full trajectories, chunked on the fly), validation and test as full trajectories [N, c, T]."""
        self.y_train_chunks, self.u_train_chunks, self.x_train_chunks = train_data_chunks
        self.y_val, self.u_val, self.x_val = val_data_full
        self.y_test, self.u_test, self.x_test = test_data_full
        self.norm_stats, self.device = norm_stats, device
        self.N_train_chunks, self.N_CV, self.N_T = len(self.y_train_chunks), len(self.y_val), len(self.y_test)

    def set_training_params(self, n_steps, n_batch, lr, wd, T_chunk_train, CompositionLoss=False, alpha=0.5,
                            fused=False):
        """fused=True: every update one HIP graph replay (chunked_batches' fused path)."""
        self.N_steps, self.N_batch, self.lr, self.wd, self.fused = n_steps, n_batch, lr, wd, fused
        self.T_train = T_chunk_train
        self.m, self.n = self.sys_model.m, self.sys_model.n
        self.CompositionLoss, self.alpha = CompositionLoss, alpha
        self.optimizer = torch.optim.AdamW(self.model.parameters(), lr=lr, weight_decay=wd)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode="min", factor=0.5,
                                                                    patience=10, min_lr=1e-7)
        self.train_loss_history_db, self.val_loss_history_db = [], []

    def _normalized(self, y, u, x):
        ns, dev = self.norm_stats, self.device
        y, u, x = y.to(dev), u.to(dev), x.to(dev)
        return (y - ns["y_mean"].to(dev)) / ns["y_std"].to(dev), u, (x - ns["x_mean"].to(dev)) / ns["x_std"].to(dev)

    def _eval_params(self, N, T):
        return {"N_CV": N, "T_val": T, "m": self.m, "n": self.n, "device": self.device,
                "CompositionLoss": self.CompositionLoss, "alpha": self.alpha}

    def train(self):
        best = float("inf")
        val_set = self._normalized(self.y_val, self.u_val, self.x_val)
        val_params = self._eval_params(self.N_CV, self.y_val.shape[2])
        train_params = {"N_batch": self.N_batch, "T_train": self.T_train, "m": self.m, "n": self.n,
                        "device": self.device, "CompositionLoss": self.CompositionLoss, "alpha": self.alpha,
                        "fused": self.fused}
        for epoch in range(self.N_steps):
            avg_train, train_db = train_epoch_chunked(self.model, self.optimizer, self.y_train_chunks,
                                                      self.u_train_chunks, self.x_train_chunks, self.norm_stats,
                                                      train_params)
            val_lin, val_db = validate_epoch(self.model, *val_set, self.norm_stats, val_params)
            self.train_loss_history_db.append(train_db)
            self.val_loss_history_db.append(val_db)
            self.scheduler.step(val_lin)
            if self.log is not None:
                self.log({"epoch": epoch, "learning_rate": self.optimizer.param_groups[0]["lr"],
                          "train_loss": avg_train, "train_loss_dB": float(train_db), "val_loss_linear": val_lin,
                          "val_loss_dB": float(val_db)})
            if val_lin < best:
                best = val_lin
                torch.save(self.model.state_dict(), self.best_model_path)

    def test(self):
        """Scores the test set with the best saved state_dict: (loss, its dB value); None when no model was saved."""
        if not os.path.exists(self.best_model_path):
            return None
        self.model.load_state_dict(torch.load(self.best_model_path, map_location=self.device))
        self.model.to(self.device)
        lin, db = validate_epoch(self.model, *self._normalized(self.y_test, self.u_test, self.x_test), self.norm_stats,
                                 self._eval_params(self.N_T, self.y_test.shape[2]))
        if self.log is not None:
            self.log({"test_loss_linear": lin, "test_loss_dB": float(db)})
        return lin, db

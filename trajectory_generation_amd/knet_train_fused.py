"""Truncated-BPTT training of KalmanNet without autograd, one HIP graph per chunk (opt-in; ``knet_train`` stays the
default path).

A chunk of K steps is a fixed launch sequence -- K forward steps that write a tape, the chunk loss, K backward steps,
one weight-gradient product per layer -- so it is captured once and replayed for every chunk and epoch:

* forward step t: the launches of ``KalmanNetNN.KNet_step`` (``traj_knet_prior_f32``, ``torch.addmm``,
  ``traj_knet_gru_gates_f32``, ``traj_knet_update_f32``) with their outputs in slot t of the tape; dropout in train
  mode is a multiply by that slot's mask;
* the loss: ``traj_knet_train_loss_f32`` (pipeline.py:22-60 and its gradient w.r.t. the stacked posteriors, an optional
  ``g_extra`` added -- how ``lambda_pred`` x the prediction loss's gradient enters);
* backward step t = K-1 .. 0, transposed products as ``torch.mm`` against the weight matrices, the HIP kernels of
  csrc/knet_bwd.h between them, in the order update, FC4, FC3, FC2, GRU_S, FC7 + FC1, GRU_Sigma, GRU_Q, FC5, prior;
  the incoming hidden-state and posterior gradients are zero at the chunk's last step (the reference's ``detach()``);
  every step writes its pre-activation gradients into the tape;
* after the sweep each weight gradient is one product over the K B rows of the tape, each bias gradient one column sum,
  into static buffers; ``add_grads`` adds them into the parameters' ``.grad``.  Clipping and the optimizer stay torch's,
  outside the graph, unless the caller passes them as the ``post`` hook of ``run_chunk`` (``pre`` / ``post``: launches
  enqueued in front of the first forward step and behind the weight gradients, captured with the chunk -- how
  pipeline_indipendent_chunking.py makes one optimizer update one replay).

tests/_knet_bptt_ref.py is the same sweep in float64 on the CPU.

Tape memory (float32): per sequence-step
  train mode  4 B x (2 dh + 46 H + 4 d5 + 432),    eval mode  4 B x (2 dh + 44 H + 2 d5 + 306)
with dh = FC2's hidden width (10240), H = 128, d5 = FC5's width (30 / 60): FC2's hidden layer and its gradient dominate
at 2 x 10240 x 4 B per sequence-step, about 1.05 GB of the 1.38 GB at B = 64, K = 200, in_mult 10 (``tape_bytes`` is
the allocator's own figure for the runner).

Dropout: train mode draws every layer's mask for the whole chunk with torch's generator, one draw per layer per chunk,
outside the graph ({0, 1/(1-p)}; p = 0.05 for FC5, FC1, FC7, FC3, FC4 and 0.1 for FC2's output).  The module path draws
per step and per layer, so for the same seed the masks here are a different, identically distributed stream.
``set_masks`` takes explicit masks instead.
"""
from __future__ import annotations

import ctypes as C
import time

import torch
from torch.nn.utils import clip_grad_norm_

from . import _lib
from .batch import params_struct
from .knet import _p, _stream, limits_struct
from .knet_train import EPS_DB

# dropout probability of each masked layer's output (NNBuild); FC1 and FC7 share the mask buffer "FC17"
MASK_P = {"FC5": 0.05, "FC17": 0.05, "FC2": 0.1, "FC3": 0.05, "FC4": 0.05}
# launches of one time step in the captured chain (eval / train mode), forward + backward: the baseline for fusing the
# small layers' backward
LAUNCHES_PER_STEP = {"forward": (27, 32), "backward": (25, 25)}


_ck = _lib.check


# ---------------------------------------------------------------------- the kernels on their own (allocating wrappers)

def prior_bwd(params: dict, Ts: float, x_post, u, x_mean, x_std, y_mean, y_std, g_prior, g_dy=None, u_mean=None,
              u_std=None):
    """traj_knet_prior_bwd_f32: x_post / g_prior [B,6], u [B,2], g_dy [B,5] or None -> g_x_post [B,6]."""
    B = x_post.shape[0]
    c = lambda t: None if t is None else t.detach().float().contiguous()   # noqa: E731
    xp, uu, gp, gd = c(x_post.reshape(B, 6)), c(u.reshape(B, 2)), c(g_prior.reshape(B, 6)), c(g_dy)
    norm = [None if t is None else c(t.reshape(-1)) for t in (x_mean, x_std, y_mean, y_std, u_mean, u_std)]
    out = torch.empty((B, 6), dtype=torch.float32, device=x_post.device)
    _ck(_lib.lib().traj_knet_prior_bwd_f32(C.byref(params_struct(params)), C.byref(limits_struct(params)), float(Ts), B,
                                           _p(xp), _p(uu), *[_p(t) for t in norm], _p(gp), _p(gd), _p(out), _stream()),
        "traj_knet_prior_bwd_f32")
    return out


def gru_gates_bwd(gi, gh, h, g_out, g_out2=None):
    """traj_knet_gru_gates_bwd_f32: gi, gh [B,3H], h [B,H], g_out (+ g_out2) [B,H] (unit column stride, any row
    stride) -> (g_gi, g_gh [B,3H], g_h [B,H])."""
    B, H = h.shape
    gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
    g_gi, g_gh, g_h = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
    _ck(_lib.lib().traj_knet_gru_gates_bwd_f32(B, H, _p(gi), _p(gh), _p(h), _p(g_out), g_out.stride(0), _p(g_out2),
                                               0 if g_out2 is None else g_out2.stride(0), _p(g_gi), _p(g_gh), _p(g_h),
                                               _stream()), "traj_knet_gru_gates_bwd_f32")
    return g_gi, g_gh, g_h


def update_bwd(KG, dy, innov_logit, g_post, g_post2=None):
    """traj_knet_update_bwd_f32 -> (g_prior [B,6], g_KG [B,30], g_dy [B,5], g_logit [B])."""
    B, dev = dy.shape[0], dy.device
    KG, dy, g_post = KG.reshape(B, 30).contiguous(), dy.contiguous(), g_post.contiguous()
    g2 = None if g_post2 is None else g_post2.contiguous()
    lg = innov_logit.detach().reshape(1).contiguous()
    outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 6), (B, 30), (B, 5), (B,))]
    _ck(_lib.lib().traj_knet_update_bwd_f32(B, _p(KG), _p(dy), _p(lg), _p(g_post), _p(g2), *[_p(o) for o in outs],
                                            _stream()), "traj_knet_update_bwd_f32")
    return tuple(outs)


def dense_bwd(g_a, act=None, mask=None, g_b=None):
    """traj_knet_dense_bwd_f32: (g_a + g_b) * mask * (act > 0) -> [rows, cols]; g_a / g_b may be column slices."""
    rows, cols = g_a.shape
    out = torch.empty((rows, cols), dtype=torch.float32, device=g_a.device)
    act = None if act is None else act.contiguous()
    mask = None if mask is None else mask.contiguous()
    _ck(_lib.lib().traj_knet_dense_bwd_f32(rows, cols, _p(g_a), g_a.stride(0), _p(g_b),
                                           0 if g_b is None else g_b.stride(0), _p(act), _p(mask), _p(out), _stream()),
        "traj_knet_dense_bwd_f32")
    return out


def train_loss(x_out, x_tgt, x_mean, x_std, y_tgt=None, alpha=1.0, g_extra=None):
    """traj_knet_train_loss_f32 on x_out [B,6,K] (read through its strides: dense, e.g. a [K,B,6] tape viewed as
    [B,6,K]): (loss [1], grad [B,6,K] with x_out's strides).  y_tgt [B,5,K] with alpha < 1: the composite loss."""
    B, _, K = x_out.shape
    c = lambda t: None if t is None else t.detach().float().contiguous()   # noqa: E731
    xo = x_out.detach().float()
    if min(xo.stride()) < 1 or not xo.permute(*sorted(range(3), key=lambda i: -xo.stride(i))).is_contiguous():
        xo = xo.contiguous()
    xt, yt, gx, xm, xs = c(x_tgt), c(y_tgt), c(g_extra), c(x_mean.reshape(-1)), c(x_std.reshape(-1))
    loss = torch.empty(1, dtype=torch.float32, device=x_out.device)
    grad = torch.empty_strided(xo.shape, xo.stride(), dtype=torch.float32, device=x_out.device)
    _ck(_lib.lib().traj_knet_train_loss_f32(B, K, _p(xo), *[int(v) for v in xo.stride()], _p(xt), _p(yt), _p(xm),
                                            _p(xs), float(alpha), _p(gx), _p(loss), _p(grad), _stream()),
        "traj_knet_train_loss_f32")
    return loss, grad


def chunk_gather(y, u, x, chunk_ids, Tc, x_mean, x_std, y_mean, y_std, noise=None, noise_std=0.0, out=None,
                 want_y_tgt=True):
    """traj_knet_chunk_gather_f32: the batch of chunks chunk_ids [B] (int32) of Tc steps out of the full trajectories
    y [n,5,T], u [n,2,T], x [n,6,T] (float32, contiguous, real units) -> (Y [Tc,B,5], U [Tc,B,2], x_tgt [B,6,Tc],
    y_tgt [B,5,Tc] or None, m1x0 [B,6]).  ``out``: the five destination buffers (y_tgt may be None) instead of new
    ones -- no allocation then, the form a captured graph takes."""
    n, _, T = y.shape
    B = chunk_ids.shape[0]
    for t, c in ((y, 5), (u, 2), (x, 6)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != (n, c, T):
            raise ValueError("chunk_gather: y [n,5,T], u [n,2,T], x [n,6,T], contiguous float32")
    if chunk_ids.dtype != torch.int32 or not chunk_ids.is_contiguous():
        raise ValueError("chunk_gather: chunk_ids is a contiguous int32 vector")
    if out is None:
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=y.device)   # noqa: E731
        out = (e(Tc, B, 5), e(Tc, B, 2), e(B, 6, Tc), e(B, 5, Tc) if want_y_tgt else None, e(B, 6))
    stats = [t.reshape(-1) for t in (x_mean, x_std, y_mean, y_std)]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in stats):
        raise ValueError("chunk_gather: contiguous float32 statistics")
    _ck(_lib.lib().traj_knet_chunk_gather_f32(n, T, int(Tc), B, _p(y), _p(u), _p(x), _p(chunk_ids),
                                              *[_p(t) for t in stats], _p(noise), float(noise_std),
                                              *[_p(o) for o in out], _stream()), "traj_knet_chunk_gather_f32")
    return out


class ClipAdamW:
    """traj_knet_clip_adamw_f32 over the tensors p / g / m / v (lists of equal length; element i of each has the same
    number of elements; float32, contiguous, on one device; any 4-byte alignment): clip_grad_norm_(max_norm) followed
    by one AdamW step, two launches per ``step()``, nothing allocated there.  ``lr`` and ``t`` are one-element device
    tensors (float32 / int32) read by the kernels -- pass existing ones to share them between instances; ``t`` is
    advanced by every step, ``total_norm`` receives the gradient norm before clipping."""

    def __init__(self, p, g, m, v, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, t=0):
        if not (len(p) == len(g) == len(m) == len(v)) or not p:
            raise ValueError("ClipAdamW: four lists of equal, positive length")
        dev = p[0].device
        tab = (_lib.KnetOptEntry * len(p))()
        for i, quad in enumerate(zip(p, g, m, v)):
            for a in quad:
                if a.dtype != torch.float32 or not a.is_contiguous() or a.device != dev or a.numel() < 1 \
                        or a.numel() != quad[0].numel():
                    raise ValueError("ClipAdamW: contiguous float32 tensors of one size per entry on one device")
            tab[i].p, tab[i].g, tab[i].m, tab[i].v = (a.data_ptr() for a in quad)
            tab[i].n = quad[0].numel()
        self.n_tensors, self.n_total = len(p), sum(a.numel() for a in p)
        self.table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self.lr = lr if torch.is_tensor(lr) else torch.tensor([float(lr)], dtype=torch.float32, device=dev)
        self.t = t if torch.is_tensor(t) else torch.tensor([int(t)], dtype=torch.int32, device=dev)
        if self.lr.dtype != torch.float32 or self.t.dtype != torch.int32:
            raise ValueError("ClipAdamW: lr float32, t int32")
        self.total_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(_lib.lib().traj_knet_clip_adamw_workspace_bytes() // 8, dtype=torch.float64, device=dev)
        self.hyper = (float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_norm))
        self._keep = (p, g, m, v)

    def step(self):
        _ck(_lib.lib().traj_knet_clip_adamw_f32(_p(self.table), self.n_tensors, self.n_total, _p(self.lr), *self.hyper,
                                                _p(self.t), _p(self.total_norm), _p(self.ws), self.ws.numel() * 8,
                                                _stream()), "traj_knet_clip_adamw_f32")


class FusedTBPTT:
    """The tape, the launch chain and the graphs of one (model, B, K).  A shorter last chunk (Kc < K) uses the first Kc
    slots and a graph of its own.  The model's mode (train / eval) at construction is the runner's."""

    def __init__(self, model, B: int, K: int):
        if B < 1 or K < 1:
            raise ValueError("FusedTBPTT: B and K must be positive")
        md = self.model = model
        self.B, self.K, self.train = int(B), int(K), bool(model.training)
        dev = self.dev = md.device
        H = self.H = md.d_hidden_Q
        if not (md.m == 6 and md.n == 5 and md.d_hidden_Sigma == H and md.d_hidden_S == H):
            raise NotImplementedError("FusedTBPTT: m = 6, n = 5 and one hidden size for the three GRUs")
        self.d5, self.d1, self.d7 = md.d_output_FC5, md.d_output_FC1, md.d_output_FC7
        self.d3, self.dh, self.dkg = md.d_output_FC3, md.d_hidden_FC2, md.d_output_FC2
        self.p, self.lim, self.Ts = params_struct(md.sys.Params), limits_struct(md.sys.Params), float(md.sys.Ts)
        xm, xs, ym, ys = (t.reshape(-1).float().contiguous() for t in md._norm_tensors())
        um = None if md.u_mean is None else md.u_mean.reshape(-1).float().contiguous()
        us = None if md.u_std is None else md.u_std.reshape(-1).float().contiguous()
        self.norm = (xm, xs, ym, ys, um, us)
        self.names = [k for k, _ in md.named_parameters()]
        self.params = dict(md.named_parameters())
        for k, v in self.params.items():
            if v.dtype != torch.float32 or not v.is_contiguous() or not v.is_cuda:
                raise ValueError(f"{k}: FusedTBPTT needs contiguous float32 device weights")
        nb0 = torch.cuda.memory_allocated(dev)
        self._alloc()
        self.tape_bytes = torch.cuda.memory_allocated(dev) - nb0
        self.grads = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.graphs, self.ptrs = {}, None
        self.graph_instantiate_s = 0.0
        self._keep = {}
        self._explicit_masks = False

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        K, B, H = self.K, self.B, self.H
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.dev)   # noqa: E731
        T = self.T = {}
        # forward tape, [K, B, .]; slot 0 of P / HQ / HSig / HS is the chunk's initial state, slot t + 1 step t's output
        T["P"], T["HQ"], T["HSig"], T["HS"] = z(K + 1, B, 6), z(K + 1, B, H), z(K + 1, B, H), z(K + 1, B, H)
        T["U"], T["Y"], T["prior"], T["dy"] = z(K, B, 2), z(K, B, 5), z(K, B, 6), z(K, B, 5)
        T["a5"], T["A17"] = z(K, B, self.d5), z(K, B, self.d1 + self.d7)
        for q in ("Q", "Sig", "S"):
            T["gi" + q], T["gh" + q] = z(K, B, 3 * H), z(K, B, 3 * H)
        T["X2"], T["hid"], T["KG"] = z(K, B, 2 * H), z(K, B, self.dh), z(K, B, self.dkg)
        T["X3"], T["a3"], T["X4"] = z(K, B, H + self.dkg), z(K, B, self.d3), z(K, B, H + self.d3)
        if self.train:   # masked layers: the post-activation (ReLU mask) and the masked output (next layer's input)
            T["o5"], T["XS"], T["a4"] = z(K, B, self.d5), z(K, B, self.d1 + self.d7), z(K, B, H)
            self.M = {"FC5": z(K, B, self.d5), "FC17": z(K, B, self.d1 + self.d7), "FC2": z(K, B, self.dkg),
                      "FC3": z(K, B, self.d3), "FC4": z(K, B, H)}
        else:
            T["o5"], T["XS"], T["a4"] = T["a5"], T["A17"], T["HSig"][1:]
            self.M = None
        # backward tape: the pre-activation gradients, and the loss gradient / per-sequence logit gradient
        T["d4"], T["d3"], T["dkg"], T["dhid"] = z(K, B, H), z(K, B, self.d3), z(K, B, self.dkg), z(K, B, self.dh)
        T["d17"], T["d5"], T["GL"], T["glogit"] = z(K, B, self.d1 + self.d7), z(K, B, self.d5), z(K, B, 6), z(K, B)
        for q in ("Q", "Sig", "S"):
            T["dgi" + q], T["dgh" + q] = z(K, B, 3 * H), z(K, B, 3 * H)
        # loss inputs [B, c, Kc] (the first B c Kc floats), g_extra likewise
        self.xt, self.yt, self.gx = z(B * 6 * K), z(B * 5 * K), z(B * 6 * K)
        self.loss = z(1)
        # per-step scratch
        S = self.S = {}
        S["m1y"], S["oSig"], S["a1"], S["a7"], S["o3"] = z(B, 5), z(B, H), z(B, self.d1), z(B, self.d7), z(B, self.d3)
        S["g_prior0"], S["g_KG0"], S["g_dy0"] = z(B, 6), z(B, self.dkg), z(B, 5)
        S["g_x4"], S["g_x3"], S["g_x2"] = z(B, H + self.d3), z(B, H + self.dkg), z(B, 2 * H)
        S["gS"], S["ghd"], S["g_xS"], S["g_oSig"] = z(B, H), z(B, H), z(B, self.d1 + self.d7), z(B, H)
        S["g_dy"], S["g_hQ"], S["g_o5"], S["g_prior"] = z(B, 5), z(B, H), z(B, self.d5), z(B, 6)
        # carried gradients (w.r.t. the step's posterior / hidden outputs), two sets in turn
        self.carry = [{"P": z(B, 6), "HQ": z(B, H), "HSig": z(B, H), "HS": z(B, H)} for _ in range(2)]
        self.zeroH = z(B, H)

    # ------------------------------------------------------------------ state and inputs
    def reset(self, m1x0, hidden=None):
        """The chunk's initial posterior m1x0 [B,6(,1)] and hidden states (h_Q, h_Sigma, h_S), zeros when None."""
        T = self.T
        T["P"][0].copy_(m1x0.reshape(self.B, 6))
        for k, h in zip(("HQ", "HSig", "HS"), hidden if hidden is not None else (None,) * 3):
            if h is None:
                T[k][0].zero_()
            else:
                T[k][0].copy_(h.reshape(self.B, self.H))

    def carry_over(self, Kc):
        """The end state of a Kc-step chunk becomes the next chunk's initial state (the reference's detach())."""
        for k in ("P", "HQ", "HSig", "HS"):
            self.T[k][0].copy_(self.T[k][Kc])

    def final_state(self, Kc):
        T = self.T
        return tuple(T[k][Kc].clone() for k in ("P", "HQ", "HSig", "HS"))

    def posteriors(self, Kc):
        """The chunk's stacked posteriors as a [B,6,Kc] view of the tape (strides 6, 1, 6 B)."""
        return self.T["P"][1:Kc + 1].permute(1, 2, 0)

    def g_extra(self, Kc):
        """The [B,6,Kc] buffer the loss kernel adds to its gradient (written by the ``extra`` hook of run_chunk)."""
        return self.gx[:self.B * 6 * Kc].view(self.B, 6, Kc)

    def g_x0(self, Kc):
        """d loss / d (initial posterior) of the last Kc-step chunk [B,6]."""
        return self.carry[(Kc + 1) % 2]["P"]

    def set_masks(self, masks):
        """Explicit dropout masks: {"FC5", "FC1", "FC7", "FC2", "FC3", "FC4"} -> [Kc,B,width] ({0, 1/(1-p)}); None
        returns to random draws."""
        if not self.train:
            raise ValueError("set_masks: the runner was built in eval mode")
        self._explicit_masks = masks is not None
        if masks is None:
            return
        Kc = masks["FC5"].shape[0]
        d = lambda k: masks[k].to(self.dev, torch.float32)   # noqa: E731
        self.M["FC5"][:Kc].copy_(d("FC5"))
        self.M["FC17"][:Kc].copy_(torch.cat((d("FC1"), d("FC7")), 2))
        for k in ("FC2", "FC3", "FC4"):
            self.M[k][:Kc].copy_(d(k))

    def _draw_masks(self, Kc):
        for k, p in MASK_P.items():
            self.M[k][:Kc].bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))

    # ------------------------------------------------------------------ the launch chain
    def _lin(self, x, lin, out, relu=True):
        torch.addmm(lin.bias, x, lin.weight.t(), out=out)
        if relu:
            torch.relu_(out)

    def _gru_fwd(self, x, h, gru, gi, gh, out):
        torch.addmm(gru.bias_ih_l0, x, gru.weight_ih_l0.t(), out=gi)
        torch.addmm(gru.bias_hh_l0, h, gru.weight_hh_l0.t(), out=gh)
        _ck(_lib.lib().traj_knet_gru_gates_f32(self.B, self.H, _p(gi), _p(gh), _p(h), _p(out), _stream()),
            "traj_knet_gru_gates_f32")

    def _forward_step(self, t):
        md, T, S, M, B = self.model, self.T, self.S, self.M, self.B
        L = _lib.lib()
        _ck(L.traj_knet_prior_f32(C.byref(self.p), C.byref(self.lim), self.Ts, B, _p(T["P"][t]), _p(T["U"][t]),
                                  _p(T["Y"][t]), *[_p(v) for v in self.norm], _p(T["prior"][t]), _p(S["m1y"]),
                                  _p(T["dy"][t]), _stream()), "traj_knet_prior_f32")
        self._lin(T["prior"][t], md.FC5[0], T["a5"][t])
        if M:
            torch.mul(T["a5"][t], M["FC5"][t], out=T["o5"][t])
        self._gru_fwd(T["o5"][t], T["HQ"][t], md.GRU_Q, T["giQ"][t], T["ghQ"][t], T["HQ"][t + 1])
        self._gru_fwd(T["HQ"][t + 1], T["HSig"][t], md.GRU_Sigma, T["giSig"][t], T["ghSig"][t], S["oSig"])
        self._lin(S["oSig"], md.FC1[0], S["a1"], relu=False)
        self._lin(T["dy"][t], md.FC7[0], S["a7"], relu=False)
        torch.cat((S["a1"], S["a7"]), 1, out=T["A17"][t])
        torch.relu_(T["A17"][t])
        if M:
            torch.mul(T["A17"][t], M["FC17"][t], out=T["XS"][t])
        self._gru_fwd(T["XS"][t], T["HS"][t], md.GRU_S, T["giS"][t], T["ghS"][t], T["HS"][t + 1])
        torch.cat((S["oSig"], T["HS"][t + 1]), 1, out=T["X2"][t])
        self._lin(T["X2"][t], md.FC2[0], T["hid"][t])
        self._lin(T["hid"][t], md.FC2[2], T["KG"][t], relu=False)
        if M:
            T["KG"][t].mul_(M["FC2"][t])
        torch.cat((T["HS"][t + 1], T["KG"][t]), 1, out=T["X3"][t])
        self._lin(T["X3"][t], md.FC3[0], T["a3"][t])
        o3 = T["a3"][t]
        if M:
            o3 = torch.mul(T["a3"][t], M["FC3"][t], out=S["o3"])
        torch.cat((S["oSig"], o3), 1, out=T["X4"][t])
        self._lin(T["X4"][t], md.FC4[0], T["a4"][t])
        if M:
            torch.mul(T["a4"][t], M["FC4"][t], out=T["HSig"][t + 1])
        _ck(L.traj_knet_update_f32(B, _p(T["prior"][t]), _p(T["KG"][t]), _p(T["dy"][t]), _p(md.innov_logit.detach()),
                                   _p(T["P"][t + 1]), _stream()), "traj_knet_update_f32")

    def _dense_bwd(self, g_a, act, mask, out, g_b=None):
        rows, cols = out.shape
        _ck(_lib.lib().traj_knet_dense_bwd_f32(rows, cols, _p(g_a), g_a.stride(0), _p(g_b),
                                               0 if g_b is None else g_b.stride(0), _p(act), _p(mask), _p(out),
                                               _stream()), "traj_knet_dense_bwd_f32")

    def _gru_bwd(self, q, t, h, g1, g2, gru, g_h_out, g_x_out):
        """Gate backward of GRU q at step t from g1 (+ g2); g_h_out = d / d h_in, g_x_out = d / d input."""
        T, S = self.T, self.S
        dgi, dgh = T["dgi" + q][t], T["dgh" + q][t]
        _ck(_lib.lib().traj_knet_gru_gates_bwd_f32(
            self.B, self.H, _p(T["gi" + q][t]), _p(T["gh" + q][t]), _p(h), _p(g1), g1.stride(0), _p(g2),
            0 if g2 is None else g2.stride(0), _p(dgi), _p(dgh), _p(S["ghd"]), _stream()), "traj_knet_gru_gates_bwd_f32")
        torch.addmm(S["ghd"], dgh, gru.weight_hh_l0, out=g_h_out)
        torch.mm(dgi, gru.weight_ih_l0, out=g_x_out)

    def _backward_step(self, t, last, cin, cout):
        """cin: the gradients carried in from step t + 1 (unused when last), cout: written for step t - 1."""
        md, T, S, B, H = self.model, self.T, self.S, self.B, self.H
        M = self.M or {}
        mk = lambda k: M[k][t] if M else None   # noqa: E731
        L = _lib.lib()
        zero = self.zeroH
        # 1. update
        _ck(L.traj_knet_update_bwd_f32(B, _p(T["KG"][t]), _p(T["dy"][t]), _p(md.innov_logit.detach()), _p(T["GL"][t]),
                                       None if last else _p(cin["P"]), _p(S["g_prior0"]), _p(S["g_KG0"]),
                                       _p(S["g_dy0"]), _p(T["glogit"][t]), _stream()), "traj_knet_update_bwd_f32")
        # 2. FC4 (its output is the next step's h_Sigma)
        self._dense_bwd(zero if last else cin["HSig"], T["a4"][t], mk("FC4"), T["d4"][t])
        torch.mm(T["d4"][t], md.FC4[0].weight, out=S["g_x4"])
        # 3. FC3
        self._dense_bwd(S["g_x4"][:, H:], T["a3"][t], mk("FC3"), T["d3"][t])
        torch.mm(T["d3"][t], md.FC3[0].weight, out=S["g_x3"])
        # 4. FC2: two products and the ReLU mask
        self._dense_bwd(S["g_KG0"], None, mk("FC2"), T["dkg"][t], g_b=S["g_x3"][:, H:])
        torch.mm(T["dkg"][t], md.FC2[2].weight, out=T["dhid"][t])
        self._dense_bwd(T["dhid"][t], T["hid"][t], None, T["dhid"][t])
        torch.mm(T["dhid"][t], md.FC2[0].weight, out=S["g_x2"])
        # 5. GRU_S
        self._dense_bwd(S["g_x3"][:, :H], None, None, S["gS"], g_b=S["g_x2"][:, H:])
        self._gru_bwd("S", t, T["HS"][t], S["gS"], None if last else cin["HS"], md.GRU_S, cout["HS"], S["g_xS"])
        # 6. FC7 and FC1 (one epilogue over the concatenated pair)
        self._dense_bwd(S["g_xS"], T["A17"][t], mk("FC17"), T["d17"][t])
        d1, d7 = T["d17"][t][:, :self.d1], T["d17"][t][:, self.d1:]
        torch.addmm(S["g_dy0"], d7, md.FC7[0].weight, out=S["g_dy"])
        torch.addmm(S["g_x2"][:, :H], d1, md.FC1[0].weight, out=S["g_oSig"])
        # 7. GRU_Sigma
        self._gru_bwd("Sig", t, T["HSig"][t], S["g_oSig"], S["g_x4"][:, :H], md.GRU_Sigma, cout["HSig"], S["g_hQ"])
        # 8. GRU_Q
        self._gru_bwd("Q", t, T["HQ"][t], S["g_hQ"], None if last else cin["HQ"], md.GRU_Q, cout["HQ"], S["g_o5"])
        # 9. FC5
        self._dense_bwd(S["g_o5"], T["a5"][t], mk("FC5"), T["d5"][t])
        torch.addmm(S["g_prior0"], T["d5"][t], md.FC5[0].weight, out=S["g_prior"])
        # 10. prior
        _ck(L.traj_knet_prior_bwd_f32(C.byref(self.p), C.byref(self.lim), self.Ts, B, _p(T["P"][t]), _p(T["U"][t]),
                                      *[_p(v) for v in self.norm], _p(S["g_prior"]), _p(S["g_dy"]), _p(cout["P"]),
                                      _stream()), "traj_knet_prior_bwd_f32")

    def _weight_grads(self, Kc):
        T, G, H, n = self.T, self.grads, self.H, Kc * self.B
        r = lambda k, lo=0: T[k][lo:lo + Kc].reshape(n, -1)   # noqa: E731

        def dense(name, D, X):
            torch.mm(D.t(), X, out=G[name + ".weight"])
            torch.sum(D, 0, out=G[name + ".bias"])

        dense("FC5.0", r("d5"), r("prior"))
        dense("FC1.0", r("d17")[:, :self.d1], r("X2")[:, :H])
        dense("FC7.0", r("d17")[:, self.d1:], r("dy"))
        dense("FC2.0", r("dhid"), r("X2"))
        dense("FC2.2", r("dkg"), r("hid"))
        dense("FC3.0", r("d3"), r("X3"))
        dense("FC4.0", r("d4"), r("X4"))
        for name, q, x in (("GRU_Q", "Q", r("o5")), ("GRU_Sigma", "Sig", r("HQ", 1)), ("GRU_S", "S", r("XS"))):
            Di, Dh = r("dgi" + q), r("dgh" + q)
            torch.mm(Di.t(), x, out=G[name + ".weight_ih_l0"])
            torch.sum(Di, 0, out=G[name + ".bias_ih_l0"])
            torch.mm(Dh.t(), r("H" + q), out=G[name + ".weight_hh_l0"])
            torch.sum(Dh, 0, out=G[name + ".bias_hh_l0"])
        torch.sum(T["glogit"][:Kc].reshape(1, n), 1, out=G["innov_logit"].reshape(1))

    def _enqueue(self, Kc, alpha, extra, pre=None, post=None):
        B = self.B
        if pre is not None:
            pre(self, Kc)
        for t in range(Kc):
            self._forward_step(t)
        gx = None
        if extra is not None:
            extra(self, Kc)
            gx = self.gx
        xm, xs = self.norm[0], self.norm[1]
        _ck(_lib.lib().traj_knet_train_loss_f32(B, Kc, _p(self.T["P"][1]), 6, 1, 6 * B, _p(self.xt),
                                                None if alpha is None else _p(self.yt), _p(xm), _p(xs),
                                                1.0 if alpha is None else float(alpha), _p(gx), _p(self.loss),
                                                _p(self.T["GL"]), _stream()), "traj_knet_train_loss_f32")
        for t in range(Kc - 1, -1, -1):
            # step t reads the set written by step t + 1 and writes the other one: step 0 writes carry[(Kc + 1) % 2]
            self._backward_step(t, t == Kc - 1, self.carry[(Kc - t) % 2], self.carry[(Kc - t + 1) % 2])
        self._weight_grads(Kc)
        if post is not None:
            post(self, Kc)

    def _param_ptrs(self):
        return tuple(v.data_ptr() for v in self.params.values())

    @torch.no_grad()
    def run_chunk(self, y, u, x_tgt, composite=True, alpha=0.8, extra=None, extra_key=None, use_graph=True, pre=None,
                  post=None, Kc=None):
        """One chunk from the state set by reset / carry_over: y [B,5,Kc] normalized observations (also the composite
        loss's target), u [B,2,Kc], x_tgt [B,6,Kc] normalized targets.  Leaves the loss in ``self.loss`` (returned, a
        1-element device tensor), the gradients in ``self.grads`` and the tape filled.  ``extra(runner, Kc)``, when
        given, is enqueued between the forward and the loss and writes ``g_extra(Kc)``; ``extra_key`` tells graphs
        with different hooks apart.

        ``pre(runner, Kc)`` is enqueued before the first forward step and ``post(runner, Kc)`` after the weight
        gradients; both are part of the graph's key.  With ``pre``, y / u / x_tgt may be None (``Kc`` given instead):
        the hook fills the tape's inputs (T["Y"], T["U"], xt, yt, T["P"][0] and the hidden slots) on the device.
        ``post`` is left out of the warm-up runs before a capture and runs once per call (an optimizer step there is
        applied exactly once)."""
        B, T = self.B, self.T
        if y is None:
            if pre is None or Kc is None or u is not None or x_tgt is not None:
                raise ValueError("run_chunk: without y / u / x_tgt, a pre hook and Kc are needed")
            if not (1 <= Kc <= self.K):
                raise ValueError("run_chunk: 1 <= Kc <= K")
        else:
            Kc = y.shape[2]
            if not (1 <= Kc <= self.K) or y.shape != (B, 5, Kc) or u.shape != (B, 2, Kc) or x_tgt.shape != (B, 6, Kc):
                raise ValueError("run_chunk: y [B,5,Kc], u [B,2,Kc], x_tgt [B,6,Kc] with Kc <= K")
        if self.model.training != self.train:
            raise ValueError("run_chunk: the model's train / eval mode changed since the runner was built")
        if y is not None:
            T["Y"][:Kc].copy_(y.permute(2, 0, 1))
            T["U"][:Kc].copy_(u.permute(2, 0, 1))
            self.xt[:B * 6 * Kc].view(B, 6, Kc).copy_(x_tgt)
            if composite:
                self.yt[:B * 5 * Kc].view(B, 5, Kc).copy_(y)
        if self.train and not self._explicit_masks:
            self._draw_masks(Kc)
        a = float(alpha) if composite else None
        if not use_graph:
            self._enqueue(Kc, a, extra, pre, post)
            return self.loss
        if self.ptrs != self._param_ptrs():   # the captured weight pointers moved: capture again
            self.graphs, self.ptrs = {}, self._param_ptrs()
        key = (Kc, a, extra_key) if pre is None and post is None else (Kc, a, extra_key, pre, post)
        if key not in self.graphs:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):   # warm up the library GEMM paths before capture (never post: it may step)
                    self._enqueue(Kc, a, extra, pre)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._enqueue(Kc, a, extra, pre, post)
            torch.cuda.synchronize()
            self.graph_instantiate_s = time.perf_counter() - t0
            self.graphs[key] = g
        self.graphs[key].replay()
        return self.loss

    def add_grads(self, scale=1.0):
        """Add the chunk's gradients (x scale) into the parameters' .grad, created when None."""
        ps = list(self.params.items())
        for _, p in ps:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        torch._foreach_add_([p.grad for _, p in ps], [self.grads[k] for k, _ in ps], alpha=float(scale))


def runner_for(model, B, K):
    """The model's cached FusedTBPTT for (B, K, train / eval mode)."""
    cache = model.__dict__.setdefault("_fused_tbptt", {})
    key = (int(B), int(K), bool(model.training))
    if key not in cache:
        cache.clear()   # one tape at a time: a runner's buffers are its dominant cost
        cache[key] = FusedTBPTT(model, B, K)
    return cache[key]


def _publish_state(model, runner, Kc):
    """Leave the module's state attributes as the module path does after a sequence (detached end state)."""
    P, HQ, HSig, HS = runner.final_state(Kc)
    model.m1x_posterior = P.unsqueeze(2)
    model.h_Q, model.h_Sigma, model.h_S = HQ.unsqueeze(0), HSig.unsqueeze(0), HS.unsqueeze(0)


def tbptt_sequence_fused(model, optimizer, y_norm, u, x_norm, m1x0, params, x_mean, x_std):
    """knet_train.tbptt_sequence on the fused path: same arguments and return values (mean chunk loss, its dB value,
    per-chunk losses), both strategies, composite and plain state loss.  x_mean / x_std must be the model's."""
    strategy, K, T = params["strategy"], params["K_TBPTT"], params["T"]
    use_composite, alpha = params["CompositionLoss"], params["alpha"]
    B = y_norm.shape[0]
    model.batch_size = B
    model.T = T
    R = runner_for(model, B, min(K, T))
    if not torch.equal(x_mean.reshape(-1).to(R.norm[0]), R.norm[0]) or \
            not torch.equal(x_std.reshape(-1).to(R.norm[1]), R.norm[1]):
        raise ValueError("tbptt_sequence_fused: x_mean / x_std differ from the model's normalization")
    R.reset(m1x0)
    optimizer.zero_grad()
    num_chunks = (T + K - 1) // K
    losses, Kc = [], 0
    for c0 in range(0, T, K):
        c1 = min(c0 + K, T)
        Kc = c1 - c0
        loss = R.run_chunk(y_norm[:, :, c0:c1], u[:, :, c0:c1], x_norm[:, :, c0:c1], composite=use_composite,
                           alpha=alpha)
        if strategy == "accumulation":
            R.add_grads(1.0 / num_chunks)
        else:
            R.add_grads()
            clip_grad_norm_(model.parameters(), max_norm=5.0)
            optimizer.step()
            optimizer.zero_grad()
        losses.append(float(loss.item()))
        R.carry_over(Kc)
    if strategy == "accumulation":
        clip_grad_norm_(model.parameters(), max_norm=5.0)
        optimizer.step()
        optimizer.zero_grad()
    _publish_state(model, R, Kc)
    avg = sum(losses) / max(1, len(losses))
    loss_db = 10 * torch.log10(torch.tensor(avg).clamp_min(EPS_DB))
    return avg, loss_db, losses

"""Float64 restatement of the manual truncated-BPTT sweep of trajectory_generation_amd/knet_train_fused.py -- TEST
INFRASTRUCTURE ONLY (plain torch on the CPU).  The blueprint the fused path and its kernels are held to.

``forward_tape`` runs K steps of tests/_knet_ref.py's stage functions (prior64, lin64, gru64, update64) and keeps what
the backward reads; ``sweep`` walks it back by hand in the order of the device path -- update, FC4, FC3, FC2, GRU_S,
FC7 and FC1, GRU_Sigma, GRU_Q, FC5, prior -- with zero incoming hidden-state / posterior gradients at the chunk's last
step, writes every layer's pre-activation gradient into the tape, and forms each weight gradient afterwards as one
product over the K B rows of the tape (bias: one column sum).  Dropout is an explicit mask per layer
({0, 1/(1-p)}, [K,B,width]; ``None`` = eval mode).  The only stage whose vector-Jacobian product is not written out is
the vehicle step of the prior, which is taken from autograd of ``prior64`` on that stage alone.

``autograd_chunk`` is the same chunk under torch.autograd (the check of the sweep, tests/test_knet_bptt_ref.py).
``dtype`` switches everything between float64 and float32, as in _knet_ref.
"""
from __future__ import annotations

import torch

from tests import _knet_ref as R

MASKED = {"FC5": 0.05, "FC1": 0.05, "FC7": 0.05, "FC2": 0.1, "FC3": 0.05, "FC4": 0.05}   # layer -> dropout p
NOT_PHI = [0, 1, 3, 4, 5]


def mask_widths(w):
    return {"FC5": w["FC5.0.weight"].shape[0], "FC1": w["FC1.0.weight"].shape[0], "FC7": w["FC7.0.weight"].shape[0],
            "FC2": w["FC2.2.weight"].shape[0], "FC3": w["FC3.0.weight"].shape[0], "FC4": w["FC4.0.weight"].shape[0]}


def draw_masks(w, K, B, seed=0):
    """Explicit dropout masks {0, 1/(1-p)} as float32 tensors [K,B,width] per masked layer."""
    g = torch.Generator().manual_seed(seed)
    return {k: ((torch.rand((K, B, n), generator=g) >= MASKED[k]).float() / (1.0 - MASKED[k])).float()
            for k, n in mask_widths(w).items()}


def _w(weights, dtype):
    return {k: R._t(v, dtype) for k, v in weights.items()}


def chunk_loss(xo, xt, yt, x_mean, x_std, alpha):
    """pipeline.py:22-60 on [B,6,K] tensors (yt None: the plain state loss); differentiable."""
    d2 = (xo - xt) ** 2
    mse = d2[:, NOT_PHI, :].mean()
    s, m = x_std.reshape(-1)[2], x_mean.reshape(-1)[2]
    df = (xo[:, 2, :] * s + m) - (xt[:, 2, :] * s + m)
    ang = (torch.atan2(torch.sin(df), torch.cos(df)) ** 2).mean()
    lx = (5.0 / 6.0) * mse + (1.0 / 6.0) * ang
    if yt is None:
        return lx
    return alpha * lx + (1.0 - alpha) * ((xo[:, NOT_PHI, :] - yt) ** 2).mean()


def chunk_loss_grad(xo, xt, yt, x_mean, x_std, alpha):
    """(loss, d loss / d xo) by hand: the wrapped difference has derivative 1."""
    B, _, K = xo.shape
    n = B * K
    a = 1.0 if yt is None else alpha
    s, m = x_std.reshape(-1)[2], x_mean.reshape(-1)[2]
    df = (xo[:, 2, :] * s + m) - (xt[:, 2, :] * s + m)
    wr = torch.atan2(torch.sin(df), torch.cos(df))
    g = a * (xo - xt) / (3.0 * n)
    g[:, 2, :] = a * wr * s / (3.0 * n)
    if yt is not None:
        g[:, NOT_PHI, :] += (1.0 - alpha) * 2.0 * (xo[:, NOT_PHI, :] - yt) / (5.0 * n)
    return chunk_loss(xo, xt, yt, x_mean, x_std, alpha), g


def _step(w, params, Ts, y, u, post, hQ, hSig, hS, norm, mk, dtype):
    """One step (kalman_net.py:145-216) from the stage functions; mk: this step's masks or None.  Returns the tape
    slot: every layer's input, post-activation (``a*``, before the mask) and output."""
    x_mean, x_std, y_mean, y_std, u_mean, u_std = norm
    mm = (lambda k, a: a) if mk is None else (lambda k, a: a * R._t(mk[k], dtype))
    s = {"post_in": post, "hQ_in": hQ, "hSig_in": hSig, "hS_in": hS, "u": u, "y": y}
    s["prior"], _, s["dy"] = R.prior64(params, Ts, post, u, y, x_mean, x_std, y_mean, y_std, u_mean, u_std, dtype)
    s["a5"] = R.lin64(s["prior"], w["FC5.0.weight"], w["FC5.0.bias"], True, dtype)[0]
    s["o5"] = mm("FC5", s["a5"])
    s["giQ"] = R.lin64(s["o5"], w["GRU_Q.weight_ih_l0"], w["GRU_Q.bias_ih_l0"], False, dtype)[0]
    s["ghQ"] = R.lin64(hQ, w["GRU_Q.weight_hh_l0"], w["GRU_Q.bias_hh_l0"], False, dtype)[0]
    s["hQ"] = R.gru64(s["giQ"], s["ghQ"], hQ, dtype)
    s["giSig"] = R.lin64(s["hQ"], w["GRU_Sigma.weight_ih_l0"], w["GRU_Sigma.bias_ih_l0"], False, dtype)[0]
    s["ghSig"] = R.lin64(hSig, w["GRU_Sigma.weight_hh_l0"], w["GRU_Sigma.bias_hh_l0"], False, dtype)[0]
    s["oSig"] = R.gru64(s["giSig"], s["ghSig"], hSig, dtype)
    s["a1"] = R.lin64(s["oSig"], w["FC1.0.weight"], w["FC1.0.bias"], True, dtype)[0]
    s["a7"] = R.lin64(s["dy"], w["FC7.0.weight"], w["FC7.0.bias"], True, dtype)[0]
    s["xS"] = torch.cat((mm("FC1", s["a1"]), mm("FC7", s["a7"])), 1)
    s["giS"] = R.lin64(s["xS"], w["GRU_S.weight_ih_l0"], w["GRU_S.bias_ih_l0"], False, dtype)[0]
    s["ghS"] = R.lin64(hS, w["GRU_S.weight_hh_l0"], w["GRU_S.bias_hh_l0"], False, dtype)[0]
    s["hS"] = R.gru64(s["giS"], s["ghS"], hS, dtype)
    s["x2"] = torch.cat((s["oSig"], s["hS"]), 1)
    s["hid"] = R.lin64(s["x2"], w["FC2.0.weight"], w["FC2.0.bias"], True, dtype)[0]
    s["KG"] = mm("FC2", R.lin64(s["hid"], w["FC2.2.weight"], w["FC2.2.bias"], False, dtype)[0])
    s["x3"] = torch.cat((s["hS"], s["KG"]), 1)
    s["a3"] = R.lin64(s["x3"], w["FC3.0.weight"], w["FC3.0.bias"], True, dtype)[0]
    s["x4"] = torch.cat((s["oSig"], mm("FC3", s["a3"])), 1)
    s["a4"] = R.lin64(s["x4"], w["FC4.0.weight"], w["FC4.0.bias"], True, dtype)[0]
    s["hSig"] = mm("FC4", s["a4"])
    s["post"] = R.update64(s["prior"], s["KG"], s["dy"], w["innov_logit"], dtype)[0]
    return s


def forward_tape(weights, params, Ts, y_seq, u_seq, m1x0, norm, masks=None, hidden0=None, dtype=torch.float64, H=128):
    """K steps from (m1x0 [B,6], hidden0 = (hQ, hSig, hS) or zeros): the list of tape slots."""
    w = weights
    y_seq, u_seq = R._t(y_seq, dtype), R._t(u_seq, dtype)
    B, K = y_seq.shape[0], y_seq.shape[2]
    post = R._t(m1x0, dtype).reshape(B, 6)
    hQ, hSig, hS = (torch.zeros(B, H, dtype=dtype),) * 3 if hidden0 is None else (R._t(h, dtype) for h in hidden0)
    tape = []
    for t in range(K):
        mk = None if masks is None else {k: v[t] for k, v in masks.items()}
        s = _step(w, params, Ts, y_seq[:, :, t], u_seq[:, :, t], post, hQ, hSig, hS, norm, mk, dtype)
        post, hQ, hSig, hS = s["post"], s["hQ"], s["hSig"], s["hS"]
        tape.append(s)
    return tape


def _gru_bwd(gi, gh, h, g):
    H = h.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    dan = g * (1 - z) * (1 - n * n)
    dar = dan * gh[:, 2 * H:] * r * (1 - r)
    daz = g * (h - n) * z * (1 - z)
    return torch.cat((dar, daz, dan), 1), torch.cat((dar, daz, dan * r), 1), g * z


def _prior_bwd(params, Ts, s, norm, g_prior, g_dy, dtype):
    x_mean, x_std, y_mean, y_std, u_mean, u_std = norm
    with torch.enable_grad():
        xp = s["post_in"].detach().clone().requires_grad_(True)
        prior, _, dy = R.prior64(params, Ts, xp, s["u"], s["y"], x_mean, x_std, y_mean, y_std, u_mean, u_std, dtype)
        return torch.autograd.grad([prior, dy], [xp], [g_prior, g_dy])[0]


def sweep(weights, params, Ts, y_seq, u_seq, x_tgt, m1x0, norm, alpha=0.8, composite=True, masks=None, hidden0=None,
          g_extra=None, dtype=torch.float64, H=128):
    """One chunk by hand.  y_seq [B,5,K] normalized (also the composite loss's y target), u_seq [B,2,K], x_tgt [B,6,K]
    normalized, m1x0 [B,6]; norm = (x_mean, x_std, y_mean, y_std, u_mean, u_std); g_extra [B,6,K] is added to the
    loss gradient.  Returns {"loss", "grads": {state-dict name: gradient}, "g_x0" [B,6], "posts" [B,6,K], "tape"}."""
    w = _w(weights, dtype)
    tape = forward_tape(w, params, Ts, y_seq, u_seq, m1x0, norm, masks, hidden0, dtype, H)
    K, B = len(tape), tape[0]["prior"].shape[0]
    xo = torch.stack([s["post"] for s in tape], 2)
    yt = R._t(y_seq, dtype) if composite else None
    loss, gl = chunk_loss_grad(xo, R._t(x_tgt, dtype), yt, R._t(norm[0], dtype), R._t(norm[1], dtype), alpha)
    if g_extra is not None:
        gl = gl + R._t(g_extra, dtype)
    mk = (lambda k, t: 1.0) if masks is None else (lambda k, t: R._t(masks[k][t], dtype))
    gamma = torch.sigmoid(w["innov_logit"])
    gP = torch.zeros(B, 6, dtype=dtype)
    gHQ, gHSig, gHS = (torch.zeros(B, H, dtype=dtype) for _ in range(3))
    g_logit = torch.zeros(K, B, dtype=dtype)
    for t in range(K - 1, -1, -1):
        s = tape[t]
        # 1. update: post = prior + gamma KG dy
        g = gl[:, :, t] + gP
        KG = s["KG"].reshape(B, 6, 5)
        g_prior = g
        g_KG = (gamma * g.unsqueeze(2) * s["dy"].unsqueeze(1)).reshape(B, 30)
        g_dy = gamma * (g.unsqueeze(2) * KG).sum(1)
        g_logit[t] = gamma * (1 - gamma) * (g * (KG * s["dy"].unsqueeze(1)).sum(2)).sum(1)
        # 2. FC4 (its output is the next step's h_Sigma)
        s["d4"] = gHSig * mk("FC4", t) * (s["a4"] > 0)
        g_x4 = s["d4"] @ w["FC4.0.weight"]
        # 3. FC3
        s["d3"] = g_x4[:, H:] * mk("FC3", t) * (s["a3"] > 0)
        g_x3 = s["d3"] @ w["FC3.0.weight"]
        # 4. FC2: two products and the ReLU mask
        s["dkg"] = (g_KG + g_x3[:, H:]) * mk("FC2", t)
        s["dhid"] = (s["dkg"] @ w["FC2.2.weight"]) * (s["hid"] > 0)
        g_x2 = s["dhid"] @ w["FC2.0.weight"]
        # 5. GRU_S
        s["dgiS"], s["dghS"], gh_direct = _gru_bwd(s["giS"], s["ghS"], s["hS_in"], g_x3[:, :H] + g_x2[:, H:] + gHS)
        gHS = gh_direct + s["dghS"] @ w["GRU_S.weight_hh_l0"]
        g_xS = s["dgiS"] @ w["GRU_S.weight_ih_l0"]
        # 6. FC7 and FC1
        n1 = s["a1"].shape[1]
        s["d1"] = g_xS[:, :n1] * mk("FC1", t) * (s["a1"] > 0)
        s["d7"] = g_xS[:, n1:] * mk("FC7", t) * (s["a7"] > 0)
        g_dy = g_dy + s["d7"] @ w["FC7.0.weight"]
        g_oSig = g_x2[:, :H] + s["d1"] @ w["FC1.0.weight"] + g_x4[:, :H]
        # 7. GRU_Sigma
        s["dgiSig"], s["dghSig"], gh_direct = _gru_bwd(s["giSig"], s["ghSig"], s["hSig_in"], g_oSig)
        gHSig = gh_direct + s["dghSig"] @ w["GRU_Sigma.weight_hh_l0"]
        # 8. GRU_Q
        s["dgiQ"], s["dghQ"], gh_direct = _gru_bwd(s["giQ"], s["ghQ"], s["hQ_in"],
                                                   s["dgiSig"] @ w["GRU_Sigma.weight_ih_l0"] + gHQ)
        gHQ = gh_direct + s["dghQ"] @ w["GRU_Q.weight_hh_l0"]
        # 9. FC5
        s["d5"] = (s["dgiQ"] @ w["GRU_Q.weight_ih_l0"]) * mk("FC5", t) * (s["a5"] > 0)
        g_prior = g_prior + s["d5"] @ w["FC5.0.weight"]
        # 10. prior
        gP = _prior_bwd(params, Ts, s, norm, g_prior, g_dy, dtype)
    # deferred weight gradients: one product per layer over the K B rows of the tape
    rows = lambda k: torch.cat([s[k] for s in tape], 0)   # noqa: E731
    G = {"innov_logit": g_logit.sum()}
    for name, d, x in (("FC5.0", "d5", "prior"), ("FC1.0", "d1", "oSig"), ("FC7.0", "d7", "dy"), ("FC2.0", "dhid", "x2"),
                       ("FC2.2", "dkg", "hid"), ("FC3.0", "d3", "x3"), ("FC4.0", "d4", "x4")):
        D = rows(d)
        G[name + ".weight"], G[name + ".bias"] = D.t() @ rows(x), D.sum(0)
    for name, q, x in (("GRU_Q", "Q", "o5"), ("GRU_Sigma", "Sig", "hQ"), ("GRU_S", "S", "xS")):
        Di, Dh = rows("dgi" + q), rows("dgh" + q)
        G[name + ".weight_ih_l0"], G[name + ".bias_ih_l0"] = Di.t() @ rows(x), Di.sum(0)
        G[name + ".weight_hh_l0"], G[name + ".bias_hh_l0"] = Dh.t() @ rows(f"h{q}_in"), Dh.sum(0)
    return {"loss": loss, "grads": G, "g_x0": gP, "posts": xo, "tape": tape}


def autograd_chunk(weights, params, Ts, y_seq, u_seq, x_tgt, m1x0, norm, alpha=0.8, composite=True, masks=None,
                   hidden0=None, g_extra=None, dtype=torch.float64, H=128):
    """The same chunk differentiated by torch.autograd: {"loss", "grads", "g_x0"}."""
    w = {k: v.detach().clone().requires_grad_(True) for k, v in _w(weights, dtype).items()}
    x0 = R._t(m1x0, dtype).reshape(-1, 6).detach().clone().requires_grad_(True)
    tape = forward_tape(w, params, Ts, y_seq, u_seq, x0, norm, masks, hidden0, dtype, H)
    xo = torch.stack([s["post"] for s in tape], 2)
    yt = R._t(y_seq, dtype) if composite else None
    loss = chunk_loss(xo, R._t(x_tgt, dtype), yt, R._t(norm[0], dtype), R._t(norm[1], dtype), alpha)
    tot = loss if g_extra is None else loss + (xo * R._t(g_extra, dtype)).sum()
    tot.backward()
    return {"loss": loss.detach(), "grads": {k: v.grad for k, v in w.items()}, "g_x0": x0.grad}


def chunk_kink_distance(params, Ts, tape, norm):
    """Per sequence, the smallest kink distance (real units) of the prior's vehicle step over the chunk's steps."""
    x_mean, x_std, _, _, u_mean, u_std = norm
    d = [R.kink_distance(params, R.prior_terms(params, Ts, s["post_in"].detach(), s["u"], x_mean, x_std, u_mean, u_std))
         for s in tape]
    return torch.stack(d, 0).min(0).values

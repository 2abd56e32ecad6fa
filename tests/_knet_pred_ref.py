"""Float64 / float32 reference of the open-loop prediction loss of training -- TEST INFRASTRUCTURE ONLY (plain torch
on the CPU).

KalmanNet/pipeline_prediction.py:45-99 (_compute_step_loss_real, compute_prediction_loss) for every (sequence, window)
pair at once, on the vehicle step of tests/_knet_ref.py (``prior_terms``): window w of sequence b starts at
t = t0 + w * step from x_est[b, :, w], runs valid = max(0, min(H, T - 1 - t)) clamped Euler steps with
u[b, :, t + k - 1] and scores each against x_gt_norm[b, :, t + k] denormalized, phi as the wrapped difference:

    part[b, w] = sum_k sum_c e^2 / (6 valid)        (part[:, w].mean() is the reference's loss at that t)
    grad[b, :, w] = d part[b, w] / d x_est[b, :, w]  (torch autograd of these expressions)

``dtype`` switches the whole evaluation between float64 (what the kernel is held to) and float32 (the same
expressions in the reference's own precision; its distance to float64 is the error a correct float32 implementation
makes on those inputs).
"""
from __future__ import annotations

import torch

from tests import _knet_ref as R


def _kink(params, terms, first):
    """kink_distance of tests/_knet_ref.py for one rollout step.  After the first step a pre-clamp input that sits
    exactly on its limit got there through the previous step's saturated post-clamp, whose zero derivative makes the
    gradient independent of the pre-clamp's convention at the limit: it does not count."""
    p, x, raw = params, terms["x"], terms["xn_raw"]
    inf = torch.full_like(x[:, 0], float("inf"))
    d = []
    for i, (lo, hi) in enumerate(R.LIMIT_PAIRS):
        if i >= 2:
            for lim in (p[lo], p[hi]):
                dist = (x[:, i] - lim).abs()
                d.append(dist if first else torch.where(x[:, i] == lim, inf, dist))
        d += [(raw[:, i] - p[lo]).abs(), (raw[:, i] - p[hi]).abs()]
    d += [(terms["vx"].abs() - p["vx_zero"]).abs(), (terms["alpha_f_raw"].abs() - p["maxAlpha"]).abs()]
    return torch.stack(d, 1).min(1).values


def window_loss(params, Ts, x_est, t0, step, u, x_gt_norm, H, x_mean, x_std, u_mean=None, u_std=None,
                dtype=torch.float64, want_grad=True):
    """x_est [B,6,nwin] normalized (indexed by window), u [B,2,T], x_gt_norm [B,6,T] -> dict with ``part`` [B,nwin],
    ``grad`` [B,6,nwin] (None without want_grad), ``valid`` [nwin] and ``kink`` [B,nwin]: the smallest distance (real
    units) of any clamped quantity of the window's rollout to its kink (inf for a window of no steps)."""
    xe = R._t(x_est, dtype).detach().clone().requires_grad_(want_grad)
    u, xg = R._t(u, dtype), R._t(x_gt_norm, dtype)
    B, _, nwin = xe.shape
    T = u.shape[2]
    xm, xs = R._t(x_mean, dtype, 6), R._t(x_std, dtype, 6)
    zero6, one6 = torch.zeros(6, dtype=dtype), torch.ones(6, dtype=dtype)
    ts = t0 + step * torch.arange(nwin)                                    # [nwin]
    valid = (T - 1 - ts).clamp(0, H)
    tw = ts.repeat(B)                                                      # window (b, w) -> row b * nwin + w
    vw = valid.repeat(B)
    bw = torch.arange(B).repeat_interleave(nwin)
    x = xe.permute(0, 2, 1).reshape(B * nwin, 6) * xs + xm                 # _denorm_x
    total = torch.zeros(B * nwin, dtype=dtype)
    kink = torch.full((B * nwin,), float("inf"), dtype=torch.float64)
    for k in range(1, int(valid.max().item()) + 1 if nwin else 1):
        act = vw >= k
        iu = (tw + k - 1).clamp(max=T - 1)
        ig = (tw + k).clamp(max=T - 1)
        terms = R.prior_terms(params, Ts, x, u[bw, :, iu], zero6, one6, u_mean, u_std, dtype)
        tgt = xg[bw, :, ig] * xs + xm
        diff = terms["xn"] - tgt
        dphi = torch.atan2(torch.sin(diff[:, 2]), torch.cos(diff[:, 2]))
        sq = torch.cat((diff[:, :2] ** 2, (dphi ** 2).unsqueeze(1), diff[:, 3:] ** 2), 1)
        total = total + torch.where(act, sq.sum(1), torch.zeros_like(total))
        with torch.no_grad():
            kd = _kink(params, {k_: v.detach().double() for k_, v in terms.items()}, k == 1)
            kink = torch.where(act, torch.minimum(kink, kd), kink)
        x = torch.where(act.unsqueeze(1), terms["xn"], x)
    part = torch.where(vw > 0, total / (6 * vw.clamp(min=1)).to(dtype), torch.zeros_like(total))
    grad = None
    if want_grad:
        if part.requires_grad:
            grad, = torch.autograd.grad(part.sum(), xe, allow_unused=True)
        grad = torch.zeros_like(xe) if grad is None else grad
        grad = grad.detach()
    return {"part": part.detach().reshape(B, nwin), "grad": grad, "valid": valid, "kink": kink.reshape(B, nwin)}


# ------------------------------------------------------------------ test inputs

def golden_case(G, GP, H, unorm=False):
    """The golden data's windows: every t < T - 1 of the B = 4 x T = 20 sequences (4 x 19 windows, the last H - 1 of
    each sequence truncated), from the reference filter's posteriors."""
    T = GP["x_est"].shape[2]
    return {"x_est": torch.tensor(GP["x_est"][:, :, :T - 1]), "t0": 0, "step": 1, "H": H,
            "u": torch.tensor(GP["u_norm"] if unorm else G["u"], dtype=torch.float32),
            "x_gt_norm": torch.tensor(GP["x_norm"]), "x_mean": torch.tensor(G["x_mean"]).reshape(6),
            "x_std": torch.tensor(G["x_std"]).reshape(6),
            "u_mean": torch.tensor(GP["u_mean"]).reshape(2) if unorm else None,
            "u_std": torch.tensor(GP["u_std"]).reshape(2) if unorm else None}


def rows_case(x_post, u, H, x_mean, x_std, seed):
    """One window per row of single-step inputs (tests/_knet_ref.py's builders): x_post [B,6] the start states, the
    row's control held for the H steps, seeded normal targets (T = H + 1)."""
    B = x_post.shape[0]
    g = torch.Generator().manual_seed(seed)
    return {"x_est": x_post.reshape(B, 6, 1).clone(), "t0": 0, "step": 1, "H": H,
            "u": u.reshape(B, 2, 1).repeat(1, 1, H + 1).contiguous(),
            "x_gt_norm": torch.randn((B, 6, H + 1), generator=g),
            "x_mean": torch.as_tensor(x_mean).reshape(6).float(), "x_std": torch.as_tensor(x_std).reshape(6).float(),
            "u_mean": None, "u_std": None}


def case_loss(params, Ts, c, dtype=torch.float64, want_grad=True):
    return window_loss(params, Ts, c["x_est"], c["t0"], c["step"], c["u"], c["x_gt_norm"], c["H"], c["x_mean"],
                       c["x_std"], c["u_mean"], c["u_std"], dtype, want_grad)

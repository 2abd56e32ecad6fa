"""Float64, stage-wise reference of one KalmanNet step -- TEST INFRASTRUCTURE ONLY (plain torch on the CPU).

The expressions of KalmanNet/vehicle_model.py:19-79,109-153 (pt_tire_forces / pt_f_cont / f / h) and
KalmanNet/kalman_net.py:138-216 (_denorm_u, step_prior, KGain_step, KNet_step; eval mode) written so that every
stage can be evaluated on its own from any upstream values.  ``dtype`` switches the whole evaluation between
float64 (the reference the kernels are held to) and float32 (the same expressions in the reference's own precision:
with it a loop of ``step64`` reproduces oracle/knet_oracle.py, and the distance between the two evaluations is the
error a correct float32 implementation makes on those inputs).

Every dense stage returns, beside its value, its abs-sum scale |b| + |W| |x| -- the size of the terms a float32
dot product rounds, as tests/test_knet_fc2.py builds it.  A stage fed by another dense stage takes that stage's
scale in place of |x| (``xscale``), so the scale of a chain is the abs-sum of the whole chain.

The second half of the file builds test inputs: prior inputs that visit every branch of the vehicle model, and
prior inputs placed a known distance away from every kink for gradient checks.
"""
from __future__ import annotations

import numpy as np
import torch

PARAMS = {"Cm1": 0.287, "Cm2": 0.0545, "Cr0": 0.0518, "Cr2": 0.00035, "Br": 3.3852, "Cr": 1.2691, "Dr": 0.1737,
          "Bf": 2.579, "Cf": 1.2, "Df": 0.192, "m": 0.041, "Iz": 27.8e-6, "lf": 0.029, "lr": 0.033, "g": 9.81,
          "maxAlpha": 0.6, "vx_zero": 0.3}
LIMIT_PAIRS = (("x_min", "x_max"), ("y_min", "y_max"), ("phi_min", "phi_max"), ("vx_min", "vx_max"),
               ("vy_min", "vy_max"), ("omega_min", "omega_max"))
H_ROWS = [0, 1, 3, 4, 5]


def _t(a, dtype, cols=None):
    """Any array / tensor -> CPU tensor of ``dtype`` (a float32 input is widened exactly; autograd history is kept),
    optionally [1, cols]."""
    t = a.cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    t = t.to(dtype)
    return t if cols is None else t.reshape(1, cols)


# ------------------------------------------------------------------ prior (kalman_net.py:145-162)

def prior_terms(params, Ts, x_post, u, x_mean, x_std, u_mean=None, u_std=None, dtype=torch.float64):
    """The vehicle step of the prior with its intermediate values (all [B] or [B,6], real units):
    x (denormalized state), u (denormalized controls), alpha_f_raw (before its clamp), vx (pre-clamped),
    xn_raw (Euler step before the clamp), xn (after it)."""
    p = params
    x = _t(x_post, dtype).reshape(-1, 6) * _t(x_std, dtype, 6) + _t(x_mean, dtype, 6)        # _denorm_x
    uu = _t(u, dtype).reshape(-1, 2)
    if u_mean is not None and u_std is not None:                                             # _denorm_u
        uu = uu * _t(u_std, dtype, 2) + _t(u_mean, dtype, 2)
    phi = torch.clamp(x[:, 2], p["phi_min"], p["phi_max"])                                   # pt_f_cont (:45-79)
    vx = torch.clamp(x[:, 3], p["vx_min"], p["vx_max"])
    vy = torch.clamp(x[:, 4], p["vy_min"], p["vy_max"])
    om = torch.clamp(x[:, 5], p["omega_min"], p["omega_max"])
    d, de = uu[:, 0], uu[:, 1]
    vx_eff = torch.maximum(vx.abs(), torch.full_like(vx, p["vx_zero"]))                      # pt_tire_forces (:19-42)
    af_raw = -torch.atan2(om * p["lf"] + vy, vx_eff) + de
    ar = torch.atan2(om * p["lr"] - vy, vx_eff)
    af = torch.clamp(af_raw, -p["maxAlpha"], p["maxAlpha"])
    Fyf = p["Df"] * torch.sin(p["Cf"] * torch.atan(p["Bf"] * af))
    Fyr = p["Dr"] * torch.sin(p["Cr"] * torch.atan(p["Br"] * ar))
    Frx = (p["Cm1"] - p["Cm2"] * vx_eff) * d - p["Cr0"] - p["Cr2"] * (vx_eff * vx_eff)
    xdot = torch.stack([vx * torch.cos(phi) - vy * torch.sin(phi), vx * torch.sin(phi) + vy * torch.cos(phi), om,
                        (Frx - Fyf * torch.sin(de) + p["m"] * vy * om) / p["m"],
                        (Fyr + Fyf * torch.cos(de) - p["m"] * vx * om) / p["m"],
                        (Fyf * p["lf"] * torch.cos(de) - Fyr * p["lr"]) / p["Iz"]], 1)
    xn_raw = x + Ts * xdot                                                                   # f (:109-134)
    xn = torch.stack([torch.clamp(xn_raw[:, i], p[lo], p[hi]) for i, (lo, hi) in enumerate(LIMIT_PAIRS)], 1)
    return {"x": x, "u": uu, "vx": vx, "alpha_f_raw": af_raw, "xn_raw": xn_raw, "xn": xn}


def prior64(params, Ts, x_post, u, y, x_mean, x_std, y_mean, y_std, u_mean=None, u_std=None, dtype=torch.float64):
    """x_post [B,6] normalized, u [B,2], y [B,5] normalized -> (prior [B,6], m1y [B,5], dy [B,5]), normalized."""
    xn = prior_terms(params, Ts, x_post, u, x_mean, x_std, u_mean, u_std, dtype)["xn"]
    prior = (xn - _t(x_mean, dtype, 6)) / _t(x_std, dtype, 6)                                 # _renorm_x
    m1y = (xn[:, H_ROWS] - _t(y_mean, dtype, 5)) / _t(y_std, dtype, 5)                        # h, _renorm_y
    return prior, m1y, _t(y, dtype).reshape(-1, 5) - m1y


# ------------------------------------------------------------------ network stages (kalman_net.py:180-212)

def lin64(x, W, b, relu=True, dtype=torch.float64, xscale=None):
    """Linear (+ ReLU): returns (value, scale) with scale = |b| + xscale |W|', xscale = |x| unless the input is itself
    a dense stage's output (then that stage's scale)."""
    x, W, b = _t(x, dtype), _t(W, dtype), _t(b, dtype)
    y = x @ W.t() + b
    xs = x.abs() if xscale is None else _t(xscale, dtype)
    scale = xs @ W.abs().t() + b.abs()
    return (torch.relu(y) if relu else y), scale


def gru64(gi, gh, h, dtype=torch.float64):
    """torch.nn.GRU's gate arithmetic (r, z, n order) on the two pre-activations gi, gh [B,3H] and h [B,H]."""
    gi, gh, h = _t(gi, dtype), _t(gh, dtype), _t(h, dtype)
    H = h.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def gru_cell64(x, h, w, name, dtype=torch.float64, xscale=None):
    """One step of the 1-layer GRU ``name`` of the state dict ``w``: returns (h', scale) with
    scale = 1 + |h| + the abs-sum scales of the i_n and h_n pre-activations."""
    gi, si = lin64(x, w[f"{name}.weight_ih_l0"], w[f"{name}.bias_ih_l0"], False, dtype, xscale)
    gh, sh = lin64(h, w[f"{name}.weight_hh_l0"], w[f"{name}.bias_hh_l0"], False, dtype)
    hp = _t(h, dtype)
    H = hp.shape[1]
    return gru64(gi, gh, hp, dtype), 1 + hp.abs() + si[:, 2 * H:] + sh[:, 2 * H:]


def update64(prior, KG, dy, logit, dtype=torch.float64):
    """kalman_net.py:169-178: returns (post, scale), post = prior + sigmoid(logit) KG dy and
    scale = |prior| + sigmoid(logit) sum_j |KG_ij dy_j|."""
    prior, dy = _t(prior, dtype), _t(dy, dtype)
    B, m = prior.shape
    n = dy.shape[1]
    KG = _t(KG, dtype).reshape(B, m, n)
    gamma = torch.sigmoid(_t(logit, dtype))
    post = prior + gamma * torch.bmm(KG, dy.unsqueeze(2)).squeeze(2)
    return post, prior.abs() + gamma * (KG * dy.unsqueeze(1)).abs().sum(2)


def fc2_64(x2, w, dtype=torch.float64):
    """FC2 = Linear(2H, dH) -> ReLU -> Linear(dH, n m): returns (KG [B, n m], scale)."""
    hid, s1 = lin64(x2, w["FC2.0.weight"], w["FC2.0.bias"], True, dtype)
    return lin64(hid, w["FC2.2.weight"], w["FC2.2.bias"], False, dtype, xscale=s1)


def back64(x2, KG, w, dtype=torch.float64):
    """FC3 on cat(h_S, KG), FC4 on cat(out_Sigma, FC3) = the new h_Sigma: returns (o3, hSig, scale of hSig)."""
    x2, KG = _t(x2, dtype), _t(KG, dtype)
    H = x2.shape[1] // 2
    o3, s3 = lin64(torch.cat((x2[:, H:], KG), 1), w["FC3.0.weight"], w["FC3.0.bias"], True, dtype)
    hSig, s4 = lin64(torch.cat((x2[:, :H], o3), 1), w["FC4.0.weight"], w["FC4.0.bias"], True, dtype,
                     xscale=torch.cat((x2[:, :H].abs(), s3), 1))
    return o3, hSig, s4


def step64(weights, params, Ts, y, u, x_post, hQ, hSig, hS, x_mean, x_std, y_mean, y_std, u_mean=None, u_std=None,
           dtype=torch.float64):
    """One whole eval-mode step from (x_post, hQ, hSig, hS).  Returns a dict of every intermediate -- prior, m1y, dy,
    o5, hQ, oSig, o1, o7, hS, KG, o3, hSig, post -- and under "scale" the abs-sum scale of each network stage."""
    w = weights
    prior, m1y, dy = prior64(params, Ts, x_post, u, y, x_mean, x_std, y_mean, y_std, u_mean, u_std, dtype)
    o5, s5 = lin64(prior, w["FC5.0.weight"], w["FC5.0.bias"], True, dtype)
    hQn, sQ = gru_cell64(o5, hQ, w, "GRU_Q", dtype, xscale=s5)
    oSig, sG = gru_cell64(hQn, hSig, w, "GRU_Sigma", dtype)
    o1, s1 = lin64(oSig, w["FC1.0.weight"], w["FC1.0.bias"], True, dtype)
    o7, s7 = lin64(dy, w["FC7.0.weight"], w["FC7.0.bias"], True, dtype)
    hSn, sS = gru_cell64(torch.cat((o1, o7), 1), hS, w, "GRU_S", dtype, xscale=torch.cat((s1, s7), 1))
    x2 = torch.cat((oSig, hSn), 1)
    KG, s2 = fc2_64(x2, w, dtype)
    o3, hSign, s4 = back64(x2, KG, w, dtype)
    post, sP = update64(prior, KG, dy, w["innov_logit"], dtype)
    return {"prior": prior, "m1y": m1y, "dy": dy, "o5": o5, "hQ": hQn, "oSig": oSig, "o1": o1, "o7": o7, "hS": hSn,
            "KG": KG, "o3": o3, "hSig": hSign, "post": post,
            "scale": {"o5": s5, "hQ": sQ, "oSig": sG, "o1": s1, "o7": s7, "hS": sS, "KG": s2, "hSig": s4, "post": sP}}


def run64(weights, params, Ts, y_seq, u_seq, m1x0, x_mean, x_std, y_mean, y_std, u_mean=None, u_std=None,
          dtype=torch.float64, hidden=128):
    """T steps of step64 from zero hidden states: y_seq [B,5,T], u_seq [B,2,T], m1x0 [B,6,1] ->
    (post [B,6,T], prior [B,6,T], KG [B,6,5,T])."""
    y_seq, u_seq = _t(y_seq, dtype), _t(u_seq, dtype)
    B, T = y_seq.shape[0], y_seq.shape[2]
    post = _t(m1x0, dtype).reshape(B, 6)
    hQ = hSig = hS = torch.zeros(B, hidden, dtype=dtype)
    posts, priors, kgs = [], [], []
    for t in range(T):
        s = step64(weights, params, Ts, y_seq[:, :, t], u_seq[:, :, t], post, hQ, hSig, hS, x_mean, x_std, y_mean,
                   y_std, u_mean, u_std, dtype)
        post, hQ, hSig, hS = s["post"], s["hQ"], s["hSig"], s["hS"]
        posts.append(post)
        priors.append(s["prior"])
        kgs.append(s["KG"].reshape(B, 6, 5))
    return torch.stack(posts, 2), torch.stack(priors, 2), torch.stack(kgs, 3)


# ------------------------------------------------------------------ test inputs

def branch_inputs(B, x_mean, x_std, seed=0, u_mean=None, u_std=None):
    """Prior inputs drawn like phys_x / phys_u of tests/golden/gen_knet_golden.py (real units), normalized with the
    given statistics and rounded to float32: x_post [B,6], u [B,2] (normalized when u statistics are given)."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-2, 30, B), rng.uniform(-3, 3, B), rng.uniform(-4, 4, B), rng.uniform(-0.5, 3.5, B),
                  rng.uniform(-1.5, 1.5, B), rng.uniform(-8, 8, B)], 1)
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.6, 0.6, B)], 1)
    e = B // 8
    x[:e, 0] = rng.uniform(-8, -5.5, e)              # X below x_min / above x_max: the draw above never leaves
    x[e:2 * e, 0] = rng.uniform(40.5, 44, e)         # [x_min, x_max]
    x[2 * e:3 * e, 1] = rng.uniform(-8, -6.2, e)     # Y likewise
    x[3 * e:4 * e, 1] = rng.uniform(6.2, 8, e)
    xm, xs = np.asarray(x_mean, np.float64).reshape(1, 6), np.asarray(x_std, np.float64).reshape(1, 6)
    xp = ((x - xm) / xs).astype(np.float32)
    if u_mean is not None:
        u = (u - np.asarray(u_mean, np.float64).reshape(1, 2)) / np.asarray(u_std, np.float64).reshape(1, 2)
    return torch.tensor(xp), torch.tensor(u.astype(np.float32))


def branch_hits(params, terms):
    """Which branches of the vehicle step the rows of ``terms`` (prior_terms, float64) take: name -> rows [B] bool."""
    p, x, raw = params, terms["x"], terms["xn_raw"]
    hits = {}
    for i, (lo, hi) in enumerate(LIMIT_PAIRS):
        if i >= 2:   # phi, vx, vy, omega are clamped before the tire model
            hits[f"pre_{lo}"], hits[f"pre_{hi}"] = x[:, i] < p[lo], x[:, i] > p[hi]
        hits[f"post_{lo}"], hits[f"post_{hi}"] = raw[:, i] < p[lo], raw[:, i] > p[hi]
        hits[f"post_{lo[:-4]}_inside"] = (raw[:, i] > p[lo]) & (raw[:, i] < p[hi])
    hits["vx_zero_floor"] = terms["vx"].abs() < p["vx_zero"]
    hits["vx_zero_above"] = terms["vx"].abs() > p["vx_zero"]
    hits["alpha_lo"] = terms["alpha_f_raw"] < -p["maxAlpha"]
    hits["alpha_hi"] = terms["alpha_f_raw"] > p["maxAlpha"]
    hits["alpha_inside"] = terms["alpha_f_raw"].abs() < p["maxAlpha"]
    return hits


def kink_distance(params, terms):
    """Per row, the smallest distance (real units, float64) of any clamped quantity of the vehicle step to its kink:
    the twelve limits before and after the Euler step, |vx| = vx_zero and |alpha_f| = maxAlpha."""
    p, x, raw = params, terms["x"], terms["xn_raw"]
    d = []
    for i, (lo, hi) in enumerate(LIMIT_PAIRS):
        if i >= 2:
            d += [(x[:, i] - p[lo]).abs(), (x[:, i] - p[hi]).abs()]
        d += [(raw[:, i] - p[lo]).abs(), (raw[:, i] - p[hi]).abs()]
    d += [(terms["vx"].abs() - p["vx_zero"]).abs(), (terms["alpha_f_raw"].abs() - p["maxAlpha"]).abs()]
    return torch.stack(d, 1).min(1).values


def smooth_inputs(params, x_mean, x_std, seed=0, u_mean=None, u_std=None, B=64):
    """Prior inputs for gradient checks, every row well away from every kink (kink_distance).  Rows [0, B/2) lie
    inside all limits -- the first quarter on the plain branch, then an eighth each on the vx_zero floor and on the
    alpha_f clamp; rows [B/2, 3B/4) have every state beyond its limit by more than one Euler step can recover (the
    whole Jacobian is zero); rows [3B/4, B) have vx, vy and omega beyond their limits and X, Y, phi inside.
    The steering angle is chosen from the wanted alpha_f, delta = alpha_f + atan2(omega lf + vy, vx_eff).
    Returns float32 x_post [B,6], u [B,2] (normalized when u statistics are given)."""
    p = params
    rng = np.random.default_rng(seed)
    q, h = B // 4, B // 2
    sgn = lambda n: rng.choice([-1.0, 1.0], n)   # noqa: E731
    x = np.stack([rng.uniform(0, 30, B), rng.uniform(-3, 3, B), rng.uniform(-2, 2, B), rng.uniform(0.6, 2.4, B),
                  rng.uniform(-0.4, 0.4, B), rng.uniform(-1.5, 1.5, B)], 1)
    alpha = rng.uniform(-0.5, 0.5, B)
    x[q:q + q // 2, 3] = rng.uniform(0.12, 0.28, q // 2)                    # |vx| below vx_zero, inside the limits
    alpha[q + q // 2:h] = sgn(q - q // 2) * rng.uniform(0.65, 0.8, q - q // 2)   # alpha_f clamped
    lo = np.array([p[a] for a, _ in LIMIT_PAIRS])
    hi = np.array([p[b] for _, b in LIMIT_PAIRS])
    margin = np.array([1.0, 0.5, 0.3, 0.5, 0.6, 6.0])   # above one Euler step's reach from the clamped state
    for r in range(h, B):
        cols = range(6) if r < h + q else (3, 4, 5)
        for i in cols:
            over = margin[i] * rng.uniform(1.0, 1.5)
            x[r, i] = hi[i] + over if rng.random() < 0.5 else lo[i] - over
    alpha[h:] = rng.uniform(-0.5, 0.5, B - h)
    vx = np.clip(x[:, 3], lo[3], hi[3])
    vy = np.clip(x[:, 4], lo[4], hi[4])
    om = np.clip(x[:, 5], lo[5], hi[5])
    delta = alpha + np.arctan2(om * p["lf"] + vy, np.maximum(np.abs(vx), p["vx_zero"]))
    u = np.stack([rng.uniform(0.0, 0.5, B), delta], 1)
    xm, xs = np.asarray(x_mean, np.float64).reshape(1, 6), np.asarray(x_std, np.float64).reshape(1, 6)
    xp = ((x - xm) / xs).astype(np.float32)
    if u_mean is not None:
        u = (u - np.asarray(u_mean, np.float64).reshape(1, 2)) / np.asarray(u_std, np.float64).reshape(1, 2)
    return torch.tensor(xp), torch.tensor(u.astype(np.float32))

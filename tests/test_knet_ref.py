"""The float64 stage-wise KalmanNet reference (tests/_knet_ref.py) pinned on the CPU: in float32 it is the oracle
(oracle/knet_oracle.py), in float64 it matches the reference module's three goldens (control normalization
included), its test-input builders do what the GPU tests rely on (every branch visited; every gradient row away from
every kink), and the float32 evaluation of the same expressions meets the bars the GPU tests hold the kernels to
with at least 2x room -- so those bars are met by a correct float32 implementation, not tuned to the kernels."""
import numpy as np
import pytest
import torch

from oracle import knet_oracle as KO
from tests import _knet_ref as R
from tests._knet_weights import LIMITS, knet_weights

G = np.load("tests/golden/knet.npz")
GU = np.load("tests/golden/knet_b9_t12_unorm.npz")


def params():
    p = dict(R.PARAMS)
    p.update(LIMITS)
    return p


def _weights(g):
    return {k: torch.tensor(v) for k, v in knet_weights(seed=int(g["seed"]), in_mult=int(g["in_mult"])).items()}


def _ustats(g):
    return (g["u_mean"], g["u_std"]) if "u_mean" in g.files else (None, None)


def test_params_are_the_oracles():
    assert R.PARAMS == KO.PARAMS


def test_float32_loop_reproduces_the_oracle():
    w = _weights(G)
    out = KO.run_sequences(w, params(), float(G["Ts"]), G["y_norm"], G["u"], G["m1x0"], G["x_mean"], G["x_std"],
                           G["y_mean"], G["y_std"])
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32)   # noqa: E731
    post, _, _ = R.run64(w, params(), float(G["Ts"]), f32(G["y_norm"]), f32(G["u"]), f32(G["m1x0"]), f32(G["x_mean"]),
                         f32(G["x_std"]), f32(G["y_mean"]), f32(G["y_std"]), dtype=torch.float32)
    assert post.dtype == torch.float32
    err = (post - out).abs().max().item()
    assert err <= 1e-6 * out.abs().max().item(), err


@pytest.mark.parametrize("name", ["knet.npz", "knet_b37_t60_im10.npz", "knet_b9_t12_unorm.npz"])
def test_float64_loop_matches_reference_goldens(name):
    g = np.load("tests/golden/" + name)
    um, us = _ustats(g)
    post, prior, kg = R.run64(_weights(g), params(), float(g["Ts"]), g["y_norm"], g["u"], g["m1x0"], g["x_mean"],
                              g["x_std"], g["y_mean"], g["y_std"], um, us)
    assert post.dtype == torch.float64
    for got, key in ((post, "x_post"), (prior, "x_prior"), (kg, "KG")):
        ref = g[key]
        err = np.abs(got.numpy() - ref).max()
        assert err <= 2e-5 * (1 + np.abs(ref).max()), (key, err)


def test_unorm_golden_really_normalizes_controls():
    """The golden's u is the normalized control; ignoring the statistics (feeding it as a real control) misses the
    golden by far more than the bar, so the u_mean / u_std path is what the golden pins."""
    g = GU
    np.testing.assert_allclose(g["u"] * g["u_std"] + g["u_mean"], g["u_real"], atol=1e-12)
    assert g["u_mean"].shape == (1, 2, 1) and g["u_std"].shape == (1, 2, 1)
    post, _, _ = R.run64(_weights(g), params(), float(g["Ts"]), g["y_norm"], g["u"], g["m1x0"], g["x_mean"],
                         g["x_std"], g["y_mean"], g["y_std"])
    assert np.abs(post.numpy() - g["x_post"]).max() > 100 * 2e-5 * (1 + np.abs(g["x_post"]).max())


def test_stage_scales_bound_the_stages():
    """Each abs-sum scale bounds its stage's value (|b + W x| <= |b| + |W| |x|), chained stages included."""
    w = _weights(G)
    rng = np.random.default_rng(0)
    B = 5
    f = lambda *s: torch.tensor(rng.normal(size=s) * 0.5)   # noqa: E731
    s = R.step64(w, params(), 0.01, f(B, 5), f(B, 2) * 0.3, f(B, 6), f(B, 128), f(B, 128), f(B, 128), G["x_mean"],
                 G["x_std"], G["y_mean"], G["y_std"])
    for k in ("o5", "o1", "o7", "KG", "hSig", "post"):
        assert (s[k].abs() <= s["scale"][k] * (1 + 1e-12)).all(), k
    for k in ("hQ", "oSig", "hS"):
        assert (s["scale"][k] >= 1).all() and s[k].shape == s["scale"][k].shape
    assert s["KG"].shape == (B, 30) and s["o3"].shape == (B, 36)


@pytest.mark.parametrize("unorm", [False, True])
def test_branch_inputs_visit_every_branch(unorm):
    um, us = _ustats(GU) if unorm else (None, None)
    xp, u = R.branch_inputs(261, G["x_mean"], G["x_std"], seed=1, u_mean=um, u_std=us)
    f32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32)   # noqa: E731
    terms = R.prior_terms(params(), float(G["Ts"]), xp, u, f32(G["x_mean"]), f32(G["x_std"]), f32(um), f32(us))
    hits = R.branch_hits(params(), terms)
    assert len(hits) == 8 + 12 + 6 + 5
    assert all(v.any() for v in hits.values()), [k for k, v in hits.items() if not v.any()]


@pytest.mark.parametrize("unorm", [False, True])
def test_smooth_inputs_keep_away_from_kinks(unorm):
    um, us = _ustats(GU) if unorm else (None, None)
    xp, u = R.smooth_inputs(params(), G["x_mean"], G["x_std"], seed=2, u_mean=um, u_std=us)
    f32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32)   # noqa: E731
    terms = R.prior_terms(params(), float(G["Ts"]), xp, u, f32(G["x_mean"]), f32(G["x_std"]), f32(um), f32(us))
    assert R.kink_distance(params(), terms).min().item() >= 1e-3
    hits = R.branch_hits(params(), terms)
    inside = torch.stack([hits[f"post_{n}_inside"] for n in ("x", "y", "phi", "vx", "vy", "omega")], 1)
    assert inside[:32].all() and not inside[32:48].any() and not inside[48:, 3:].any() and inside[48:, :3].all()
    assert hits["vx_zero_floor"][:32].any() and (hits["alpha_lo"] | hits["alpha_hi"])[:32].any()


# ------------------------------------------------------------------ the GPU tests' bars, met by float32 on the CPU

def test_float32_gates_and_update_meet_their_bars_with_room():
    """tests/test_knet_stages.py holds the gate kernel to 1e-6 (1 + |h| + |gi_n| + |gh_n|) and the update kernel to
    1e-6 (|prior| + sigmoid(logit) sum_j |KG_ij dy_j|): float32 torch meets both with >= 2x room."""
    rng = np.random.default_rng(4)
    f = lambda *s: torch.tensor(rng.normal(size=s) * 3, dtype=torch.float32)   # noqa: E731
    B, H = 70, 128
    gi, gh, h = f(B, 3 * H), f(B, 3 * H), f(B, H)
    err = (R.gru64(gi, gh, h, torch.float32).double() - R.gru64(gi, gh, h)).abs()
    bar = 1e-6 * (1 + h.abs() + gi[:, 2 * H:].abs() + gh[:, 2 * H:].abs()).double()
    assert (err <= 0.5 * bar).all(), (err / bar).max().item()
    pr, KG, dy, lg = f(261, 6), f(261, 30), f(261, 5), torch.tensor(0.3)
    ref, scale = R.update64(pr, KG, dy, lg)
    err = (R.update64(pr, KG, dy, lg, torch.float32)[0].double() - ref).abs()
    assert (err <= 0.5 * 1e-6 * scale).all(), (err / (1e-6 * scale)).max().item()


def grad_bar(g64):
    return 1e-5 * (g64.abs() + g64.abs().max(1, keepdim=True).values)


def prior_grad(p, Ts, xp, u, y, norm, cot, dtype):
    x = xp.to(dtype).requires_grad_(True)
    outs = R.prior64(p, Ts, x, u, y, *norm, dtype=dtype)
    g, = torch.autograd.grad(outs, [x], [c.to(dtype) for c in cot])
    return g


@pytest.mark.parametrize("unorm", [False, True])
def test_float32_autograd_meets_the_gradient_bar_with_room(unorm):
    """The gradient bar of the GPU test, 1e-5 (|g64| + max_row |g64|): float32 CPU autograd of the same expressions
    meets it with >= 2x room, for the prior (away from the kinks), the gates and the update."""
    p, Ts = params(), float(G["Ts"])
    um, us = _ustats(GU) if unorm else (None, None)
    f32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32)   # noqa: E731
    norm = [f32(G["x_mean"]), f32(G["x_std"]), f32(G["y_mean"]), f32(G["y_std"]), f32(um), f32(us)]
    xp, u = R.smooth_inputs(p, G["x_mean"], G["x_std"], seed=2, u_mean=um, u_std=us)
    rng = np.random.default_rng(8)
    f = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    y, cot = f(64, 5), [f(64, 6), f(64, 5), f(64, 5)]
    g64 = prior_grad(p, Ts, xp, u, y, norm, cot, torch.float64)
    g32 = prior_grad(p, Ts, xp, u, y, norm, cot, torch.float32)
    assert (g64[32:48] == 0).all() and (g32[32:48] == 0).all()
    assert (g64[:32].abs().max(1).values > 0).all()
    assert ((g32.double() - g64).abs() <= 0.5 * grad_bar(g64)).all()
    if unorm:
        return
    B, H = 64, 128
    ins = [f(B, 3 * H) * 3, f(B, 3 * H) * 3, f(B, H) * 3]
    go = f(B, H)
    grads = {}
    for dt in (torch.float64, torch.float32):
        a = [t.to(dt).requires_grad_(True) for t in ins]
        grads[dt] = torch.autograd.grad(R.gru64(*a, dtype=dt), a, [go.to(dt)])
    for a, b in zip(grads[torch.float32], grads[torch.float64]):
        assert ((a.double() - b).abs() <= 0.5 * grad_bar(b)).all()
    ins = [f(B, 6), f(B, 30), f(B, 5)]
    go = f(B, 6)
    for dt in (torch.float64, torch.float32):
        a = [t.to(dt).requires_grad_(True) for t in ins]
        grads[dt] = torch.autograd.grad(R.update64(*a, torch.tensor(0.3), dtype=dt)[0], a, [go.to(dt)])
    for a, b in zip(grads[torch.float32], grads[torch.float64]):
        assert ((a.double() - b).abs() <= 0.5 * grad_bar(b)).all()

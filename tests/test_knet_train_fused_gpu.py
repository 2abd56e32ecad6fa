"""The fused truncated-BPTT training path on the GPU (trajectory_generation_amd/knet_train_fused.py, csrc/knet_bwd.h):
its kernels alone against float64 autograd of the matching tests/_knet_ref.py stage, the whole chunk against the
float64 sweep of tests/_knet_bptt_ref.py, against the reference's own gradients and losses (tests/golden/knet_train.npz,
knet_pred.npz), against the module path under autograd, graph replay, and a short training run.

Bars (none is derived from what the code under test gives):
  stage kernels   per row  max_c |gpu - ref64| <= (4 E + 2^-22) max_c |ref64|,  E = the same figure of a float32
                  torch-CPU evaluation (autograd of the same expression) over the input set's compared rows; prior rows
                  are compared when >= 1e-3 (real units) from every kink; B = 3 (three rows of the set) and B = 67
  dense epilogue  bit-exact against the float32 torch expression (one add, one multiply, one select)
  chunk           per parameter  ||gpu - ref64|| <= (4 E + 1e-6) ||ref64||,  E = the float32 CPU sweep's own relative
                  error against the float64 sweep; sequences within 1e-3 of a kink at any step are left out (at most
                  one of four: none with these inputs, tests/test_knet_bptt_ref.py)
  vs reference    tests/test_knet_train.py's tolerances: loss 1e-4 (1e-3 after an optimizer step), gradients 2e-3 of
                  the parameter's gradient norm
Every test prints its own worst err / bar with -s.

Measured on an MI355X (worst err / bar):
  prior_bwd <= 0.19 (float32-CPU E 1.1e-7 .. 1.4e-7), gru_gates_bwd <= 0.25, update_bwd <= 0.22, loss 0.08, loss gradient
  <= 0.20; chunk vs float64 <= 0.31 (in_mult 5 / 10, composite / plain), masked 0.27, vs the module path with the same
  masks 0.038; replay vs a fresh runner 0.000, vs float64 0.25; vs the reference: first-chunk gradients 0.034 / 0.032 of
  the 2e-3 norm bar (composite / prediction loss), chunk losses <= 1.7e-7 relative
"""
import random

import numpy as np
import pytest
import torch

from tests import _knet_bptt_ref as BR
from tests import _knet_ref as R
from tests._knet_weights import LIMITS
from tests.test_knet_bptt_ref import chunk_inputs

pytestmark = pytest.mark.gpu
G = np.load("tests/golden/knet.npz")
GP = np.load("tests/golden/knet_pred.npz")
TG = np.load("tests/golden/knet_train.npz")
TS = float(G["Ts"])
KINK_MIN = 1e-3
FLOOR = 2.0 ** -22
K = 10
SUB = [0, 20, 60]   # the B = 3 launches: three rows of the B = 67 input sets


def params():
    p = dict(R.PARAMS)
    p.update(LIMITS)
    return p


def row_err(got, ref):
    """Per row: max_c |got - ref| / max_c |ref| (rows whose reference is all zero: the error itself)."""
    scale = ref.abs().amax(1)
    return (got.double() - ref).abs().amax(1) / torch.where(scale > 0, scale, torch.ones_like(scale)), scale > 0


def check_rows(name, got, r64, r32, keep=None):
    keep = torch.ones(r64.shape[0], dtype=torch.bool) if keep is None else keep
    e32, on = row_err(r32, r64)
    err, _ = row_err(got, r64)
    sel = keep & on
    assert sel.any(), name
    bar = 4 * e32[sel].max().item() + FLOOR
    print(f"[knet-fused] {name} ({sel.sum().item()} / {keep.numel()} rows): float32-CPU E = {e32[sel].max().item():.3g}, "
          f"gpu worst = {err[sel].max().item():.3g}, worst err / bar = {err[sel].max().item() / bar:.3f}")
    assert torch.isfinite(got).all(), name
    assert (err[sel] <= bar).all(), (name, err[sel].max().item(), bar)
    return bar


def both_batches(fn, inputs, dev):
    """fn(*device inputs) -> tuple of outputs, launched on all 67 rows and on the three rows SUB; twice on the full
    set (bit-identical), and the sub-batch must give the full launch's rows.  Returns the full launch's outputs."""
    d = lambda t: t if not torch.is_tensor(t) or t.dim() == 0 else t.to(dev)   # noqa: E731
    full = [o.cpu() for o in fn(*[d(t) for t in inputs])]
    again = [o.cpu() for o in fn(*[d(t) for t in inputs])]
    sub = [o.cpu() for o in fn(*[d(t[SUB]) if torch.is_tensor(t) and t.dim() > 1 else d(t) for t in inputs])]
    for a, b, c in zip(full, again, sub):
        assert torch.equal(a, b)
        assert torch.equal(a[SUB], c)
    return full


# ------------------------------------------------------------------ 1. stage kernels against float64

def prior_case(kind, unorm):
    p = params()
    um, us = (GP["u_mean"], GP["u_std"]) if unorm else (None, None)
    if kind == "smooth":
        # (smooth_inputs lays its rows out in quarters of B: 68 rows, the first 67 used)
        xs, u = (t[:67] for t in R.smooth_inputs(p, G["x_mean"], G["x_std"], seed=1, u_mean=um, u_std=us, B=68))
    else:
        xs, u = R.branch_inputs(67, G["x_mean"], G["x_std"], seed=2, u_mean=um, u_std=us)
    rng = np.random.default_rng(3)
    y = torch.tensor(rng.normal(size=(67, 5)), dtype=torch.float32)
    gp = torch.tensor(rng.normal(size=(67, 6)), dtype=torch.float32)
    gd = torch.tensor(rng.normal(size=(67, 5)), dtype=torch.float32)
    f = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32).reshape(-1)   # noqa: E731
    norm = [f(G[k]) for k in ("x_mean", "x_std", "y_mean", "y_std")] + [f(um), f(us)]
    ref = {}
    for dt in (torch.float64, torch.float32):
        xp = xs.to(dt).requires_grad_(True)
        prior, _, dy = R.prior64(p, TS, xp, u, y, *norm, dtype=dt)
        ref[dt] = torch.autograd.grad([prior, dy], [xp], [gp.to(dt), gd.to(dt)])[0].double()
    keep = R.kink_distance(p, R.prior_terms(p, TS, xs, u, norm[0], norm[1], norm[4], norm[5])) >= KINK_MIN
    return xs, u, gp, gd, norm, ref, keep


@pytest.mark.parametrize("kind,unorm", [("smooth", False), ("smooth", True), ("branch", False), ("branch", True)])
def test_prior_bwd_vs_float64(gpu, kind, unorm):
    from trajectory_generation_amd import knet_train_fused as F
    xs, u, gp, gd, norm, ref, keep = prior_case(kind, unorm)
    nd = [None if t is None else t.to(gpu) for t in norm]

    def fn(x, uu, a, b):
        return (F.prior_bwd(params(), TS, x, uu, nd[0], nd[1], nd[2], nd[3], a, b, nd[4], nd[5]),)

    got, = both_batches(fn, (xs, u, gp, gd), gpu)
    assert keep.sum().item() >= (50 if kind == "smooth" else 34), keep.sum().item()
    check_rows(f"prior_bwd {kind} unorm={unorm}", got, ref[torch.float64], ref[torch.float32], keep)
    if kind == "smooth":
        # rows [34, 51): every state beyond its limit -> the whole row is exactly zero; rows [51, 67): vx, vy, omega
        # beyond theirs -> those three entries exactly zero, X, Y, phi not
        r64 = ref[torch.float64]
        assert (r64[34:51] == 0).all() and (r64[51:, 3:] == 0).all() and (r64[51:, :3].abs() > 0).all()
        assert (got[34:51] == 0).all() and (got[51:, 3:] == 0).all() and (got[51:, :3].abs() > 0).all()
        # g_dy = NULL is g_dy = 0
        z = fn(xs.to(gpu), u.to(gpu), gp.to(gpu), torch.zeros_like(gd).to(gpu))[0]
        n = F.prior_bwd(params(), TS, xs.to(gpu), u.to(gpu), nd[0], nd[1], nd[2], nd[3], gp.to(gpu), None, nd[4], nd[5])
        assert torch.equal(z, n)


def test_gru_gates_bwd_vs_float64(gpu):
    from trajectory_generation_amd import knet_train_fused as F
    rng = np.random.default_rng(4)
    H = 128
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    gi, gh, h, g1, g2 = t(67, 3 * H), t(67, 3 * H), torch.tanh(t(67, H)), t(67, H), t(67, H)
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b, c = (x.to(dt).requires_grad_(True) for x in (gi, gh, h))
        ref[dt] = [x.double() for x in torch.autograd.grad(R.gru64(a, b, c, dt), [a, b, c], [(g1 + g2).to(dt)])]
    got = both_batches(lambda a, b, c, d, e: F.gru_gates_bwd(a, b, c, d, e), (gi, gh, h, g1, g2), gpu)
    for name, g, r64, r32 in zip(("g_gi", "g_gh", "g_h"), got, ref[torch.float64], ref[torch.float32]):
        check_rows("gru_gates_bwd " + name, g, r64, r32)
    # a column slice of a wider matrix is read in place, and one addend alone
    wide = torch.cat((t(67, 36), g1 + g2), 1).to(gpu)
    dv = [x.to(gpu) for x in (gi, gh, h)]
    one = F.gru_gates_bwd(*dv, wide[:, 36:])
    for a, b in zip(one, F.gru_gates_bwd(*dv, wide[:, 36:].contiguous())):
        assert torch.equal(a, b)
    for g, r64, r32 in zip(one, ref[torch.float64], ref[torch.float32]):
        check_rows("gru_gates_bwd slice", g.cpu(), r64, r32)


def test_update_bwd_vs_float64(gpu):
    from trajectory_generation_amd import knet_train_fused as F
    rng = np.random.default_rng(5)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    prior, KG, dy, g1, g2 = t(67, 6), 0.3 * t(67, 30), t(67, 5), t(67, 6), t(67, 6)
    logit = torch.tensor(0.3)
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b, c = (x.to(dt).requires_grad_(True) for x in (prior, KG, dy))
        lg = logit.to(dt).expand(67, 1).clone().requires_grad_(True)   # one logit per row: per-sequence gradients
        post = R.update64(a, b, c, lg, dt)[0]
        ref[dt] = [x.double() for x in torch.autograd.grad(post, [a, b, c, lg], [(g1 + g2).to(dt)])]
    got = both_batches(lambda a, b, c, d: F.update_bwd(a, b, logit.to(gpu), c, d), (KG, dy, g1, g2), gpu)
    for name, g, r64, r32 in zip(("g_prior", "g_KG", "g_dy", "g_logit"), got, ref[torch.float64], ref[torch.float32]):
        check_rows("update_bwd " + name, g.reshape(67, -1), r64.reshape(67, -1), r32.reshape(67, -1))
    assert torch.equal(got[0], g1 + g2)


def test_dense_bwd_is_exact(gpu):
    from trajectory_generation_amd import knet_train_fused as F
    rng = np.random.default_rng(6)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    for rows in (3, 67):
        for cols in (36, 128):
            wa, wb, act = t(rows, cols + 128), t(rows, cols + 30), torch.relu(t(rows, cols))
            mask = (torch.tensor(rng.random((rows, cols))) >= 0.05).float() / 0.95
            ga, gb = wa[:, 128:], wb[:, :cols]
            da, db = wa.to(gpu)[:, 128:], wb.to(gpu)[:, :cols]
            full = F.dense_bwd(da, act.to(gpu), mask.to(gpu), db)
            assert torch.equal(full.cpu(), torch.where(act > 0, (ga + gb) * mask, torch.zeros(())))
            assert torch.equal(full, F.dense_bwd(da, act.to(gpu), mask.to(gpu), db))
            assert torch.equal(F.dense_bwd(da, None, None, db).cpu(), ga + gb)
            assert torch.equal(F.dense_bwd(da, None, mask.to(gpu)).cpu(), ga * mask)
            assert torch.equal(F.dense_bwd(da, act.to(gpu)).cpu(), torch.where(act > 0, ga, torch.zeros(())))


@pytest.mark.parametrize("composite", [True, False])
def test_train_loss_vs_float64(gpu, composite):
    from trajectory_generation_amd import knet_train as KT
    from trajectory_generation_amd import knet_train_fused as F
    rng = np.random.default_rng(7)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    Kc = 7
    x_mean, x_std = torch.tensor(G["x_mean"]).float(), torch.tensor(G["x_std"]).float()
    s2 = float(x_std.reshape(-1)[2])
    xo, xt, yt, gx = t(67, 6, Kc), t(67, 6, Kc), t(67, 5, Kc), 1e-3 * t(67, 6, Kc)
    # phi differences (real units) on both sides of +pi and -pi
    around = torch.tensor(rng.choice([-1.0, 1.0], (67, Kc)) * (np.pi + rng.uniform(-0.2, 0.2, (67, Kc))))
    xt[:, 2, :] = xo[:, 2, :] - (around / s2).float()
    dreal = (xo[:, 2, :].double() * s2) - (xt[:, 2, :].double() * s2)
    assert (dreal.abs() > np.pi + 1e-3).any() and (dreal.abs() < np.pi - 1e-3).any() and (dreal > 0).any() \
        and (dreal < 0).any()
    for B in (67, 3):
        rows = slice(None) if B == 67 else SUB
        a, b, c, e = xo[rows], xt[rows], yt[rows], gx[rows]
        ref = {}
        for dt in (torch.float64, torch.float32):
            x = a.to(dt).requires_grad_(True)
            if composite:
                loss = KT.compute_composite_loss(x, b.to(dt), c.to(dt), x_mean.to(dt), x_std.to(dt), 6, 5, 0.8)
            else:
                loss = KT.loss_x_with_angular(x, b.to(dt), x_mean.to(dt), x_std.to(dt), 6)
            ref[dt] = (float(loss.detach()), torch.autograd.grad(loss, x)[0].double())
        d = lambda v: v.to(gpu)   # noqa: E731
        kw = dict(y_tgt=d(c), alpha=0.8) if composite else {}
        loss, grad = F.train_loss(d(a), d(b), d(x_mean), d(x_std), **kw)
        loss2, grad2 = F.train_loss(d(a), d(b), d(x_mean), d(x_std), **kw)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
        l64, l32 = ref[torch.float64][0], ref[torch.float32][0]
        bar_l = 4 * abs(l32 - l64) / l64 + FLOOR
        print(f"[knet-fused] train_loss composite={composite} B={B}: loss err / bar = "
              f"{abs(float(loss) - l64) / l64 / bar_l:.3f}")
        assert abs(float(loss) - l64) <= bar_l * l64
        rows2 = lambda g: g.permute(0, 2, 1).reshape(-1, 6)   # noqa: E731  (one row per (b, k))
        check_rows(f"train_loss grad composite={composite} B={B}", rows2(grad.cpu()), rows2(ref[torch.float64][1]),
                   rows2(ref[torch.float32][1]))
        lx, gxx = F.train_loss(d(a), d(b), d(x_mean), d(x_std), g_extra=d(e), **kw)
        assert torch.equal(lx, loss) and torch.equal(gxx, grad + d(e))   # g_extra: one separate add, bit for bit
        # the tape's layout [K,B,6] read through strides gives the same bits
        tape = d(a).permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not tape.is_contiguous()
        xm, xs = d(x_mean).reshape(-1), d(x_std).reshape(-1)
        lt, gt = F.train_loss(tape, d(b), xm, xs, **kw)
        assert torch.equal(lt, loss) and torch.equal(gt, grad)


# ------------------------------------------------------------------ models, data, float64 chunks

def build(dev, in_mult=5, train=False, weights=None):
    from tests.test_knet_gpu import build as build_knet
    _, _, model = build_knet(dev, seed=0, in_mult=in_mult, u_stats=None)
    if weights is not None:
        model.load_state_dict(weights, strict=True)
    model.train(train)
    return model


def golden_data(dev):
    d = lambda k: torch.tensor(G[k], dtype=torch.float32, device=dev)   # noqa: E731
    x_mean, x_std = d("x_mean"), d("x_std")
    return dict(y_norm=d("y_norm"), u=d("u"), x_norm=(d("x_true") - x_mean) / x_std, m1x0=d("m1x0"), x_mean=x_mean,
                x_std=x_std)


_CHUNKS = {}


def chunk_ref(in_mult, masked=False, second=False):
    """The float64 and float32 CPU sweeps of a chunk (computed once and shared): steps [0, 10) of the golden data from
    m1x0, or (second) steps [10, 20) from the golden posterior of step 9 with non-zero hidden states left out."""
    key = (in_mult, masked, second)
    if key not in _CHUNKS:
        w, D = chunk_inputs(in_mult)
        if second:
            f = lambda k: torch.tensor(G[k], dtype=torch.float32)   # noqa: E731
            D = dict(D, y_seq=f("y_norm")[:, :, K:], u_seq=f("u")[:, :, K:],
                     x_tgt=((f("x_true") - f("x_mean")) / f("x_std"))[:, :, K:], m1x0=f("x_post")[:, :, K - 1])
        masks = BR.draw_masks(w, K, 4, seed=11) if masked else None
        _CHUNKS[key] = (w, D, masks)
    return _CHUNKS[key]


_SWEEPS = {}


def sweeps(key, w, D, masks, composite=True):
    if key not in _SWEEPS:
        kw = dict(D, alpha=0.8, composite=composite, masks=masks)
        r64 = BR.sweep(w, params(), TS, **kw)
        r32 = BR.sweep(w, params(), TS, dtype=torch.float32, **kw)
        kink = BR.chunk_kink_distance(params(), TS, r64["tape"], D["norm"])
        assert (kink < KINK_MIN).sum().item() <= 1   # no sequence is left out with these inputs (CPU test)
        assert (kink >= KINK_MIN).all()
        _SWEEPS[key] = (r64, r32)
    return _SWEEPS[key]


def grad_bars(r64, r32):
    """Per tensor (4 E + 1e-6), E = ||g32 - g64|| / ||g64||; "g_x0" included."""
    out = {}
    for k, g in list(r64["grads"].items()) + [("g_x0", r64["g_x0"])]:
        g32 = r32["g_x0"] if k == "g_x0" else r32["grads"][k]
        assert g.norm() > 0, k
        out[k] = 4 * ((g32.double() - g).norm() / g.norm()).item() + 1e-6
    return out


def check_grads(name, got, ref, bars):
    worst = 0.0
    for k, r in ref.items():
        err = ((got[k].detach().cpu().double().reshape(r.shape) - r.double()).norm() / r.double().norm()).item()
        worst = max(worst, err / bars[k])
        assert err <= bars[k], (name, k, err, bars[k])
    print(f"[knet-fused] {name}: worst gradient err / bar = {worst:.3f}")


def run_fused(model, D, masks=None, composite=True, use_graph=True):
    from trajectory_generation_amd import knet_train_fused as F
    dev = model.device
    R_ = F.FusedTBPTT(model, 4, K)
    if masks is not None:
        R_.set_masks(masks)
    R_.reset(D["m1x0"].to(dev))
    loss = R_.run_chunk(D["y_seq"].to(dev), D["u_seq"].to(dev), D["x_tgt"].to(dev), composite=composite, alpha=0.8,
                        use_graph=use_graph)
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in R_.grads.items()}
    got["g_x0"] = R_.g_x0(K).clone()
    return R_, float(loss), got


# ------------------------------------------------------------------ 2. first-chunk gradients against the reference

def test_first_chunk_gradients_vs_reference(gpu):
    from tests.test_knet_train import _build
    from trajectory_generation_amd import knet_train_fused as F
    model, D = _build(gpu)
    R_ = F.FusedTBPTT(model, 4, 10)
    R_.reset(D["m1x0"])
    loss = R_.run_chunk(D["y_norm"][:, :, :10], D["u"][:, :, :10], D["x_norm"][:, :, :10], composite=True, alpha=0.8)
    assert abs(float(loss) - float(TG["chunk1_loss"])) <= 1e-4 * float(TG["chunk1_loss"])
    assert all(p.grad is None for p in model.parameters())
    R_.add_grads()
    grads = dict(model.named_parameters())
    worst = 0.0
    for name, ref_norm, ref_head in zip(TG["grad_names"], TG["grad_norm"], TG["grad_head"]):
        g = grads[str(name)].grad
        assert g is not None, name
        gn = float(g.norm())
        head = g.reshape(-1)[:8].cpu().numpy()
        worst = max(worst, abs(gn - ref_norm) / ref_norm, np.abs(head - ref_head[:head.size]).max() / ref_norm)
        assert abs(gn - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, gn, ref_norm)
        assert np.abs(head - ref_head[:head.size]).max() <= 2e-3 * ref_norm + 1e-9, name
    print(f"[knet-fused] first-chunk gradients vs reference: worst err / (2e-3 norm) = {worst / 2e-3:.3f}")
    R_.add_grads(0.5)   # accumulates
    assert torch.equal(grads["FC5.0.weight"].grad, R_.grads["FC5.0.weight"] + 0.5 * R_.grads["FC5.0.weight"])


# ------------------------------------------------------------------ 3. the fused chunk against the float64 sweep

@pytest.mark.parametrize("in_mult", [5, 10])
@pytest.mark.parametrize("composite", [True, False])
def test_fused_chunk_vs_float64(gpu, in_mult, composite):
    w, D, _ = chunk_ref(in_mult)
    r64, r32 = sweeps((in_mult, False, False, composite), w, D, None, composite)
    bars = grad_bars(r64, r32)
    _, loss, got = run_fused(build(gpu, in_mult), D, composite=composite)
    l64 = float(r64["loss"])
    assert abs(loss - l64) <= (4 * abs(float(r32["loss"]) - l64) / l64 + 1e-6) * l64
    check_grads(f"fused chunk in_mult {in_mult} composite={composite}", got, dict(r64["grads"], g_x0=r64["g_x0"]), bars)
    if in_mult == 5 and composite:   # the launch chain run eagerly, without a graph
        _, loss_e, got_e = run_fused(build(gpu, in_mult), D, use_graph=False)
        assert abs(loss_e - loss) <= 1e-6 * loss
        check_grads("eager launch chain", got_e, dict(r64["grads"], g_x0=r64["g_x0"]), bars)


# ------------------------------------------------------------------ 4. dropout

class MaskDrop(torch.nn.Module):
    """Stands in for nn.Dropout in the module path: multiplies by the mask slot of the current step."""

    def __init__(self, mask, clock):
        super().__init__()
        self.mask, self.clock = mask, clock

    def forward(self, x):
        return x * self.mask[self.clock["t"]]


def test_dropout_masks_equal_module_path(gpu):
    from trajectory_generation_amd import knet_train as KT
    w, D, masks = chunk_ref(5, masked=True)
    r64, r32 = sweeps((5, True, False, True), w, D, masks)
    bars = grad_bars(r64, r32)
    _, loss, got = run_fused(build(gpu, 5, train=True), D, masks=masks)
    check_grads("fused train mode vs float64 (masked)", got, dict(r64["grads"], g_x0=r64["g_x0"]), bars)
    # the module path under autograd with the same masks
    model = build(gpu, 5, train=True)
    clock = {"t": 0}
    for name, seq, i in (("FC5", model.FC5, 2), ("FC1", model.FC1, 2), ("FC7", model.FC7, 2), ("FC2", model.FC2, 3),
                         ("FC3", model.FC3, 2), ("FC4", model.FC4, 2)):
        assert isinstance(seq[i], torch.nn.Dropout) and seq[i].p == BR.MASKED[name]
        seq[i] = MaskDrop(masks[name].to(gpu), clock)
    model.batch_size = 4
    model.init_hidden_KNet()
    x0 = D["m1x0"].to(gpu).reshape(4, 6, 1).requires_grad_(True)
    model.InitSequence(x0, K)
    outs = []
    for t in range(K):
        clock["t"] = t
        outs.append(model(D["y_seq"][:, :, t:t + 1].to(gpu), D["u_seq"][:, :, t:t + 1].to(gpu)).squeeze(2))
    lm = KT.compute_composite_loss(torch.stack(outs, 2), D["x_tgt"].to(gpu), D["y_seq"].to(gpu),
                                   torch.tensor(G["x_mean"]).float().to(gpu), torch.tensor(G["x_std"]).float().to(gpu),
                                   6, 5, 0.8)
    lm.backward()
    ref = {k: v.grad.detach().cpu() for k, v in model.named_parameters()}
    ref["g_x0"] = x0.grad.reshape(4, 6).cpu()
    assert abs(loss - lm.item()) <= 1e-6 * lm.item()
    check_grads("fused train mode vs module path (same masks)", got, ref, bars)
    eval_loss = run_fused(build(gpu, 5), D)[1]
    assert abs(eval_loss - loss) > 1e-4 * loss   # the masks reach the forward


# ------------------------------------------------------------------ 5. both strategies against the reference

@pytest.mark.parametrize("strategy", ["standard", "accumulation"])
def test_tbptt_chunk_losses_vs_reference(gpu, strategy):
    from tests.test_knet_train import PARAMS, _build
    from trajectory_generation_amd import knet_train_fused as F
    model, D = _build(gpu)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    avg, db, losses = F.tbptt_sequence_fused(model, opt, D["y_norm"], D["u"], D["x_norm"], D["m1x0"],
                                             dict(PARAMS, strategy=strategy), D["x_mean"], D["x_std"])
    ref = TG["losses_" + strategy]
    assert len(losses) == len(ref) == 2
    print(f"[knet-fused] chunk losses {strategy}: rel err {abs(losses[0] - ref[0]) / ref[0]:.2e}, "
          f"{abs(losses[1] - ref[1]) / ref[1]:.2e}")
    assert abs(losses[0] - ref[0]) <= 1e-4 * ref[0]
    assert abs(losses[1] - ref[1]) <= 1e-3 * ref[1]
    assert np.isfinite(float(db)) and abs(avg - sum(losses) / 2) < 1e-12


@pytest.mark.parametrize("strategy,composite", [("standard", True), ("accumulation", False)])
def test_shorter_last_chunk_vs_module_path(gpu, strategy, composite):
    """T = 15, K = 10: the last chunk has 5 steps and a graph of its own."""
    from tests.test_knet_train import PARAMS, _build
    from trajectory_generation_amd import knet_train as KT
    from trajectory_generation_amd import knet_train_fused as F
    p = dict(PARAMS, strategy=strategy, T=15, CompositionLoss=composite)
    res = []
    for fn in (KT.tbptt_sequence, F.tbptt_sequence_fused):
        model, D = _build(gpu)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
        res.append(fn(model, opt, D["y_norm"][:, :, :15], D["u"][:, :, :15], D["x_norm"][:, :, :15], D["m1x0"], p,
                      D["x_mean"], D["x_std"]) + (model.m1x_posterior.detach().clone(),))
    (_, _, lm, pm), (_, _, lf, pf) = res
    assert len(lm) == len(lf) == 2
    print(f"[knet-fused] T = 15 {strategy} composite={composite}: rel err {abs(lf[0] - lm[0]) / lm[0]:.2e}, "
          f"{abs(lf[1] - lm[1]) / lm[1]:.2e}")
    assert abs(lf[0] - lm[0]) <= 1e-4 * lm[0] and abs(lf[1] - lm[1]) <= 1e-3 * lm[1]
    assert pf.shape == pm.shape and torch.isfinite(pf).all()   # the module's state is left as the module path does
    assert len(model._fused_tbptt[(4, 10, False)].graphs) == 2


# ------------------------------------------------------------------ 6. replay

def test_replay_after_optimizer_step_equals_fresh_runner(gpu):
    w, D2, _ = chunk_ref(5, second=True)
    _, D1, _ = chunk_ref(5)
    model = build(gpu, 5)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    R_, _, g1 = run_fused(model, D1)
    ptrs = R_._param_ptrs()
    R_.add_grads()
    opt.step()
    opt.zero_grad()
    assert R_._param_ptrs() == ptrs and len(R_.graphs) == 1
    d = lambda t: t.to(gpu)   # noqa: E731
    R_.reset(d(D2["m1x0"]))
    loss = float(R_.run_chunk(d(D2["y_seq"]), d(D2["u_seq"]), d(D2["x_tgt"])))
    assert len(R_.graphs) == 1   # replayed, not captured again
    got = dict({k: v.clone() for k, v in R_.grads.items()}, g_x0=R_.g_x0(K).clone())
    moved = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert (moved["FC2.0.weight"] - w["FC2.0.weight"]).abs().max() > 1e-4
    r64, r32 = sweeps("replay", moved, D2, None)
    bars = grad_bars(r64, r32)
    _, loss_f, fresh = run_fused(build(gpu, 5, weights=moved), D2)
    assert abs(loss - loss_f) <= 1e-6 * loss_f
    check_grads("replay after an optimizer step vs a fresh runner", got,
                {k: v.cpu() for k, v in fresh.items()}, bars)
    check_grads("replay after an optimizer step vs float64", got, dict(r64["grads"], g_x0=r64["g_x0"]), bars)
    assert (got["FC2.2.weight"] - g1["FC2.2.weight"]).norm() > 1e-3 * g1["FC2.2.weight"].norm()


# ------------------------------------------------------------------ 7. prediction loss

TRAIN = dict(K_TBPTT=10, T=20, m=6, n=5, lambda_pred=0.5, pred_horizon=5)


def test_prediction_loss_training_vs_reference(gpu):
    """tests/golden/knet_pred.npz (K = 10, lambda_pred 0.5, H = 5, AdamW lr 1e-4 wd 1e-5, clip 1.0), eval mode: the first
    chunk's gradients and both chunks' filter and prediction losses, at tests/test_knet_train.py's tolerances."""
    from trajectory_generation_amd import pipeline_prediction as PP
    model = build(gpu, 5)
    d = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)   # noqa: E731
    D = {"y_norm": d(G["y_norm"]), "u": d(G["u"]), "x_norm": d(GP["x_norm"]), "m1x0": d(G["m1x0"]),
         "x_mean": d(G["x_mean"]), "x_std": d(G["x_std"])}
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    first = {}

    def grab(md):
        if not first:
            first.update({k: v.grad.detach().clone() for k, v in md.named_parameters()})

    lf, lp = PP.tbptt_prediction_sequence_fused(model, opt, D["y_norm"], D["u"], D["x_norm"], D["m1x0"], TRAIN,
                                                D["x_mean"], D["x_std"], on_chunk=grab)
    for got, ref in ((lf, GP["losses_filter"]), (lp, GP["losses_pred"])):
        assert len(got) == len(ref) == 2
        print(f"[knet-fused] prediction-loss training chunk losses: rel err {abs(got[0] - ref[0]) / ref[0]:.2e}, "
              f"{abs(got[1] - ref[1]) / ref[1]:.2e}")
        assert abs(got[0] - ref[0]) <= 1e-4 * ref[0]
        assert abs(got[1] - ref[1]) <= 1e-3 * ref[1]
    worst = 0.0
    for name, ref_norm, ref_head in zip(GP["grad_names"], GP["grad_norm"], GP["grad_head"]):
        g = first[str(name)]
        gn = float(g.norm())
        head = g.reshape(-1)[:8].cpu().numpy()
        worst = max(worst, abs(gn - ref_norm) / ref_norm, np.abs(head - ref_head[:head.size]).max() / ref_norm)
        assert abs(gn - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, gn, ref_norm)
        assert np.abs(head - ref_head[:head.size]).max() <= 2e-3 * ref_norm + 1e-9, name
    print(f"[knet-fused] prediction-loss first-chunk gradients: worst err / (2e-3 norm) = {worst / 2e-3:.3f}")


# ------------------------------------------------------------------ 8. it trains

def test_train_epoch_learns_fused(gpu):
    from tests.test_knet_train import PARAMS, _build
    from trajectory_generation_amd import knet_train as KT
    torch.manual_seed(3)
    random.seed(3)
    model, D = _build(gpu)
    x_real = D["x_norm"] * D["x_std"] + D["x_mean"]
    y_real = D["y_norm"] * torch.tensor(G["y_std"], dtype=torch.float32, device=gpu) + \
        torch.tensor(G["y_mean"], dtype=torch.float32, device=gpu)
    norm = {k: torch.tensor(G[k], dtype=torch.float32) for k in ("x_mean", "x_std", "y_mean", "y_std")}
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    p = dict(PARAMS, N_E=4, N_batch=4, device=gpu, fused=True)
    losses = [KT.train_epoch(model, opt, y_real, D["u"], x_real, norm, p)[0] for _ in range(8)]
    assert all(np.isfinite(losses))
    assert min(losses[-3:]) < losses[0]
    runner = model._fused_tbptt[(4, 10, True)]
    assert runner.train and len(runner.graphs) == 1   # every chunk of every epoch replayed one graph
    assert all((m == 0).any() and ((m == 0) | (m > 1)).all() for m in runner.M.values())   # masks were drawn
    model.eval()
    with torch.no_grad():
        model.batch_size = 4
        model.init_hidden_KNet()
        model.InitSequence(D["m1x0"], 20)
        assert torch.isfinite(model(D["y_norm"][:, :, :1], D["u"][:, :, :1])).all()

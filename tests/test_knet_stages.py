"""Every KalmanNet kernel of csrc/knet.hip (its stage headers csrc/knet_*.h) on its own against the float64 reference of tests/_knet_ref.py:
the stand-alone ops (trajknet::prior / gru_gates / update), each stage of the fused step (front / FC2 / back and the
merged back+front launch) teacher-forced from the GPU's own upstream outputs, the EKF across a launch block, batch
independence and NaN isolation of the fused runner, the forward / backward pairing of the training ops, and the
support envelope.  All comparisons are elementwise.

Bars (none is derived from what the kernels give; tests/test_knet_ref.py checks on the CPU that a float32 torch
evaluation of the same expressions meets the gate, update and gradient bars with at least 2x room):
  prior / m1y / dy   per column j:  max_b |gpu - ref64| <= 4 E_j + 2^-22 max_b |ref64_j|, with
                     E_j = max_b |prior64(float32) - prior64(float64)| measured on the same inputs
  gates              1e-6 (1 + |h| + |gi_n| + |gh_n|)
  update / post      1e-6 (|prior| + sigmoid(logit) sum_j |KG_ij dy_j|)
  fused dense / GRU  1e-6 x the stage's abs-sum scale (GRU: 1 + |h| + the scales of its i_n and h_n pre-activations),
                     the bar tests/test_knet_fc2.py holds FC2 to
  gradients          1e-5 (|g64| + max_row |g64|) per row; rows whose every state is clamped are exactly zero
  EKF                1e-8 (1 + max |ref|)

Measured on an MI355X (worst element of each check over all its cases; every test prints its own figures with -s):
  prior op           max_b |gpu - ref64| / E_j = 1.00 in every column of prior, m1y and dy except omega's (0.77 .. 1.01
                     there), with and without control statistics: the worst rows are clamped outputs, where the kernel
                     and float32 torch round (limit - mean) / std alike.  As a fraction of the bar: 0.18 / 0.18 / 0.16
  torch_prior        vs float64 0.18 of the bar, vs the op 0.12
  gates 0.10, update 0.17 of their bars
  fused stages       err / (1e-6 x abs-sum scale):  hQ 0.034, out_Sigma 0.027, hS 0.023, KG 0.001, hSig 0.049, post 0.12
  merged launch      bit-identical to two launch triples; its second step's stages: hQ 0.014, out_Sigma 0.019, hS 0.011,
                     KG 0.001, hSig 0.057, post 0.073
  gradients          prior 0.028, gates 0.10, update 0.015 of the bar; the all-clamped rows exactly zero
  EKF 0.038 of its bar; in_mult 1 / 7 end to end 0.0012 of 2e-4 (1 + max)
(float32 torch on the CPU, standing in for the kernels in the same checks, gives fused-stage figures of the same size:
0.035 / 0.035 / 0.033 / 0.001 / 0.081 / 0.11.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _knet_ref as R
from tests._knet_weights import LIMITS, knet_weights

pytestmark = pytest.mark.gpu
G = np.load("tests/golden/knet.npz")
GU = np.load("tests/golden/knet_b9_t12_unorm.npz")
TS = float(G["Ts"])
H = 128


def params():
    p = dict(R.PARAMS)
    p.update(LIMITS)
    return p


_CTX = {}


def ctx(dev, in_mult=5, unorm=False, seed=1):
    """A built model of the given architecture (weights of tests/_knet_weights.py), with what the ops need; cached."""
    key = (in_mult, unorm, seed)
    if key not in _CTX:
        from tests.test_knet_gpu import build
        from trajectory_generation_amd import knet_ops as KO
        K, sysm, model = build(dev, seed=seed, in_mult=in_mult, u_stats=(GU["u_mean"], GU["u_std"]) if unorm else None)
        ws, dims = KO.step_weights(model), KO.step_dims(model)
        norm = [t.reshape(-1).contiguous() for t in model._norm_tensors()]
        if unorm:
            norm += [model.u_mean.reshape(-1).contiguous(), model.u_std.reshape(-1).contiguous()]
        _CTX[key] = {"K": K, "sysm": sysm, "model": model, "ws": ws, "dims": dims,
                     "pk": torch.ops.trajknet.pack(ws, dims), "norm": norm,
                     "params": KO.params_list(sysm.Params), "limits": KO.limits_list(sysm.Params),
                     "w": {k: torch.tensor(v) for k, v in knet_weights(seed=seed, in_mult=in_mult).items()}}
    return _CTX[key]


def norm6(c):
    n = [t.cpu() for t in c["norm"]]
    return n + [None, None] if len(n) == 4 else n


def step_inputs(B, dev, c, seed):
    """One step's inputs with non-zero hidden states: y, u (normalized when the model normalizes controls), x_post,
    h_q, h_sigma, h_s."""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)   # noqa: E731
    u = np.stack([rng.uniform(0, 0.5, B), rng.uniform(-0.3, 0.3, B)], 1)
    if len(c["norm"]) == 6:
        u = (u - GU["u_mean"].reshape(1, 2)) / GU["u_std"].reshape(1, 2)
    return (f(rng.normal(size=(B, 5))), f(u), f(rng.normal(size=(B, 6)) * 0.5), f(rng.normal(size=(B, H)) * 0.5),
            f(rng.normal(size=(B, H)) * 0.5), f(rng.normal(size=(B, H)) * 0.5))


def launch_step(c, y, u, post, hq, hsig, hs):
    """The three launches of trajknet::step (front, fc2, back) with every buffer they write kept: prior, dy, x2, hQ,
    hS, KG, hSig, post.  Outputs start as NaN, so an element a kernel leaves unwritten shows."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd.batch import params_struct
    K, model, sysm = c["K"], c["model"], c["sysm"]
    L, net, dev = _lib.lib(), K.net_struct(model), post.device
    B = post.shape[0]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
    hq, hsig, hs = hq.clone(), hsig.clone(), hs.clone()
    o = {"prior": nan(B, 6), "dy": nan(B, 5), "x2": nan(B, 2 * H), "KG": nan(B, 30), "post": nan(B, 6)}
    ws = nan(L.traj_knet_fc2_workspace_bytes(C.byref(net), B) // 4)
    nrm = c["norm"] + [None] * (6 - len(c["norm"]))
    _lib.check(L.traj_knet_front_f32(C.byref(params_struct(sysm.Params)), C.byref(K.limits_struct(sysm.Params)),
                                     float(sysm.Ts), C.byref(net), p(c["pk"]), B, p(post), p(u), 2, 1, p(y), 5, 1,
                                     *[p(t) for t in nrm], p(hq), p(hsig), p(hs), p(o["prior"]), p(o["dy"]),
                                     p(o["x2"]), st), "front")
    _lib.check(L.traj_knet_fc2_f32(C.byref(net), B, p(o["x2"]), p(ws), ws.numel() * 4, st), "fc2")
    _lib.check(L.traj_knet_back_f32(C.byref(net), p(c["pk"]), B, p(o["x2"]), p(ws), p(o["prior"]), p(o["dy"]),
                                    p(hsig), p(o["post"]), None, 0, 0, p(o["KG"]), st), "back")
    torch.cuda.synchronize()
    o.update(hQ=hq, hS=hs, hSig=hsig)
    return o


def worst(name, err, bar):
    """Print the worst element's error as a fraction of its bar, then assert every element meets its bar."""
    err, bar = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bar, dtype=torch.float64)
    assert torch.isfinite(err).all(), name
    ratio = (err / bar.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"[knet-stages] {name}: worst err / bar = {ratio:.3f}")
    assert (err <= bar).all(), (name, ratio)
    return ratio


# ------------------------------------------------------------------ stand-alone ops

_PRIOR = {}


def prior_case(dev, unorm):
    """B = 261 prior inputs that visit every branch, the float64 reference, the float32-CPU error E_j and the GPU
    outputs of trajknet::prior; computed once for the tests that share it."""
    if unorm not in _PRIOR:
        c = ctx(dev, 5, unorm)
        n = norm6(c)
        xp, u = R.branch_inputs(261, G["x_mean"], G["x_std"], seed=1, u_mean=GU["u_mean"] if unorm else None,
                                u_std=GU["u_std"] if unorm else None)
        y = torch.tensor(np.random.default_rng(2).normal(size=(261, 5)), dtype=torch.float32)
        p = params()
        hits = R.branch_hits(p, R.prior_terms(p, TS, xp, u, n[0], n[1], n[4], n[5]))
        missed = [k for k, v in hits.items() if not v.any()]
        assert not missed, missed
        ref = R.prior64(p, TS, xp, u, y, *n)
        r32 = R.prior64(p, TS, xp, u, y, *n, dtype=torch.float32)
        E = [(a.double() - b).abs().max(0).values for a, b in zip(r32, ref)]
        bar = [4 * e + 2.0 ** -22 * b.abs().max(0).values for e, b in zip(E, ref)]
        g = [t.to(dev) for t in (xp, u, y)]
        dn = c["norm"] + [None] * (6 - len(c["norm"]))
        got = torch.ops.trajknet.prior(*g, *dn, c["params"], c["limits"], TS)
        _PRIOR[unorm] = {"c": c, "in": g, "dn": dn, "ref": ref, "E": E, "bar": bar, "got": [t.cpu() for t in got]}
    return _PRIOR[unorm]


@pytest.mark.parametrize("unorm", [False, True])
def test_prior_op_vs_float64(gpu, unorm):
    """knet_prior_kernel across a 256-thread block with a ragged tail (B = 261), real normalization statistics, every
    clamp / floor branch visited, without and with control statistics."""
    s = prior_case(gpu, unorm)
    for name, got, ref, E, bar in zip(("prior", "m1y", "dy"), s["got"], s["ref"], s["E"], s["bar"]):
        err = (got.double() - ref).abs().max(0).values
        print(f"[knet-stages] prior op unorm={unorm} {name}: max_b err / E_j =",
              np.round((err / E.clamp_min(1e-300)).numpy(), 2))
        worst(f"prior op unorm={unorm} {name}", err, bar)
    if unorm:   # the statistics matter: the same inputs without them give another prior
        c = s["c"]
        plain = torch.ops.trajknet.prior(*s["in"], *c["norm"][:4], None, None, c["params"], c["limits"], TS)
        assert (plain[0].cpu() - s["got"][0]).abs().max() > 1e-2


@pytest.mark.parametrize("unorm", [False, True])
def test_torch_prior_is_the_prior_ops_function(gpu, unorm):
    """What the training backward differentiates (knet.torch_prior, float32 on the device) computes the function the
    HIP forward computes: both within the prior bar of each other and of the float64 reference."""
    s = prior_case(gpu, unorm)
    c = s["c"]
    tp = c["K"].torch_prior(c["sysm"].Params, TS, *s["in"], *s["dn"])
    for name, t, got, ref, bar in zip(("prior", "m1y", "dy"), tp, s["got"], s["ref"], s["bar"]):
        worst(f"torch_prior unorm={unorm} {name} vs float64", (t.cpu().double() - ref).abs().max(0).values, bar)
        worst(f"torch_prior unorm={unorm} {name} vs op", (t.cpu().double() - got.double()).abs().max(0).values, bar)


@pytest.mark.parametrize("B", [3, 70])
def test_gru_gates_op_vs_float64(gpu, B):
    """knet_gru_kernel (a thread per hidden unit: B = 3 is 384 threads, B = 70 is 35 blocks); inputs normal * 3 reach
    both sigmoid tails and the tanh tails."""
    rng = np.random.default_rng(B)
    f = lambda *s: torch.tensor(rng.normal(size=s) * 3, dtype=torch.float32)   # noqa: E731
    gi, gh, h = f(B, 3 * H), f(B, 3 * H), f(B, H)
    got = torch.ops.trajknet.gru_gates(gi.to(gpu), gh.to(gpu), h.to(gpu)).cpu()
    bar = 1e-6 * (1 + h.abs() + gi[:, 2 * H:].abs() + gh[:, 2 * H:].abs()).double()
    worst(f"gru_gates op B={B}", (got.double() - R.gru64(gi, gh, h)).abs(), bar)


def test_update_op_vs_float64(gpu):
    """knet_update_kernel across a 256-thread block with a ragged tail (B = 261)."""
    rng = np.random.default_rng(9)
    f = lambda *s: torch.tensor(rng.normal(size=s) * 3, dtype=torch.float32)   # noqa: E731
    pr, KG, dy, lg = f(261, 6), f(261, 30), f(261, 5), torch.tensor(0.3)
    got = torch.ops.trajknet.update(pr.to(gpu), KG.to(gpu), dy.to(gpu), lg.to(gpu)).cpu()
    ref, scale = R.update64(pr, KG, dy, lg)
    worst("update op", (got.double() - ref).abs(), 1e-6 * scale)


# ------------------------------------------------------------------ fused stages, teacher-forced

def check_stages(c, tag, ins, o):
    """Every stage of one fused step against its float64 reference fed the GPU's own upstream outputs."""
    w = c["w"]
    y, u, post, hq, hsig, hs = (t.cpu() for t in ins)
    g = {k: v.cpu() for k, v in o.items()}
    assert all(torch.isfinite(v).all() for v in g.values())
    oSig = g["x2"][:, :H]
    assert torch.equal(g["x2"][:, H:], g["hS"])
    o5, s5 = R.lin64(g["prior"], w["FC5.0.weight"], w["FC5.0.bias"])
    ref, sc = R.gru_cell64(o5, hq, w, "GRU_Q", xscale=s5)
    worst(f"{tag} hQ", (g["hQ"].double() - ref).abs(), 1e-6 * sc)
    ref, sc = R.gru_cell64(g["hQ"], hsig, w, "GRU_Sigma")
    worst(f"{tag} oSig", (oSig.double() - ref).abs(), 1e-6 * sc)
    o1, s1 = R.lin64(oSig, w["FC1.0.weight"], w["FC1.0.bias"])
    o7, s7 = R.lin64(g["dy"], w["FC7.0.weight"], w["FC7.0.bias"])
    ref, sc = R.gru_cell64(torch.cat((o1, o7), 1), hs, w, "GRU_S", xscale=torch.cat((s1, s7), 1))
    worst(f"{tag} hS", (g["hS"].double() - ref).abs(), 1e-6 * sc)
    ref, sc = R.fc2_64(g["x2"], w)
    worst(f"{tag} KG", (g["KG"].double() - ref).abs(), 1e-6 * sc)
    _, ref, sc = R.back64(g["x2"], g["KG"], w)
    worst(f"{tag} hSig", (g["hSig"].double() - ref).abs(), 1e-6 * sc)
    ref, sc = R.update64(g["prior"], g["KG"], g["dy"], w["innov_logit"])
    worst(f"{tag} post", (g["post"].double() - ref).abs(), 1e-6 * sc)


@pytest.mark.parametrize("in_mult,B,unorm", [(1, 1, False), (1, 5, False), (1, 70, False), (5, 1, False),
                                              (5, 5, False), (5, 70, False), (10, 1, False), (10, 5, False),
                                              (10, 70, False), (5, 5, True)])
def test_fused_stages_vs_float64(gpu, in_mult, B, unorm):
    """trajknet::step from non-zero hidden states: d_fc5 6 / 30 / 60 (inside one packed row of 4 x 16, and near the
    64-wide LDS row), a lone sequence / a ragged workgroup / a second FC2 batch tile, once with the 6-entry norm."""
    c = ctx(gpu, in_mult, unorm)
    ins = step_inputs(B, gpu, c, seed=100 * in_mult + B)
    y, u, post, hq, hsig, hs = ins
    o = launch_step(c, *ins)
    op = torch.ops.trajknet.step(y, u, post, hq, hsig, hs, c["pk"], c["ws"], c["dims"], c["params"], c["limits"], TS,
                                 c["norm"])
    for got, key in zip(op, ("post", "hQ", "hSig", "hS", "KG")):   # the op is these three launches
        assert torch.equal(got, o[key]), key
    # the fused prior is the stand-alone kernel's function (the same device code): same bits
    dn = c["norm"] + [None] * (6 - len(c["norm"]))
    pr, _, dy = torch.ops.trajknet.prior(post, u, y, *dn, c["params"], c["limits"], TS)
    assert torch.equal(pr, o["prior"]) and torch.equal(dy, o["dy"])
    check_stages(c, f"fused im={in_mult} B={B} unorm={unorm}", ins, o)


@pytest.mark.parametrize("in_mult,B,unorm", [(1, 5, False), (5, 70, True), (10, 37, False)])
def test_merged_back_front_state_is_two_steps(gpu, in_mult, B, unorm):
    """traj_knet_back_front_f32: after two steps of the merged runner its state buffers (the second step's prior, dy,
    h_Q, h_S, x2 written by the merged launch, h_Sigma by the last back launch from them) are bit for bit those of two
    trajknet::step launch triples, whose stages the test above holds to float64."""
    from trajectory_generation_amd.knet import KNetSequenceRunner
    c = ctx(gpu, in_mult, unorm)
    rng = np.random.default_rng(B)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)   # noqa: E731
    y, m1x0 = f(rng.normal(size=(B, 5, 2))), f(rng.normal(size=(B, 6, 1)) * 0.5)
    u = np.stack([rng.uniform(0, 0.5, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], 1)
    if unorm:
        u = (u - GU["u_mean"]) / GU["u_std"]
    u = f(u)
    run = KNetSequenceRunner(c["model"], B, merge=True)
    out = run.run(y, u, m1x0, use_graph=False, fused=True)
    z = torch.zeros(B, H, device=gpu)
    s0 = launch_step(c, y[:, :, 0].contiguous(), u[:, :, 0].contiguous(), m1x0.reshape(B, 6), z, z, z)
    ins1 = (y[:, :, 1].contiguous(), u[:, :, 1].contiguous(), s0["post"], s0["hQ"], s0["hSig"], s0["hS"])
    s1 = launch_step(c, *ins1)
    assert torch.equal(out[:, :, 0], s0["post"]) and torch.equal(out[:, :, 1], s1["post"])
    for k in ("hQ", "hSig", "hS", "prior", "dy", "x2"):
        assert torch.equal(run.fs[k], s1[k]), k
    check_stages(c, f"merged im={in_mult} B={B} step 2", ins1, {k: run.fs[k] for k in ("hQ", "hSig", "hS", "prior",
                                                                                         "dy", "x2")}
                 | {"KG": s1["KG"], "post": out[:, :, 1]})


# ------------------------------------------------------------------ EKF

def test_ekf_across_a_block_with_clamped_states(gpu):
    """ekf_kernel at B = 70 (64-thread blocks), T = 12, from states at vx_min and omega_max: for half the rows those
    components start beyond the limit, so the finite-difference Jacobian has the zero rows of clamped components."""
    from oracle import knet_oracle as KO
    from trajectory_generation_amd import knet as K
    p = params()
    B, T = 70, 12
    rng = np.random.default_rng(12)
    x0 = np.stack([rng.uniform(0, 2, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.3, 0.3, B),
                   rng.uniform(0.0, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(5.8, 6.0, B)], 1)
    x0[::2, 3] = rng.uniform(-0.05, -0.01, x0[::2].shape[0])    # below vx_min
    x0[::2, 5] = rng.uniform(6.05, 6.4, x0[::2].shape[0])       # above omega_max
    U = np.stack([rng.uniform(0.0, 0.5, (B, T)), rng.uniform(-0.3, 0.3, (B, T))], 1)
    X, x = [], x0
    for t in range(T):
        x = np.array([KO._veh_f64(x[b], U[b, 0, t], U[b, 1, t], p, TS) for b in range(B)])
        X.append(x)
    X = np.stack(X, 2)
    assert (X[:, 3] == p["vx_min"]).any() or (X[:, 5] == p["omega_max"]).any()   # the truth itself rides a limit
    Y = X[:, [0, 1, 3, 4, 5], :] + rng.normal(size=(B, 5, T)) * np.sqrt(np.array(K.EKF_R))[None, :, None]
    est = K.ekf_run(p, TS, Y, U, x0).cpu().numpy()
    ref = KO.ekf_run(p, TS, Y, U, x0, K.EKF_P0, K.EKF_Q, K.EKF_R)
    err = np.abs(est - ref)
    print(f"[knet-stages] ekf: worst err / bar = {err.max() / (1e-8 * (1 + np.abs(ref).max())):.3g}")
    assert np.isfinite(est).all() and (err <= 1e-8 * (1 + np.abs(ref).max())).all()


# ------------------------------------------------------------------ batch independence and isolation

def seq_inputs(B, T, dev, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)   # noqa: E731
    return (f(rng.normal(size=(B, 5, T))),
            f(np.stack([rng.uniform(0, 0.5, (B, T)), rng.uniform(-0.3, 0.3, (B, T))], 1)),
            f(rng.normal(size=(B, 6, 1)) * 0.5))


@pytest.mark.parametrize("groups", [1, 3])
def test_batch_independence_and_determinism(gpu, groups):
    """A sequence's posterior does not depend on its neighbours, its slot in the workgroup of four, its FC2 tile or its
    launch group: sub-batches and the reversed batch reproduce the full batch's rows bit for bit, and so does a second
    call."""
    from trajectory_generation_amd.knet import KNetSequenceRunner
    c = ctx(gpu, 5)
    B, T = 37, 4
    y, u, m = seq_inputs(B, T, gpu, 21)
    run = KNetSequenceRunner(c["model"], B, groups=groups)
    full = run.run(y, u, m, fused=True)
    assert torch.isfinite(full).all()
    assert torch.equal(run.run(y, u, m, fused=True), full)
    for a, b in ((0, 1), (0, 4), (3, 8), (33, 37)):
        sub = KNetSequenceRunner(c["model"], b - a, groups=groups).run(
            y[a:b].contiguous(), u[a:b].contiguous(), m[a:b].contiguous(), use_graph=False, fused=True)
        assert torch.equal(sub, full[a:b]), (a, b)
    rev = KNetSequenceRunner(c["model"], B, groups=groups).run(
        y.flip(0).contiguous(), u.flip(0).contiguous(), m.flip(0).contiguous(), use_graph=False, fused=True)
    assert torch.equal(rev.flip(0), full)


@pytest.mark.parametrize("groups", [1, 3])
def test_nan_stays_in_its_sequence(gpu, groups):
    """NaN is ordinary float data: a NaN measurement of sequence 5 at t = 1 makes that sequence's posterior NaN from
    t = 1 on and leaves every other sequence's bits alone at every t.  Sequence 5's hidden states are not asserted:
    the fused ReLU is fmaxf, which drops a NaN where torch.relu keeps it."""
    from trajectory_generation_amd.knet import KNetSequenceRunner
    c = ctx(gpu, 5)
    B, T = 37, 4
    y, u, m = seq_inputs(B, T, gpu, 21)
    run = KNetSequenceRunner(c["model"], B, groups=groups)
    clean = run.run(y, u, m, use_graph=False, fused=True)
    yn = y.clone()
    yn[5, :, 1] = float("nan")
    bad = run.run(yn, u, m, use_graph=False, fused=True)
    others = [b for b in range(B) if b != 5]
    assert torch.equal(bad[others], clean[others])
    assert torch.equal(bad[5, :, 0], clean[5, :, 0])
    assert torch.isnan(bad[5, :, 1:]).all()


# ------------------------------------------------------------------ forward / backward pairing

def grad_bar(g64):
    return 1e-5 * (g64.abs() + g64.abs().max(1, keepdim=True).values)


@pytest.mark.parametrize("unorm", [False, True])
def test_prior_op_gradient_vs_float64_autograd(gpu, unorm):
    """d(prior, m1y, dy) / d x_post of trajknet::prior (random cotangents, B = 64) against float64 CPU autograd of the
    reference expressions.  Every row is at least 1e-3 away from every kink (verified in float64 here); rows 32..47
    have every state clamped before and after the Euler step and must come back exactly zero."""
    c = ctx(gpu, 5, unorm)
    n, p = norm6(c), params()
    xp, u = R.smooth_inputs(p, G["x_mean"], G["x_std"], seed=2, u_mean=GU["u_mean"] if unorm else None,
                            u_std=GU["u_std"] if unorm else None)
    assert R.kink_distance(p, R.prior_terms(p, TS, xp, u, n[0], n[1], n[4], n[5])).min().item() >= 1e-3
    rng = np.random.default_rng(8)
    f = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    y, cot = f(64, 5), [f(64, 6), f(64, 5), f(64, 5)]
    x64 = xp.double().requires_grad_(True)
    g64, = torch.autograd.grad(R.prior64(p, TS, x64, u, y, *n), [x64], [t.double() for t in cot])
    xg = xp.to(gpu).requires_grad_(True)
    dn = c["norm"] + [None] * (6 - len(c["norm"]))
    outs = torch.ops.trajknet.prior(xg, u.to(gpu), y.to(gpu), *dn, c["params"], c["limits"], TS)
    gg, = torch.autograd.grad(outs, [xg], [t.to(gpu) for t in cot])
    gg = gg.cpu()
    assert (g64[32:48] == 0).all() and (gg[32:48] == 0).all()
    assert (g64[:32].abs().max(1).values > 0).all()
    worst(f"prior gradient unorm={unorm}", (gg.double() - g64).abs(), grad_bar(g64))


def test_gates_and_update_op_gradients_vs_float64_autograd(gpu):
    rng = np.random.default_rng(10)
    f = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32)   # noqa: E731
    B = 64
    for name, op, ref, ins, go in (
            ("gru_gates", torch.ops.trajknet.gru_gates, R.gru64, [f(B, 3 * H) * 3, f(B, 3 * H) * 3, f(B, H) * 3],
             f(B, H)),
            ("update", lambda a, b, d: torch.ops.trajknet.update(a, b, d, torch.tensor(0.3, device=gpu)),
             lambda a, b, d: R.update64(a, b, d, torch.tensor(0.3))[0], [f(B, 6), f(B, 30), f(B, 5)], f(B, 6))):
        a64 = [t.double().requires_grad_(True) for t in ins]
        g64 = torch.autograd.grad(ref(*a64), a64, [go.double()])
        ag = [t.to(gpu).requires_grad_(True) for t in ins]
        gg = torch.autograd.grad(op(*ag), ag, [go.to(gpu)])
        for i, (a, b) in enumerate(zip(gg, g64)):
            worst(f"{name} gradient, input {i}", (a.cpu().double() - b).abs(), grad_bar(b))


# ------------------------------------------------------------------ support envelope

def test_unsupported_shapes_are_refused(gpu):
    """in_mult 11 (FC5 66 wide, past the 64-wide LDS row): no packed size, NotImplementedError from the runner and from
    trajknet::pack, TRAJ_E_UNSUPPORTED from the three step entry points with nothing written; a d_fc2h that is no
    multiple of 256 (not constructible through NNBuild) has no FC2 workspace."""
    from trajectory_generation_amd import _lib
    from trajectory_generation_amd import knet as K
    from trajectory_generation_amd import knet_ops as KO
    from trajectory_generation_amd.batch import params_struct
    sysm = K.VehicleModel(TS, 1, 1, torch.zeros(6, 1))
    sysm.Params.update(LIMITS)
    model = K.KalmanNetNN(gpu)
    model.NNBuild(sysm, in_mult_KNet=11)
    model.eval()
    L, net = _lib.lib(), K.net_struct(model)
    assert net.d_fc5 == 66
    assert L.traj_knet_packed_bytes(C.byref(net)) == 0
    assert L.traj_knet_fc2_workspace_bytes(C.byref(net), 4) == 0
    B = 4
    y, u, m = seq_inputs(B, 2, gpu, 3)
    with pytest.raises(NotImplementedError):
        K.KNetSequenceRunner(model, B).run(y, u, m, fused=True)
    with pytest.raises(NotImplementedError):
        torch.ops.trajknet.pack(KO.step_weights(model), KO.step_dims(model))
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=gpu)   # noqa: E731
    pk, ws = torch.zeros(1 << 20, device=gpu), nan(64 * B * 32)
    one6, one5 = torch.ones(6, device=gpu), torch.ones(5, device=gpu)
    hq, hsig, hs = nan(B, H), nan(B, H), nan(B, H)
    prior, dy, x2, KG, post = nan(B, 6), nan(B, 5), nan(B, 2 * H), nan(B, 30), nan(B, 6)
    outs = (ws, hq, hsig, hs, prior, dy, x2, KG, post)
    assert L.traj_knet_front_f32(C.byref(params_struct(sysm.Params)), C.byref(K.limits_struct(sysm.Params)), TS,
                                 C.byref(net), p(pk), B, p(m), p(u), 4, 2, p(y), 10, 2, p(one6), p(one6), p(one5),
                                 p(one5), None, None, p(hq), p(hsig), p(hs), p(prior), p(dy), p(x2),
                                 st) == _lib.TRAJ_E_UNSUPPORTED
    assert L.traj_knet_fc2_f32(C.byref(net), B, p(x2), p(ws), ws.numel() * 4, st) == _lib.TRAJ_E_UNSUPPORTED
    assert L.traj_knet_back_f32(C.byref(net), p(pk), B, p(x2), p(ws), p(prior), p(dy), p(hsig), p(post), None, 0, 0,
                                p(KG), st) == _lib.TRAJ_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs)
    good = K.net_struct(ctx(gpu, 5)["model"])
    assert L.traj_knet_fc2_workspace_bytes(C.byref(good), B) == (10240 // 320) * B * 32 * 4
    good.d_fc2h = 10240 + 128
    assert L.traj_knet_fc2_workspace_bytes(C.byref(good), B) == 0
    assert L.traj_knet_packed_bytes(C.byref(good)) == 0


@pytest.mark.parametrize("in_mult", [1, 7])
def test_other_supported_widths_run_fused(gpu, in_mult):
    """knet_ok accepts any d_fc5 <= 64: in_mult 1 (FC5 6 wide) and 7 (42) through the fused runner, merged and
    unmerged, against the float64 reference at the end-to-end bar."""
    from trajectory_generation_amd.knet import KNetSequenceRunner
    c = ctx(gpu, in_mult)
    B, T = 9, 3
    y, u, m = seq_inputs(B, T, gpu, in_mult)
    got = KNetSequenceRunner(c["model"], B).run(y, u, m, fused=True)
    assert torch.equal(KNetSequenceRunner(c["model"], B, merge=False).run(y, u, m, use_graph=False, fused=True), got)
    ref = R.run64(c["w"], params(), TS, y, u, m, *norm6(c)[:4])[0]
    err = (got.cpu().double() - ref).abs().max().item()
    print(f"[knet-stages] fused im={in_mult}: worst err / bar = {err / (2e-4 * (1 + ref.abs().max().item())):.3g}")
    assert err <= 2e-4 * (1 + ref.abs().max().item())

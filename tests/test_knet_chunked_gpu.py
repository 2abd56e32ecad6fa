"""Chunk-and-shuffle KalmanNet training on the GPU (trajectory_generation_amd/pipeline_indipendent_chunking.py,
csrc/knet_opt.h): the gather kernel and the clip + AdamW kernel alone, then the pipeline -- against the reference's own
run (tests/golden/knet_chunked.npz), against the module path, graph replay, a short training run and the driver.

Bars (none is derived from what the code under test gives):
  gather        bit-equal to the float32 torch expression on the device (one subtraction, one division per value; the
                noisy start one multiplication and one addition).  n_traj 5, T_full 23, Tc 5 (cpt 4, a tail of 3);
                B = 67 carries repeats, chunk 0, the last chunk and ids out of range on both sides; B = 3 has room for
                chunk 0, the last chunk and one id out of range only.
  clip + AdamW  total within 2^-22 relative of the float64 norm; per element |q - q64| <= max(8 E, S spacing(|q64|))
                for q = p, m, v, with q64 a float64 evaluation of the documented formulas on the same float32 inputs,
                S = 3 calls and E the worst deviation of torch.optim.AdamW + clip_grad_norm_ (float32, on the device)
                from the same q64 over all tensors.
  vs reference  tests/test_knet_train.py's tolerances: epoch mean loss 1e-4 relative (first epoch) and 1e-3 (second),
                the recorded parameter deltas 2e-3 of the delta's norm.
  plain step    after the fused epochs one torch optimizer.step() on the device: the clip + AdamW bar with S = 1,
                E the worst deviation of torch.optim.AdamW in float32 on the CPU from the same state and gradients.
Every test prints its own worst err / bar with -s.
"""
import numpy as np
import pytest
import torch

from tests.test_knet_chunked import CG, real_data

pytestmark = pytest.mark.gpu
NAMES = [str(k) for k in CG["delta_names"]]
PARAMS = dict(N_batch=int(CG["N_batch"]), T_train=int(CG["T_train"]), m=6, n=5, CompositionLoss=True, alpha=0.8)


# ------------------------------------------------------------------ 1. the gather kernel

@pytest.mark.parametrize("B", [3, 67])
def test_chunk_gather_is_exact(gpu, B):
    from trajectory_generation_amd import knet_train_fused as F
    from trajectory_generation_amd.pipeline_indipendent_chunking import create_chunks
    rng = np.random.default_rng(21)
    n_traj, T_full, Tc, cpt = 5, 23, 5, 4
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=gpu)   # noqa: E731
    y, u, x = 3.0 * t(n_traj, 5, T_full) + 1.0, t(n_traj, 2, T_full), 2.0 * t(n_traj, 6, T_full) - 0.5
    xm, xs, ym, ys = t(1, 6, 1), 0.5 + t(1, 6, 1).abs(), t(1, 5, 1), 0.5 + t(1, 5, 1).abs()
    noise = t(B, 6)
    if B == 3:
        ids = [n_traj * cpt - 1, n_traj * cpt, 0]
    else:
        ids = rng.integers(0, n_traj * cpt, B).tolist()
        ids[:6] = [0, n_traj * cpt - 1, 7, 7, n_traj * cpt, -1]
    ids_t = torch.tensor(ids, dtype=torch.int32, device=gpu)
    bad = torch.tensor([not (0 <= c < n_traj * cpt) for c in ids], device=gpu)
    assert bad.any() and 0 in ids and n_traj * cpt - 1 in ids and (B == 3 or len(set(ids)) < B)
    pick = torch.tensor([c if 0 <= c < n_traj * cpt else 0 for c in ids], device=gpu)
    yc, uc, xc = (create_chunks(a, Tc)[pick] for a in (y, u, x))
    y_norm, x_norm = (yc - ym) / ys, (xc - xm) / xs   # the expressions the pipelines use
    m1x0 = x_norm[:, :, 0] + noise * 0.3
    zero = lambda a: torch.where(bad.reshape(-1, *([1] * (a.dim() - 1))), torch.zeros((), device=gpu), a)   # noqa: E731
    ref = [zero(y_norm).permute(2, 0, 1), zero(uc).permute(2, 0, 1), zero(x_norm), zero(y_norm), zero(m1x0)]
    got = F.chunk_gather(y, u, x, ids_t, Tc, xm, xs, ym, ys, noise=noise, noise_std=0.3)
    for name, a, r in zip(("Y", "U", "x_tgt", "y_tgt", "m1x0"), got, ref):
        assert a.shape == r.shape, name
        nd = (a != r).sum().item()
        print(f"[knet-chunked] gather B={B} {name}: {nd} of {a.numel()} values differ")
        assert torch.equal(a, r.contiguous()), name
    for a in got:   # the out-of-range rows are all zeros
        rows = a[:, bad] if a.shape[0] == Tc else a[bad]
        assert rows.numel() > 0 and (rows == 0).all()
    again = F.chunk_gather(y, u, x, ids_t, Tc, xm, xs, ym, ys, noise=noise, noise_std=0.3)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    no_yt = F.chunk_gather(y, u, x, ids_t, Tc, xm, xs, ym, ys, noise=noise, noise_std=0.3, want_y_tgt=False)
    assert no_yt[3] is None and all(torch.equal(a, b) for a, b in zip(got[:3] + got[4:], no_yt[:3] + no_yt[4:]))
    no_noise = F.chunk_gather(y, u, x, ids_t, Tc, xm, xs, ym, ys, noise=None, noise_std=0.3)
    zero_noise = F.chunk_gather(y, u, x, ids_t, Tc, xm, xs, ym, ys, noise=torch.zeros_like(noise), noise_std=0.3)
    assert all(torch.equal(a, b) for a, b in zip(no_noise, zero_noise))
    assert torch.equal(no_noise[4], got[2][:, :, 0])


# ------------------------------------------------------------------ 2. the clip + AdamW kernel

LENGTHS = (1, 5, 36, 1000, 4099, 65539)
HYPER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
LRS = (1e-3, 1e-3, 5e-4)   # the third call's lr is changed through the device scalar


def opt_inputs(scale):
    """Host float32 p, g, m, v per tensor; m / v as a few earlier steps would leave them; a few exact-zero gradients."""
    rng = np.random.default_rng(31)
    out = []
    for n in LENGTHS:
        p, g = rng.normal(size=n), scale * rng.normal(size=n)
        if n >= 36:
            g[rng.integers(0, n, 5)] = 0.0
        m, v = 0.1 * scale * rng.normal(size=n), 1e-3 * (scale * rng.normal(size=n)) ** 2
        out.append([torch.tensor(a, dtype=torch.float32) for a in (p, g, m, v)])
    return out


def adamw64(P, G, M, V, t, lr, max_norm, betas, eps, weight_decay):
    """The documented formulas in float64 on lists of tensors; returns the pre-clip norm."""
    b1, b2 = betas
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in G)).item()
    coef = min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0
    for p, g, m, v in zip(P, G, M, V):
        g = coef * g.double()
        p.mul_(1 - lr * weight_decay)
        m.add_((1 - b1) * (g - m))
        v.mul_(b2).add_((1 - b2) * g * g)
        p.sub_((lr / (1 - b1 ** t)) * m / (v.sqrt() / np.sqrt(1 - b2 ** t) + eps))
    return total


def on_device(inputs, dev):
    """p / g / m / v on the device.  Tensor 4 (4099): all four are slices at element offset 1 of larger buffers (a
    scalar head, then the float4 body); tensor 3 (1000): p alone at offset 3 (mixed offsets: element by element)."""
    out = []
    for i, quad in enumerate(inputs):
        dq = []
        for j, a in enumerate(quad):
            off = 1 if i == 4 else (3 if i == 3 and j == 0 else 0)
            buf = torch.zeros(a.numel() + 8, dtype=torch.float32, device=dev)
            buf[off:off + a.numel()].copy_(a)
            dq.append(buf[off:off + a.numel()])
        out.append(dq)
    assert out[4][0].data_ptr() % 16 == 4 and out[3][0].data_ptr() % 16 == 12 and out[3][1].data_ptr() % 16 == 0
    return out


def run_kernel(inputs, dev, max_norm):
    from trajectory_generation_amd import knet_train_fused as F
    d = on_device(inputs, dev)
    P, G, M, V = ([q[j] for q in d] for j in range(4))
    opt = F.ClipAdamW(P, G, M, V, LRS[0], max_norm=max_norm, **HYPER)
    totals = []
    for lr in LRS:
        opt.lr.fill_(lr)
        opt.step()
        totals.append(opt.total_norm.item())
    assert opt.t.item() == len(LRS)
    assert all(torch.equal(g.cpu(), q[1]) for g, q in zip(G, inputs))   # g is only read
    return [[a.cpu() for a in x] for x in (P, M, V)], totals


def run_torch(inputs, dev, max_norm):
    ps = [torch.nn.Parameter(q[0].to(dev)) for q in inputs]
    opt = torch.optim.AdamW(ps, lr=LRS[0], **HYPER)
    for p, q in zip(ps, inputs):   # the state three earlier steps would have left: m, v given, the step count 0
        opt.state[p].update(step=torch.tensor(0.0), exp_avg=q[2].to(dev), exp_avg_sq=q[3].to(dev))
    for lr in LRS:
        opt.param_groups[0]["lr"] = lr
        for p, q in zip(ps, inputs):
            p.grad = q[1].to(dev).clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm)
        opt.step()
    return [[p.detach().cpu() for p in ps], [opt.state[p]["exp_avg"].cpu() for p in ps],
            [opt.state[p]["exp_avg_sq"].cpu() for p in ps]]


@pytest.mark.parametrize("scale,max_norm,clipped", [(0.01, 5.0, False), (0.1, 5.0, True), (0.1, 0.0, False)])
def test_clip_adamw_vs_float64(gpu, scale, max_norm, clipped):
    inputs = opt_inputs(scale)
    P64, G, M64, V64 = ([q[j].double().clone() for q in inputs] for j in range(4))
    tot64 = [adamw64(P64, G, M64, V64, t + 1, lr, max_norm, **HYPER) for t, lr in enumerate(LRS)]
    assert (tot64[0] > 5.0) == (scale == 0.1) and clipped == (max_norm > 0 and tot64[0] > max_norm)
    got, totals = run_kernel(inputs, gpu, max_norm)
    again, totals2 = run_kernel(inputs, gpu, max_norm)
    assert totals == totals2
    for a, b in zip(got, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))   # equal inputs, equal bits
    for t, t64 in zip(totals, tot64):
        assert abs(t - t64) <= 2.0 ** -22 * t64, (t, t64)
    ref32 = run_torch(inputs, gpu, max_norm)
    S = len(LRS)
    for name, g_, r32, r64 in zip(("p", "m", "v"), got, ref32, (P64, M64, V64)):
        E = max((a.double() - b).abs().max().item() for a, b in zip(r32, r64))
        worst = 0.0
        for a, b in zip(g_, r64):
            bar = np.maximum(8 * E, S * np.spacing(b.abs().numpy().astype(np.float32)).astype(np.float64))
            err = (a.double() - b).abs().numpy()
            worst = max(worst, float((err / bar).max()))
            assert np.isfinite(err).all() and (err <= bar).all(), (name, a.numel(), float((err / bar).max()))
        print(f"[knet-chunked] clip+AdamW scale={scale} max_norm={max_norm} {name}: torch float32 E = {E:.3g}, "
              f"worst err / bar = {worst:.3f}")
    if clipped:   # the clip reaches the update
        free = run_kernel(inputs, gpu, 0.0)[0]
        assert (free[1][5] - got[1][5]).abs().max() > 1e-3 * scale


# ------------------------------------------------------------------ 3. the pipeline on the golden configuration

def setup(dev, train=False, lr=1e-4, wd=1e-5):
    from tests.test_knet_train import _build
    model, _ = _build(dev)
    model.train(train)
    y, u, x, stats = real_data()
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd)
    return model, opt, (y, u, x), stats


def snapshot(model, names=None):
    return {k: v.detach().clone() for k, v in model.named_parameters() if names is None or k in names}


_RUNS = {}


def two_epochs(dev, fused):
    """Two epochs with the golden permutations and noise, eval mode (computed once per path and shared)."""
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    if fused not in _RUNS:
        model, opt, data, stats = setup(dev)
        r = dict(model=model, opt=opt, losses=[], delta=[], graph_ids=[])
        for e in range(2):
            before = snapshot(model, NAMES)
            r["losses"].append(PC.chunked_batches(model, opt, *data, stats, dict(PARAMS, device=dev, fused=fused),
                                                  perm=torch.tensor(CG["perm"][e]), noise=torch.tensor(CG["noise"][e])))
            r["delta"].append({k: (v - before[k]).cpu() for k, v in snapshot(model, NAMES).items()})
            if fused:
                st = PC.fused_state(model)
                r["graph_ids"].append({B: [id(g) for g in b.R.graphs.values()] for B, b in st.batch.items()})
        _RUNS[fused] = r
    return _RUNS[fused]


@pytest.mark.parametrize("fused", [True, False])
def test_two_epochs_vs_reference(gpu, fused):
    r = two_epochs(gpu, fused)
    worst = 0.0
    for e, tol in ((0, 1e-4), (1, 1e-3)):
        assert len(r["losses"][e]) == 3
        mean, ref = sum(r["losses"][e]) / 3, float(CG["epoch_loss"][e])
        print(f"[knet-chunked] fused={fused} epoch {e}: mean loss {mean:.8f} vs reference {ref:.8f}, "
              f"rel err / tol = {abs(mean - ref) / ref / tol:.3f}")
        assert abs(mean - ref) <= tol * ref
        for i, k in enumerate(NAMES):
            d, ref_norm, ref_head = r["delta"][e][k], float(CG["delta_norm"][e][i]), CG["delta_head"][e][i]
            head = d.reshape(-1)[:8].numpy()
            err = max(abs(float(d.norm()) - ref_norm), np.abs(head - ref_head[:head.size]).max()) / ref_norm
            worst = max(worst, err)
            assert err <= 2e-3, (e, k, err)
    print(f"[knet-chunked] fused={fused}: worst parameter-delta err / (2e-3 norm) = {worst / 2e-3:.3f}")


def test_fused_vs_module_path(gpu):
    f, m = two_epochs(gpu, True), two_epochs(gpu, False)
    for e, tol in ((0, 1e-4), (1, 1e-3)):
        for a, b in zip(f["losses"][e], m["losses"][e]):
            print(f"[knet-chunked] epoch {e} batch loss fused {a:.8f} module {b:.8f}: rel err / tol = "
                  f"{abs(a - b) / b / tol:.3f}")
            assert abs(a - b) <= tol * b


def test_replay_and_optimizer_state(gpu):
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    r = two_epochs(gpu, True)
    model, opt = r["model"], r["opt"]
    st = PC.fused_state(model)
    # one graph per batch size, captured in the first epoch and replayed since
    assert sorted(st.batch) == [4, 6] and st.graphs == 2
    assert r["graph_ids"][0] == r["graph_ids"][1] and all(len(v) == 1 for v in r["graph_ids"][1].values())
    assert all(p.grad is None for p in model.parameters())   # the update reads the runner's buffers
    for p in model.parameters():
        s = opt.state[p]
        assert float(s["step"]) == 6 and s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # one plain torch step continues from the fused epochs' state: float64 AdamW at t = 7
    gen = torch.Generator().manual_seed(5)
    ps = list(model.parameters())
    G = [0.01 * torch.randn(p.shape, generator=gen) for p in ps]
    P64 = [p.detach().cpu().double() for p in ps]
    M64 = [opt.state[p]["exp_avg"].cpu().double() for p in ps]
    V64 = [opt.state[p]["exp_avg_sq"].cpu().double() for p in ps]
    g = opt.param_groups[0]
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]   # the same step in float32 on the CPU: E
    opt_cpu = torch.optim.AdamW(cpu, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
    for c, p, gr in zip(cpu, ps, G):
        opt_cpu.state[c].update(step=torch.tensor(6.0), exp_avg=opt.state[p]["exp_avg"].cpu().clone(),
                                exp_avg_sq=opt.state[p]["exp_avg_sq"].cpu().clone())
        c.grad = gr.clone()
        p.grad = gr.to(gpu)
    adamw64(P64, G, M64, V64, 7, g["lr"], 0.0, g["betas"], g["eps"], g["weight_decay"])
    opt_cpu.step()
    opt.step()
    opt.zero_grad()
    E = max((c.detach().double() - p64).abs().max().item() for c, p64 in zip(cpu, P64))
    worst = 0.0
    for p, p64 in zip(ps, P64):
        err = (p.detach().cpu().double() - p64).abs().numpy()
        bar = np.maximum(8 * E, np.spacing(p64.abs().numpy().astype(np.float32)).astype(np.float64))
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all()
    print(f"[knet-chunked] plain optimizer.step() after the fused epochs: float32-CPU E = {E:.3g}, "
          f"worst err / bar = {worst:.3f}")
    assert all(float(opt.state[p]["step"]) == 7 for p in ps)


def test_lr_is_read_from_the_device(gpu):
    """Halving the learning rate between two calls halves the next batch's update (wd = 0: the step is linear in lr
    for the same gradient and moments), through the same graph."""
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    delta = []
    for halve in (False, True):
        model, opt, data, stats = setup(gpu, wd=0.0)
        p = dict(PARAMS, device=gpu, fused=True)
        PC.chunked_batches(model, opt, *data, stats, p, perm=torch.tensor(CG["perm"][0]),
                           noise=torch.tensor(CG["noise"][0]))
        st = PC.fused_state(model)
        ids = {B: [id(g) for g in b.R.graphs.values()] for B, b in st.batch.items()}
        if halve:
            opt.param_groups[0]["lr"] *= 0.5
        before = snapshot(model, NAMES)
        PC.chunked_batches(model, opt, *data, stats, p, perm=torch.tensor(CG["perm"][1][:6]),   # one batch of 6
                           noise=torch.tensor(CG["noise"][1][:6]))
        assert PC.fused_state(model) is st and st.graphs == 2
        assert ids == {B: [id(g) for g in b.R.graphs.values()] for B, b in st.batch.items()}
        assert all(float(opt.state[q]["step"]) == 4 for q in model.parameters())
        delta.append({k: float((v - before[k]).norm()) for k, v in snapshot(model, NAMES).items()})
    for k in NAMES:
        ratio = delta[1][k] / delta[0][k]
        print(f"[knet-chunked] lr halved: ||dp|| ratio of {k} = {ratio:.6f}")
        assert abs(ratio - 0.5) <= 1e-3 * 0.5, (k, ratio)


def test_longer_chunks_fused_vs_module_path(gpu):
    """T_train = 20 (the golden trajectories whole, one batch of 4), three updates at lr 1e-3: the two paths' losses
    before the first update within 1e-4, after it within 1e-3 (tests/test_knet_train.py's tolerances)."""
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    gen = torch.Generator().manual_seed(9)
    noise = torch.randn(3, 4, 6, generator=gen)
    losses = {}
    for fused in (True, False):
        model, opt, data, stats = setup(gpu, lr=1e-3)
        p = dict(PARAMS, T_train=20, N_batch=4, device=gpu, fused=fused)
        losses[fused] = [PC.chunked_batches(model, opt, *data, stats, p, perm=torch.arange(4), noise=noise[i])[0]
                         for i in range(3)]
    for i, (a, b) in enumerate(zip(losses[True], losses[False])):
        tol = 1e-4 if i == 0 else 1e-3
        print(f"[knet-chunked] K = 20 update {i}: fused {a:.8f} module {b:.8f}, rel err / tol = "
              f"{abs(a - b) / b / tol:.3f}")
        assert abs(a - b) <= tol * b
    assert losses[False][2] != losses[False][0]


def test_state_follows_parameters_and_statistics(gpu):
    """A parameter whose storage moved is updated where it now lives (the kernel's table is rebuilt), and statistics
    other than the model's are refused, the y pair included."""
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    model, opt, data, stats = setup(gpu, lr=1e-3)
    p = dict(PARAMS, device=gpu, fused=True)
    one = dict(perm=torch.tensor(CG["perm"][0][:6]), noise=torch.tensor(CG["noise"][0][:6]))
    PC.chunked_batches(model, opt, *data, stats, p, **one)
    st = PC.fused_state(model)
    w = model.FC7[0].bias
    w.data = w.data.clone()
    before = w.detach().clone()
    PC.chunked_batches(model, opt, *data, stats, p, **one)
    assert PC.fused_state(model) is not st
    assert (w.detach() - before).abs().max() > 1e-4 and float(opt.state[w]["step"]) == 2
    for k in ("x_mean", "x_std", "y_mean", "y_std"):
        with pytest.raises(ValueError):
            PC.chunked_batches(model, opt, *data, dict(stats, **{k: stats[k] * 1.5 + 0.1}), p, **one)


def test_refuses_other_optimizers(gpu):
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    model, _, data, stats = setup(gpu)
    p = dict(PARAMS, device=gpu, fused=True)
    halves = [list(model.parameters())[:3], list(model.parameters())[3:]]
    for opt in (torch.optim.Adam(model.parameters(), lr=1e-4), torch.optim.AdamW(model.parameters(), amsgrad=True),
                torch.optim.AdamW(model.parameters(), maximize=True),
                torch.optim.AdamW([{"params": halves[0]}, {"params": halves[1]}])):
        with pytest.raises(NotImplementedError):
            PC.chunked_batches(model, opt, *data, stats, p)


def test_train_epoch_chunked_learns_fused(gpu):
    from trajectory_generation_amd import pipeline_indipendent_chunking as PC
    torch.manual_seed(3)
    model, opt, data, stats = setup(gpu, lr=1e-3)
    p = dict(PARAMS, device=gpu, fused=True)
    losses = [PC.train_epoch_chunked(model, opt, *data, stats, p)[0] for _ in range(8)]
    print(f"[knet-chunked] train mode, lr 1e-3: epoch losses {[round(v, 5) for v in losses]}")
    assert all(np.isfinite(losses))
    assert min(losses[-3:]) < losses[0]
    st = PC.fused_state(model)
    assert model.training and st.graphs == 2
    for b in st.batch.values():
        assert b.R.train
        assert all((m == 0).any() and ((m == 0) | (m > 1)).all() for m in b.R.M.values())   # masks were drawn


def test_pipeline_driver(gpu, tmp_path):
    from trajectory_generation_amd import knet as K
    from trajectory_generation_amd import pipeline_chunk_shuffle as PS
    torch.manual_seed(4)
    model, _, (y, u, x), stats = setup(gpu)
    records = []
    pipe = PS.Pipeline_Vehicle_KNet(str(tmp_path), "chunked", log=records.append)
    pipe.set_models(model.sys, model)
    assert isinstance(model.sys, K.VehicleModel)
    chunks = tuple(PS.create_chunks(a[:2], 5) for a in (y, u, x))   # 8 chunks: batches of 6 and 2
    pipe.set_data(chunks, tuple(a[2:3] for a in (y, u, x)), tuple(a[3:4] for a in (y, u, x)), stats, gpu)
    pipe.set_training_params(2, 6, 1e-4, 1e-5, 5, CompositionLoss=True, alpha=0.8, fused=True)
    pipe.train()
    assert (tmp_path / "best_model_chunked.pt").exists()
    out = pipe.test()
    assert out is not None and np.isfinite(out[0]) and np.isfinite(float(out[1]))
    epochs = [r for r in records if "epoch" in r]
    assert [r["epoch"] for r in epochs] == [0, 1]
    assert all(np.isfinite(r["train_loss"]) and np.isfinite(r["val_loss_linear"]) for r in epochs)
    assert sorted(PS.fused_state(model).batch) == [2, 6]

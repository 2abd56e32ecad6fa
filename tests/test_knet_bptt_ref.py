"""The float64 manual truncated-BPTT sweep of tests/_knet_bptt_ref.py (the blueprint of knet_train_fused.py) against
torch.autograd on the same float64 chunk: every parameter's gradient and d loss / d (initial posterior) to 1e-10 of the
gradient's norm.  B = 4, K = 10 (the first ten steps of tests/golden/knet.npz, weights of tests/_knet_weights.py);
composite and plain loss, eval mode and explicit dropout masks.  CPU only.

Also held here, with the reference alone: the chunk inputs the GPU tests compare on (tests/test_knet_train_fused_gpu.py)
leave at most one of the four sequences within 1e-3 of a kink of the vehicle step, for both network widths."""
import numpy as np
import pytest
import torch

from tests import _knet_bptt_ref as BR
from tests import _knet_ref as R
from tests._knet_weights import LIMITS, knet_weights

G = np.load("tests/golden/knet.npz")
K = 10
KINK_MIN = 1e-3


def params():
    p = dict(R.PARAMS)
    p.update(LIMITS)
    return p


def chunk_inputs(in_mult=5, seed=0):
    w = {k: torch.tensor(v) for k, v in knet_weights(seed=seed, in_mult=in_mult).items()}
    f = lambda k: torch.tensor(G[k], dtype=torch.float32)   # noqa: E731
    norm = (f("x_mean"), f("x_std"), f("y_mean"), f("y_std"), None, None)
    x_norm = ((f("x_true") - f("x_mean")) / f("x_std"))[:, :, :K]
    return w, dict(y_seq=f("y_norm")[:, :, :K], u_seq=f("u")[:, :, :K], x_tgt=x_norm, m1x0=f("m1x0").reshape(-1, 6),
                   norm=norm)


@pytest.mark.parametrize("composite", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_manual_sweep_equals_autograd(composite, masked):
    w, D = chunk_inputs()
    masks = BR.draw_masks(w, K, 4, seed=5) if masked else None
    gx = torch.tensor(np.random.default_rng(2).normal(size=(4, 6, K)) * 1e-3) if masked else None
    kw = dict(D, alpha=0.8, composite=composite, masks=masks, g_extra=gx)
    a = BR.sweep(w, params(), float(G["Ts"]), **kw)
    b = BR.autograd_chunk(w, params(), float(G["Ts"]), **kw)
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-12 * abs(float(b["loss"]))
    assert set(a["grads"]) == set(b["grads"]) == set(w)
    worst = 0.0
    for k, ref in list(b["grads"].items()) + [("g_x0", b["g_x0"])]:
        got = a["g_x0"] if k == "g_x0" else a["grads"][k]
        assert got.shape == ref.shape, k
        assert ref.norm() > 0, k
        err = ((got - ref).norm() / ref.norm()).item()
        worst = max(worst, err)
        assert err <= 1e-10, (k, err)
    print(f"[knet-bptt] composite={composite} masked={masked}: worst relative gradient error {worst:.2e}")


@pytest.mark.parametrize("in_mult", [5, 10])
def test_chunk_inputs_stay_clear_of_kinks(in_mult):
    """What the GPU comparison relies on: at most one sequence comes within 1e-3 of a kink over the chunk."""
    w, D = chunk_inputs(in_mult)
    tape = BR.forward_tape(BR._w(w, torch.float64), params(), float(G["Ts"]), D["y_seq"], D["u_seq"], D["m1x0"],
                           D["norm"])
    d = BR.chunk_kink_distance(params(), float(G["Ts"]), tape, D["norm"])
    print(f"[knet-bptt] in_mult {in_mult}: kink distance per sequence {d.tolist()}")
    assert (d < KINK_MIN).sum().item() <= 1

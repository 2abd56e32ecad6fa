"""csrc/workload.hip on the GPU: the spline coefficient kernel and the workload builder against the same text on the CPU
(traj_gen_spline_coef_host, traj_gen_workload_host), sharding by id_offset, and the plumbing through
PathSet.build_device, make_workload_device and dataset.generate(device_workload=True)."""
import numpy as np
import pytest
import torch

from tests._workload_cases import CASE_IDS, CASES, KINDS
from trajectory_generation_amd import _lib
from trajectory_generation_amd import batch as TB
from trajectory_generation_amd.workload import make_workload, make_workload_device, workload_rows_host

pytestmark = pytest.mark.gpu

# What the device's libm can round differently from the host's: atan in phi (every kind) and sincos in a sinusoid
# row's Y and phi.  The bar is 4 x the worst absolute difference measured over the nine (kind, case) workloads below,
# capped at 1e-13.  Measured on an MI355X with ROCm's device library against glibc: 0 in every row of all nine -- the
# device's atan and sincos returned the host's bits on these inputs -- so the bar is 0: equality.  A device library or
# libc whose last bits differ here fails this test; the bar is then re-measured by the same rule.
LIBM_BAR = min(4 * 0.0, 1e-13)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return (a.view(np.int64) if a.dtype == np.float64 else a).tolist()


def coef_rows():
    """B = 67 (one wave plus three lanes), kmax = 12: nk cycling 2, 3, 4, 5, 12 on irregular knots, every seventh row of
    kind 0 or 1 (with knots that must not be read as a spline's), and row 41 with a repeated knot."""
    rng = np.random.default_rng(31)
    B, kmax = 67, 12
    kinds = np.full(B, 2, np.int32)
    nk = np.zeros(B, np.int32)
    xk, yk = np.zeros((B, kmax)), np.zeros((B, kmax))
    for b in range(B):
        n = (2, 3, 4, 5, 12)[b % 5]
        nk[b] = n
        xk[b, :n] = rng.uniform(-10.0, 10.0) + np.cumsum(rng.uniform(0.2, 5.0, n))
        yk[b, :n] = rng.uniform(-3.0, 3.0, n)
        if b % 7 == 3:
            kinds[b] = (b // 7) % 2
    xk[41, 2] = xk[41, 1]
    assert kinds[41] == 2 and nk[41] == 3
    return kinds, nk, xk, yk


def test_spline_coef_batch_equals_host(gpu):
    kinds, nk, xk, yk = coef_rows()
    B, kmax = xk.shape
    want, want_flag = TB.spline_coef_host(kinds, nk, xk, yk)
    assert want_flag.tolist() == [1 if b == 41 else 0 for b in range(B)]
    d = [torch.as_tensor(a, device=gpu) for a in (kinds, nk, xk, yk)]
    coef = torch.full((B, kmax - 1, 4), float("nan"), dtype=torch.float64, device=gpu)
    flag = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    _lib.check(_lib.lib().traj_gen_spline_coef_batch(B, kmax, *[_lib.ptr(t) for t in d], _lib.ptr(coef), _lib.ptr(flag),
                                                     _lib.stream()), "traj_gen_spline_coef_batch")
    assert flag.cpu().tolist() == want_flag.tolist()
    assert bits(coef) == bits(want)
    ps = TB.PathSet.build_device(kinds, np.zeros((B, 4)), nk, xk, yk, check=False)
    assert bits(ps.coef) == bits(want) and ps.xk.shape == (B, kmax)
    with pytest.raises(ValueError, match="trajectory 41:"):
        TB.PathSet.build_device(kinds, np.zeros((B, 4)), nk, xk, yk)


@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_workload_batch_against_host(gpu, kind, case):
    """The kernel and traj_gen_workload_host are one text: everything bit for bit, except phi (the device's atan) and a
    sinusoid row's Y and phi (the device's sincos), which stay within LIBM_BAR (4 x the measured worst, which is 0)."""
    seed, off, B = CASES[case]
    h = workload_rows_host(B, kind, seed, off)
    w = make_workload_device(B, kind=kind, seed=seed, id_offset=off, device=gpu)
    p = w["paths"]
    assert w["knots"] is None and w["ids"].tolist() == list(range(off, off + B)) and w["vref"].shape == (21,)
    assert bits(w["kinds"]) == bits(h["kinds"]) and bits(p.nk) == bits(h["nk"])
    for got, key in ((w["pcs"], "pcs"), (p.xk, "xk"), (w["yk"], "yk"), (p.coef, "coef"), (w["u0"], "u0")):
        assert bits(got) == bits(h[key]), key
    assert p.kind is w["kinds"] and p.pc is w["pcs"]
    x0 = w["x0"].cpu().numpy()
    for col in (0, 3, 4, 5):
        assert bits(x0[:, col].copy()) == bits(h["x0"][:, col].copy()), col
    sinus = h["kinds"] == 1
    dY = np.abs(x0[:, 1] - h["x0"][:, 1])
    dphi = np.abs(x0[:, 2] - h["x0"][:, 2])
    print(f"{kind} {CASE_IDS[case]}: |dY| sinusoid {dY[sinus].max(initial=0.0):.3e} "
          f"other {dY[~sinus].max(initial=0.0):.3e} |dphi| {dphi.max():.3e}")
    assert bits(x0[~sinus, 1].copy()) == bits(h["x0"][~sinus, 1].copy())
    assert dY.max() <= LIBM_BAR and dphi.max() <= LIBM_BAR


@pytest.mark.parametrize("kind", ["spline", "mixed"])
def test_sharding_by_id_offset(gpu, kind):
    whole = make_workload_device(8, kind=kind, seed=3, device=gpu)
    part = make_workload_device(5, kind=kind, seed=3, id_offset=3, device=gpu)
    assert part["ids"].tolist() == whole["ids"][3:].tolist()
    for key in ("kinds", "pcs", "yk", "x0", "u0"):
        assert bits(part[key]) == bits(whole[key][3:]), key
    for f in ("nk", "xk", "coef"):
        assert bits(getattr(part["paths"], f)) == bits(getattr(whole["paths"], f)[3:]), f


def test_generate_with_the_device_workload(gpu):
    """dataset.generate(device_workload=True): the closed loop starts from the device builder's x0 on its PathSet -- the
    result is run_closed_loop on the builder's tensors, bit for bit -- and an injected closed_loop gets that dict."""
    from trajectory_generation_amd import dataset as D
    from trajectory_generation_amd.dataset.schema import FAILED_STATUS
    B, T, N, Ts = 8, 3, 20, 0.05
    X, U, st = D.generate(B, T, N=N, Ts=Ts, device_workload=True)
    w = make_workload_device(B, N, Ts, device=gpu)
    assert bits(X[:, 0]) == bits(w["x0"])
    assert int(st.max()) < FAILED_STATUS
    ref = TB.run_closed_loop(w["x0"], w["u0"], w["paths"], w["vref"], T, TB.config_struct(N=N, Ts=Ts, polish_mode=0))
    assert bits(X) == bits(ref["X"]) and bits(U) == bits(ref["U"]) and bits(st) == bits(ref["status"])
    assert bits(w["x0"]) == bits(X[:, 0])            # run_closed_loop works on copies: the workload is unchanged
    seen = {}

    def closed_loop(wl, T_, cfg):
        seen.update(wl)
        return dict(X=torch.zeros((B, T_ + 1, 6), dtype=torch.float64), U=torch.zeros((B, T_, 2), dtype=torch.float64),
                    status=torch.zeros((T_, B), dtype=torch.int32))

    D.generate(B, T, N=N, Ts=Ts, device_workload=True, closed_loop=closed_loop)
    assert seen["knots"] is None and isinstance(seen["paths"], TB.PathSet) and bits(seen["x0"]) == bits(w["x0"])
    with pytest.raises(ValueError):
        make_workload_device(2, seed=-1)
    with pytest.raises(ValueError):
        make_workload_device(2, seed=2 ** 192)


def test_build_device_drives_the_reference_window(gpu):
    """PathSet.build_device on a host workload's knots against PathSet.build (spline_natural) through ref_window_batch:
    within test_workload_host's bar between the two solves, 1e-15 scaled by max(1, max |coef|) of the trajectory."""
    B, N, Ts = 16, 20, 0.05
    w = make_workload(B, N, Ts, kind="spline", seed=5)
    host = TB.PathSet.build(w["kinds"], w["pcs"], w["knots"], device=gpu)
    xk = np.array([k[0] for k in w["knots"]])
    yk = np.array([k[1] for k in w["knots"]])
    dev = TB.PathSet.build_device(w["kinds"], w["pcs"], np.full(B, xk.shape[1]), xk, yk, device=gpu)
    assert bits(dev.xk) == bits(host.xk) and bits(dev.nk) == bits(host.nk) and bits(dev.kind) == bits(host.kind)
    xs = np.linspace(-8.0, 24.0, B)            # windows from before the first knot to past the last (36 m at most)
    vref = np.tile(TB.vref_ramp(N, Ts) * 12.0, (B, 1))
    a = TB.ref_window_batch(host, xs, vref, N, Ts).cpu().numpy()
    b = TB.ref_window_batch(dev, xs, vref, N, Ts).cpu().numpy()
    assert a[:, -1, 0].max() > 34.0 and a[:, 0, 0].min() < -6.0
    scale = np.maximum(1.0, np.abs(host.coef.cpu().numpy()).reshape(B, -1).max(axis=1))
    err = np.abs(a - b).reshape(B, -1).max(axis=1) / scale
    print(f"ref_window: worst scaled difference {err.max():.3e}")
    assert bits(a[:, :, 0].copy()) == bits(b[:, :, 0].copy())
    assert err.max() <= 1e-15

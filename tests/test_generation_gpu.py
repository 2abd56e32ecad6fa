"""The open-loop generator kernel (include/trajgen.h, csrc/openloop.hip) on the MI355X against
tests/golden/generation.npz -- the reference's generation_type1.py / generation_type2.py run by
tests/golden/gen_generation_golden.py.

Bars (none taken from the code under test):
  controls   the limiter and the clips are exact float64 operations in the reference's order: bit-identical.
  one step   |X1 - X_ref[k+1]| <= Ts 1e-12 (1 + |f_ref|) + 2 eps (1 + |X_ref[k+1]|): the project's physics bar
             (1e-12 (1 + |f|), tests/test_gpu_parity.py) through one Euler step, plus the rounding of the step itself.
  free run   |X - X_ref| <= T Ts 1e-12 (1 + Fmax): the per-evaluation bar accumulated linearly over T steps, Fmax =
             max |f| along the trajectory (stored in the fixture).  The fixture script checks that the reference itself
             does not amplify such an error: with f +- 1e-12 (1 + |f|) every trajectory stays within half of this bar (0.03 - 0.23 measured).
  layout     trajectories do not depend on the batch they run in, on T, or on the kernel form: bit-identical; canary
             pads around X and U stay untouched.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from trajectory_generation_amd import _lib, batch as TB, dataset as DS
from trajectory_generation_amd import generation_type1 as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "generation.npz"))
TS = 0.01
EPS = np.finfo(np.float64).eps
K = _lib.GEN_STAGE_STEPS
TYPE1_CASES = ("t1", "l", "c_vx", "c_om", "c_slew")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def simulate(model, x0, u_raw, **kw):
    out = TB.simulate_open_loop(x0, u_raw, TB.gen_config_struct(model, TS, **kw))
    torch.cuda.synchronize()
    return out["X"].cpu().numpy(), out["U"].cpu().numpy()


@pytest.fixture(scope="module")
def runs(gpu):
    """One launch per fixture case, shared by the tests below: name -> (X, U)."""
    r = {pre: simulate(_lib.GEN_MODEL_TYPE1, GOLD[f"{pre}_x0"], GOLD[f"{pre}_u_raw"]) for pre in TYPE1_CASES}
    r["t2"] = simulate(_lib.GEN_MODEL_TYPE2, GOLD["t2_x0"], GOLD["t2_U"])
    return r


# ---------------------------------------------------------------- slew and clip

@pytest.mark.parametrize("pre", TYPE1_CASES)
def test_controls_are_bit_identical(runs, pre):
    U = runs[pre][1]
    ref = GOLD[f"{pre}_U"]
    assert U.shape == ref.shape
    assert same_bits(U, ref), f"{pre}: {np.sum(bits(U) != bits(ref))} of {ref.size} samples differ"


def test_replayed_controls_pass_unchanged(runs):
    """Model 2's defaults have no limiter and no output clip: logged controls come back bit for bit."""
    assert same_bits(runs["t2"][1], GOLD["t2_U"])


# ---------------------------------------------------------------- one step, teacher-forced

def _f_type2(x, u, p):
    """generation_type2.py:52-86 on the host: type 1's model with the rear slip angle clamped as well."""
    vx, vy, omega = x[3], x[4], x[5]
    vx_eff = max(abs(vx), p["vx_zero"])
    a_r = G.clamp(np.arctan2(omega * p["lr"] - vy, vx_eff), -p["maxAlpha"], p["maxAlpha"])
    f = G.f_cont(x, u, p)
    Fy_f, _, _ = G.tire_forces(x, u, p)
    Fy_r = p["Dr"] * np.sin(p["Cr"] * np.arctan(p["Br"] * a_r))
    f[4] = (Fy_r + Fy_f * np.cos(u[1]) - p["m"] * vx * omega) / p["m"]
    f[5] = (Fy_f * p["lf"] * np.cos(u[1]) - Fy_r * p["lr"]) / p["Iz"]
    return f


def _points(cases):
    xs = np.concatenate([GOLD[f"{pre}_X"][:, :-1].reshape(-1, 6) for pre in cases])
    us = np.concatenate([GOLD[f"{pre}_U"].reshape(-1, 2) for pre in cases])
    nxt = np.concatenate([GOLD[f"{pre}_X"][:, 1:].reshape(-1, 6) for pre in cases])
    return xs, us, nxt


def _one_step_report(name, X1, nxt, f_ref):
    bar = TS * 1e-12 * (1.0 + np.abs(f_ref)) + 2 * EPS * (1.0 + np.abs(nxt))
    ratio = np.abs(X1 - nxt) / bar
    print(f"{name}: {len(nxt)} points, worst |err| / bar per state {np.round(ratio.max(axis=0), 4).tolist()}, "
          f"worst |err| per state {np.abs(X1 - nxt).max(axis=0).tolist()}")
    assert (ratio <= 1.0).all(), (name, ratio.max(axis=0))


@pytest.mark.parametrize("model,cases,f_host", [(_lib.GEN_MODEL_TYPE1, TYPE1_CASES, G.f_cont),
                                                (_lib.GEN_MODEL_TYPE2, ("t2",), _f_type2)])
def test_one_step_teacher_forced(gpu, model, cases, f_host):
    """Every (X_ref[k], U_ref[k]) of the fixtures is one instance of T = 1."""
    xs, us, nxt = _points(cases)
    assert len(xs) >= 1600
    X, U = simulate(model, xs, us[:, None, :])
    assert same_bits(X[:, 0], xs) and same_bits(U[:, 0], us)
    f_ref = np.array([f_host(x, u, G.Params) for x, u in zip(xs, us)])
    _one_step_report(f"model {model}", X[:, 1], nxt, f_ref)


def test_one_step_mpc_model_against_f_cont_batch(gpu):
    """Model 0 is the model of traj_f_cont_batch: one step from the same points, no state clip."""
    xs, us, _ = _points(("t1", "c_vx", "c_om"))
    X, _ = simulate(_lib.GEN_MODEL_MPC, xs, us[:, None, :])
    f = TB.f_cont_batch(xs, us).cpu().numpy()
    _one_step_report("model 0", X[:, 1], xs + TS * f, f)
    # the signed vx_eff and Frx of the MPC copy are another model where it matters (vx below vx_zero)
    slow = np.abs(xs[:, 3]) < G.Params["vx_zero"]
    X1, _ = simulate(_lib.GEN_MODEL_TYPE1, xs, us[:, None, :], clip_state=False)
    assert slow.any() and (X1[slow, 1, 3] != X[slow, 1, 3]).any()


# ---------------------------------------------------------------- free run

@pytest.mark.parametrize("pre", TYPE1_CASES + ("t2",))
def test_free_run(runs, pre):
    X = runs[pre][0]
    ref, x0, Fmax = GOLD[f"{pre}_X"], GOLD[f"{pre}_x0"], GOLD[f"{pre}_Fmax"]
    T = ref.shape[1] - 1
    assert X.shape == ref.shape and same_bits(X[:, 0], x0)
    bar = T * TS * 1e-12 * (1.0 + Fmax)
    err = np.abs(X - ref).max(axis=1)                       # [B,6]
    print(f"{pre}: T = {T}, bar {bar.tolist()}, worst |err| per trajectory and state {err.tolist()}")
    assert (err <= bar[:, None]).all(), (pre, (err / bar[:, None]).max())
    vx_clipped = ref[:, 1:, 3] == 0.0
    om_clipped = np.abs(ref[:, 1:, 5]) == 6.0
    assert same_bits(X[:, 1:, 3][vx_clipped], ref[:, 1:, 3][vx_clipped])      # exactly 0.0 where the reference clipped
    assert same_bits(X[:, 1:, 5][om_clipped], ref[:, 1:, 5][om_clipped])      # exactly +-6.0
    assert (X[:, 1:, 3] >= 0.0).all() and (np.abs(X[:, 1:, 5]) <= 6.0).all()
    if pre == "c_vx":
        assert vx_clipped.sum() == 40
    if pre == "c_om":
        assert om_clipped.sum() >= 26


# ---------------------------------------------------------------- edges: batch and chunk remainders, canaries, forms

CANARY = -7.25e300
PAD = 512   # doubles: 4 KB


def _raw_run(B, T, form):
    """traj_gen_simulate_batch on buffers with canary pads before and after X and U."""
    dev = torch.device("cuda", 0)
    idx = np.arange(B) % 6
    x0 = torch.as_tensor(GOLD["t1_x0"][idx], device=dev).contiguous()
    u_raw = torch.as_tensor(GOLD["t1_u_raw"][idx, :T], device=dev).contiguous()
    nX, nU = B * (T + 1) * 6, B * T * 2
    buf = torch.full((4 * PAD + nX + nU,), CANARY, dtype=torch.float64, device=dev)
    oX, oU = PAD, 3 * PAD + nX
    base = buf.data_ptr()
    TB.set_gen_store_form(form)
    try:
        cfg = TB.gen_config_struct(_lib.GEN_MODEL_TYPE1, TS)
        rc = _lib.lib().traj_gen_simulate_batch(C.byref(_lib.default_params()), C.byref(cfg), B, T,
                                                C.c_void_p(x0.data_ptr()), C.c_void_p(u_raw.data_ptr()),
                                                C.c_void_p(base + 8 * oX), C.c_void_p(base + 8 * oU),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        TB.set_gen_store_form(_lib.GEN_FORM_DEFAULT)
    assert rc == _lib.TRAJ_OK
    h = buf.cpu().numpy()
    pads = np.concatenate([h[:oX], h[oX + nX:oU], h[oU + nU:]])
    assert len(pads) == 4 * PAD and (pads == CANARY).all(), "a canary pad around X / U was overwritten"
    return h[oX:oX + nX].reshape(B, T + 1, 6), h[oU:oU + nU].reshape(B, T, 2), idx


@pytest.mark.parametrize("T", [1, K - 1, K, K + 1, 2 * K + 3])
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_edges(runs, B, T):
    """B not a multiple of the wave, T not a multiple of the staged chunk: every trajectory equals the same trajectory
    of the B = 6, T = 400 run (its first T steps: the simulation is causal), in both kernel forms."""
    X6, U6 = runs["t1"]
    Xs, Us, idx = _raw_run(B, T, _lib.GEN_FORM_STAGED)
    Xd, Ud, _ = _raw_run(B, T, _lib.GEN_FORM_DIRECT)
    assert same_bits(Xs, Xd) and same_bits(Us, Ud), "staged and direct forms differ"
    assert same_bits(Xs, X6[idx, :T + 1]) and same_bits(Us, U6[idx, :T])


def test_forms_agree_on_the_long_and_clipped_cases(runs):
    for pre in ("l", "c_vx", "c_om", "c_slew"):
        TB.set_gen_store_form(_lib.GEN_FORM_DIRECT)
        try:
            Xd, Ud = simulate(_lib.GEN_MODEL_TYPE1, GOLD[f"{pre}_x0"], GOLD[f"{pre}_u_raw"])
        finally:
            TB.set_gen_store_form(_lib.GEN_FORM_DEFAULT)
        TB.set_gen_store_form(_lib.GEN_FORM_STAGED)
        try:
            Xs, Us = simulate(_lib.GEN_MODEL_TYPE1, GOLD[f"{pre}_x0"], GOLD[f"{pre}_u_raw"])
        finally:
            TB.set_gen_store_form(_lib.GEN_FORM_DEFAULT)
        assert same_bits(Xd, Xs) and same_bits(Ud, Us), pre
        assert same_bits(runs[pre][0], Xs), pre     # the default is one of them


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def dataset6(gpu):
    d = G.generate_dataset(6, 4.0, 0.01, seed=42)
    torch.cuda.synchronize()
    return d


def test_generate_dataset(runs, dataset6):
    d = dataset6
    assert d["X"].is_cuda and d["U"].is_cuda and tuple(d["X"].shape) == (6, 401, 6)
    assert same_bits(d["U"].cpu().numpy(), GOLD["t1_U"])
    assert d["modes"] == [str(m) for m in GOLD["t1_mode"]] and d["ids"].tolist() == list(range(6))
    assert same_bits(d["X"].cpu().numpy(), runs["t1"][0])    # the same launch as the fixture run: held to its bar there


def test_generate_dataset_shard(dataset6):
    s = G.generate_dataset(3, 4.0, 0.01, seed=42, id_offset=3)
    assert s["ids"].tolist() == [3, 4, 5] and s["modes"] == dataset6["modes"][3:]
    assert same_bits(s["X"].cpu().numpy(), dataset6["X"][3:].cpu().numpy())
    assert same_bits(s["U"].cpu().numpy(), dataset6["U"][3:].cpu().numpy())


def _columns(path, names):
    lines = open(path).read().split("\n")
    header = lines[0].split(",")
    rows = [ln.split(",") for ln in lines[1:-1]]
    return lines[0], [[r[header.index(n)] for n in names] for r in rows]


def test_generate_open_loop_files(gpu, dataset6, tmp_path):
    import pandas as pd
    out, ref = str(tmp_path / "gen"), str(tmp_path / "ref")
    X, U = DS.generate_open_loop(B=6, T=400, out_prefix=out)
    assert same_bits(U.cpu().numpy(), GOLD["t1_U"]) and same_bits(X.cpu().numpy(), dataset6["X"].cpu().numpy())
    assert not os.path.exists(f"{out}_status.csv")
    DS.write_csv(ref, GOLD["t1_X"], GOLD["t1_U"], np.arange(6), TS, native=False)
    names = ["t", "d", "delta", "trajectory_id"]
    for kind in ("clean", "noisy"):
        hg, cg = _columns(f"{out}_{kind}.csv", names)
        hr, cr = _columns(f"{ref}_{kind}.csv", names)
        assert hg == hr and len(cg) == 6 * 401 and cg == cr, kind
    rd = lambda p: pd.read_csv(p, float_precision="round_trip")   # noqa: E731
    clean, noisy = rd(f"{out}_clean.csv"), rd(f"{out}_noisy.csv")
    Xh = X.cpu().numpy()
    for i in range(6):
        n = DS.measurement_noise(i, 401)
        c, z = clean[clean["trajectory_id"] == i], noisy[noisy["trajectory_id"] == i]
        for j, col in ((0, "X"), (1, "Y"), (3, "vx"), (4, "vy"), (5, "omega")):
            assert same_bits(c[col].to_numpy(), Xh[i, :, j])
            assert same_bits(z[col].to_numpy(), c[col].to_numpy() + n[:, j]), (i, col)
    parts = DS.load_vehicle_dataset(f"{out}_noisy.csv", f"{out}_clean.csv", T_steps=400)
    assert parts is not None and sum(p[0].shape[0] for p in parts) == 6
    assert all(p[0].shape[1:] == (5, 400) and p[1].shape[1:] == (2, 400) and p[2].shape[1:] == (6, 400) for p in parts)

"""The type-2 (piecewise state machine) generator kernel (include/trajgen.h traj_gen_piecewise_batch,
csrc/piecewise.hip) and numpy's stream in the kernel (csrc/gen_rng.h, traj_gen_rng_draw_batch) on the MI355X, against
numpy itself and against tests/golden/generation2.npz -- the reference's generation_type2.py run by
tests/golden/gen_generation2_golden.py.

Bars (none taken from the code under test):
  stream     PCG64, next_double and the ziggurat's at-once and wedge draws are integer arithmetic and exact float64
             products: bit-identical.  A tail draw (|z| > r) is r + xx with xx = -log1p(-u) / r from the device
             library: log1p within 2 ulp of libm's on either side, carried into r + xx (xx < r / 2 almost surely, so
             its error weighs less than half there) -- 4 ulp.
  modes, d   the controller reads the state only through comparisons: identical / bit-identical.  The fixture script
             asserts that no normal draw of the fixtures is a tail draw.
  delta      bit-identical up to the first step of the first turn segment entered with v > v_turn_max (the fixture's
             `fast` mask), from where on delta = mag * v_turn_max / v carries the device hypot and the state's error.
  free run   |X - X_ref| <= T Ts 1e-12 (1 + Fmax), the bar tests/test_generation_gpu.py holds model 2 to; delta
             everywhere is held to the same bar (|d delta / d v| = mag v_turn_max / v^2 < 1 in every case here).
  layout     a trajectory does not depend on the batch it runs in, on T (the walk is causal) or on the shard; canary
             pads around X, U, mode and the state output stay untouched; the kernel's own U replayed through
             traj_gen_simulate_batch (model 2) gives the kernel's X bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from trajectory_generation_amd import _lib, batch as TB, dataset as DS
from trajectory_generation_amd import generation_type2 as G2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "generation2.npz"))
ZIG_R = 3.6541528853610087963519472518
CASES = ("a", "b", "c")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def case_rules(pre):
    return G2.ControlRules(v_turn_max=0.6, v_high=1.0) if pre == "b" else G2.ControlRules()


def state_int(words):
    return (int(words[0]) << 64) | int(words[1])


@pytest.fixture(scope="module")
def runs(gpu):
    """One launch per fixture case, shared by the tests below: name -> dict of numpy X, U, mode, rng_state."""
    r = {}
    for pre in CASES:
        T = GOLD[f"{pre}_U"].shape[1]
        out = TB.simulate_piecewise(GOLD[f"{pre}_x0"], G2.pcg64_states(GOLD[f"{pre}_seeds"]), T,
                                    float(GOLD[f"{pre}_Ts"]), case_rules(pre), want_rng_state=True)
        torch.cuda.synchronize()
        r[pre] = {k: v.cpu().numpy() for k, v in out.items()}
        r[pre]["rng_state"] = r[pre]["rng_state"].view(np.uint64)
    return r


# ---------------------------------------------------------------- the stream on the GPU

RNG_B, RNG_N = 65, 4096


@pytest.fixture(scope="module")
def streams():
    seeds = np.arange(1000, 1000 + RNG_B)
    return seeds, G2.pcg64_states(seeds)


@pytest.mark.parametrize("kind", [_lib.RNG_RAW, _lib.RNG_DOUBLE])
def test_words_and_doubles_match_numpy(gpu, streams, kind):
    seeds, states = streams
    got, st = TB.rng_draw_batch(states, RNG_N, kind)
    for b, seed in enumerate(seeds):
        g = np.random.default_rng(int(seed))
        want = g.bit_generator.random_raw(RNG_N) if kind == _lib.RNG_RAW else g.random(RNG_N)
        assert np.array_equal(got[b].view(np.uint64), want.view(np.uint64)), (kind, b)
        assert state_int(st[b]) == g.bit_generator.state["state"]["state"], (kind, b)
        assert st[b, 2:].tolist() == states[b, 2:].tolist()


def test_normals_match_numpy(gpu, streams):
    seeds, states = streams
    got, st = TB.rng_draw_batch(states, RNG_N, _lib.RNG_NORMAL)
    tails, worst = 0, 0
    for b, seed in enumerate(seeds):
        g = np.random.default_rng(int(seed))
        want = g.standard_normal(RNG_N)
        body = np.abs(want) <= ZIG_R
        assert same_bits(got[b][body], want[body]), (b, int(np.sum(bits(got[b][body]) != bits(want[body]))))
        if (~body).any():
            assert (np.sign(got[b][~body]) == np.sign(want[~body])).all()
            ulps = np.abs(bits(got[b][~body]) - bits(want[~body]))
            tails += int((~body).sum())
            worst = max(worst, int(ulps.max()))
        assert state_int(st[b]) == g.bit_generator.state["state"]["state"], b
    print(f"{RNG_B} x {RNG_N} normals: {tails} tail draws, worst tail difference {worst} ulp")
    assert tails >= 20 and worst <= 4


# ---------------------------------------------------------------- the three fixture cases

@pytest.mark.parametrize("pre", CASES)
def test_modes_and_throttle_are_identical(runs, pre):
    assert np.array_equal(runs[pre]["mode"], GOLD[f"{pre}_mode"]), pre
    d, ref = runs[pre]["U"][:, :, 0], GOLD[f"{pre}_U"][:, :, 0]
    assert same_bits(d, ref), f"{pre}: {np.sum(bits(d) != bits(ref))} of {ref.size} samples of d differ"


@pytest.mark.parametrize("pre", CASES)
def test_steering_is_bit_identical_until_the_first_fast_turn(runs, pre):
    delta, ref, fast = runs[pre]["U"][:, :, 1], GOLD[f"{pre}_U"][:, :, 1], GOLD[f"{pre}_fast"]
    T = ref.shape[1]
    checked = 0
    for b in range(ref.shape[0]):
        first = int(np.argmax(fast[b])) if fast[b].any() else T
        assert same_bits(delta[b, :first], ref[b, :first]), (pre, b, first)
        checked += first
    print(f"{pre}: {checked} of {ref.size} steering samples precede a fast turn")
    assert checked >= ref.size // 4
    if pre == "b":
        assert GOLD["b_fast"].sum() >= 100      # the case is there for the fast turns


@pytest.mark.parametrize("pre", CASES)
def test_free_run(runs, pre):
    X, U = runs[pre]["X"], runs[pre]["U"]
    ref, Uref, Fmax = GOLD[f"{pre}_X"], GOLD[f"{pre}_U"], GOLD[f"{pre}_Fmax"]
    T, Ts = Uref.shape[1], float(GOLD[f"{pre}_Ts"])
    assert X.shape == ref.shape and same_bits(X[:, 0], GOLD[f"{pre}_x0"])
    bar = T * Ts * 1e-12 * (1.0 + Fmax)
    err = np.abs(X - ref).max(axis=1)                        # [B,6]
    derr = np.abs(U[:, :, 1] - Uref[:, :, 1]).max(axis=1)    # [B]
    print(f"{pre}: T = {T}, bar {bar.tolist()}, worst |X err| per trajectory {err.max(axis=1).tolist()}, "
          f"worst |delta err| per trajectory {derr.tolist()}, worst err / bar {float((err / bar[:, None]).max()):.4f}")
    assert (err <= bar[:, None]).all(), (pre, (err / bar[:, None]).max())
    assert (derr <= bar).all(), (pre, (derr / bar).max())
    assert (X[:, 1:, 3] >= 0.0).all() and (np.abs(X[:, 1:, 5]) <= 6.0).all()


@pytest.mark.parametrize("pre", CASES)
def test_replaying_the_kernels_controls_gives_its_states(runs, pre):
    cfg = TB.gen_config_struct(_lib.GEN_MODEL_TYPE2, float(GOLD[f"{pre}_Ts"]))
    out = TB.simulate_open_loop(GOLD[f"{pre}_x0"], runs[pre]["U"], cfg)
    torch.cuda.synchronize()
    assert same_bits(out["U"].cpu().numpy(), runs[pre]["U"])
    assert same_bits(out["X"].cpu().numpy(), runs[pre]["X"])


@pytest.mark.parametrize("pre", CASES)
def test_final_stream_state_is_numpys(runs, pre):
    """The host specification on the same trajectory leaves its Generator where the kernel leaves the lane's."""
    T, Ts = GOLD[f"{pre}_U"].shape[1], float(GOLD[f"{pre}_Ts"])
    for b, seed in enumerate(GOLD[f"{pre}_seeds"]):
        g = np.random.default_rng(int(seed))
        G2.sample_controls_piecewise(T, Ts, GOLD[f"{pre}_x0"][b], G2.Params, case_rules(pre), rng=g)
        s = g.bit_generator.state["state"]
        assert state_int(runs[pre]["rng_state"][b]) == s["state"], (pre, b)
        assert state_int(runs[pre]["rng_state"][b, 2:]) == s["inc"], (pre, b)


# ---------------------------------------------------------------- edges: batch remainders, short walks, canaries

CANARY = -7.25e300
CANARY_U8 = 0xA5
CANARY_I64 = -0x5A5A5A5A5A5A5A5B
PAD = 512   # elements


def _raw_run(B, T):
    """traj_gen_piecewise_batch on buffers with canary pads before and after X, U, mode and the state output."""
    dev = torch.device("cuda", 0)
    idx = np.arange(B) % 12
    x0 = torch.as_tensor(GOLD["a_x0"][idx], device=dev).contiguous()
    st = torch.from_numpy(G2.pcg64_states(GOLD["a_seeds"][idx]).view(np.int64)).to(dev)
    nX, nU, nM, nS = B * (T + 1) * 6, B * T * 2, B * T, B * 4
    buf = torch.full((4 * PAD + nX + nU,), CANARY, dtype=torch.float64, device=dev)
    mbuf = torch.full((2 * PAD + nM,), CANARY_U8, dtype=torch.uint8, device=dev)
    sbuf = torch.full((2 * PAD + nS,), CANARY_I64, dtype=torch.int64, device=dev)
    oX, oU = PAD, 3 * PAD + nX
    cfg = TB.gen_config_struct(_lib.GEN_MODEL_TYPE2, 0.01)
    rc = _lib.lib().traj_gen_piecewise_batch(
        C.byref(_lib.default_params()), C.byref(cfg), C.byref(TB.fsm_rules_struct(None)), B, T,
        C.c_void_p(x0.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(buf.data_ptr() + 8 * oX),
        C.c_void_p(buf.data_ptr() + 8 * oU), C.c_void_p(mbuf.data_ptr() + PAD), C.c_void_p(sbuf.data_ptr() + 8 * PAD),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.TRAJ_OK
    h, hm, hs = buf.cpu().numpy(), mbuf.cpu().numpy(), sbuf.cpu().numpy()
    pads = np.concatenate([h[:oX], h[oX + nX:oU], h[oU + nU:]])
    assert len(pads) == 4 * PAD and (pads == CANARY).all(), "a canary pad around X / U was overwritten"
    assert (hm[:PAD] == CANARY_U8).all() and (hm[PAD + nM:] == CANARY_U8).all(), "a canary pad around mode"
    assert (hs[:PAD] == CANARY_I64).all() and (hs[PAD + nS:] == CANARY_I64).all(), "a canary pad around the states"
    return (h[oX:oX + nX].reshape(B, T + 1, 6), h[oU:oU + nU].reshape(B, T, 2), hm[PAD:PAD + nM].reshape(B, T),
            hs[PAD:PAD + nS].reshape(B, 4).view(np.uint64), idx)


@pytest.mark.parametrize("T", [1, 29, 40, 41])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_edges(runs, B, T):
    """B around the wave size, T below the stall minimum (30 steps), at the shortest segment (40) and one past it:
    every trajectory equals the first T steps of the same trajectory in the B = 12, T = 240 run."""
    X, U, M, S, idx = _raw_run(B, T)
    a = runs["a"]
    assert same_bits(X, a["X"][idx, :T + 1]) and same_bits(U, a["U"][idx, :T])
    assert np.array_equal(M, a["mode"][idx, :T]) and (M <= 3).all()
    assert np.array_equal(S[:, 2:], G2.pcg64_states(GOLD["a_seeds"][idx])[:, 2:])


# ---------------------------------------------------------------- end to end

def test_generate_dataset_and_shards(runs):
    d = G2.generate_dataset(12, 2.4, 0.01, seed=42)
    torch.cuda.synchronize()
    assert d["X"].is_cuda and tuple(d["X"].shape) == (12, 241, 6) and tuple(d["U"].shape) == (12, 240, 2)
    assert d["modes"].dtype == torch.uint8 and d["ids"].tolist() == list(range(12))
    X, U, M = d["X"].cpu().numpy(), d["U"].cpu().numpy(), d["modes"].cpu().numpy()
    assert same_bits(X, runs["a"]["X"]) and same_bits(U, runs["a"]["U"]) and np.array_equal(M, GOLD["a_mode"])
    lo = G2.generate_dataset(5, 2.4, 0.01, seed=42)
    hi = G2.generate_dataset(7, 2.4, 0.01, seed=42, id_offset=5)
    assert lo["ids"].tolist() == [0, 1, 2, 3, 4] and hi["ids"].tolist() == list(range(5, 12))
    for k, ref in (("X", X), ("U", U), ("modes", M)):
        both = np.concatenate([lo[k].cpu().numpy(), hi[k].cpu().numpy()])
        assert np.array_equal(both.view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), k


def test_piecewise_files_merge_and_load(runs, tmp_path):
    import pandas as pd
    t1, t2, out = (str(tmp_path / n) for n in ("type1", "type2", "merged"))
    X2, U2 = DS.generate_piecewise(B=4, T=240, out_prefix=t2)
    assert same_bits(X2.cpu().numpy(), runs["a"]["X"][:4]) and same_bits(U2.cpu().numpy(), runs["a"]["U"][:4])
    DS.generate_open_loop(B=3, T=240, out_prefix=t1)
    assert DS.merge_datasets(t1, t2, out) == 3
    rd = lambda p: pd.read_csv(p, float_precision="round_trip")   # noqa: E731
    clean, noisy = rd(f"{out}_clean.csv"), rd(f"{out}_noisy.csv")
    assert list(clean.columns) == DS.CLEAN_COLUMNS and list(noisy.columns) == DS.NOISY_COLUMNS
    assert sorted(clean["trajectory_id"].unique().tolist()) == list(range(7)) and len(clean) == len(noisy) == 7 * 241
    # type 2's rows are ids 3 .. 6 of the merged pair, with the noise of their own ids 0 .. 3
    c3, n3 = clean[clean["trajectory_id"] == 3], noisy[noisy["trajectory_id"] == 3]
    assert same_bits(c3["phi"].to_numpy(), runs["a"]["X"][0, :, 2])
    assert same_bits(c3["delta"].to_numpy()[:-1], runs["a"]["U"][0, :, 1]) and np.isnan(c3["d"].to_numpy()[-1])
    noise = DS.measurement_noise(0, 241)      # tests/test_generation2_host.py ties it to the reference's noisy states
    for j, col in ((0, "X"), (1, "Y"), (3, "vx"), (4, "vy"), (5, "omega")):
        assert same_bits(c3[col].to_numpy(), runs["a"]["X"][0, :, j]), col
        assert same_bits(n3[col].to_numpy(), runs["a"]["X"][0, :, j] + noise[:, j]), col
    parts = DS.load_vehicle_dataset(f"{out}_noisy.csv", f"{out}_clean.csv", T_steps=240)
    assert parts is not None and sum(p[0].shape[0] for p in parts) == 7
    assert all(p[0].shape[1:] == (5, 240) and p[1].shape[1:] == (2, 240) and p[2].shape[1:] == (6, 240) for p in parts)

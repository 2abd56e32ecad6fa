"""tests/golden/generation.npz: the REFERENCE's generation_traj/generation_type1.py and generation_type2.py run on a
few short trajectories (tests/test_generation_host.py and tests/test_generation_gpu.py compare against them).
Build container only:  python tests/golden/gen_generation_golden.py

Contents (float64 unless noted; B trajectories, T steps):
  t1_*   type 1, np.random.seed(42), the first 6 trajectories at total_steps = 400, Ts = 0.01, drawn and simulated by the
         reference's own functions in its __main__ order: x0 [6,6], d_clean / delta_clean [6,400], mode [6] (str),
         u_raw [6,400,2] (clean + control noise), U [6,400,2] (after slew limit and clip), X [6,401,6], Fmax [6]
  l_*    the same for trajectory 0 at total_steps = 1200 (the reference's real length), B = 1
  t2_*   type 2, seed 2025, 4 trajectories x 400 steps: x0, U (sample_controls_piecewise), X (the loop of
         generation_type2.py:180-187), Fmax
  c_vx_* / c_om_* / c_slew_*  crafted type-1 cases (B = 1): x0, u_raw, U, X, Fmax; the vx clip, the omega clip and the
         clip-after-scan rule of the limiter each fire (c_vx_fired / c_om_fired: number of steps whose clip changed
         the state)
  Fmax = max |f_cont(X[k], U[k])| over the trajectory, with the model that made it (the free-run bar's scale).

The script asserts what the tests rely on: both modes occur, the slew limit bites in every type-1 trajectory, each
crafted case fires its clip, and the reference is insensitive to the error the free-run bar allows: with f replaced
by f +- 1e-12 (1 + |f|) (all plus, all minus) every trajectory stays within half of T Ts 1e-12 (1 + Fmax).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TRAJ_REFERENCE", "/root/reference")
TS = 0.01
STATS = {'d_mean': 0.2161, 'd_std': 0.1314, 'delta_mean': 0.0035, 'delta_std': 0.0338}
DU = ((-0.1, 0.1), (-0.04, 0.04))
U_LIM = ((-1.0, 1.0), (-0.6, 0.6))
X0_RANGES = ((-2.0, 2.0), (-2.0, 2.0), (-np.pi, np.pi), (0.4, 1.5), (-0.05, 0.05), (-1.0, 1.0))


def type1_draw(G, n, steps):
    """generation_type1.py's __main__ loop for n trajectories (the caller has seeded the global stream)."""
    out = {k: [] for k in ("x0", "d_clean", "delta_clean", "mode", "u_raw", "U", "X")}
    for _ in range(n):
        x0 = np.array([np.random.uniform(*r) for r in X0_RANGES])
        d_clean, delta_clean, mode = G.generate_smooth_profiles(steps, TS, STATS)
        noise_d = np.random.normal(0, STATS['d_std'] * 0.1, steps)
        noise_delta = np.random.normal(0, STATS['delta_std'] * 0.1, steps)
        u_raw = np.stack([d_clean + noise_d, delta_clean + noise_delta], axis=1)
        U, X = type1_run(G, x0, u_raw)
        for k, v in (("x0", x0), ("d_clean", d_clean), ("delta_clean", delta_clean), ("mode", str(mode)),
                     ("u_raw", u_raw), ("U", U), ("X", X)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def type1_run(G, x0, u_raw):
    d = np.clip(G.apply_du_bounds(u_raw[:, 0], *DU[0]), *U_LIM[0])
    delta = np.clip(G.apply_du_bounds(u_raw[:, 1], *DU[1]), *U_LIM[1])
    U = np.stack([d, delta], axis=1)
    return U, G.simulate_trajectory(x0, U, TS, G.Params)


def euler_loop(f, x0, U, pert=0.0):
    """The integration loop both generators share (type 1 :70-84, type 2 :180-187), f perturbed by pert (1 + |f|)."""
    X = np.empty((len(U) + 1, 6))
    X[0] = x0
    fired = [0, 0]
    for k in range(len(U)):
        fk = f(X[k], U[k])
        fk = fk + pert * (1.0 + np.abs(fk))
        X[k + 1] = X[k] + TS * fk
        fired[0] += X[k + 1, 3] < 0.0
        fired[1] += abs(X[k + 1, 5]) > 6.0
        X[k + 1, 3] = max(X[k + 1, 3], 0.0)
        X[k + 1, 5] = float(np.clip(X[k + 1, 5], -6.0, 6.0))
    return X, fired


def fmax(f, X, U):
    return max(np.abs(f(X[k], U[k])).max() for k in range(len(U)))


def check_insensitive(name, f, x0, U, X, Fm):
    bar = len(U) * TS * 1e-12 * (1.0 + Fm)
    X0, _ = euler_loop(f, x0, U)
    assert np.array_equal(X0, X), name            # the loop here is the reference's loop
    worst = 0.0
    for sgn in (1.0, -1.0):
        Xp, _ = euler_loop(f, x0, U, pert=sgn * 1e-12)
        worst = max(worst, np.abs(Xp - X).max())
    assert worst <= 0.5 * bar, (name, worst, bar)
    return worst / bar


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, "generation_traj"))
    import generation_type1 as G1
    import generation_type2 as G2
    f1 = lambda x, u: G1.f_cont(x, u, G1.Params)   # noqa: E731
    f2 = lambda x, u: G2.f_cont(x, u, G2.Params)   # noqa: E731
    arrs, ratios = {}, {}

    np.random.seed(42)
    t1 = type1_draw(G1, 6, 400)
    np.random.seed(42)
    lg = type1_draw(G1, 1, 1200)
    assert set(t1["mode"]) == {"straight", "sinusoid"}, t1["mode"]
    for pre, d in (("t1", t1), ("l", lg)):
        d["Fmax"] = np.array([fmax(f1, X, U) for X, U in zip(d["X"], d["U"])])
        for b in range(len(d["X"])):
            changed = int((d["U"][b] != d["u_raw"][b]).any(axis=1).sum())
            assert changed > 0, (pre, b)                       # the slew limit bites in every trajectory
            ratios[f"{pre}[{b}]"] = (check_insensitive(f"{pre}{b}", f1, d["x0"][b], d["U"][b], d["X"][b], d["Fmax"][b]),
                                     changed)
        for k, v in d.items():
            arrs[f"{pre}_{k}"] = v

    rng = np.random.default_rng(2025)
    rules = G2.ControlRules()
    x0s, Us, Xs = [], [], []
    for i in range(4):
        x0 = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-np.pi, np.pi), rng.uniform(0.2, 0.6),
                       rng.uniform(-0.05, 0.05), rng.uniform(-1, 1)], dtype=float)
        U, _ = G2.sample_controls_piecewise(400, TS, x0, G2.Params, rules, seed=2025 + i)
        X = np.empty((401, 6))
        X[0] = x0
        for k in range(400):
            X[k + 1] = X[k] + TS * G2.f_cont(X[k], U[k], G2.Params)
            X[k + 1, 3] = max(X[k + 1, 3], 0.0)
            X[k + 1, 5] = float(np.clip(X[k + 1, 5], -6, 6))
        x0s.append(x0), Us.append(U), Xs.append(X)
    arrs.update(t2_x0=np.array(x0s), t2_U=np.array(Us), t2_X=np.array(Xs),
                t2_Fmax=np.array([fmax(f2, X, U) for X, U in zip(Xs, Us)]))
    for b in range(4):
        ratios[f"t2[{b}]"] = (check_insensitive(f"t2{b}", f2, x0s[b], Us[b], Xs[b], arrs["t2_Fmax"][b]), 0)

    crafted = {
        "c_vx": (np.array([0, 0, 0, 0.02, 0, 5.9]), np.tile([-1.0, 0.6], (40, 1))),
        "c_om": (np.array([0, 0, 0, 1.5, 0, 5.5]), np.tile([0.5, 0.6], (60, 1))),
        # leaves [-1, 1] / [-0.6, 0.6] and comes back while the limiter is still catching up
        "c_slew": (np.array([0, 0, 0, 1.0, 0, 0.0]),
                   np.stack([np.r_[[0.5] * 5, [3.0] * 15, [0.2] * 40], np.r_[[0.0] * 5, [1.5] * 25, [-0.1] * 30]], 1)),
    }
    for name, (x0, u_raw) in crafted.items():
        x0 = x0.astype(float)
        U, X = type1_run(G1, x0, u_raw)
        Fm = fmax(f1, X, U)
        _, fired = euler_loop(f1, x0, U)
        arrs.update({f"{name}_x0": x0[None], f"{name}_u_raw": u_raw[None], f"{name}_U": U[None], f"{name}_X": X[None],
                     f"{name}_Fmax": np.array([Fm])})
        ratios[name] = (check_insensitive(name, f1, x0, U, X, Fm), fired)
        if name == "c_vx":
            assert fired[0] >= 1 and (X[1:, 3] == 0.0).sum() == fired[0], fired
            arrs["c_vx_fired"] = np.array(fired[0])
        if name == "c_om":
            assert fired[1] >= 1 and (np.abs(X[1:, 5]) == 6.0).sum() >= fired[1], fired
            arrs["c_om_fired"] = np.array(fired[1])
        if name == "c_slew":
            # the wrong order (clip inside the scan) gives other controls: the case tells the two apart
            wrong = np.empty_like(u_raw)
            for c in range(2):
                w = np.empty(len(u_raw))
                w[0] = np.clip(u_raw[0, c], *U_LIM[c])
                for k in range(1, len(u_raw)):
                    w[k] = np.clip(w[k - 1] + np.clip(u_raw[k, c] - w[k - 1], *DU[c]), *U_LIM[c])
                wrong[:, c] = w
                assert (wrong[:, c] != U[:, c]).sum() >= 5, c
            assert (np.abs(U[:, 0]) == 1.0).any() and (np.abs(U[:, 1]) == 0.6).any()

    path = os.path.join(HERE, "generation.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, size
    print({k: (v.shape, str(v.dtype)) for k, v in arrs.items()})
    print("drift / bar (f +- 1e-12 (1 + |f|)), slew-limited samples:", {k: (float(f"{r:.3g}"), c)
                                                                      for k, (r, c) in ratios.items()})
    print("Fmax:", {k: np.round(v, 2).tolist() for k, v in arrs.items() if k.endswith("Fmax")})
    print("modes:", t1["mode"].tolist(), " bytes:", size)


if __name__ == "__main__":
    main()

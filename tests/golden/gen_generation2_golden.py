"""tests/golden/generation2.npz: the REFERENCE's generation_traj/generation_type2.py (the piecewise state-machine
generator) run on three small cases (tests/test_generation2_host.py and tests/test_generation2_gpu.py compare against
them).  Build container only:  python tests/golden/gen_generation2_golden.py

Per case (prefix a_, b_, c_; B trajectories, T steps; float64 unless noted):
  x0 [B,6], U [B,T,2], mode [B,T] uint8 (0 accelerate, 1 cruise, 2 turn_left, 3 turn_right), X [B,T+1,6],
  seeds [B] int64 (the seed of each trajectory's controller stream), Ts, Fmax [B] (max |f_cont(X[k], U[k])|, the
  free-run bar's scale), fast [B,T] uint8 (1 on the steps of a turn segment entered with v > v_turn_max: from there on
  delta has passed through the speed by arithmetic, not only by comparisons)
  a_  generate_dataset(12, 2.4, 0.01, seed=42) as is (default rules; x0 drawn by the reference); also
      a_noisy_ids [2] and a_noisy [2,T+1,6]: the noisy states of two ids (phi included, before the reference drops it)
  b_  ControlRules(v_turn_max=0.6, v_high=1.0), x0 = [0,0,0,1.5,0,0], Ts = 0.02, T = 150, seeds 100..107; X by the
      reference's euler_step and the clips of :186-187
  c_  default rules, x0 = 0 (vx = 0), Ts = 0.01, T = 100, seeds 7..10

The script hands the reference a recording proxy around its generator and asserts what the tests rely on: every
branch named below is hit (a: stall, boost, slow and fast turns, rate limit; b: relabel, fast turns; c: boost from
the first step, stall override), and no normal draw in the fixtures is a tail draw (|z| > r), so every draw of the
fixtures is one the kernel reproduces bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TRAJ_REFERENCE", "/root/reference")
MODES = ("accelerate", "cruise", "turn_left", "turn_right")
ZIG_R = 3.6541528853610087963519472518


class Recorder:
    """A Generator that logs (name, args, result) of every call the controller makes."""

    def __init__(self, rng, log):
        self._rng, self._log = rng, log

    def choice(self, a, p=None):
        r = self._rng.choice(a, p=p)
        self._log.append(("choice", len(a), str(r)))
        return r

    def uniform(self, lo, hi):
        r = self._rng.uniform(lo, hi)
        self._log.append(("uniform", (lo, hi), r))
        return r

    def normal(self, loc, scale):
        r = self._rng.normal(loc, scale)
        self._log.append(("normal", scale, r))
        return r


def recorded(G2, logs):
    """Context: np.random.default_rng hands out recording proxies for the controller's streams (not for others)."""
    real = np.random.default_rng

    class Ctx:
        def __enter__(self):
            def patched(seed=None):
                g = real(seed)
                if seed in logs:
                    return Recorder(g, logs[seed])
                return g
            np.random.default_rng = patched

        def __exit__(self, *a):
            np.random.default_rng = real
    return Ctx()


def walk(log, modes, T, Ts, X, rules):
    """Per trajectory: the segments of the call log laid over the steps.  Returns counts and the fast-turn mask."""
    c = dict(stall=0, relabel_steps=0, fast_turn_steps=0, slow_turn_segs=0, segs=0, tail=0)
    fast = np.zeros(T, dtype=np.uint8)
    i = k = 0
    while i < len(log):
        assert log[i][0] == "choice", log[i]
        chosen = log[i][2]
        assert log[i + 1][:2] == ("uniform", (0.4, 1.5))
        seg = max(1, int(np.round(log[i + 1][2] / Ts)))
        j = i + 2
        calls = []
        while j < len(log) and log[j][0] != "choice":
            calls.append(log[j])
            j += 1
        stall = any(cl[:2] == ("uniform", (0.5, 1.0)) for cl in calls)
        if stall:
            seg = max(seg, int(round(0.3 / Ts)))
            c["stall"] += 1
        is_fast = any(cl[:2] == ("uniform", (0.0, 0.15)) for cl in calls)
        c["slow_turn_segs"] += any(cl[:2] == ("uniform", (0.05, 0.25)) for cl in calls)
        c["tail"] += sum(cl[0] == "normal" and abs(cl[2] / cl[1]) > ZIG_R for cl in calls)
        end = min(T, k + seg)
        assert k < T
        v = np.hypot(X[k, 3], X[k, 4])
        assert is_fast == (chosen.startswith("turn") and v > rules.v_turn_max)
        assert stall == (v < 0.5)
        if is_fast and not stall:
            fast[k:end] = 1
            c["fast_turn_steps"] += end - k
        if chosen == "accelerate" and modes[k] == "cruise":
            assert not stall and v >= rules.v_high
            c["relabel_steps"] += end - k
        c["segs"] += 1
        k, i = end, j
    assert k == T, (k, T)
    return c, fast


def run_case(G2, rules, x0s, seeds, T, Ts):
    f2 = lambda x, u: G2.f_cont(x, u, G2.Params)   # noqa: E731
    out = {k: [] for k in ("U", "mode", "X", "Fmax", "fast")}
    tot = dict(stall=0, relabel_steps=0, fast_turn_steps=0, slow_turn_segs=0, segs=0, tail=0, boost_steps=0,
               rate_limited_steps=0, boost_first_step=0)
    for x0, seed in zip(x0s, seeds):
        logs = {int(seed): []}
        with recorded(G2, logs):
            U, modes = G2.sample_controls_piecewise(T, Ts, x0, G2.Params, rules, seed=int(seed))
        X = np.empty((T + 1, 6))
        X[0] = x0
        for k in range(T):
            X[k + 1] = G2.euler_step(X[k], U[k], G2.Params, Ts)
            X[k + 1, 3] = max(X[k + 1, 3], 0.0)
            X[k + 1, 5] = float(np.clip(X[k + 1, 5], -6, 6))
        c, fast = walk(logs[int(seed)], modes, T, Ts, X, rules)
        for k in c:
            tot[k] += c[k]
        v = np.hypot(X[:-1, 3], X[:-1, 4])
        tot["boost_steps"] += int((v < 0.35).sum())
        tot["boost_first_step"] += int(v[0] < 0.35)
        prev = np.r_[0.0, U[:-1, 1]]
        tot["rate_limited_steps"] += int((np.abs(np.abs(U[:, 1] - prev) - 0.30 * Ts) <= 1e-15).sum())
        out["U"].append(U), out["X"].append(X), out["fast"].append(fast)
        out["mode"].append(np.array([MODES.index(m) for m in modes], dtype=np.uint8))
        out["Fmax"].append(max(np.abs(f2(X[k], U[k])).max() for k in range(T)))
    res = {k: np.array(v) for k, v in out.items()}
    res.update(x0=np.array(x0s, dtype=float), seeds=np.array(seeds, dtype=np.int64), Ts=np.array(Ts))
    return res, tot


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, "generation_traj"))
    import generation_type2 as G2
    arrs = {}

    # ---- a: generate_dataset as is
    nA, Ts, seed = 12, 0.01, 42
    T = int(np.round(2.4 / Ts))
    df = G2.generate_dataset(nA, 2.4, Ts, seed=seed)
    clean, noisy = df[df["noise_type"] == "clean"], df[df["noise_type"] == "noisy"]
    cols = ["X", "Y", "phi", "vx", "vy", "omega"]
    XA = np.stack([clean[clean["trajectory_id"] == i][cols].to_numpy() for i in range(nA)])
    UA = np.stack([clean[clean["trajectory_id"] == i][["d", "delta"]].to_numpy()[:-1] for i in range(nA)])
    MA = [clean[clean["trajectory_id"] == i]["mode"].tolist()[:-1] for i in range(nA)]
    assert XA.shape == (nA, T + 1, 6) and UA.shape == (nA, T, 2)
    a, tot = run_case(G2, G2.ControlRules(), XA[:, 0], [seed + i for i in range(nA)], T, Ts)
    # the case runner restates generate_dataset's loop: it must give the DataFrame's numbers
    assert np.array_equal(a["X"], XA) and np.array_equal(a["U"], UA)
    assert all([MODES[c] for c in a["mode"][i]] == MA[i] for i in range(nA))
    print("a:", tot)
    assert tot["stall"] and tot["boost_steps"] and tot["slow_turn_segs"] and tot["fast_turn_steps"]
    assert tot["rate_limited_steps"] and tot["tail"] == 0
    ids = np.array([0, 7])
    a["noisy_ids"] = ids
    a["noisy"] = np.stack([noisy[noisy["trajectory_id"] == i][cols].to_numpy() for i in ids])
    arrs.update({f"a_{k}": v for k, v in a.items()})

    # ---- b: relabel and fast turns
    rules = G2.ControlRules(v_turn_max=0.6, v_high=1.0)
    b, tot = run_case(G2, rules, [[0, 0, 0, 1.5, 0, 0]] * 8, list(range(100, 108)), 150, 0.02)
    print("b:", tot)
    assert tot["relabel_steps"] and tot["fast_turn_steps"] and tot["tail"] == 0
    arrs.update({f"b_{k}": v for k, v in b.items()})

    # ---- c: from standstill
    c, tot = run_case(G2, G2.ControlRules(), [[0.0] * 6] * 4, [7, 8, 9, 10], 100, 0.01)
    print("c:", tot)
    assert tot["boost_first_step"] == 4 and tot["stall"] >= 4 and tot["tail"] == 0
    arrs.update({f"c_{k}": v for k, v in c.items()})

    path = os.path.join(HERE, "generation2.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, "generation.npz")), size
    print({k: (v.shape, str(v.dtype)) for k, v in arrs.items()})
    print("Fmax:", {k: np.round(v, 2).tolist() for k, v in arrs.items() if k.endswith("Fmax")}, " bytes:", size)


if __name__ == "__main__":
    main()

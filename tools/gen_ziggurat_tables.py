"""Writes trajectory_generation_amd/csrc/gen_zig_tables.h: the three 256-entry tables of the ziggurat that numpy's
Generator.standard_normal walks (wi: layer widths / 2^52, ki: the accept-at-once thresholds, fi: the density at the
layer edges), and checks them against numpy itself.

  python tools/gen_ziggurat_tables.py [--draws 400000] [--check-only]      (needs numpy and mpmath)

Provenance.  numpy's tables are not the textbook ones.  The Marsaglia-Tsang recursion for 256 layers with
r = 3.6541528853610087963519472518, evaluated here with mpmath at 200 bits,
    v      = r f(r) + sqrt(pi / 2) erfc(r / sqrt 2)         (f(x) = exp(-x^2 / 2), the area of every layer)
    x_255  = r,   x_i = f^-1(v / x_{i+1} + f(x_{i+1}))       i = 254 .. 1
    wi[i]  = x_i / 2^52,   wi[0] = v / f(r) / 2^52
gives widths that differ from numpy's by up to about 1e-14 relative (tens of ulps; with the 12-digit area
0.00492867323399 of the papers, 3e-10), and then every draw differs.  So the recursion is only the first guess, and
numpy's source is not read either: wi is RECOVERED FROM NUMPY'S OWN DRAWS.
  * A pure-Python replica of random_standard_normal runs on the raw words of PCG64(seed) next to Generator's draws.
    A draw accepted at once or in the wedge is sign * rabs * wi[idx] with rabs a known 52-bit integer, so each such
    draw leaves only the doubles w with rabs * w == |z|; the candidates within 4096 ulps of the guess that satisfy
    every draw of a layer are intersected.  Exactly one must be left per layer (layer 1 has ki[1] = 0 and is pinned by
    its wedge-accepted draws), or the script stops.
  * The other two tables follow from the recovered widths at 200 bits:
        ki[i+1] = floor(wi[i] / wi[i+1] 2^52),  ki[0] = floor(wi[255] / wi[0] 2^52),  ki[1] = 0
        fi[i]   = f(wi[i] 2^52),  fi[0] = 1
    They enter a draw only through comparisons (rabs < ki[idx]; the wedge test), so numpy's draws cannot pin them:
    whatever error is left there is at most a few units of ki or an ulp of fi and moves a draw with probability of
    order 2^-52 per draw.  That uncertainty remains (DESIGN.md says so).
  * The finished tables are then checked on fresh seeds: every draw bit-identical and the stream position equal, or
    the header is not written.
"""
import argparse
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "trajectory_generation_amd", "csrc", "gen_zig_tables.h")
R_STR = "3.6541528853610087963519472518"
INV_R_STR = "0.27366123732975827203338247596"
N = 256


def tables():
    """The first guess: the recursion at 200 bits (wi, ki, fi, layer area v)."""
    import mpmath as mp
    mp.mp.prec = 200
    r = mp.mpf(R_STR)
    f = lambda x: mp.exp(-x * x / 2)   # noqa: E731
    v = r * f(r) + mp.sqrt(mp.pi / 2) * mp.erfc(r / mp.sqrt(2))
    two52 = mp.mpf(2) ** 52
    x = [None] * N
    x[N - 1] = r
    for i in range(N - 2, 0, -1):
        x[i] = mp.sqrt(-2 * mp.log(v / x[i + 1] + f(x[i + 1])))
    wi, ki, fi = [0.0] * N, [0] * N, [0.0] * N
    wi[0] = float(v / f(r) / two52)
    ki[0] = int(mp.floor(r * f(r) / v * two52))
    fi[0] = 1.0
    for i in range(1, N):
        wi[i] = float(x[i] / two52)
        fi[i] = float(f(x[i]))
    ki[1] = 0
    for i in range(1, N - 1):
        ki[i + 1] = int(mp.floor(x[i] / x[i + 1] * two52))
    return wi, ki, fi, float(v)


def replica_normals(raw, n, wi, ki, fi):
    """random_standard_normal on the word stream `raw` (python ints): n draws, per draw its path (0 at once, 1 wedge,
    2 tail), layer and 52-bit integer rabs, and the number of words consumed."""
    r, inv_r = float(R_STR), float(INV_R_STR)
    pos = 0
    out, path, layer, mant = [], [], [], []

    def nd():
        nonlocal pos
        w = raw[pos]
        pos += 1
        return (w >> 11) * (1.0 / 9007199254740992.0)

    while len(out) < n:
        w = raw[pos]
        pos += 1
        idx = w & 0xFF
        w >>= 8
        sign = w & 1
        rabs = (w >> 1) & 0x000FFFFFFFFFFFFF
        x = rabs * wi[idx]
        if sign:
            x = -x
        if rabs < ki[idx]:
            out.append(x), path.append(0), layer.append(idx), mant.append(rabs)
            continue
        if idx == 0:
            while True:
                xx = -inv_r * math.log1p(-nd())
                yy = -math.log1p(-nd())
                if yy + yy > xx * xx:
                    out.append(-(r + xx) if (rabs >> 8) & 1 else r + xx)
                    path.append(2), layer.append(0), mant.append(rabs)
                    break
        elif (fi[idx - 1] - fi[idx]) * nd() + fi[idx] < math.exp(-0.5 * x * x):
            out.append(x), path.append(1), layer.append(idx), mant.append(rabs)
    return np.array(out), np.array(path), np.array(layer), np.array(mant, dtype=np.float64), pos


def recover(wi0, ki0, fi0, draws, seeds=(1, 2, 3), span=4096):
    """numpy's wi from numpy's draws (see the module docstring); ki and fi from the recovered wi."""
    import mpmath as mp
    mp.mp.prec = 200
    lay, mant, absz = [], [], []
    for seed in seeds:
        want = np.random.Generator(np.random.PCG64(seed)).standard_normal(draws)
        raw = np.random.PCG64(seed).random_raw(2 * draws + 1024).tolist()
        _, path, layer, m, _ = replica_normals(raw, draws, wi0, ki0, fi0)
        keep = path != 2
        lay.append(layer[keep]), mant.append(m[keep]), absz.append(np.abs(want[keep]))
    lay, mant, absz = np.concatenate(lay), np.concatenate(mant), np.concatenate(absz)
    wi = [0.0] * N
    for i in range(N):
        sel = lay == i
        g = np.float64(wi0[i])
        cand = (g.view(np.int64) + np.arange(-span, span + 1)).view(np.float64)
        ok = np.ones(cand.size, dtype=bool)
        for s in range(0, int(sel.sum()), 512):
            ok &= (mant[sel][s:s + 512, None] * cand[None, :] == absz[sel][s:s + 512, None]).all(axis=0)
        if ok.sum() != 1:
            raise SystemExit(f"layer {i}: {int(ok.sum())} candidate widths fit its {int(sel.sum())} draws")
        wi[i] = float(cand[ok][0])
    two52 = mp.mpf(2) ** 52
    ki, fi = [0] * N, [1.0] * N
    ki[0] = int(mp.floor(mp.mpf(wi[N - 1]) / mp.mpf(wi[0]) * two52))
    for i in range(1, N):
        x = mp.mpf(wi[i]) * two52
        fi[i] = float(mp.exp(-x * x / 2))
        if i + 1 < N:
            ki[i + 1] = int(mp.floor(mp.mpf(wi[i]) / mp.mpf(wi[i + 1]) * two52))
    ki[1] = 0
    ulps = np.array(wi).view(np.int64) - np.array(wi0).view(np.int64)
    return wi, ki, fi, ulps


def check(wi, ki, fi, draws, seeds=(0, 12345)):
    """The replica with these tables against Generator.standard_normal on seeds the recovery did not use."""
    worst = {}
    for seed in seeds:
        want = np.random.Generator(np.random.PCG64(seed)).standard_normal(draws)
        raw = np.random.PCG64(seed).random_raw(2 * draws + 1024).tolist()
        got, path, layer, _, used = replica_normals(raw, draws, wi, ki, fi)
        bad = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]
        # numpy's own stream position after the same draws
        bg = np.random.PCG64(seed)
        np.random.Generator(bg).standard_normal(draws)
        ref = np.random.PCG64(seed)
        ref.advance(used)
        same_pos = bg.state["state"]["state"] == ref.state["state"]["state"]
        worst[seed] = dict(draws=draws, mismatches=int(bad.size), first=bad[:5].tolist(),
                           layers_hit_at_once=int(np.unique(layer[path == 0]).size),
                           wedge=int((path == 1).sum()), tail=int((path == 2).sum()),
                           same_stream_position=bool(same_pos))
    return worst


def emit(wi, ki, fi, path):
    def block(ctype, name, vals, fmt, per):
        lines = [f"GEN_ZIG_DECL {ctype} GEN_ZIG_NAME({name})[256] = {{"]
        for i in range(0, N, per):
            lines.append("    " + ", ".join(fmt(v) for v in vals[i:i + per]) + ",")
        lines.append("};")
        return "\n".join(lines)
    text = "\n".join([
        "// gen_zig_tables.h -- written by tools/gen_ziggurat_tables.py (do not edit): the 256-layer ziggurat tables"
        " of",
        "// numpy's Generator.standard_normal, wi (layer widths / 2^52), ki (accept-at-once thresholds), fi (density"
        " at the",
        "// layer edges).  Plain constant arrays; the includer sets GEN_ZIG_DECL (storage, e.g. `static const`) and",
        "// GEN_ZIG_NAME(x) (the arrays' names) and may include the file once per copy it needs.  Doubles are hex"
        " floats:",
        "// exact.",
        block("double", "wi", wi, lambda v: float(v).hex(), 4),
        block("unsigned long long", "ki", ki, lambda v: f"0x{v:016X}ULL", 4),
        block("double", "fi", fi, lambda v: float(v).hex(), 4),
        "",
    ])
    with open(path, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=400000)
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    wi, ki, fi, v = tables()
    print(f"recursion: layer area v = {v!r}, wi[0] = {wi[0]!r}, wi[255] = {wi[255]!r}, ki[0] = {ki[0]:#x}")
    wi, ki, fi, ulps = recover(wi, ki, fi, a.draws)
    print(f"recovered wi: {int((ulps != 0).sum())} of 256 differ from the 200-bit recursion, by up to "
          f"{int(np.abs(ulps).max())} ulps; wi[0] = {wi[0]!r}, ki[0] = {ki[0]:#x}")
    res = check(wi, ki, fi, a.draws)
    print(res)
    if any(r["mismatches"] or not r["same_stream_position"] for r in res.values()):
        raise SystemExit("the tables do not reproduce numpy's draws: header not written")
    if not a.check_only:
        emit(wi, ki, fi, a.out)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

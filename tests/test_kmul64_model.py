"""The 64-lane K^-1 v of the fused capacity-40 solve kernel (csrc/mpc_solve.h, TGMPC_KMUL_64) as a dataflow model of its
lane program, beside the row-per-lane mat-vec it replaces.

Both programs run on TAGGED operands: every value is a node of a hash-consed expression graph (a leaf -- an entry of
the negated swept blocks, an entry of v, a constant -- or fma / add of nodes), so two values are the same node exactly
when they are the same operations on the same operands in the same order: the condition for equal bits on the GPU.  No
identity is used at all (fma's two factors keep their order, too).

The class-form model follows the kernel statement by statement, from the blocks the 8 x 8 sweep leaves: the staging of
local block row k of every lane at class-major addresses, the five masked reads of lane 16 c + m into a static slot per
round, the class-major publication of v, the three chains of ten fma from +0.0, the partial sums' words in the scratch
region and lane r's combination (p0 + p1) + (p2 + p3).  LDS words carry what they were written for (staging round;
mat-vec call and kind), so a read of a stale, unwritten or absent-slot word fails the test; every index is checked
against the region's size.

CPU only: the dataflow, not the kernel (tests/test_kmul64_gpu.py compares the kernel's results with the row form's
instances bit for bit)."""
import pytest

NN = 40
BS = NN // 8          # block edge of the 8 x 8 sweep
ST = NN + 2           # row stride of the staging area
KCL = NN // 4         # entries of a row per column class
KPA = NN              # partial sums of classes 0, 1 (after the vector)
KPB = KPA + 2 * 64    # classes 2, 3
KPD = KPB + 2 * 64    # 32 words nobody reads
NU = 8 * ST           # the scratch region (s_u) of the instance
MASKS = (0x00FF00FF00FF00FF, 0xFF00FF00FF00FF00)


class Graph:
    """Hash-consed expression nodes: equal id <=> equal expression."""

    def __init__(self):
        self.ids = {}

    def node(self, *key):
        return self.ids.setdefault(key, len(self.ids))

    def kinv(self, i, j):
        return self.node("Kinv", i, j)

    def v(self, call, t):
        return self.node("v", call, t)

    def const(self, x):
        return self.node("const", x)

    def fma(self, a, b, c):
        return self.node("fma", a, b, c)

    def add(self, a, b):
        return self.node("add", a, b)


class Lds:
    """Words tagged with what they were written for."""

    def __init__(self, size):
        self.w = [None] * size

    def write(self, i, tag, node):
        assert 0 <= i < len(self.w), ("LDS write out of the region", i)
        self.w[i] = (tag, node)

    def read(self, i, tag):
        assert 0 <= i < len(self.w), ("LDS read out of the region", i)
        got = self.w[i]
        assert got is not None and got[0] == tag, ("stale, unwritten or absent-slot word", i, tag, got)
        return got[1]


def blocks(G):
    """What the sweep leaves: lane 8 g + s holds the BS x BS block (g, s) of K^-1 (identity on the padding: the same
    leaves stand for whatever both forms stage)."""
    return {(t >> 3, t & 7): [[G.kinv(BS * (t >> 3) + k, BS * (t & 7) + l) for l in range(BS)] for k in range(BS)]
            for t in range(64)}


def stage_rows(G, lds):
    """The row form's tail: row-major staging, lane r reads row r whole in round r % BS (lanes >= NN: row 0's slot)."""
    Kb = blocks(G)
    rows = [None] * 64
    for k in range(BS):
        for (g, s), B in Kb.items():
            for l in range(BS):
                lds.write(g * ST + BS * s + l, ("stage", k), B[k][l])
        for t in range(64):
            if t % BS == k:
                rg = t // BS if t < NN else 0
                rows[t] = [lds.read(rg * ST + j, ("stage", k)) for j in range(NN)]
    return rows


def row_of(m, slot):
    """The row -> (lane, slot) map of the class form: the row in slot `slot` of the lanes 16 c + m (None: absent)."""
    if slot == 2:
        return BS * m + 4 if m < 8 else None
    return BS * (m & 7) + (m >> 3) + 2 * slot


def stage_classes(G, lds):
    """The class form's tail: class-major staging, lane 16 c + m reads the KCL entries of class c of staged row m % 8
    into slot k / 2 under round k's constant mask.  Returns Kc[lane][slot][i] (absent slot: exact zeros)."""
    Kb = blocks(G)
    zero = G.const(0.0)
    Kc = [[[zero] * KCL for _ in range(3)] for _ in range(64)]
    for k in range(BS):
        for (g, s), B in Kb.items():
            for l in range(BS):
                col = BS * s + l
                lds.write(g * ST + (col & 3) * KCL + (col >> 2), ("stage", k), B[k][l])
        for t in range(64):
            if (MASKS[k & 1] >> t) & 1:
                lc, lm = t >> 4, t & 15
                ra = (lm & 7) * ST + KCL * lc
                Kc[t][k >> 1] = [lds.read(ra + i, ("stage", k)) for i in range(KCL)]
    return Kc


def kmul_rows(G, lds, rows, n, call):
    """Row form: lane t < NN publishes v_t (0.0 on the padding), every lane reads the whole vector and runs four chains
    of NN / 4 fma from +0.0, chain c over the columns = c mod 4 ascending; (sa0 + sa1) + (sa2 + sa3)."""
    zero = G.const(0.0)
    for t in range(NN):
        lds.write(t, ("v", call), G.v(call, t) if t < n else zero)
    out = [None] * NN
    for t in range(n):   # own lanes (the others return 0.0)
        vb = [lds.read(j, ("v", call)) for j in range(NN)]
        sa = [zero] * 4
        for j in range(NN):
            sa[j % 4] = G.fma(rows[t][j], vb[j], sa[j % 4])
        out[t] = G.add(G.add(sa[0], sa[1]), G.add(sa[2], sa[3]))
    return out


def kmul_classes(G, lds, Kc, n, call):
    """Class form: the kernel's Kmul under K64."""
    zero = G.const(0.0)
    for t in range(NN):
        lds.write((t & 3) * KCL + (t >> 2), ("v", call), G.v(call, t) if t < n else zero)
    for t in range(64):
        lc, lm = t >> 4, t & 15
        vc = [lds.read(KCL * lc + i, ("v", call)) for i in range(KCL)]
        pa = [zero] * 3
        for i in range(KCL):
            for s in range(3):
                pa[s] = G.fma(Kc[t][s][i], vc[i], pa[s])
        r0 = BS * (lm & 7) + (lm >> 3)
        kw0 = (KPB if lc & 2 else KPA) + 2 * r0 + (lc & 1)
        kw2 = kw0 + 8 if lm < 8 else KPD + 8 * lc + (lm & 7)
        lds.write(kw0, ("p", call), pa[0])
        lds.write(kw0 + 4, ("p", call), pa[1])
        lds.write(kw2, ("p", call) if lm < 8 else ("absent", call), pa[2])
    out = [None] * NN
    for t in range(n):   # own lanes; lanes n .. 63 read in bounds (checked below) and return 0.0
        p = [lds.read(KPA + 2 * t, ("p", call)), lds.read(KPA + 2 * t + 1, ("p", call)),
             lds.read(KPB + 2 * t, ("p", call)), lds.read(KPB + 2 * t + 1, ("p", call))]
        out[t] = G.add(G.add(p[0], p[1]), G.add(p[2], p[3]))
    return out


CASES = [(40, 40), (40, 34), (40, 26), (40, 10), (40, 2)]


@pytest.mark.parametrize("nn,n", CASES)
def test_kmul64_same_expressions_as_row_form(nn, n):
    """Staging from the blocks, then two mat-vecs in the same scratch region (the second must see none of the first's
    words): every own row's result is the same expression node in both programs."""
    assert nn == NN
    G = Graph()
    rows = stage_rows(G, Lds(NU))
    lds = Lds(NU)
    Kc = stage_classes(G, lds)
    for call in range(2):
        ref = kmul_rows(G, Lds(NU), rows, n, call)
        got = kmul_classes(G, lds, Kc, n, call)
        bad = [t for t in range(n) if ref[t] != got[t]]
        assert not bad, (call, bad[:10])


def test_kmul64_slots_hold_the_rows_classes():
    """After the staging, slot s of lane 16 c + m holds row_of(m, s)'s entries of the columns c, c + 4, ... ascending,
    and an absent slot exact zeros."""
    G = Graph()
    Kc = stage_classes(G, Lds(NU))
    zero = G.const(0.0)
    for t in range(64):
        lc, lm = t >> 4, t & 15
        for s in range(3):
            r = row_of(lm, s)
            want = [zero] * KCL if r is None else [G.kinv(r, lc + 4 * i) for i in range(KCL)]
            assert Kc[t][s] == want, (t, s)


def test_kmul64_row_map_is_a_bijection():
    """Each class deals the 40 rows over its 16 lanes exactly once: 8 lanes hold three rows, 8 hold two."""
    held = [[row_of(m, s) for s in range(3)] for m in range(16)]
    rows = sorted(r for h in held for r in h if r is not None)
    assert rows == list(range(NN))
    assert sorted(sum(r is not None for r in h) for h in held) == [2] * 8 + [3] * 8


def test_kmul64_absent_slots_never_reach_the_combine():
    """The words the absent slots store to lie outside everything a lane reads back (lanes >= NN included), inside the
    region, and no two stores of one mat-vec share a word."""
    read = set()
    for t in range(64):
        read |= {KPA + 2 * t, KPA + 2 * t + 1, KPB + 2 * t, KPB + 2 * t + 1}
    assert max(read) < NU and min(read) >= NN   # past the vector
    real, absent = [], []
    for t in range(64):
        lc, lm = t >> 4, t & 15
        kw0 = (KPB if lc & 2 else KPA) + 2 * (BS * (lm & 7) + (lm >> 3)) + (lc & 1)
        real += [kw0, kw0 + 4] + ([kw0 + 8] if lm < 8 else [])
        absent += [] if lm < 8 else [KPD + 8 * lc + (lm & 7)]
    assert len(set(real)) == len(real) == 4 * NN and len(set(absent)) == len(absent) == 32
    assert not set(absent) & read and not set(absent) & set(real)
    assert all(NN <= w < NU for w in real + absent)
    # the combine of the rows reads exactly the real words
    assert set(real) == {w for t in range(NN) for w in (KPA + 2 * t, KPA + 2 * t + 1, KPB + 2 * t, KPB + 2 * t + 1)}

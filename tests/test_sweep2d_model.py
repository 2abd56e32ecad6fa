"""The 8 x 8 block sweep of the fused capacity-40 solve kernel (csrc/mpc_solve.h, TGMPC_SWEEP_2D) as a dataflow model
of its lane program, beside the row-per-lane receiver sweep it replaces.

Both programs are run on TAGGED operands: every value is a node of a hash-consed expression graph (leaf K[i][j], or
rcp / mul / fma / neg of nodes), so two values are the same node exactly when they are the same operations on the same
operands in the same order -- the condition for equal bits on the GPU.  The only identity used is neg(neg(x)) = x, which
is exact in IEEE arithmetic (the kernel forms the pivot row as fma(-(-dinv), c_j, +0.0) with the fma's source modifier).

The 2D model follows the kernel statement by statement: lane 8 g + s holds the BS x BS block (g, s); the pivot column is
published in two alternating LDS slots by the lanes that hold it, after they have formed it first; every lane reads
c[BS g ..], c[BS s ..] and c[p] from the slot; the lanes of block row p / BS zero their pivot row and take -dinv as its
factor; the lanes of block column p / BS overwrite local column p % BS; at the end the negated blocks go through an
8-row LDS staging area, one local row per round, from which lane r reads row r under a mask.  LDS words carry the pivot
(or round) they were written for, so a read of a stale or unwritten word fails the test.

CPU only: the algebra and the dataflow, not the kernel (tests/test_sweep2d_gpu.py compares the kernel's results with
the parent commit's bit for bit)."""
import numpy as np
import pytest


class Graph:
    """Hash-consed expression nodes: equal id <=> equal expression."""

    def __init__(self):
        self.ids = {}
        self.nodes = []

    def node(self, *key):
        i = self.ids.get(key)
        if i is None:
            i = len(self.nodes)
            self.ids[key] = i
            self.nodes.append(key)
        return i

    def leaf(self, i, j):
        return self.node("K", i, j)

    def const(self, v):
        return self.node("const", v)

    def rcp(self, a):
        return self.node("rcp", a)

    def mul(self, a, b):
        return self.node("mul", a, b)

    def fma(self, a, b, c):
        return self.node("fma", a, b, c)

    def neg(self, a):
        k = self.nodes[a]
        return k[1] if k[0] == "neg" else self.node("neg", a)   # -(-x) = x, exact

    def evaluate(self, K):
        """Every node's value in float64 for the real matrix K (the fma as a * b + c: a model of the values only)."""
        v = np.zeros(len(self.nodes))
        for i, k in enumerate(self.nodes):
            op = k[0]
            if op == "K":
                v[i] = K[k[1], k[2]]
            elif op == "const":
                v[i] = k[1]
            elif op == "rcp":
                v[i] = 1.0 / v[k[1]]
            elif op == "mul":
                v[i] = v[k[1]] * v[k[2]]
            elif op == "fma":
                v[i] = v[k[1]] * v[k[2]] + v[k[3]]
            else:
                v[i] = -v[k[1]]
        return v


def initial(G, NN, n):
    """K as the kernels load it: the real n x n block, identity padding up to NN."""
    return [[G.leaf(i, j) if (i < n and j < n) else G.const(1.0 if i == j else 0.0) for j in range(NN)]
            for i in range(NN)]


def sweep_rows(G, NN, n):
    """The row-per-lane receiver sweep (the parent's form): per pivot p every row's lane publishes c_r = K_rp, and
    K_ij <- fma(-(c_i dinv), c_j, K_ij); the receiver lane (an exact +0.0 row) takes fma(dinv, c_j, +0.0) as the new
    row p; K_ip <- c_i dinv, K_pp <- -dinv; all entries negated at the end."""
    K = initial(G, NN, n)
    zero = G.const(0.0)
    for p in range(NN):
        c = [K[r][p] for r in range(NN)]
        dinv = G.rcp(c[p])
        new = [[None] * NN for _ in range(NN)]
        for i in range(NN):
            if i == p:
                for j in range(NN):
                    new[i][j] = G.neg(dinv) if j == p else G.fma(dinv, c[j], zero)
            else:
                fd = G.mul(c[i], dinv)
                for j in range(NN):
                    new[i][j] = fd if j == p else G.fma(G.neg(fd), c[j], K[i][j])
        K = new
    return [[G.neg(K[i][j]) for j in range(NN)] for i in range(NN)]


def sweep_2d(G, NN, n):
    """The lane program of the 8 x 8 block sweep.  Returns the rows as lanes 0 .. NN-1 hold them afterwards."""
    BS = NN // 8
    assert BS * 8 == NN
    ST = NN + 2
    K0 = initial(G, NN, n)
    zero = G.const(0.0)
    lanes = [(t >> 3, t & 7) for t in range(64)]
    Kb = {(g, s): [[K0[BS * g + k][BS * s + l] for l in range(BS)] for k in range(BS)] for g, s in lanes}
    slot = [[None] * NN, [None] * NN]   # the two pivot-column slots: (pivot, node) per word

    def read(p, r):
        w = slot[p & 1][r]
        assert w is not None and w[0] == p, ("stale or unwritten pivot column word", p, r, w)
        return w[1]

    for g, s in lanes:
        if s == 0:
            for k in range(BS):
                slot[0][BS * g + k] = (0, Kb[g, s][k][0])
    for pb in range(8):
        for q in range(BS):
            p = pb * BS + q
            # (barrier) -- every lane reads the slot of pivot p before any lane writes the other slot's words, and the
            # words a lane writes below are read only after the next barrier
            rd = {(g, s): ([read(p, BS * g + k) for k in range(BS)], [read(p, BS * s + k) for k in range(BS)], read(p, p))
                  for g, s in lanes}
            writes = []
            for g, s in lanes:
                cg, cs, d = rd[g, s]
                B = Kb[g, s]
                prow, pcol = g == pb, s == pb
                dinv = G.rcp(d)
                f = [G.mul(cg[k], dinv) for k in range(BS)]
                if prow:
                    f[q] = G.neg(dinv)
                    for l in range(BS):
                        B[q][l] = zero
                q1 = (q + 1) % BS
                for k in range(BS):
                    B[k][q1] = G.fma(G.neg(f[k]), cs[q1], B[k][q1])
                if p + 1 < NN and (pcol if q + 1 < BS else s == pb + 1):
                    for k in range(BS):
                        writes.append((BS * g + k, B[k][q1]))
                for k in range(BS):
                    for l in range(BS):
                        if l != q1:
                            B[k][l] = G.fma(G.neg(f[k]), cs[l], B[k][l])
                if pcol:
                    for k in range(BS):
                        B[k][q] = f[k]
            rows_written = sorted(r for r, _ in writes)
            assert rows_written == (list(range(NN)) if p + 1 < NN else []), "column p + 1: every row exactly once"
            for r, v in writes:
                slot[(p + 1) & 1][r] = (p + 1, v)
    # the blocks, negated, back to rows through the staging area
    for g, s in lanes:
        Kb[g, s] = [[G.neg(v) for v in row] for row in Kb[g, s]]
    stage = [None] * (8 * ST)
    rows = [None] * 64
    for k in range(BS):
        for g, s in lanes:
            for l in range(BS):
                stage[g * ST + BS * s + l] = (k, Kb[g, s][k][l])
        for t in range(64):
            if t % BS == k:
                rg = t // BS if t < NN else 0
                got = stage[rg * ST:rg * ST + NN]
                assert all(w is not None and w[0] == k for w in got), ("stale staging word", k, t)
                rows[t] = [w[1] for w in got]
    return rows[:NN]


CASES = [(40, 40), (40, 34), (32, 26), (16, 16), (16, 10)]


@pytest.mark.parametrize("NN,n", CASES)
def test_sweep2d_same_expressions_as_row_form(NN, n):
    """Every entry of the result, and so every intermediate it depends on, is the same expression in both programs."""
    G = Graph()
    ref = sweep_rows(G, NN, n)
    got = sweep_2d(G, NN, n)
    bad = [(i, j) for i in range(NN) for j in range(NN) if ref[i][j] != got[i][j]]
    assert not bad, bad[:10]


@pytest.mark.parametrize("NN,n", [(40, 40), (40, 34), (16, 10)])
def test_sweep2d_model_is_the_inverse(NN, n):
    """The modelled program is the sweep operator: evaluated in float64 it gives K^-1 on the real block and the
    identity on the padding."""
    rng = np.random.default_rng(NN + n)
    A = rng.standard_normal((n, n))
    Kr = A @ A.T + n * np.eye(n)
    K = np.eye(NN)
    K[:n, :n] = Kr
    G = Graph()
    got = sweep_2d(G, NN, n)
    v = G.evaluate(K)
    R = np.array([[v[got[i][j]] for j in range(NN)] for i in range(NN)])
    inv = np.linalg.inv(K)
    assert np.abs(R - inv).max() <= 1e-12 * np.abs(inv).max()

"""The device CSV reader on the MI355X (csrc/dataset_parse.hip, dataset.read_csv_device, load_vehicle_dataset(device_csv=
True)) against the host reader (read_csv_native, traj_dataset_read_csv), Python's float() and the pandas loader: bit
for bit, no tolerance.  The files are the smallest that reach every path: the formatter tests' shapes (1, 0), (3, 5)
and (67, 130) = 8,777 rows (69 workgroups of the 128-row parse kernel, a few hundred chunks of the line index), bodies
of TRAJ_CSV_PARSE_CHUNK - 1, + 0 and + 1 bytes, a row longer than the parse kernel's 32 KiB of LDS."""
import functools
import os

import numpy as np
import pytest

import torch

from tests import _csv_parse_cases as K
from tests.test_csv_format_gpu import SHAPES, TS, case
from trajectory_generation_amd import _lib
from trajectory_generation_amd import dataset as D

pytestmark = pytest.mark.gpu

CHUNK = _lib.CSV_PARSE_CHUNK
LDS_STAGE = 128 * 256        # csrc/dataset_parse.hip CSV_PARSE_STAGE


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("csvparse"))


def assert_same_block(got, want):
    """Two float64 blocks, bit for bit, NaN compared as NaN."""
    got, want = got.cpu().numpy(), want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), np.argwhere(gn != wn)[:5]
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~gn)
    assert bad.size == 0, [(tuple(i), got[tuple(i)].hex(), want[tuple(i)].hex()) for i in bad[:5]]


def assert_reads_like_host(path, **kw):
    """read_csv_device(path) == read_csv_native(path); returns the device call's timings."""
    tm = {}
    names, got = D.read_csv_device(path, timings=tm, **kw)
    hnames, want = D.read_csv_native(path)
    assert names == hnames and got.is_cuda and got.dtype == torch.float64
    assert_same_block(got, want)
    assert tm["rows"] == want.shape[0] and tm["bytes"] == os.path.getsize(path)
    return tm


def write(tmp, name, data):
    p = os.path.join(tmp, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@functools.lru_cache(maxsize=None)
def host_bits(which):
    """float()'s bits of a token set: computed once, shared."""
    return K.float_bits(getattr(K, which)())


def test_parse_f64_batch_equals_the_host_and_float():
    tokens = K.edge_spellings() + K.random_reprs() + K.halfway_integers() + K.RANGE_EDGES[:5] + K.FALLBACKS + \
        [b"", b"nan", b"NaN", b"inf", b"-inf", b"-0.0", b"12345678901234567890e-5"]
    assert len(tokens) % 64 != 0
    fill = -7.25
    got, st = D.parse_f64_batch(tokens, fill=fill)
    hv, hs = D.parse_f64_host(tokens, fill=fill)
    got, st = got.cpu().numpy().view(np.uint64), st.cpu().numpy()
    assert np.array_equal(st, hs)
    bad = np.nonzero(got != hv.view(np.uint64))[0]
    assert bad.size == 0, [(tokens[i], hex(got[i]), hex(hv.view(np.uint64)[i])) for i in bad[:5]]
    n = len(K.edge_spellings()) + len(K.random_reprs()) + len(K.halfway_integers()) + 5
    want = np.concatenate([host_bits("edge_spellings"), host_bits("random_reprs"), host_bits("halfway_integers"),
                           K.float_bits(K.RANGE_EDGES[:5])])
    assert (st[:n] == _lib.PARSE_OK).all() and np.array_equal(got[:n], want)
    assert (st[n:n + len(K.FALLBACKS)] == _lib.PARSE_FALLBACK).all()


def nonfinite_case():
    X, U, ids, nids = (a.copy() for a in case(3, 5))
    X[0, 1, 0], X[1, 2, 2], X[2, 5, 5], X[0, 0, 3] = np.nan, np.inf, -np.inf, -0.0
    U[1, 0, 0], U[2, 4, 1], U[0, 3, 1] = np.nan, np.inf, -np.inf
    return X, U, ids, nids


@pytest.mark.parametrize("B,T,nonfinite", [(*s, False) for s in SHAPES] + [(3, 5, True)])
def test_files_equal_the_host_readers(B, T, nonfinite, tmp):
    X, U, ids, nids = nonfinite_case() if nonfinite else case(B, T)
    prefix = os.path.join(tmp, f"host_{B}_{T}_{int(nonfinite)}")
    D.write_csv(prefix, X, U, ids, TS, native=True, noise_ids=nids)
    for kind in ("clean", "noisy"):
        tm = assert_reads_like_host(f"{prefix}_{kind}.csv")
        assert tm["fallback_fields"] == 0 and tm["rows"] == B * (T + 1)
        assert set(tm["kernel_ms"]) == {"count", "scan", "starts", "parse"}
    if nonfinite:
        _, t = D.read_csv_device(prefix + "_clean.csv")
        assert bool(t.isnan().any()) and bool(t.isinf().any())
    if (B, T) == (67, 130):
        # many slabs through both pinned buffers give the same block
        assert_reads_like_host(prefix + "_clean.csv", slab_bytes=4096)


def test_degenerate_files(tmp):
    for name, data, shape in (("empty", b"", (0, 1)), ("header_no_newline", b"X,Y,phi", (0, 3)),
                              ("header_only", b"X,Y,phi\n", (0, 3)), ("no_final_newline", b"X,Y,phi\n1,2,3\n4,5,6", (2, 3)),
                              ("crlf", b"X,Y,phi\r\n1,2,3\r\n4,5.5,6\r\n", (2, 3)), ("one_row", b"X,Y,phi\n1,-2e-3,\n", (1, 3)),
                              ("one_row_no_newline", b"X,Y,phi\n7,8,9", (1, 3)),
                              ("empty_fields", b"X,Y,phi\n,,\n1,,3\nnan,inf,-inf\n", (3, 3)),
                              ("extra_fields", b"X,Y,phi\n1,2,3,4,5\n6,7,8\n", (2, 3))):
        p = write(tmp, name + ".csv", data)
        names, t = D.read_csv_device(p)
        assert tuple(t.shape) == shape, name
        assert_reads_like_host(p)
    names, t = D.read_csv_device(os.path.join(tmp, "header_only.csv"))
    assert names == ["X", "Y", "phi"] and tuple(t.shape) == (0, 3) and t.is_cuda
    # a row with a field missing, a blank line, a field that is no number: the host's error
    for name, data in (("short_row", b"X,Y,phi\n1,2,3\n1,2\n4,5,6\n"), ("blank_line", b"X,Y,phi\n1,2,3\n\n4,5,6\n"),
                       ("garbage", b"X,Y,phi\n1,zz,3\n"), ("cr_inside", b"X,Y,phi\n1\r,2,3\n")):
        p = write(tmp, name + ".csv", data)
        with pytest.raises(RuntimeError) as host:
            D.read_csv_native(p)
        with pytest.raises(type(host.value)):
            D.read_csv_device(p)
    with pytest.raises(FileNotFoundError):
        D.read_csv_device(os.path.join(tmp, "missing.csv"))


def body_of(length):
    """A body of exactly `length` bytes that ends in a newline: ordinary rows, then one whose first field is padded
    with leading zeros."""
    row = b"1.5,-2.25,3e-05\n"
    n = max(0, length // len(row) - 1)
    last = b"7.125,8,9\n"
    pad = length - n * len(row) - len(last)
    assert pad >= 0
    return row * n + b"0" * pad + last


def test_chunk_edges(tmp):
    more = b"0.1,0.2,0.3\n-4,5e3,6\n"
    bodies = {f"len_{d:+d}": body_of(CHUNK + d) for d in (-1, 0, 1)}
    bodies["newline_on_last_byte_of_a_chunk"] = body_of(CHUNK) + more          # '\n' at byte CHUNK - 1
    bodies["newline_on_first_byte_of_a_chunk"] = body_of(CHUNK + 1) + more     # '\n' at byte CHUNK
    bodies["second_chunk_edge"] = body_of(CHUNK) + body_of(CHUNK) + more
    for d in (-1, 0, 1):
        bodies[f"len_{d:+d}_no_final_newline"] = body_of(CHUNK + d + 1)[:-1]
    assert bodies["newline_on_last_byte_of_a_chunk"][CHUNK - 1:CHUNK] == b"\n"
    assert bodies["newline_on_first_byte_of_a_chunk"][CHUNK:CHUNK + 1] == b"\n"
    assert [len(bodies[f"len_{d:+d}"]) for d in (-1, 0, 1)] == [CHUNK - 1, CHUNK, CHUNK + 1]
    for name, body in bodies.items():
        tm = assert_reads_like_host(write(tmp, name + ".csv", b"X,Y,phi\n" + body))
        assert tm["rows"] == body.count(b"\n") + (0 if body.endswith(b"\n") else 1) and tm["fallback_fields"] == 0


def test_a_row_longer_than_the_lds_buffer(tmp):
    """Row 150 of 400 is 40,000 bytes long: its workgroup's span exceeds the staging buffer and takes the direct
    path, the other workgroups stage theirs."""
    rng = np.random.default_rng(9)
    rows = [",".join(repr(x) for x in rng.standard_normal(4).tolist()).encode() for _ in range(400)]
    long_field = b"0" * 40_000 + b"2.5"
    assert len(long_field) > LDS_STAGE
    rows[150] = b"-1.25," + long_field + b",3,4"
    p = write(tmp, "long_row.csv", b"a,b,c,d\n" + b"\n".join(rows) + b"\n")
    tm = assert_reads_like_host(p)
    assert tm["fallback_fields"] == 0
    _, t = D.read_csv_device(p)
    assert t[150].tolist() == [-1.25, 2.5, 3.0, 4.0]


def test_fallback_path(tmp):
    rng = np.random.default_rng(10)
    cells = [[repr(x).encode() for x in rng.standard_normal(3).tolist()] for _ in range(300)]
    cells[7][1] = b"1234567890123456789012345"
    cells[130][0] = b"1e999"
    cells[131][2] = b"-1234567890123456789012345e-30"
    cells[299][2] = b"infinity"
    tokens = [c for r in cells for c in r]
    declined = int((D.parse_f64_host(tokens)[1] == _lib.PARSE_FALLBACK).sum())
    assert declined == 3                                   # 1e999 is the device's own: inf
    body = b"\n".join(b",".join(r) for r in cells) + b"\n"
    p = write(tmp, "fallback.csv", b"X,Y,phi\n" + body)
    tm = assert_reads_like_host(p)
    assert tm["fallback_fields"] == declined
    _, t = D.read_csv_device(p)
    assert t[7, 1].item() == float("1234567890123456789012345") and t[130, 0].item() == float("inf")
    assert t[131, 2].item() == float("-1234567890123456789012345e-30") and t[299, 2].item() == float("inf")
    # more declined fields than records: the whole file goes through the host reader, the same block
    tm = assert_reads_like_host(p, fallback_cap=1)
    assert tm["fallback_fields"] == declined
    assert_reads_like_host(p, fallback_cap=0)
    assert_reads_like_host(p, fallback_cap=declined)
    # a field neither reader takes raises the host's error, through either path
    cells[200][1] = b"+1.5"
    p = write(tmp, "fallback_bad.csv", b"X,Y,phi\n" + b"\n".join(b",".join(r) for r in cells) + b"\n")
    with pytest.raises(RuntimeError) as host:
        D.read_csv_native(p)
    for cap in (None, 1):
        with pytest.raises(type(host.value)):
            D.read_csv_device(p, fallback_cap=cap)


def test_parse_pass_reads_and_writes_inside_what_it_was_given(tmp):
    """The bounds guard: the parse pass is given the text's size minus one byte (digits follow the text in its
    allocation, so a byte read past nbytes would change the last value) and fewer rows than the text holds, inside a
    guard-padded output.  Only the given rows are written; everything else stays 0xA5."""
    B, T = 67, 130
    X, U, ids, nids = case(B, T)
    prefix = os.path.join(tmp, "bounds")
    D.write_csv(prefix, X, U, ids, TS, native=True, noise_ids=nids)
    body = open(prefix + "_clean.csv", "rb").read().split(b"\n", 1)[1]
    _, want = D.read_csv_native(prefix + "_clean.csv")
    want = want.numpy()
    size, ncols = len(body), want.shape[1]
    text = torch.from_numpy(np.frombuffer(body + b"7" * 4096, dtype=np.uint8).copy()).cuda()
    rows, starts = D.csv_parse_index(text, size)
    assert rows == B * (T + 1) == want.shape[0]
    newlines = np.flatnonzero(np.frombuffer(body[:-1], dtype=np.uint8) == 10)
    assert np.array_equal(starts.cpu().numpy(), np.concatenate([[0], newlines + 1]))
    guard = 512
    for nbytes, given in ((size, rows), (size - 1, rows), (size - 1, rows - 5), (size - 1, 1)):
        out = torch.full(((rows + guard) * ncols * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        rec = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
        D.csv_parse_rows(text, nbytes, starts, given, ncols, out.view(torch.float64), err, cnt, rec)
        torch.cuda.synchronize()
        assert int(err[0]) == 0 and int(cnt[0]) == 0
        h = out.cpu().numpy()
        assert (h[given * ncols * 8:] == 0xA5).all()
        assert_same_block(torch.from_numpy(h[:given * ncols * 8].view(np.float64).reshape(given, ncols)), want[:given])
    # starts that do not describe the text are flagged, and nothing is read or written for them
    bad = starts.clone()
    bad[200] = size + 100
    out = torch.full((rows * ncols * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    D.csv_parse_rows(text, size, bad, rows, ncols, out.view(torch.float64), err, cnt, rec)
    assert int(err[0]) & 2
    assert (out.cpu().numpy().reshape(rows, ncols * 8)[200] == 0xA5).all()


def test_gather_cast_equals_numpy():
    """The gather pass's cast on the bits against numpy.astype(np.float32): random float64 patterns, random float32s,
    the exact ties between neighbouring float32s (subnormal ones included) and the doubles next to the ties, the
    subnormal and overflow boundaries; and the [n, C, T] layout with a permuted row index."""
    rng = np.random.default_rng(0)
    f = rng.integers(0, 2 ** 32, size=200_000, dtype=np.uint32).view(np.float32)
    f = f[np.isfinite(f)]
    with np.errstate(over="ignore"):
        tie = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    v = np.concatenate([rng.integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64), f.astype(np.float64),
                        tie, np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf),
                        [1e-40, 1e39, -1e39, 1e-46, 7e-46, 2.0 ** -150, -2.0 ** -150, 2.0 ** -149, 2.0 ** -126, 5e-324,
                         3.4028235677973366e38, 3.4028234663852886e38, 0.0, -0.0, np.inf, -np.inf, np.nan]])
    n, T, C = 7, v.size // 7, 3
    src = np.zeros((n * T, C))
    src[:, 2] = v[:n * T]
    src[:, 0] = -v[:n * T]
    perm = rng.permutation(n * T)
    got = D.csv_gather_f32(torch.from_numpy(src).cuda(), torch.from_numpy(perm).cuda(), n, T, [2, 0]).cpu().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        want = src[perm][:, [2, 0]].astype(np.float32).reshape(n, T, 2).transpose(0, 2, 1)
    assert got.shape == want.shape == (n, 2, T)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ok)
    assert bad.size == 0, [(tuple(i), hex(got.view(np.uint32)[tuple(i)]), hex(want.view(np.uint32)[tuple(i)])) for i in bad[:5]]
    with pytest.raises(RuntimeError):        # a row index outside the block is refused, not read
        D.csv_gather_f32(torch.from_numpy(src).cuda(), torch.tensor([0, n * T], device="cuda"), 1, 2, [0])


def shuffled_dataset(tmp, name, X, U, Ts):
    """The host writer's files with each file's rows shuffled and stably re-sorted by id (the construction of
    test_native_loader_matches_pandas_loader): rows out of order inside every trajectory."""
    import pandas as pd
    p = os.path.join(tmp, name)
    D.write_csv(p, X, U, np.arange(X.shape[0]), Ts)
    for s in ("clean", "noisy"):
        df = pd.read_csv(f"{p}_{s}.csv")
        df.sample(frac=1.0, random_state=3).sort_values("trajectory_id", kind="stable").to_csv(f"{p}_{s}.csv", index=False)
    return f"{p}_noisy.csv", f"{p}_clean.csv"


def assert_same_parts(a, b, on_device=True):
    for pa, pb in zip(a, b):
        for ta, tb in zip(pa, pb):
            assert ta.dtype == torch.float32 and ta.is_cuda == on_device and ta.shape == tb.shape
            ta, tb = ta.cpu(), torch.as_tensor(tb).cpu()
            assert torch.equal(ta.isnan(), tb.isnan())
            assert torch.equal(ta.nan_to_num().view(torch.int32), tb.nan_to_num().view(torch.int32))


def test_loader_equals_the_pandas_loader(tmp):
    pytest.importorskip("pandas")
    rng = np.random.default_rng(1)
    B, T = 12, 30
    X = np.cumsum(rng.normal(size=(B, T + 1, 6)) * 0.01, axis=1)
    U = rng.normal(size=(B, T, 2)) * 0.1
    # float32 subnormals, float32 overflow, ties of the float32 cast: in every trajectory, in columns the noise leaves
    X[:, 0::3, 2], X[:, 1::3, 4], X[:, 2::3, 0] = 1e-40, 1e39, 1.0 + 2.0 ** -24
    U[:, 0::3, 0], U[:, 1::3, 1], U[:, 2::3, 1] = -1e-40, -1e39, 1.0 + 3 * 2.0 ** -24
    noisy, clean = shuffled_dataset(tmp, "ds", X, U, 0.05)
    with np.errstate(over="ignore"):
        want = D.load_vehicle_dataset(noisy, clean, T_steps=25)
    got = D.load_vehicle_dataset(noisy, clean, T_steps=25, device_csv=True)
    assert_same_parts(got, want)
    y, u, x = got[0]
    assert bool(u.isinf().any()) and bool(x.isinf().any())
    assert bool(((u != 0) & (u.abs() < 1.1754944e-38)).any()) and bool(((x != 0) & (x.abs() < 1.1754944e-38)).any())
    assert D.load_vehicle_dataset(noisy, clean, T_steps=40, device_csv=True) is None
    assert D.load_vehicle_dataset(os.path.join(tmp, "missing.csv"), clean, device_csv=True) is None
    # an id column that is not all non-negative integers hands the call to the host loader: its tensors
    data = open(noisy, "rb").read()
    assert data.endswith(b",11\n")
    frac = write(tmp, "ds_frac_noisy.csv", data[:-4] + b",11.5\n")
    with np.errstate(over="ignore"):
        host = D.load_vehicle_dataset(frac, clean, T_steps=25, native=True, device="cuda")
        assert_same_parts(D.load_vehicle_dataset(frac, clean, T_steps=25, device_csv=True), host)


def test_loader_equals_the_references_golden(tmp):
    """tests/golden/loader.npz is the reference's own loader on the files of tests/golden/gen_loader_golden.py; the
    device path gives its tensors bit for bit."""
    pytest.importorskip("pandas")
    rng = np.random.default_rng(11)
    B, T = 10, 30
    X, U, Ts = rng.normal(size=(B, T + 1, 6)), rng.normal(size=(B, T, 2)), 0.01
    clean, noisy = D.frames(X, U, np.arange(B), Ts)
    clean.to_csv(os.path.join(tmp, "gold_c.csv"), index=False)
    noisy.to_csv(os.path.join(tmp, "gold_n.csv"), index=False)
    got = D.load_vehicle_dataset(os.path.join(tmp, "gold_n.csv"), os.path.join(tmp, "gold_c.csv"), T_steps=25,
                                 device_csv=True)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loader.npz"))
    want = tuple(tuple(g[f"{part}_{k}"] for k in "yux") for part in ("train", "val", "test"))
    assert_same_parts(got, want)


def test_round_trip_of_the_generated_dataset(tmp):
    """generate_open_loop(device_csv=True) writes on the device, read_csv_device reads on the device: exactly the
    doubles that were written (the noisy file's recomputed as x + noise)."""
    B, T, Ts = 4, 6, 0.01
    prefix = os.path.join(tmp, "round_trip")
    X, U = D.generate_open_loop(B, T, Ts=Ts, out_prefix=prefix, device_csv=True)
    X, U = X.cpu().numpy(), U.cpu().numpy()
    R = T + 1
    t = np.tile(np.arange(R) * Ts, B)
    dU = np.concatenate([U, np.full((B, 1, 2), np.nan)], axis=1).reshape(B * R, 2)
    tid = np.repeat(np.arange(B, dtype=np.float64), R)
    Xn = X + np.stack([D.measurement_noise(i, R) for i in range(B)])
    names, c = D.read_csv_device(prefix + "_clean.csv")
    assert names == D.CLEAN_COLUMNS
    assert_same_block(c, np.column_stack([t, X.reshape(B * R, 6), dU, tid]))
    names, n = D.read_csv_device(prefix + "_noisy.csv")
    assert names == D.NOISY_COLUMNS
    assert_same_block(n, np.column_stack([t, Xn.reshape(B * R, 6)[:, [0, 1, 3, 4, 5]], dU, tid]))

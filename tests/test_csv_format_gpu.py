"""The device CSV path on the MI355X (csrc/dataset_fmt.hip, dataset.write_csv_device) against the host writer
(write_csv(native=True), traj_dataset_write_csv) and Python's repr: byte for byte, no tolerance.  The shapes are the
smallest that reach every path: (1, 0) one row and no controls, (3, 5) one partial workgroup, (67, 130) = 8,777 rows
(69 workgroups of the 128-row format kernel, 35 of the 256-thread length kernel, no multiple of 64, 128 or 256)."""
import functools
import os

import numpy as np
import pytest

import torch

from tests._csv_fmt_cases import edge_values, py_fields
from trajectory_generation_amd import _lib
from trajectory_generation_amd import dataset as D

pytestmark = pytest.mark.gpu

TS = 0.01
SHAPES = [(1, 0), (3, 5), (67, 130)]


@functools.lru_cache(maxsize=None)
def case(B, T):
    """Seeded X, U, ids, noise ids with deliberately uneven row lengths: short values (0.5, 0.0, -2.0), long ones
    (1.2345678901234567e-300), an id above 2^40 and noise ids that differ from the ids."""
    rng = np.random.default_rng(1000 * B + T)
    X = rng.standard_normal((B, T + 1, 6)) * 10.0 ** rng.uniform(-4, 3, (B, T + 1, 6))
    U = rng.uniform(-1, 1, (B, T, 2))
    pick = rng.random(X.shape)
    X[pick < 0.10] = 0.5
    X[(pick >= 0.10) & (pick < 0.15)] = 1.2345678901234567e-300
    X[(pick >= 0.15) & (pick < 0.18)] = 0.0
    X[(pick >= 0.18) & (pick < 0.20)] = -2.0
    X[(pick >= 0.20) & (pick < 0.22)] = 123456789012345.6
    if T:
        U[rng.random(U.shape) < 0.2] = 0.25
    ids = np.arange(B, dtype=np.int64) * 7 + 3
    ids[B // 2] = (1 << 40) + 12345
    noise_ids = np.arange(B, dtype=np.int64)[::-1] + 100
    return X, U, ids, noise_ids


@functools.lru_cache(maxsize=None)
def host_files(B, T, tmp):
    """The host writer's two files for case(B, T): computed once, shared."""
    X, U, ids, nids = case(B, T)
    prefix = os.path.join(tmp, f"host_{B}_{T}")
    D.write_csv(prefix, X, U, ids, TS, native=True, noise_ids=nids)
    return open(prefix + "_clean.csv", "rb").read(), open(prefix + "_noisy.csv", "rb").read()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("csvdev"))


def device_files(prefix, X, U, ids, nids, **kw):
    Xd, Ud = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(np.ascontiguousarray(U)).cuda()
    D.write_csv_device(prefix, Xd, Ud, ids, TS, noise_ids=nids, **kw)
    return open(prefix + "_clean.csv", "rb").read(), open(prefix + "_noisy.csv", "rb").read()


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    i = int(d[0]) if d.size else n
    return f"lengths {len(a)} / {len(b)}, first difference at byte {i}: {a[max(0, i - 40):i + 40]!r} / {b[max(0, i - 40):i + 40]!r}"


def assert_same(got, want):
    for g, w in zip(got, want):
        assert g == w, first_difference(g, w)


def test_format_f64_batch_equals_repr():
    bits = np.random.default_rng(5).integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64)
    v = np.concatenate([edge_values(), bits])
    assert v.size % 64 != 0
    got = D.format_f64_batch(torch.from_numpy(v).cuda())
    want = py_fields(v)
    bad = [i for i in range(v.size) if got[i] != want[i]]
    assert not bad, [(v[i].hex(), got[i], want[i]) for i in bad[:5]]


@pytest.mark.parametrize("B,T", SHAPES)
def test_files_equal_the_host_writers(B, T, tmp):
    X, U, ids, nids = case(B, T)
    tm = {}
    got = device_files(os.path.join(tmp, f"dev_{B}_{T}"), X, U, ids, nids, timings=tm)
    want = host_files(B, T, tmp)
    assert_same(got, want)
    assert tm["bytes"] == len(want[0]) + len(want[1]) and tm["slabs"] == (2 if B else 0)
    rows = want[0].split(b"\n")[1:-1]
    assert len(rows) == B * (T + 1) and len({len(r) for r in rows}) > (1 if B * (T + 1) > 1 else 0)   # uneven rows


def test_files_equal_pandas(tmp):
    pytest.importorskip("pandas")
    X, U, ids, nids = case(3, 5)
    clean, noisy = D.frames(X, U, ids, TS, noise_ids=nids)
    want = (clean.to_csv(index=False).encode(), noisy.to_csv(index=False).encode())
    assert_same(device_files(os.path.join(tmp, "dev_pd"), X, U, ids, nids), want)


def test_many_slabs_give_the_same_bytes(tmp):
    """slab_bytes = 4096: slabs of at most 2048 bytes of whole rows, hundreds of them through both staging buffers."""
    X, U, ids, nids = case(67, 130)
    tm = {}
    got = device_files(os.path.join(tmp, "dev_slabs"), X, U, ids, nids, slab_bytes=4096, timings=tm)
    assert_same(got, host_files(67, 130, tmp))
    assert tm["slabs"] > 600
    with pytest.raises(ValueError):
        device_files(os.path.join(tmp, "dev_small"), X, U, ids, nids, slab_bytes=256)


def test_nan_and_inf_fields(tmp):
    X, U, ids, nids = (a.copy() for a in case(3, 5))
    X[0, 1, 0], X[1, 2, 2], X[2, 5, 5], X[0, 0, 3] = np.nan, np.inf, -np.inf, -0.0
    U[1, 0, 0], U[2, 4, 1], U[0, 3, 1] = np.nan, np.inf, -np.inf
    prefix = os.path.join(tmp, "host_nonfinite")
    D.write_csv(prefix, X, U, ids, TS, native=True, noise_ids=nids)
    want = (open(prefix + "_clean.csv", "rb").read(), open(prefix + "_noisy.csv", "rb").read())
    assert b",inf," in want[0] and b",-inf," in want[0] and b",," in want[0] and b",-0.0," in want[0]
    assert_same(device_files(os.path.join(tmp, "dev_nonfinite"), X, U, ids, nids), want)


def test_empty_dataset_is_header_only(tmp):
    X, U = np.zeros((0, 8, 6)), np.zeros((0, 7, 2))
    ids = np.zeros(0, dtype=np.int64)
    got = device_files(os.path.join(tmp, "dev_empty"), X, U, ids, ids)
    assert got == ((",".join(D.CLEAN_COLUMNS) + "\n").encode(), (",".join(D.NOISY_COLUMNS) + "\n").encode())


def test_write_pass_refuses_a_buffer_one_byte_short(tmp):
    """The bounds guard: the write pass is given the text's size minus one byte inside a guard-padded allocation.  It
    must return the error code and leave every byte from the given size on as it was; with the full size it writes
    the host writer's body and reports no error.  Nothing here stores out of range: the guard is what is checked."""
    B, T = 67, 130
    X, U, ids, _ = case(B, T)
    Xd, Ud, idd = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda(), torch.from_numpy(ids).cuda()
    n = B * (T + 1)
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    D.csv_device_rows(0, Xd, Ud, None, idd, TS, 0, n, ln, total)
    cum = torch.cumsum(ln, 0, dtype=torch.int64)
    off = cum - ln
    size = int(cum[-1])
    body = host_files(B, T, tmp)[0].split(b"\n", 1)[1]
    assert size == len(body) and int(total[0]) == size
    guard = 4096
    for given, code in ((size, _lib.TRAJ_OK), (size - 1, _lib.TRAJ_E_LAUNCH)):
        buf = torch.full((size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        D.csv_device_format(0, Xd, Ud, None, idd, TS, 0, n, off, ln, 0, buf, given, err)
        assert D.csv_device_check(err) == code
        h = buf.cpu().numpy()
        assert (h[given:] == 0xA5).all()
        if code == _lib.TRAJ_OK:
            assert h[:size].tobytes() == body
        else:
            # only the last workgroup's rows were refused: what was written is the body's, the rest untouched
            last = (n - 1) // 128 * 128
            cut = int(off[last])
            assert h[:cut].tobytes() == body[:cut] and (h[cut:] == 0xA5).all()


@pytest.mark.parametrize("gen", ["generate_piecewise", "generate_open_loop", "generate"])
def test_generators_write_the_same_files_either_way(gen, tmp):
    fn = getattr(D, gen)
    out = {}
    for dev in (False, True):
        prefix = os.path.join(tmp, f"{gen}_{int(dev)}")
        fn(4, 6, out_prefix=prefix, device_csv=dev)
        out[dev] = (open(prefix + "_clean.csv", "rb").read(), open(prefix + "_noisy.csv", "rb").read())
    assert out[False][0].count(b"\n") == 1 + 4 * 7
    assert_same(out[True], out[False])


def test_drop_failed_writes_the_same_files_three_ways(tmp):
    """_write_with_sidecar(drop_failed=True) on device tensors through the device writer, on device tensors through
    the host writer and on numpy arrays: trajectories 2 and 4 of 6 have a failed step, the other four are re-indexed
    0..3 and keep the noise of their generation ids 10, 11, 13, 15.  One warning each, the same bytes in all three
    files."""
    B, T = 6, 4
    rng = np.random.default_rng(64)
    X, U = rng.standard_normal((B, T + 1, 6)), rng.uniform(-1, 1, (B, T, 2))
    st = np.zeros((T, B), dtype=np.int32)
    st[0, 1], st[1, 2], st[3, 4] = 1, 6, 2
    ids = np.arange(10, 16)
    Xd, Ud, std = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda(), torch.from_numpy(st).cuda()
    out = {}
    for name, args, dev in (("dev", (Xd, Ud, std), True), ("host", (Xd, Ud, std), False), ("np", (X, U, st), False)):
        prefix = os.path.join(tmp, f"drop_{name}")
        with pytest.warns(UserWarning, match="left out 2 of 6"):
            D._write_with_sidecar(prefix, *args, ids, TS, True, dev)
        out[name] = tuple(open(f"{prefix}_{part}.csv", "rb").read() for part in ("clean", "noisy", "status"))
    assert_same(out["dev"], out["np"])
    assert_same(out["host"], out["np"])
    status = [ln.split(b",") for ln in out["np"][2].splitlines()[1:]]
    assert [int(r[0]) for r in status] == [0, 1, 2, 3] and [int(r[1]) for r in status] == [10, 11, 13, 15]
    for text in out["np"][:2]:
        rows = text.splitlines()[1:]
        assert [int(r.rsplit(b",", 1)[1]) for r in rows] == [i for i in range(4) for _ in range(T + 1)]
    # the noise is that of the generation ids, not of the written ids
    want = os.path.join(tmp, "drop_want")
    keep = [0, 1, 3, 5]
    D.write_csv(want, X[keep], U[keep], np.arange(4), TS, noise_ids=ids[keep])
    assert_same(out["np"][:2], (open(want + "_clean.csv", "rb").read(), open(want + "_noisy.csv", "rb").read()))


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("gen", ["generate_open_loop", "generate_piecewise"])
def test_open_loop_shard_equals_the_single_file(gen, dev, tmp):
    """shards=True without a process group: rank 0's shard is the whole dataset, so its files are the shards=False
    files byte for byte; no status sidecar either way."""
    fn = getattr(D, gen)
    one, sh = os.path.join(tmp, f"{gen}_one_{int(dev)}"), os.path.join(tmp, f"{gen}_sh_{int(dev)}")
    fn(4, 6, out_prefix=one, device_csv=dev)
    r = fn(4, 6, out_prefix=sh, shards=True, device_csv=dev)
    assert len(r) == 2 and tuple(r[0].shape) == (4, 7, 6) and tuple(r[1].shape) == (4, 6, 2)
    assert_same([open(f"{sh}_rank0_{part}.csv", "rb").read() for part in ("clean", "noisy")],
                [open(f"{one}_{part}.csv", "rb").read() for part in ("clean", "noisy")])
    assert not os.path.exists(f"{sh}_rank0_status.csv") and not os.path.exists(f"{one}_status.csv")

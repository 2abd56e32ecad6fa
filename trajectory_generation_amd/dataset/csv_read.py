"""The two CSV readers: read_csv_native (the library's parallel host parser) and read_csv_device (the text parsed on the
GPU, csrc/dataset_parse.hip, the same bits), with the per-token and per-pass entry points the tests drive."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .._lib import event_pair, ptr, stream


def read_csv_native(path, nthreads=None, pin=False):
    """All columns of a dataset CSV as {name: float64 array} through the library's parallel parser
    (traj_dataset_read_csv) into one [rows, C] buffer -- pinned host memory with pin=True."""
    import ctypes as C
    import os
    import torch
    with open(path) as f:
        names = f.readline().strip().split(",")
    nc = C.c_int(0)
    rows = int(_lib.lib().traj_dataset_csv_rows(str(path).encode(), C.byref(nc)))
    if rows < 0 or nc.value != len(names):
        raise ValueError(f"{path}: not a dataset CSV ({rows}, {nc.value} columns)")
    buf = torch.empty((rows, len(names)), dtype=torch.float64, pin_memory=pin)
    nt = int(nthreads or min(16, os.cpu_count() or 1))
    _lib.check(_lib.lib().traj_dataset_read_csv(str(path).encode(), rows, len(names), ptr(buf), nt),
               "traj_dataset_read_csv")
    return names, buf


DEVICE_CSV_READ_SLAB_BYTES = 64 << 20   # read_csv_device: pinned staging, two slabs of this size
DEVICE_CSV_FALLBACK_CAP = 4096          # read_csv_device: declined fields settled one by one; more: the host reader


def _tokens_block(tokens):
    """A list of bytes as (one uint8 array, int64 offsets, int32 lengths)."""
    ln = np.array([len(t) for t in tokens], dtype=np.int32)
    off = np.zeros(len(tokens), dtype=np.int64)
    if len(tokens):
        off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
    text = np.frombuffer(b"".join(tokens) + b"\0", dtype=np.uint8).copy()   # never empty; the last byte is no field's
    return text, off, ln


def parse_f64_host(tokens, fill=0.0):
    """csrc/parse_f64.h on the CPU (traj_dataset_parse_f64_host) on a list of bytes: (float64 array, int32 statuses);
    a declined token (status _lib.PARSE_FALLBACK) leaves `fill`."""
    text, off, ln = _tokens_block(tokens)
    out = np.full(len(tokens), fill, dtype=np.float64)
    st = np.full(len(tokens), -7, dtype=np.int32)
    _lib.check(_lib.lib().traj_dataset_parse_f64_host(ptr(text), ptr(off), ptr(ln), len(tokens), ptr(out), ptr(st)),
               "traj_dataset_parse_f64_host")
    return out, st


def parse_f64_batch(tokens, fill=0.0, device=None):
    """The same header on the GPU (traj_dataset_parse_f64_batch), one field per thread: a list of bytes ->
    (float64 CUDA tensor, int32 statuses); a declined token leaves `fill`."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    text, off, ln = _tokens_block(tokens)
    n = len(tokens)
    with torch.cuda.device(dev):
        td, od, ld = (torch.from_numpy(a).to(dev) for a in (text, off, ln))
        out = torch.full((n,), fill, dtype=torch.float64, device=dev)
        st = torch.full((n,), -7, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().traj_dataset_parse_f64_batch(ptr(td), ptr(od), ptr(ld), n, ptr(out), ptr(st), stream()),
                   "traj_dataset_parse_f64_batch")
        torch.cuda.current_stream().synchronize()
    return out, st


def csv_tokens_host(tokens):
    """The host reader's own token code (traj_dataset_csv_token_host: std::from_chars, strtod past the double range,
    the nan / inf spellings) on a list of non-empty bytes: (float64 array, True if every token is a number)."""
    text, off, ln = _tokens_block(tokens)
    out = np.zeros(len(tokens), dtype=np.float64)
    rc = _lib.lib().traj_dataset_csv_token_host(ptr(text), ptr(off), ptr(ln), len(tokens), ptr(out))
    return out, rc == _lib.TRAJ_OK


def csv_parse_index(text, nbytes, events=None):
    """The line index of a file body on the device (uint8 CUDA tensor `text`, its first nbytes bytes), on the current
    stream: (rows, starts) with starts the int64 CUDA tensor of every row's first byte.  events: a dict that receives
    (start, end) CUDA event pairs named count, scan and starts."""
    import contextlib
    import torch
    L = _lib.lib()
    dev = text.device
    st = stream()
    timed = (lambda name: event_pair(events, name)) if events is not None else (lambda name: contextlib.nullcontext())
    chunks = int(L.traj_dataset_csv_parse_chunks(int(nbytes)))
    if chunks < 0:
        raise ValueError(f"csv_parse_index: {nbytes} bytes")
    if chunks == 0:
        return 0, torch.empty(0, dtype=torch.int64, device=dev)
    counts = torch.empty(chunks, dtype=torch.int64, device=dev)
    with timed("count"):
        _lib.check(L.traj_dataset_csv_parse_count(ptr(text), int(nbytes), ptr(counts), st),
                   "traj_dataset_csv_parse_count")
    with timed("scan"):
        cum = torch.cumsum(counts, 0)
    chunk_off = cum - counts
    # a last line without its newline is a row; a trailing newline starts none
    rows = int(cum[-1]) + (0 if int(text[nbytes - 1]) == 0x0A else 1)
    starts = torch.empty(rows, dtype=torch.int64, device=dev)
    with timed("starts"):
        _lib.check(L.traj_dataset_csv_parse_starts(ptr(text), int(nbytes), ptr(chunk_off), ptr(starts), rows, st),
                   "traj_dataset_csv_parse_starts")
    return rows, starts


def csv_parse_rows(text, nbytes, starts, rows, ncols, out, err, fb_count, fb_rec):
    """traj_dataset_csv_parse_rows on the current stream: the rows at `starts` of the body `text` (its first nbytes
    bytes) into the float64 CUDA tensor out [rows, ncols]; err (int32), fb_count (int64) and fb_rec ([cap, 4] int64)
    are the device error word, the declined fields' counter and their records."""
    _lib.check(_lib.lib().traj_dataset_csv_parse_rows(ptr(text), int(nbytes), ptr(starts), int(rows), int(ncols),
                                                      ptr(out), ptr(err), ptr(fb_count), ptr(fb_rec),
                                                      int(fb_rec.shape[0]), stream()), "traj_dataset_csv_parse_rows")


def csv_gather_f32(src, rowidx, n, T_steps, cols):
    """traj_dataset_csv_gather_f32 on the current stream: src [rows, C] float64 (CUDA), rowidx [n * T_steps] int64 row
    numbers, cols a list of column numbers -> [n, len(cols), T_steps] float32, cast with round to nearest even."""
    import torch
    dev = src.device
    out = torch.empty((n, len(cols), T_steps), dtype=torch.float32, device=dev)
    cd = torch.tensor(list(cols), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().traj_dataset_csv_gather_f32(ptr(src), src.shape[0], src.shape[1], ptr(rowidx), int(n),
                                                      int(T_steps), ptr(cd), len(cols), ptr(out), ptr(err), stream()),
               "traj_dataset_csv_gather_f32")
    if int(err[0]):
        raise RuntimeError("traj_dataset_csv_gather_f32: a row or column index outside the parsed block")
    return out


def _upload_body(f, nbytes, dev, slab_bytes, tm):
    """nbytes bytes of the open file f into a new uint8 CUDA tensor through two pinned slabs: a thread reads slab k + 1
    from the file while slab k is copied up."""
    import threading
    import queue
    import time
    import torch
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)     # the tail is never read
    slab = max(1, min(int(slab_bytes), nbytes))
    hbuf = [torch.empty(slab, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    hnp = [h.numpy() for h in hbuf]
    free = [threading.Semaphore(1), threading.Semaphore(1)]
    filled = queue.Queue()
    failed = []

    def reader():
        try:
            done, k = 0, 0
            while done < nbytes:
                i = k & 1
                free[i].acquire()
                t0 = time.perf_counter()
                want = min(slab, nbytes - done)
                mv, got = memoryview(hnp[i])[:want], 0
                while got < want:
                    r = f.readinto(mv[got:])
                    if not r:
                        raise ValueError("read_csv_device: the file shrank while it was read")
                    got += r
                tm["file_read_s"] += time.perf_counter() - t0
                filled.put((i, done, want))
                done += want
                k += 1
        except BaseException as e:   # noqa: BLE001  (reported by the caller's thread)
            failed.append(e)
        filled.put(None)

    th = threading.Thread(target=reader, daemon=True)
    th.start()
    copy_stream = torch.cuda.Stream(device=dev)
    copies, prev = [], None
    while True:
        item = filled.get()
        if item is None:
            break
        i, o, nb = item
        with torch.cuda.stream(copy_stream), event_pair(copies) as (_, c1):
            text[o:o + nb].copy_(hbuf[i][:nb], non_blocking=True)
        if prev is not None:           # the copy before this one has left its slab: the reader may fill it again
            prev[1].synchronize()
            free[prev[0]].release()
        prev = (i, c1)
    th.join()
    copy_stream.synchronize()
    if failed:
        raise failed[0]
    torch.cuda.current_stream().wait_stream(copy_stream)
    tm["h2d_s"] += sum(a.elapsed_time(b) for a, b in copies) * 1e-3
    return text


def read_csv_device(path, device=None, timings=None, fallback_cap=None, slab_bytes=DEVICE_CSV_READ_SLAB_BYTES):
    """read_csv_native with the text parsed on the GPU (csrc/dataset_parse.hip): (names, [rows, C] float64 CUDA tensor),
    the tensor equal to read_csv_native's bit for bit.  Opt-in; read_csv_native stays the check of this one.

    The header line is parsed on the host; the body goes through two pinned slabs of slab_bytes to the device whole
    (read and copy overlapped), where a count pass, a 64-bit scan and a starts pass index its lines and a parse pass
    takes one row per thread (csrc/parse_f64.h: Eisel-Lemire on at most 19 significant digits).  A field the device
    declines (more digits, a '+' sign, any other spelling) is recorded; the host reader's own token code
    (traj_dataset_csv_token_host) settles up to fallback_cap (default DEVICE_CSV_FALLBACK_CAP) of them from the file's
    bytes and the values are scattered into the tensor; with more, the whole file goes through read_csv_native and is
    copied up.  So the two readers agree by construction on everything the device declines.  Raises what read_csv_native
    raises: RuntimeError for a field that is no number or a row with too few fields.
    timings: a dict that receives file_read_s, h2d_s, kernels_s, kernel_ms (count, scan, starts, parse), fallback_s,
    fallback_fields, rows, bytes and total_s."""
    import os
    import time
    import torch
    t_start = time.perf_counter()
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("read_csv_device parses on a CUDA device (read_csv_native reads into host memory)")
    cap = DEVICE_CSV_FALLBACK_CAP if fallback_cap is None else int(fallback_cap)
    tm = {"file_read_s": 0.0, "h2d_s": 0.0, "kernels_s": 0.0, "kernel_ms": {}, "fallback_s": 0.0, "fallback_fields": 0,
          "rows": 0, "bytes": 0}

    def finish(names, t):
        tm["total_s"] = time.perf_counter() - t_start
        if timings is not None:
            timings.update(tm)
        return names, t

    with open(path, "rb") as f:
        header = f.readline()
    names = header.decode().strip().split(",")
    if header.count(b",") + 1 != len(names):
        raise ValueError(f"{path}: not a dataset CSV ({header.count(b',') + 1} columns)")
    ncols = len(names)
    with torch.cuda.device(dev):
        with open(path, "rb", buffering=0) as f:
            nbytes = os.fstat(f.fileno()).st_size - len(header)
            tm["bytes"] = nbytes + len(header)
            if nbytes <= 0 or not header.endswith(b"\n"):
                return finish(names, torch.empty((0, ncols), dtype=torch.float64, device=dev))
            f.seek(len(header))
            text = _upload_body(f, nbytes, dev, slab_bytes, tm)
        ev = {}
        rows, starts = csv_parse_index(text, nbytes, ev)
        out = torch.empty((rows, ncols), dtype=torch.float64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        fb_count = torch.zeros(1, dtype=torch.int64, device=dev)
        fb_rec = torch.zeros((max(cap, 1), 4), dtype=torch.int64, device=dev)
        with event_pair(ev, "parse"):
            csv_parse_rows(text, nbytes, starts, rows, ncols, out, err, fb_count, fb_rec[:cap])
        n_fb, flag = int(fb_count[0]), int(err[0])      # waits for the stream
        tm["kernel_ms"] = {k: a.elapsed_time(b) for k, (a, b) in ev.items()}
        tm["kernels_s"] = sum(tm["kernel_ms"].values()) * 1e-3
        tm["fallback_fields"], tm["rows"] = n_fb, rows
        if flag & 2:
            raise RuntimeError("traj_dataset_csv_parse_rows: the line index does not describe the text")
        if flag & 1:
            _lib.check(_lib.TRAJ_E_ARG, "read_csv_device (a row with too few fields)")
        if n_fb > cap:
            del text, out, starts
            t0 = time.perf_counter()
            names, buf = read_csv_native(path, pin=True)
            out = buf.to(dev)
            tm["fallback_s"] = time.perf_counter() - t0
            return finish(names, out)
        if n_fb:
            t0 = time.perf_counter()
            rec = fb_rec[:n_fb].cpu().numpy()
            tokens = []
            with open(path, "rb") as f:
                for _, _, off, ln in rec:
                    f.seek(len(header) + int(off))
                    tokens.append(f.read(int(ln)))
            vals, ok = csv_tokens_host(tokens)
            if not ok:
                _lib.check(_lib.TRAJ_E_ARG, "read_csv_device (a field that is no number)")
            flat = torch.from_numpy(rec[:, 0] * ncols + rec[:, 1]).to(dev)
            out.view(-1)[flat] = torch.from_numpy(vals).to(dev)
            tm["fallback_s"] = time.perf_counter() - t0
    return finish(names, out)

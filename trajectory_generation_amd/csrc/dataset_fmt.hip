// dataset_fmt.hip -- the dataset CSVs' text formatted on the GPU (dataset.write_csv_device): the bytes of
// dataset_csv.cpp's traj_dataset_write_csv body, made from X / U / noise / ids that are already on the device.
//
// One row of the file per thread, rows being (trajectory, step) pairs in file order.  Two passes around a 64-bit
// exclusive scan of the row lengths (the caller's: torch.cumsum):
//   csv_len_kernel     decomposes every field (fmt_f64.h: Schubfach digits in a 64-bit integer) and stores the row's
//                      length;
//   csv_format_kernel  decomposes again and writes the characters.  A workgroup's 128 rows are contiguous in the file,
//                      so they are staged in LDS (at most 128 x 256 B) at their offsets relative to the workgroup's
//                      first byte, shifted by that byte's address mod 16, and copied out as aligned 16-byte stores
//                      (measured against every thread storing its row straight to global memory, 1.0 GB of text:
//                      1.49 ms against 4.34 ms; the direct form was not kept).
// The format kernel trusts neither offsets nor lengths: a workgroup whose byte range does not lie inside the buffer
// it was given (or is larger than its LDS), a row that does not lie inside its workgroup's range, and a field that
// would pass its row's end are not written -- they set the error flag that traj_dataset_csv_device_check returns as
// TRAJ_E_LAUNCH.  No store ever leaves [out, out + out_bytes).
//
// Built with the library's plain FLAGS (x + w of the noisy file is one IEEE add, as on the host).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/trajmpc.h"
#include "fmt_f64.h"

namespace tgmpc {

// the table twice: the host's copy (traj_dataset_format_f64_host) and the device's
#define FMT_POW10_DECL static const
#define FMT_POW10_NAME fmt_pow10_host
#include "fmt_pow10_tables.h"
#undef FMT_POW10_DECL
#undef FMT_POW10_NAME
#define FMT_POW10_DECL static __device__ const
#define FMT_POW10_NAME fmt_pow10_dev
#include "fmt_pow10_tables.h"
#undef FMT_POW10_DECL
#undef FMT_POW10_NAME
static_assert(sizeof(fmt_pow10_host) == (FMT_POW10_HI - FMT_POW10_LO + 1) * 16, "fmt_pow10_tables.h: range");

constexpr int CSV_LEN_THREADS = 256;
constexpr int CSV_FMT_ROWS = 128;            // rows (threads) per workgroup of the format kernel
constexpr int CSV_ROW_MAX = 256;             // 9 doubles x 24 + int64 x 20 + 10 separators = 246
constexpr int CSV_STAGE = CSV_FMT_ROWS * CSV_ROW_MAX;

struct CsvSrc {
    int which;              // 0 clean, 1 noisy
    int T;
    long long R;            // T + 1 rows per trajectory
    double Ts;
    const double* X;        // [B,R,6]
    const double* U;        // [B,T,2]
    const double* noise;    // [B,R,6] (noisy)
    const long long* ids;   // [B]
};

// Row `row` of the file: its length; with EMIT also its characters at p, where `room` bytes are the row's (-1 and
// nothing further written if a field would pass them).  Values are read where they are used: no private array.
template <bool EMIT>
__device__ __forceinline__ int csv_row(const CsvSrc& s, long long row, char* p, int room) {
    const long long b = row / s.R;
    const int r = (int)(row - b * s.R);
    const double* x = s.X + row * 6;
    const double* w = s.which == 1 ? s.noise + row * 6 : nullptr;
    int n = 0;
    for (int f = 0; f < 9; ++f) {
        if (s.which == 1 && f == 3) continue;             // phi is not measured
        double v;
        if (f == 0) {
            v = (double)r * s.Ts;
        } else if (f <= 6) {
            v = x[f - 1];
            if (s.which == 1) v = v + w[f - 1];
        } else {
            v = r < s.T ? s.U[(b * s.T + r) * 2 + (f - 7)] : __builtin_nan("");
        }
        const tgfmt::FmtDec d = tgfmt::fmt_decompose(v, fmt_pow10_dev);
        const int fl = tgfmt::fmt_len(d);
        if (EMIT) {
            if (n + fl + 1 > room) return -1;
            tgfmt::fmt_emit(d, p + n);
            p[n + fl] = ',';
        }
        n += fl + 1;
    }
    const long long id = s.ids[b];
    const int il = tgfmt::fmt_i64_len(id);
    if (EMIT) {
        if (n + il + 1 > room) return -1;
        tgfmt::fmt_i64_emit(id, il, p + n);
        p[n + il] = '\n';
    }
    return n + il + 1;
}

__global__ void __launch_bounds__(CSV_LEN_THREADS)
csv_len_kernel(CsvSrc s, long long row0, long long nrows, int* __restrict__ len, unsigned long long* total) {
    const long long i = (long long)blockIdx.x * CSV_LEN_THREADS + threadIdx.x;
    int n = 0;
    if (i < nrows) {
        n = csv_row<false>(s, row0 + i, nullptr, 0);
        len[i] = n;
    }
    if (total) {
        for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(total, (unsigned long long)n);
    }
}

__global__ void __launch_bounds__(CSV_FMT_ROWS)
csv_format_kernel(CsvSrc s, long long row0, long long nrows, const long long* __restrict__ off,
                  const int* __restrict__ len, long long base, char* out, long long out_bytes, int* err) {
    __shared__ __attribute__((aligned(16))) char stage[CSV_STAGE + 16];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * CSV_FMT_ROWS;
    const long long il = (i0 + CSV_FMT_ROWS < nrows ? i0 + CSV_FMT_ROWS : nrows) - 1;
    // the workgroup's byte range [b0, b0 + span) of out, from the first row's offset and the last row's end: the
    // same loads in every thread, so the decision is uniform.  Differences in unsigned arithmetic (any input wraps).
    const unsigned long long o0 = (unsigned long long)off[i0];
    const long long b0 = (long long)(o0 - (unsigned long long)base);
    const int last_len = len[il];
    const long long span = (long long)((unsigned long long)off[il] - o0) + last_len;
    if (last_len < 0 || last_len > CSV_ROW_MAX || span < 0 || span > CSV_STAGE || b0 < 0 || b0 > out_bytes ||
        span > out_bytes - b0) {
        if (tid == 0) atomicOr(err, 1);
        return;
    }
    char* const gdst = out + b0;
    const int sh = (int)((uintptr_t)gdst & 15);
    const long long i = i0 + tid;
    if (i < nrows) {
        const long long loc = (long long)((unsigned long long)off[i] - o0);
        const int L = len[i];
        int n = -1;
        if (L >= 0 && L <= CSV_ROW_MAX && loc >= 0 && loc <= span - L)
            n = csv_row<true>(s, row0 + i, stage + sh + loc, L);
        if (n != L) atomicOr(err, 1);
    }
    __syncthreads();
    // out: bytes up to the first 16-byte boundary, aligned 16-byte stores, the rest
    const int sp = (int)span;
    const int head = sp < ((16 - sh) & 15) ? sp : ((16 - sh) & 15);
    for (int j = tid; j < head; j += CSV_FMT_ROWS) gdst[j] = stage[sh + j];
    const int nvec = (sp - head) >> 4;
    const uint4* ls = reinterpret_cast<const uint4*>(stage + sh + head);
    uint4* gd = reinterpret_cast<uint4*>(gdst + head);
    for (int j = tid; j < nvec; j += CSV_FMT_ROWS) gd[j] = ls[j];
    for (int j = head + nvec * 16 + tid; j < sp; j += CSV_FMT_ROWS) gdst[j] = stage[sh + j];
}

__global__ void __launch_bounds__(256)
format_f64_kernel(const double* __restrict__ v, long long n, char* out, int* __restrict__ len) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const tgfmt::FmtDec d = tgfmt::fmt_decompose(v[i], fmt_pow10_dev);
    const int fl = tgfmt::fmt_len(d);
    if (fl <= FMT_F64_MAX) tgfmt::fmt_emit(d, out + i * FMT_F64_MAX);
    len[i] = fl <= FMT_F64_MAX ? fl : -1;
}

static int csv_args(int which, int B, int T, const double* X, const double* U, const double* noise,
                    const long long* ids, long long row0, long long nrows) {
    if (which < 0 || which > 1 || B < 0 || T < 0 || row0 < 0 || nrows < 0 || nrows > INT_MAX) return TRAJ_E_ARG;
    if (row0 + nrows > (long long)B * ((long long)T + 1)) return TRAJ_E_ARG;
    if (nrows > 0 && (!X || (T > 0 && !U) || !ids || (which == 1 && !noise))) return TRAJ_E_ARG;
    return TRAJ_OK;
}

}  // namespace tgmpc

extern "C" {

int traj_dataset_format_f64_host(const double* v, long long n, char* out, int* len) {
    if (n < 0 || (n > 0 && (!v || !out || !len))) return TRAJ_E_ARG;
    for (long long i = 0; i < n; ++i) len[i] = tgfmt::fmt_f64(v[i], tgmpc::fmt_pow10_host, out + i * FMT_F64_MAX);
    return TRAJ_OK;
}

int traj_dataset_format_f64_batch(const double* v, long long n, char* out, int* len, void* stream) {
    using namespace tgmpc;
    if (n < 0 || n > (long long)INT_MAX * 256 || (n > 0 && (!v || !out || !len))) return TRAJ_E_ARG;
    if (n == 0) return TRAJ_OK;
    hipLaunchKernelGGL(format_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, n,
                       out, len);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_device_rows(int which, int B, int T, double Ts, const double* X, const double* U,
                                 const double* noise, const long long* ids, long long row0, long long nrows, int* len,
                                 unsigned long long* total, void* stream) {
    using namespace tgmpc;
    const int rc = csv_args(which, B, T, X, U, noise, ids, row0, nrows);
    if (rc != TRAJ_OK || (nrows > 0 && !len)) return TRAJ_E_ARG;
    if (nrows == 0) return TRAJ_OK;
    const CsvSrc s{which, T, (long long)T + 1, Ts, X, U, noise, ids};
    const unsigned grid = (unsigned)((nrows + CSV_LEN_THREADS - 1) / CSV_LEN_THREADS);
    hipLaunchKernelGGL(csv_len_kernel, dim3(grid), dim3(CSV_LEN_THREADS), 0, (hipStream_t)stream, s, row0, nrows, len,
                       total);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_device_format(int which, int B, int T, double Ts, const double* X, const double* U,
                                   const double* noise, const long long* ids, long long row0, long long nrows,
                                   const long long* off, const int* len, long long base, char* out,
                                   long long out_bytes, int* err, void* stream) {
    using namespace tgmpc;
    const int rc = csv_args(which, B, T, X, U, noise, ids, row0, nrows);
    if (rc != TRAJ_OK || out_bytes < 0 || !err || (nrows > 0 && (!off || !len || !out))) return TRAJ_E_ARG;
    if (nrows == 0) return TRAJ_OK;
    const CsvSrc s{which, T, (long long)T + 1, Ts, X, U, noise, ids};
    const unsigned grid = (unsigned)((nrows + CSV_FMT_ROWS - 1) / CSV_FMT_ROWS);
    hipLaunchKernelGGL(csv_format_kernel, dim3(grid), dim3(CSV_FMT_ROWS), 0, (hipStream_t)stream, s, row0, nrows, off,
                       len, base, out, out_bytes, err);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_device_check(const int* err, void* stream) {
    if (!err) return TRAJ_E_ARG;
    int flag = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return TRAJ_E_LAUNCH;
    if (hipMemcpy(&flag, err, sizeof(flag), hipMemcpyDeviceToHost) != hipSuccess) return TRAJ_E_LAUNCH;
    return flag ? TRAJ_E_LAUNCH : TRAJ_OK;
}

}  // extern "C"

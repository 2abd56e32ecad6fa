// dataset_parse.hip -- the dataset CSVs' text parsed on the GPU (dataset.read_csv_device): the [rows, C] float64 block
// of dataset_csv.cpp's traj_dataset_read_csv, made from the file body's bytes that are already on the device.  The
// inverse of dataset_fmt.hip.
//
// Line index, around a 64-bit exclusive scan of per-chunk counts (the caller's: torch.cumsum):
//   csv_count_kernel   the '\n's of each chunk of TRAJ_CSV_PARSE_CHUNK bytes, 16 bytes per thread;
//   csv_starts_kernel  finds them again and stores the byte offset after each as the start of its row (row 0 starts
//                      at byte 0; a '\n' on the last byte starts no row).
// Parse:
//   csv_parse_kernel   one row per thread.  A workgroup's 128 rows are contiguous in the text, so their byte span
//                      starts[r0] .. starts[r0 + 128] is staged in LDS with aligned 16-byte loads and every thread walks
//                      its row there (parse_f64.h: Eisel-Lemire, digits in a 64-bit integer); a span larger than the
//                      LDS buffer is walked in global memory by the same code.  A field parse_f64.h declines is
//                      recorded (row, column, byte offset, length) for the host's std::from_chars and counted.
// Gather:
//   csv_gather_kernel  the loader's row gather, column pick, float32 cast and [n, C, T] transpose in one pass; the cast
//                      is done on the bits (round to nearest even, subnormals kept) so no float mode decides it.
// The kernels trust neither starts nor the row index: no byte at or past nbytes is read, a workgroup whose span does
// not lie inside the text or a row that does not start inside its workgroup's span is skipped and flagged, and a row
// index outside [0, rows) is skipped and flagged.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/trajmpc.h"
#include "parse_f64.h"

namespace tgmpc {

// the table twice: the host's copy (traj_dataset_parse_f64_host) and the device's
#define PARSE_POW5_DECL static const
#define PARSE_POW5_NAME parse_pow5_host
#include "parse_pow5_tables.h"
#undef PARSE_POW5_DECL
#undef PARSE_POW5_NAME
#define PARSE_POW5_DECL static __device__ const
#define PARSE_POW5_NAME parse_pow5_dev
#include "parse_pow5_tables.h"
#undef PARSE_POW5_DECL
#undef PARSE_POW5_NAME
static_assert(sizeof(parse_pow5_host) == (PARSE_POW5_HI - PARSE_POW5_LO + 1) * 16, "parse_pow5_tables.h: range");

constexpr int CSV_CHUNK_THREADS = TRAJ_CSV_PARSE_CHUNK / 16;   // 16 bytes per thread
constexpr int CSV_PARSE_ROWS = 128;                            // rows (threads) per workgroup of the parse kernel
constexpr int CSV_PARSE_STAGE = CSV_PARSE_ROWS * 256;          // LDS bytes: the writer's rows are at most 246 long
constexpr int CSV_ERR_SHORT_ROW = 1;                           // a row with too few fields (the host's *e != ',')
constexpr int CSV_ERR_INDEX = 2;                               // starts / row index outside what was given
static_assert(TRAJ_CSV_PARSE_CHUNK % 1024 == 0 && CSV_CHUNK_THREADS <= 1024, "whole waves, one workgroup per chunk");

// 0x80 in every byte of w that is '\n' (exact: no borrow crosses a byte)
__device__ __forceinline__ uint32_t csv_nl_mask(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// bytes pos .. pos + 3 as a little-endian word, zero at and past nbytes
__device__ __forceinline__ uint32_t csv_word(const unsigned char* text, long long nbytes, long long pos) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (pos + k < nbytes) w |= (uint32_t)text[pos + k] << (8 * k);
    return w;
}

// this thread's 16 bytes of its chunk as '\n' masks: one aligned 16-byte load, or guarded bytes at the text's end /
// for a text that is not 16-byte aligned (uniform per launch)
__device__ __forceinline__ uint4 csv_thread_masks(const unsigned char* text, long long nbytes, long long pos) {
    uint4 v;
    if (pos + 16 <= nbytes && ((uintptr_t)(text + pos) & 15) == 0) {
        v = *reinterpret_cast<const uint4*>(text + pos);
    } else {
        v.x = csv_word(text, nbytes, pos);
        v.y = csv_word(text, nbytes, pos + 4);
        v.z = csv_word(text, nbytes, pos + 8);
        v.w = csv_word(text, nbytes, pos + 12);
    }
    return make_uint4(csv_nl_mask(v.x), csv_nl_mask(v.y), csv_nl_mask(v.z), csv_nl_mask(v.w));
}

__global__ void __launch_bounds__(CSV_CHUNK_THREADS)
csv_count_kernel(const unsigned char* __restrict__ text, long long nbytes, long long* __restrict__ counts) {
    __shared__ int wave_sum[CSV_CHUNK_THREADS / 64];
    const int tid = threadIdx.x;
    const long long pos = (long long)blockIdx.x * TRAJ_CSV_PARSE_CHUNK + tid * 16;
    const uint4 m = csv_thread_masks(text, nbytes, pos);
    int n = __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < CSV_CHUNK_THREADS / 64; ++k) t += wave_sum[k];
        counts[blockIdx.x] = t;
    }
}

// the rows that start after the '\n's of one word: first_row is the row index of the first of them
__device__ __forceinline__ int csv_put_starts(uint32_t m, long long pos, long long nbytes, long long first_row,
                                              long long rows, long long* __restrict__ starts) {
    int k = 0;
    while (m) {
        const long long st = pos + ((__ffs((int)m) - 1) >> 3) + 1;
        if (st < nbytes && first_row + k > 0 && first_row + k < rows) starts[first_row + k] = st;
        m &= m - 1;
        ++k;
    }
    return k;
}

__global__ void __launch_bounds__(CSV_CHUNK_THREADS)
csv_starts_kernel(const unsigned char* __restrict__ text, long long nbytes, const long long* __restrict__ chunk_off,
                  long long* __restrict__ starts, long long rows) {
    __shared__ int wave_sum[CSV_CHUNK_THREADS / 64];
    const int tid = threadIdx.x;
    const long long pos = (long long)blockIdx.x * TRAJ_CSV_PARSE_CHUNK + tid * 16;
    const uint4 m = csv_thread_masks(text, nbytes, pos);
    const int n = __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    int incl = n;                                     // inclusive scan over the wave
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
    __syncthreads();
    int before = incl - n;
#pragma unroll
    for (int k = 0; k < CSV_CHUNK_THREADS / 64; ++k)
        if (k < (tid >> 6)) before += wave_sum[k];
    if (blockIdx.x == 0 && tid == 0 && rows > 0 && nbytes > 0) starts[0] = 0;
    // newline number j of the text (from 0) ends row j: row j + 1 starts behind it
    long long row = chunk_off[blockIdx.x] + before + 1;
    row += csv_put_starts(m.x, pos, nbytes, row, rows, starts);
    row += csv_put_starts(m.y, pos + 4, nbytes, row, rows, starts);
    row += csv_put_starts(m.z, pos + 8, nbytes, row, rows, starts);
    csv_put_starts(m.w, pos + 12, nbytes, row, rows, starts);
}

struct CsvParseOut {
    double* out;                    // [rows, ncols]
    int* err;
    unsigned long long* fb_count;   // fields declined
    long long* fb_rec;              // [cap, 4]: row, column, byte offset, length
    long long cap;
};

// One row: its text starts at s (byte `off` of the body), no byte at or past lim is read (the text's end is a line end,
// as the host's sentinel).  s and lim point into LDS or into global memory.
__device__ __forceinline__ void csv_parse_row(const char* s, const char* lim, long long off, long long row, int ncols,
                                              const CsvParseOut& o) {
    const char* const row_s = s;
    double* dst = o.out + row * ncols;
    for (int c = 0; c < ncols; ++c) {
        const char* e = s;
        while (e < lim && *e != ',' && *e != '\n' && *e != '\r') ++e;
        double v;
        if (tgparse::parse_field(s, e, parse_pow5_dev, &v) != PARSE_OK) {
            v = __builtin_nan("");
            const unsigned long long k = atomicAdd(o.fb_count, 1ull);
            if (k < (unsigned long long)o.cap) {
                long long* rec = o.fb_rec + 4 * k;
                rec[0] = row;
                rec[1] = c;
                rec[2] = off + (s - row_s);
                rec[3] = e - s;
            }
        }
        dst[c] = v;
        if (c + 1 < ncols) {
            if (e >= lim || *e != ',') {
                atomicOr(o.err, CSV_ERR_SHORT_ROW);
                break;
            }
            s = e + 1;
        }
    }
}

__global__ void __launch_bounds__(CSV_PARSE_ROWS)
csv_parse_kernel(const char* __restrict__ text, long long nbytes, const long long* __restrict__ starts, long long rows,
                 int ncols, CsvParseOut o) {
    __shared__ __attribute__((aligned(16))) char stage[CSV_PARSE_STAGE + 16];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * CSV_PARSE_ROWS;
    // the workgroup's byte span [b0, b1): the same loads in every thread, so the decisions are uniform
    const long long b0 = starts[r0];
    const long long b1 = r0 + CSV_PARSE_ROWS < rows ? starts[r0 + CSV_PARSE_ROWS] : nbytes;
    if (b0 < 0 || b1 < b0 || b1 > nbytes) {
        if (tid == 0) atomicOr(o.err, CSV_ERR_INDEX);
        return;
    }
    const long long span = b1 - b0;
    const long long r = r0 + tid;
    const long long st = r < rows ? starts[r] : b0;
    const bool mine = r < rows && st >= b0 && st <= b1;
    if (r < rows && !mine) atomicOr(o.err, CSV_ERR_INDEX);
    if (span > CSV_PARSE_STAGE) {                     // a long row among these: walk global memory
        if (mine) csv_parse_row(text + st, text + b1, st, r, ncols, o);
        return;
    }
    // in: bytes up to the first 16-byte boundary, aligned 16-byte loads, the rest; at the text's address mod 16
    const char* const gsrc = text + b0;
    const int sh = (int)((uintptr_t)gsrc & 15);
    const int sp = (int)span;
    const int head = sp < ((16 - sh) & 15) ? sp : ((16 - sh) & 15);
    for (int j = tid; j < head; j += CSV_PARSE_ROWS) stage[sh + j] = gsrc[j];
    const int nvec = (sp - head) >> 4;
    const uint4* gs = reinterpret_cast<const uint4*>(gsrc + head);
    uint4* ls = reinterpret_cast<uint4*>(stage + sh + head);
    for (int j = tid; j < nvec; j += CSV_PARSE_ROWS) ls[j] = gs[j];
    for (int j = head + nvec * 16 + tid; j < sp; j += CSV_PARSE_ROWS) stage[sh + j] = gsrc[j];
    __syncthreads();
    if (mine) csv_parse_row(stage + sh + (int)(st - b0), stage + sh + sp, st, r, ncols, o);
}

__global__ void __launch_bounds__(256)
parse_f64_kernel(const char* __restrict__ text, const long long* __restrict__ off, const int* __restrict__ len,
                 long long n, double* __restrict__ out, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int st = PARSE_FALLBACK;
    if (off[i] >= 0 && len[i] >= 0) {
        const char* s = text + off[i];
        double v;
        st = tgparse::parse_field(s, s + len[i], parse_pow5_dev, &v);
        if (st == PARSE_OK) out[i] = v;
    }
    status[i] = st;
}

// float64 bits to the nearest float32's, ties to even, float32 subnormals kept (numpy's astype(np.float32))
__host__ __device__ __forceinline__ uint32_t csv_f64_to_f32_bits(uint64_t b) {
    const uint32_t sign = (uint32_t)(b >> 63) << 31;
    const int bexp = (int)((b >> 52) & 0x7FF);
    const uint64_t frac = b & ((1ull << 52) - 1);
    if (bexp == 0x7FF) return sign | 0x7F800000u | (frac ? 0x00400000u | (uint32_t)(frac >> 29) : 0u);
    const int e = bexp - 1023 + 127;                  // the float32's biased exponent, if it is normal
    if (e >= 255) return sign | 0x7F800000u;
    uint64_t m, rest, half;
    uint32_t hi;
    if (e > 0) {
        m = frac >> 29;
        rest = frac & ((1ull << 29) - 1);
        half = 1ull << 28;
        hi = (uint32_t)e << 23;
    } else {
        // subnormal: k = value / 2^-149 = (2^52 + frac) >> (30 - e); float64 subnormals (bexp = 0) are far below half a step
        const int shift = 30 - e;
        if (bexp == 0 || shift > 63) return sign;
        const uint64_t full = (1ull << 52) | frac;
        m = full >> shift;
        rest = full & ((1ull << shift) - 1);
        half = 1ull << (shift - 1);
        hi = 0;
    }
    uint32_t r = hi | (uint32_t)m;
    if (rest > half || (rest == half && (r & 1))) ++r;   // a carry runs into the exponent, up to inf: as it should
    return sign | r;
}

__global__ void __launch_bounds__(256)
csv_gather_kernel(const double* __restrict__ src, long long rows, int C, const long long* __restrict__ rowidx,
                  long long n, int T, const int* __restrict__ cols, int ncols, float* __restrict__ out, int* err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // (trajectory, step)
    if (i >= n * T) return;
    const long long r = rowidx[i];
    if (r < 0 || r >= rows) {
        atomicOr(err, CSV_ERR_INDEX);
        return;
    }
    const long long b = i / T;
    const int t = (int)(i - b * T);
    const unsigned long long* row = reinterpret_cast<const unsigned long long*>(src) + r * C;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (b * ncols) * T + t;
    for (int k = 0; k < ncols; ++k) {
        const int c = cols[k];
        if (c < 0 || c >= C) {
            atomicOr(err, CSV_ERR_INDEX);
            continue;
        }
        dst[(long long)k * T] = csv_f64_to_f32_bits(row[c]);
    }
}

}  // namespace tgmpc

extern "C" {

int traj_dataset_parse_f64_host(const char* text, const long long* off, const int* len, long long n, double* out,
                                int* status) {
    if (n < 0 || (n > 0 && (!text || !off || !len || !out || !status))) return TRAJ_E_ARG;
    for (long long i = 0; i < n; ++i) {
        status[i] = PARSE_FALLBACK;
        if (off[i] < 0 || len[i] < 0) continue;
        const char* s = text + off[i];
        status[i] = tgparse::parse_field(s, s + len[i], tgmpc::parse_pow5_host, &out[i]);
    }
    return TRAJ_OK;
}

int traj_dataset_parse_f64_batch(const char* text, const long long* off, const int* len, long long n, double* out,
                                 int* status, void* stream) {
    using namespace tgmpc;
    if (n < 0 || n > (long long)INT_MAX * 256 || (n > 0 && (!text || !off || !len || !out || !status)))
        return TRAJ_E_ARG;
    if (n == 0) return TRAJ_OK;
    hipLaunchKernelGGL(parse_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, text,
                       off, len, n, out, status);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

long long traj_dataset_csv_parse_chunks(long long nbytes) {
    if (nbytes < 0 || nbytes > (long long)INT_MAX * TRAJ_CSV_PARSE_CHUNK) return TRAJ_E_ARG;
    return (nbytes + TRAJ_CSV_PARSE_CHUNK - 1) / TRAJ_CSV_PARSE_CHUNK;
}

int traj_dataset_csv_parse_count(const char* text, long long nbytes, long long* counts, void* stream) {
    using namespace tgmpc;
    const long long chunks = traj_dataset_csv_parse_chunks(nbytes);
    if (chunks < 0 || (chunks > 0 && (!text || !counts))) return TRAJ_E_ARG;
    if (chunks == 0) return TRAJ_OK;
    hipLaunchKernelGGL(csv_count_kernel, dim3((unsigned)chunks), dim3(CSV_CHUNK_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(text), nbytes, counts);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_parse_starts(const char* text, long long nbytes, const long long* chunk_off, long long* starts,
                                  long long rows, void* stream) {
    using namespace tgmpc;
    const long long chunks = traj_dataset_csv_parse_chunks(nbytes);
    if (chunks < 0 || rows < 0 || (chunks > 0 && (!text || !chunk_off)) || (rows > 0 && (!starts || chunks == 0)))
        return TRAJ_E_ARG;
    if (chunks == 0 || rows == 0) return TRAJ_OK;
    hipLaunchKernelGGL(csv_starts_kernel, dim3((unsigned)chunks), dim3(CSV_CHUNK_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(text), nbytes, chunk_off, starts, rows);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_parse_rows(const char* text, long long nbytes, const long long* starts, long long rows, int ncols,
                                double* out, int* err, unsigned long long* fb_count, long long* fb_rec, long long cap,
                                void* stream) {
    using namespace tgmpc;
    if (nbytes < 0 || rows < 0 || rows > (long long)INT_MAX * CSV_PARSE_ROWS || ncols < 1 || cap < 0 || !err ||
        !fb_count || (cap > 0 && !fb_rec) || (rows > 0 && (!text || !starts || !out || nbytes == 0)))
        return TRAJ_E_ARG;
    if (rows == 0) return TRAJ_OK;
    const CsvParseOut o{out, err, fb_count, fb_rec, cap};
    const unsigned grid = (unsigned)((rows + CSV_PARSE_ROWS - 1) / CSV_PARSE_ROWS);
    hipLaunchKernelGGL(csv_parse_kernel, dim3(grid), dim3(CSV_PARSE_ROWS), 0, (hipStream_t)stream, text, nbytes, starts,
                       rows, ncols, o);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

int traj_dataset_csv_gather_f32(const double* src, long long rows, int src_cols, const long long* rowidx, long long n,
                                int T_steps, const int* cols, int ncols, float* out, int* err, void* stream) {
    using namespace tgmpc;
    if (rows < 0 || src_cols < 1 || n < 0 || T_steps < 0 || ncols < 0 || !err) return TRAJ_E_ARG;
    if (n > 0 && T_steps > 0 && n > (long long)INT_MAX * 256 / T_steps) return TRAJ_E_ARG;
    const long long items = n * T_steps;
    if (items > 0 && ncols > 0 && (!src || !rowidx || !cols || !out)) return TRAJ_E_ARG;
    if (items == 0 || ncols == 0) return TRAJ_OK;
    hipLaunchKernelGGL(csv_gather_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                       rows, src_cols, rowidx, n, T_steps, cols, ncols, out, err);
    return hipGetLastError() == hipSuccess ? TRAJ_OK : TRAJ_E_LAUNCH;
}

}  // extern "C"

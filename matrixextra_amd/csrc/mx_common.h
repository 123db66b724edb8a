// mx_common.h — shared host/device helpers of libmxgpu (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <climits>
#include "../../include/mxgpu.h"

#define MX_WAVE 64
#define MX_NA_INT INT_MIN                       // R NA_INTEGER / NA_LOGICAL
#define MX_NA_REAL_BITS 0x7FF00000000007A2ULL   // R NA_real_ (NaN, low word 1954)

namespace mx {

// thread-local error text behind mx_last_error()
int set_error(const char *fmt, ...);
inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

#define MX_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return mx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                 __FILE__, __LINE__);                                  \
    } while (0)

#define MX_LAUNCH_CHECK()                                                              \
    do {                                                                               \
        hipError_t _e = hipGetLastError();                                             \
        if (_e != hipSuccess)                                                          \
            return mx::set_error("kernel launch failed: %s (%s:%d)",                   \
                                 hipGetErrorString(_e), __FILE__, __LINE__);           \
    } while (0)

#define MX_REQUIRE(cond, ...)                                                          \
    do { if (!(cond)) return mx::set_error(__VA_ARGS__); } while (0)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// blocks of `block` threads for n items (at least one), at most cap
inline unsigned grid_for(int64_t n, int block, int64_t cap = UINT_MAX)
{
    const int64_t g = ceil_div(n > 0 ? n : 1, block);
    return (unsigned)(g < cap ? g : cap);
}

// scan.hip: exclusive scan of counts[0..n) into out[0..n]; the int64 total goes to *total_dev (the workspace's
// first word when null)
size_t scan_workspace_bytes(int64_t n);
int exclusive_scan_i32(const int32_t *counts, int64_t n, int32_t *out, int64_t *total_dev, void *workspace,
                       hipStream_t st);
// (hidden: internal to libmxgpu, kept out of its dynamic symbol table)
#pragma GCC visibility push(hidden)
// bytes of an int32 array of max(n, 1) entries, padded to 16 B
size_t padded_i32_bytes(int64_t n);
// count -> scan -> read-back: workspace is [int32 counts[n], padded_i32_bytes(n)][scan workspace]; counts are
// scanned into indptr[0..n], and the total is read back into *nnz_out_host (when non-null) and checked against R's
// int32 index range
size_t count_workspace_bytes(int64_t n);
int finish_count(int64_t n, void *workspace, int32_t *indptr, int64_t *nnz_out_host, hipStream_t st);
#pragma GCC visibility pop

// xfer.hip: synchronous host <-> device copies, pipelined through pinned slots + a host copy pool when large
int xfer_h2d(void *dst_dev, const void *src_host, size_t bytes);
int xfer_d2h(void *dst_host, const void *src_dev, size_t bytes);
// many host arrays into one device buffer, part k at dst_dev + at (ascending, disjoint, below total)
struct XferPart { const void *host; size_t bytes, at; };
int xfer_h2d_parts(void *dst_dev, size_t total, const XferPart *parts, size_t nparts);

// spmv.hip; v_dtype is an mx_dtype, or SPMV_F32_PATTERN: a float32 vector and a matrix without values (values unread)
constexpr int SPMV_F32_PATTERN = 100;
int spmv_launch(int m, int64_t nnz, const int32_t *indptr, const int32_t *indices, const double *values,
                const void *v, int v_dtype, void *y, hipStream_t st);

// lanes-per-row for the sub-wave ("group") kernels: smallest power of two
// >= avg row length, clamped to [lo, 64]
inline int pick_group(double avg_len, int lo = 4)
{
    int g = lo;
    while (g < 64 && (double)g < avg_len) g <<= 1;
    return g;
}

#ifdef __HIPCC__
__device__ __forceinline__ int lane_id() { return threadIdx.x & (MX_WAVE - 1); }

// wave-uniform broadcast of a value known to be uniform (moves it to an SGPR)
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ballot restricted to this lane's G-wide group
template <int G>
__device__ __forceinline__ unsigned long long group_ballot(bool pred)
{
    const unsigned long long b = __ballot(pred);
    if constexpr (G == 64) return b;
    else return (b >> (lane_id() & ~(G - 1))) & ((1ULL << G) - 1ULL);
}

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane);
    return u.d;
}

__device__ __forceinline__ double na_real()
{
    return __longlong_as_double((long long)MX_NA_REAL_BITS);
}

// R's three-valued logic, src/operators.cpp:17-25
__device__ __forceinline__ int r_logical_or(int x, int y)
{
    if (x == MX_NA_INT) return (y == MX_NA_INT) ? MX_NA_INT : (y ? 1 : MX_NA_INT);
    if (y == MX_NA_INT) return x ? 1 : MX_NA_INT;
    return (x != 0) || (y != 0);
}
__device__ __forceinline__ int r_logical_and(int x, int y)
{
    if (x == MX_NA_INT) return (y == MX_NA_INT) ? MX_NA_INT : (y ? MX_NA_INT : 0);
    if (y == MX_NA_INT) return x ? MX_NA_INT : 0;
    return (x != 0) && (y != 0);
}
__device__ __forceinline__ int r_logical_xor(int x, int y)
{
    if (x == MX_NA_INT || y == MX_NA_INT) return MX_NA_INT;
    return (x != 0) != (y != 0);
}

// a row's [indptr[r], indptr[r + 1]) clamped into [0, nnz], whatever the two words hold (they are taken as loaded,
// int32, so that the compiler knows their range as it did when the clamp was written out in each kernel)
struct RowBounds { int64_t start, len; };
__device__ __forceinline__ RowBounds row_bounds(int32_t first, int32_t next, int64_t nnz)
{
    int64_t s = first, e = next;
    s = s < 0 ? 0 : s > nnz ? nnz : s;
    e = e < s ? s : e > nnz ? nnz : e;
    return {s, e - s};
}

// first position in [first, first+count) whose value is >= key
__device__ __forceinline__ int lower_bound_dev(const int32_t *__restrict__ first, int count, int key)
{
    int lo = 0;
    while (count > 0) {
        const int step = count >> 1;
        if (first[lo + step] < key) { lo += step + 1; count -= step + 1; }
        else count = step;
    }
    return lo;
}
#endif  // __HIPCC__

}  // namespace mx

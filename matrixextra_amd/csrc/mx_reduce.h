// mx_reduce.h — the reduction family inside libmxgpu: its C-ABI (include/mxgpu_reduce.h), what the export level
// (api_reduce.hip) takes from reduce.hip besides it, and the tile scheme's device helpers, host layout and the two
// launches around the tile kernel, which the fused product of tprod.hip shares with reduce.hip.
#pragma once
#include "mx_common.h"
#include "mx_workspace.h"
#include "../../include/mxgpu_reduce.h"

namespace mx {

constexpr int RD_BLOCK = 256;
constexpr int RD_ITEMS = 16;
constexpr int RD_TILE = RD_BLOCK * RD_ITEMS;        // 4096 entries per tile, the tile of mxd_compact_workspace_bytes
constexpr int RD_CHUNKS = RD_TILE / RD_ITEMS;       // one chunk partial per thread
constexpr int RD_SPAN_CAP = 1024;                   // segments of a tile whose segptr is staged in LDS
static_assert(RD_CHUNKS == RD_BLOCK, "one chunk per thread");
constexpr int64_t RD_GRID_CAP = 2048;

#pragma GCC visibility push(hidden)
// out[s] /= cells - skipped[s] for s < n (skipped may be null): the divisor of rowMeans / colMeans
int reduce_mean_divide(double *out, const int32_t *skipped, int64_t n, double cells, hipStream_t st);
// the tile scheme's first launch for a matrix with values: out[s] = 0 (and skipped[s] = 0 when given) for every
// segment without entries
int reduce_fill_empty(const int32_t *segptr, int nseg, int64_t nnz, double *out, int32_t *skipped, hipStream_t st);
// the tile scheme's last launch: the tile carries of every segment that spans tiles, joined in tile order (nothing to
// do for a single tile)
int reduce_combine(int64_t nnz, const int32_t *segptr, int nseg, int is_max, const double *head, const double *tail,
                   const int32_t *head_cnt, const int32_t *tail_cnt, double *out, int32_t *skipped, hipStream_t st);

inline int64_t rd_ntiles(int64_t nnz) { return ceil_div(nnz > 0 ? nnz : 0, RD_TILE); }

// per tile: the partial of the segment it starts inside, of the one it ends inside, and their skipped counts
struct ReduceLayout {
    WsCursor c;
    int64_t t;
    double *head = c.take<double>(8 * (size_t)t), *tail = c.take<double>(8 * (size_t)t);
    int32_t *head_cnt = c.take<int32_t>(4 * (size_t)t), *tail_cnt = c.take<int32_t>(4 * (size_t)t);
    size_t bytes = c.bytes();
    ReduceLayout(const void *ws, int64_t nnz) : c(ws), t(rd_ntiles(nnz)) {}
};
#pragma GCC visibility pop

#ifdef __HIPCC__
// staged entry i lives at i + i / 16: a lane that walks its own chunk (stride 17 doubles between lanes) meets no
// bank conflict with ds_read_b64, and the lane-strided staging writes stay consecutive
__device__ __forceinline__ int rd_slot(int i) { return i + (i >> 4); }

template <int OP> __device__ __forceinline__ double rd_map(double v)
{
    if constexpr (OP == MX_RED_SUM) return v;
    else if constexpr (OP == MX_RED_SQ_SUM) return v * v;
    else return fabs(v);
}

template <int OP> __device__ __forceinline__ double rd_join(double a, double b)
{
    if constexpr (OP == MX_RED_ABS_MAX) return (b > a || b != b) ? b : a;
    else return a + b;
}

// last s in [0, nseg) with segptr[s] <= q (0 when there is none)
__device__ __forceinline__ int rd_seg_of(const int32_t *__restrict__ segptr, int nseg, int64_t q)
{
    int lo = 0, count = nseg;                       // first s with segptr[s] > q
    while (count > 0) {
        const int step = count >> 1;
        if ((int64_t)segptr[lo + step] <= q) { lo += step + 1; count -= step + 1; }
        else count = step;
    }
    return lo > 0 ? lo - 1 : 0;
}

// the part of segment [a, b) that holds entries: clipped into [0, nnz]
__device__ __forceinline__ void rd_clip(int64_t &a, int64_t &b, int64_t nnz)
{
    a = a < 0 ? 0 : a;
    b = b > nnz ? nnz : b;
}

// OP over the staged entries [lo, hi) of the tile, left to right, through the chunk partials where a chunk is whole
template <int OP>
__device__ __forceinline__ double rd_range(const double *val, const double *csum, int lo, int hi)
{
    double acc = 0.0;
    const int c0 = (lo + RD_ITEMS - 1) / RD_ITEMS, c1 = hi / RD_ITEMS;
    if (c0 < c1) {
        for (int i = lo; i < c0 * RD_ITEMS; i++) acc = rd_join<OP>(acc, val[rd_slot(i)]);
        for (int c = c0; c < c1; c++) acc = rd_join<OP>(acc, csum[c]);
        for (int i = c1 * RD_ITEMS; i < hi; i++) acc = rd_join<OP>(acc, val[rd_slot(i)]);
    } else {
        for (int i = lo; i < hi; i++) acc = rd_join<OP>(acc, val[rd_slot(i)]);
    }
    return acc;
}
#endif  // __HIPCC__

}  // namespace mx

// reduce.hip — segmented reduction over entries, and the batched diagonal.
//
// Stands for: colMeans(X * v) of the vignette's gradient (vignettes/Introducing_MatrixExtra.Rmd:454-470), the margin
// sums behind norm "O" / "I" and the whole-matrix reductions behind norm "F" / "M" (norm_csr, R/csr_linalg.R:13-31),
// diag of an RsparseMatrix (R/csr_linalg.R), and rowSums / colSums / rowMeans / colMeans, which the reference leaves
// to Matrix.
//
// Segmented reduction: out[s] = OP over q in [segptr[s], segptr[s + 1]) of f(values[perm ? perm[q] : q]).
//   fill     one thread per segment: a segment without entries gets 0 (so leading, trailing and runs of empty
//            segments, and nnz == 0, need no tile); a matrix without values is answered here altogether, from the
//            segptr differences.
//   tile     one workgroup per RD_TILE = 256 x 16 consecutive entries, whatever segments they fall into.  The
//            entries are loaded lane-strided (16 independent loads per lane, issued together), mapped by f and
//            staged in LDS; every run of 16 staged entries is summed into a chunk partial.  The tile finds its first
//            and last segment by a binary search of segptr and stages that span of segptr in LDS (up to RD_SPAN_CAP
//            segments; a longer span is read from global memory).  Then one thread per segment of the span reduces
//            the segment's part of the tile, left to right: single entries up to the next chunk boundary, whole chunk
//            partials, single entries again.  A segment that lies wholly inside the tile is written to out; the
//            segment the tile starts in the middle of leaves its partial in head[tile], the one it ends in the middle
//            of in tail[tile].
//   combine  one thread per tile that starts a segment it does not end: tail[tile] + head[tile + 1] + ... in tile
//            order.
// Nothing is partitioned by segment, so cbind(1, X)'s intercept column costs what its entries cost, and there is no
// atomic on a value anywhere: the grouping of every sum is fixed by the positions alone and repeated calls give the
// same bits.  NaN: sums propagate it by themselves; the maximum is written as (b > a || b != b) ? b : a, which keeps
// a NaN once it has one (fmax would drop it).
// The tile's device helpers, its workspace layout and the fill / combine launches are declared in mx_reduce.h: the
// segmented dot product of tprod.hip is the same scheme around a tile kernel of its own.
#include "mx_dispatch.h"
#include "mx_reduce.h"
#include "mx_workspace.h"

namespace mx {

// the skipped entries among the staged [lo, hi)
__device__ __forceinline__ int rd_count(const uint8_t *isna, const int32_t *ccnt, int lo, int hi)
{
    int n = 0;
    const int c0 = (lo + RD_ITEMS - 1) / RD_ITEMS, c1 = hi / RD_ITEMS;
    if (c0 < c1) {
        for (int i = lo; i < c0 * RD_ITEMS; i++) n += isna[i];
        for (int c = c0; c < c1; c++) n += ccnt[c];
        for (int i = c1 * RD_ITEMS; i < hi; i++) n += isna[i];
    } else {
        for (int i = lo; i < hi; i++) n += isna[i];
    }
    return n;
}

// segments without entries get 0; PATTERN: every segment is answered from its length
template <bool PATTERN>
__global__ __launch_bounds__(256)
void rd_fill_kernel(const int32_t *__restrict__ segptr, int nseg, int64_t nnz, int is_max, double *__restrict__ out,
                    int32_t *__restrict__ skipped)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += (int64_t)gridDim.x * blockDim.x) {
        int64_t a = segptr[s], b = segptr[s + 1];
        rd_clip(a, b, nnz);
        const int64_t len = b > a ? b - a : 0;
        if (PATTERN) out[s] = is_max ? (len > 0 ? 1.0 : 0.0) : (double)len;
        else if (len == 0) out[s] = 0.0;
        if (skipped && (PATTERN || len == 0)) skipped[s] = 0;
    }
}

// VK: 0 f64, 1 R logical
template <int OP, int VK, bool PERM>
__global__ __launch_bounds__(RD_BLOCK)
void rd_tile_kernel(const void *__restrict__ values, const int32_t *__restrict__ perm, int64_t nnz,
                    const int32_t *__restrict__ segptr, int nseg, int na_rm, double *__restrict__ out,
                    int32_t *__restrict__ skipped, double *__restrict__ head, double *__restrict__ tail,
                    int32_t *__restrict__ head_cnt, int32_t *__restrict__ tail_cnt)
{
    __shared__ double val[RD_TILE + RD_CHUNKS];
    __shared__ double csum[RD_CHUNKS];
    __shared__ int32_t ccnt[RD_CHUNKS];
    __shared__ __attribute__((aligned(16))) uint8_t isna[RD_TILE];
    __shared__ int32_t span[RD_SPAN_CAP + 1];
    __shared__ int32_t ends[2];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * RD_TILE;
    const int tile_n = nnz - t0 < RD_TILE ? (int)(nnz - t0) : RD_TILE;      // >= 1: the grid is ceil(nnz / RD_TILE)
    const int64_t t_end = t0 + tile_n;

    if (tid < 2) ends[tid] = rd_seg_of(segptr, nseg, tid == 0 ? t0 : t_end - 1);

    // the tile's entries: every load is unconditional (a lane past the end re-reads the tile's first entry), so all
    // 16 (32 with a permutation) are in flight together
    int64_t src[RD_ITEMS];
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) {
        const int i = it * RD_BLOCK + tid;
        src[it] = t0 + (i < tile_n ? i : 0);
    }
    if (PERM) {
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) {
            const int32_t p = perm[src[it]];
            src[it] = (uint32_t)p < (uint64_t)nnz ? p : 0;                  // a bad position reads entry 0, in bounds
        }
    }
    double v[RD_ITEMS];
    bool na[RD_ITEMS];
    if constexpr (VK == 0) {
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) v[it] = ((const double *)values)[src[it]];
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) na[it] = v[it] != v[it];
    } else {
        int32_t x[RD_ITEMS];
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) x[it] = ((const int32_t *)values)[src[it]];
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) {
            na[it] = x[it] == MX_NA_INT;
            v[it] = na[it] ? na_real() : (x[it] != 0 ? 1.0 : 0.0);
        }
    }
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) {
        const int i = it * RD_BLOCK + tid;
        const bool in = i < tile_n, skip = in && na_rm && na[it];
        val[rd_slot(i)] = in && !skip ? rd_map<OP>(v[it]) : 0.0;
        isna[i] = skip ? 1 : 0;
    }
    __syncthreads();

    {   // chunk partials: thread t owns staged entries [16 t, 16 t + 16)
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < RD_ITEMS; k++) acc = rd_join<OP>(acc, val[tid * (RD_ITEMS + 1) + k]);
        csum[tid] = acc;
        const uint4 w = ((const uint4 *)isna)[tid];                         // 16 flags of 0 / 1
        ccnt[tid] = __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    }
    const int s_first = ends[0], s_last = ends[1];
    const bool staged = s_last - s_first + 1 <= RD_SPAN_CAP;
    if (staged)
        for (int i = tid; i <= s_last - s_first + 1; i += RD_BLOCK) span[i] = segptr[s_first + i];
    __syncthreads();

    for (int s = s_first + tid; s <= s_last; s += RD_BLOCK) {
        int64_t a = staged ? span[s - s_first] : segptr[s], b = staged ? span[s - s_first + 1] : segptr[s + 1];
        rd_clip(a, b, nnz);
        const int64_t lo = a > t0 ? a : t0, hi = b < t_end ? b : t_end;
        if (hi <= lo) continue;                                             // no entry of it in this tile
        const double acc = rd_range<OP>(val, csum, (int)(lo - t0), (int)(hi - t0));
        const int cnt = na_rm ? rd_count(isna, ccnt, (int)(lo - t0), (int)(hi - t0)) : 0;
        if (a >= t0 && b <= t_end) {
            out[s] = acc;
            if (skipped) skipped[s] = cnt;
        } else if (a < t0) {                                                // started in an earlier tile
            head[blockIdx.x] = acc;
            head_cnt[blockIdx.x] = cnt;
        } else {                                                            // starts here, goes on
            tail[blockIdx.x] = acc;
            tail_cnt[blockIdx.x] = cnt;
        }
    }
}

// one thread per tile: the tile in which a segment starts that ends in a later one adds the partials in tile order
__global__ __launch_bounds__(256)
void rd_combine_kernel(int64_t nnz, int64_t ntiles, const int32_t *__restrict__ segptr, int nseg, int is_max,
                       const double *__restrict__ head, const double *__restrict__ tail,
                       const int32_t *__restrict__ head_cnt, const int32_t *__restrict__ tail_cnt,
                       double *__restrict__ out, int32_t *__restrict__ skipped)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const int64_t t0 = t * RD_TILE, t_end = t0 + RD_TILE;
    if (t_end >= nnz) return;                                               // the last tile starts nothing that goes on
    const int s = rd_seg_of(segptr, nseg, t_end - 1);                       // the segment of the tile's last entry
    int64_t a = segptr[s], b = segptr[s + 1];
    rd_clip(a, b, nnz);
    if (!(a >= t0 && a < t_end && b > t_end)) return;
    double acc = tail[t];
    int cnt = tail_cnt[t];
    const int64_t last = (b - 1) / RD_TILE;
    for (int64_t u = t + 1; u <= last; u++) {
        acc = is_max ? rd_join<MX_RED_ABS_MAX>(acc, head[u]) : acc + head[u];
        cnt += head_cnt[u];
    }
    out[s] = acc;
    if (skipped) skipped[s] = cnt;
}

// out[s] /= cells - skipped[s]
__global__ __launch_bounds__(256)
void rd_mean_kernel(double *__restrict__ out, const int32_t *__restrict__ skipped, int64_t n, double cells)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x)
        out[s] = out[s] / (cells - (skipped ? (double)skipped[s] : 0.0));
}

// G lanes per row k < d: the first stored (k, k) of row k in storage order
template <int G, int VK, bool SORTED>
__global__ __launch_bounds__(256)
void rd_diag_kernel(int d, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                    const void *__restrict__ values, int64_t nnz, void *__restrict__ out)
{
    const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int gl = lane_id() & (G - 1);
    const bool live = k < d;
    RowBounds rb = {0, 0};
    if (live) rb = row_bounds(indptr[k], indptr[k + 1], nnz);
    int pos = INT_MAX;                                                      // nnz <= INT_MAX
    if (SORTED) {
        if (gl == 0 && rb.len > 0) {
            const int lb = lower_bound_dev(indices + rb.start, (int)rb.len, (int)k);
            if (lb < rb.len && indices[rb.start + lb] == (int)k) pos = (int)(rb.start + lb);
        }
    } else {
        for (int64_t e = gl; e < rb.len; e += G)
            if (indices[rb.start + e] == (int)k) { pos = (int)(rb.start + e); break; }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(pos, off, G);
        pos = o < pos ? o : pos;
    }
    if (!live || gl != 0) return;
    const bool found = pos != INT_MAX;
    if constexpr (VK == 0) ((double *)out)[k] = found ? ((const double *)values)[pos] : 0.0;
    else if constexpr (VK == 1) ((int32_t *)out)[k] = found ? ((const int32_t *)values)[pos] : 0;
    else ((int32_t *)out)[k] = found ? 1 : 0;
}

// ---- host side ----------------------------------------------------------------------------------------------
int reduce_fill_empty(const int32_t *segptr, int nseg, int64_t nnz, double *out, int32_t *skipped, hipStream_t st)
{
    hipLaunchKernelGGL(rd_fill_kernel<false>, dim3(grid_for(nseg, 256, RD_GRID_CAP)), dim3(256), 0, st, segptr, nseg, nnz,
                       0, out, skipped);
    MX_LAUNCH_CHECK();
    return 0;
}

int reduce_combine(int64_t nnz, const int32_t *segptr, int nseg, int is_max, const double *head, const double *tail,
                   const int32_t *head_cnt, const int32_t *tail_cnt, double *out, int32_t *skipped, hipStream_t st)
{
    const int64_t ntiles = rd_ntiles(nnz);
    if (ntiles <= 1) return 0;
    hipLaunchKernelGGL(rd_combine_kernel, dim3((unsigned)ceil_div(ntiles, 256)), dim3(256), 0, st, nnz, ntiles, segptr,
                       nseg, is_max, head, tail, head_cnt, tail_cnt, out, skipped);
    MX_LAUNCH_CHECK();
    return 0;
}

static int segment_reduce(int op, const void *values, int value_dtype, const int32_t *perm, int64_t nnz,
                          const int32_t *segptr, int nseg, int na_rm, double *out, int32_t *skipped, void *workspace,
                          hipStream_t st)
{
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX && nseg >= 0 && nseg < INT_MAX, "mxd_segment_reduce: bad size");
    MX_REQUIRE(op >= MX_RED_SUM && op <= MX_RED_ABS_MAX, "mxd_segment_reduce: unknown operation %d", op);
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_segment_reduce: unsupported value dtype %d", value_dtype);
    if (nseg == 0) return 0;
    MX_REQUIRE(segptr && out, "mxd_segment_reduce: null pointer");
    const bool pattern = value_dtype == MX_NONE, is_max = op == MX_RED_ABS_MAX;
    MX_REQUIRE(pattern || nnz == 0 || (values && workspace), "mxd_segment_reduce: null pointer");
    const ReduceLayout L(workspace, nnz);
    MX_REQUIRE(L.bytes <= 4 * mxd_compact_workspace_bytes(nnz), "mxd_segment_reduce: the tile carries outgrew the workspace");
    if (pattern) {
        hipLaunchKernelGGL(rd_fill_kernel<true>, dim3(grid_for(nseg, 256, RD_GRID_CAP)), dim3(256), 0, st, segptr, nseg,
                           nnz, (int)is_max, out, skipped);
        MX_LAUNCH_CHECK();
        return 0;
    }
    if (reduce_fill_empty(segptr, nseg, nnz, out, skipped, st)) return 1;
    if (nnz == 0) return 0;
    const int64_t ntiles = rd_ntiles(nnz);
    const int rc = dispatch_int(int_list<MX_RED_SUM, MX_RED_ABS_SUM, MX_RED_SQ_SUM, MX_RED_ABS_MAX>{},
                                "mxd_segment_reduce", "operation", op, [&](auto o) {
        constexpr int OP = decltype(o)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(RD_BLOCK), 0, st, values, perm, nnz, segptr, nseg,
                               na_rm ? 1 : 0, out, skipped, L.head, L.tail, L.head_cnt, L.tail_cnt);
        };
        if (value_dtype == MX_F64) {
            if (perm) launch(rd_tile_kernel<OP, 0, true>); else launch(rd_tile_kernel<OP, 0, false>);
        } else {
            if (perm) launch(rd_tile_kernel<OP, 1, true>); else launch(rd_tile_kernel<OP, 1, false>);
        }
        MX_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    return reduce_combine(nnz, segptr, nseg, (int)is_max, L.head, L.tail, L.head_cnt, L.tail_cnt, out, skipped, st);
}

int reduce_mean_divide(double *out, const int32_t *skipped, int64_t n, double cells, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(rd_mean_kernel, dim3(grid_for(n, 256, RD_GRID_CAP)), dim3(256), 0, st, out, skipped, n, cells);
    MX_LAUNCH_CHECK();
    return 0;
}

static int csr_diag(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values, int value_dtype,
                    int64_t nnz, int rows_sorted, void *out, hipStream_t st)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_diag: bad size");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_csr_diag: unsupported value dtype %d", value_dtype);
    const int d = m < n ? m : n;
    if (d == 0) return 0;
    MX_REQUIRE(indptr && out && (nnz == 0 || (indices && (value_dtype == MX_NONE || values))), "mxd_csr_diag: null pointer");
    const int G = rows_sorted ? 4 : pick_group((double)nnz / (double)m);
    const int vk = value_dtype == MX_F64 ? 0 : value_dtype == MX_LGL ? 1 : 2;
    return launch_rows(lane_groups{}, "mxd_csr_diag", G, d, 256, [&](auto g, dim3 grid, dim3 block) {
        constexpr int GG = decltype(g)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, d, indptr, indices, values, nnz, out);
        };
        if (rows_sorted) {
            if (vk == 0) launch(rd_diag_kernel<GG, 0, true>);
            else if (vk == 1) launch(rd_diag_kernel<GG, 1, true>);
            else launch(rd_diag_kernel<GG, 2, true>);
        } else {
            if (vk == 0) launch(rd_diag_kernel<GG, 0, false>);
            else if (vk == 1) launch(rd_diag_kernel<GG, 1, false>);
            else launch(rd_diag_kernel<GG, 2, false>);
        }
    });
}

}  // namespace mx

extern "C" int mxd_segment_reduce(int op, const void *values, int value_dtype, const int32_t *perm, int64_t nnz,
                                  const int32_t *segptr, int nseg, int na_rm, double *out, int32_t *skipped_out,
                                  void *workspace, void *stream)
{
    return mx::segment_reduce(op, values, value_dtype, perm, nnz, segptr, nseg, na_rm, out, skipped_out, workspace,
                              mx::as_stream(stream));
}

extern "C" int mxd_csr_diag(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values,
                            int value_dtype, int64_t nnz, int rows_sorted, void *out, void *stream)
{
    return mx::csr_diag(m, n, indptr, indices, values, value_dtype, nnz, rows_sorted, out, mx::as_stream(stream));
}

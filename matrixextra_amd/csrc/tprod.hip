// tprod.hip — the transposed products' device level (include/mxgpu_tprod.h): a segmented dot product
// on the tile scheme of reduce.hip, and the gather that turns a cached column order into the CSR of X^T.
//
// Stands for: crossprod(X, r), the gradient colMeans(X * r) of the vignette (vignettes/Introducing_MatrixExtra.Rmd:
// 454-470) without its product matrix, and the X^T products that the reference leaves to Matrix.
//
// Segmented dot: out[s] = sum over q in [segptr[s], segptr[s + 1]) of x[perm ? perm[q] : q] * w[key[q]].
//   fill     reduce.hip's: a segment without entries gets 0.
//   tile     one workgroup per RD_TILE consecutive entries.  A lane's loads are issued in two rounds: perm[q] and
//            key[q], which are coalesced, then x[p] and w[key], which are not.  The product is rounded to f64 by
//            itself (__dmul_rn under a contract-off pragma: the library is built with -ffp-contract=on, and a product
//            fused into the addition that follows would differ in the last bit from the written-out X * w) and staged
//            with rd_slot; from there on the tile is reduce.hip's MX_RED_SUM tile: chunk partials, one thread per
//            segment of the span, head / tail carries.
//   combine  reduce.hip's: the carries in tile order.
// The grouping of every sum is therefore that of mxd_segment_reduce(MX_RED_SUM) over the products, and the result the
// same bits; tests/test_gpu_tprod.py compares the two.  No atomic touches a value.
#include "mx_dispatch.h"
#include "mx_reduce.h"
#include "../../include/mxgpu_tprod.h"

namespace mx {

template <bool VALUES, bool PERM>
__global__ __launch_bounds__(RD_BLOCK)
void td_tile_kernel(const double *__restrict__ values, const int32_t *__restrict__ perm,
                    const int32_t *__restrict__ key, const double *__restrict__ w, int64_t nw, int64_t nnz,
                    const int32_t *__restrict__ segptr, int nseg, double *__restrict__ out, double *__restrict__ head,
                    double *__restrict__ tail, int32_t *__restrict__ head_cnt, int32_t *__restrict__ tail_cnt)
{
    __shared__ double val[RD_TILE + RD_CHUNKS];
    __shared__ double csum[RD_CHUNKS];
    __shared__ int32_t span[RD_SPAN_CAP + 1];
    __shared__ int32_t ends[2];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * RD_TILE;
    const int tile_n = nnz - t0 < RD_TILE ? (int)(nnz - t0) : RD_TILE;      // >= 1: the grid is ceil(nnz / RD_TILE)
    const int64_t t_end = t0 + tile_n;

    if (tid < 2) ends[tid] = rd_seg_of(segptr, nseg, tid == 0 ? t0 : t_end - 1);

    // every load is unconditional (a lane past the end re-reads the tile's first entry): first the 32 coalesced loads
    // of positions and keys, then the 32 scattered ones of entries and weights
    int64_t src[RD_ITEMS];
    int32_t kk[RD_ITEMS];
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) {
        const int i = it * RD_BLOCK + tid;
        src[it] = t0 + (i < tile_n ? i : 0);
    }
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) kk[it] = key[src[it]];
    if (PERM) {
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) {
            const int32_t p = perm[src[it]];
            src[it] = (uint32_t)p < (uint64_t)nnz ? p : 0;                  // a bad position reads entry 0, in bounds
        }
    }
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) kk[it] = (uint32_t)kk[it] < (uint64_t)nw ? kk[it] : 0;   // and a bad key w[0]
    double x[RD_ITEMS], ww[RD_ITEMS];
    if (VALUES) {
#pragma unroll
        for (int it = 0; it < RD_ITEMS; it++) x[it] = values[src[it]];
    }
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) ww[it] = w[kk[it]];
#pragma unroll
    for (int it = 0; it < RD_ITEMS; it++) {
        const int i = it * RD_BLOCK + tid;
        double term = ww[it];
        if (VALUES) {
#pragma clang fp contract(off)
            term = __dmul_rn(x[it], ww[it]);                                // rounded here: never part of an fma
        }
        val[rd_slot(i)] = i < tile_n ? term : 0.0;
    }
    __syncthreads();

    {   // chunk partials: thread t owns staged entries [16 t, 16 t + 16)
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < RD_ITEMS; k++) acc = rd_join<MX_RED_SUM>(acc, val[tid * (RD_ITEMS + 1) + k]);
        csum[tid] = acc;
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
        const double acc = rd_range<MX_RED_SUM>(val, csum, (int)(lo - t0), (int)(hi - t0));
        if (a >= t0 && b <= t_end) {
            out[s] = acc;
        } else if (a < t0) {                                                // started in an earlier tile
            head[blockIdx.x] = acc;
            head_cnt[blockIdx.x] = 0;                                       // the combine step adds the counts up too
        } else {                                                            // starts here, goes on
            tail[blockIdx.x] = acc;
            tail_cnt[blockIdx.x] = 0;
        }
    }
}

// one thread per entry q of the column order: its source row by a search of indptr, its value by a bit copy
template <typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(256)
void tb_gather_kernel(int m, int64_t nnz, const int32_t *__restrict__ indptr, const VT *__restrict__ values,
                      const int32_t *__restrict__ perm, int32_t *__restrict__ out_rows, VT *__restrict__ out_values)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    int32_t p = perm[q];
    p = (uint32_t)p < (uint64_t)nnz ? p : 0;                                // a bad position reads entry 0, in bounds
    if (out_rows) out_rows[q] = rd_seg_of(indptr, m, p);                    // last row r with indptr[r] <= p
    if (HAS_VALUES) out_values[q] = values[p];
}

static int segment_dot(const void *values, int value_dtype, const int32_t *perm, const int32_t *key, const double *w,
                       int64_t nw, int64_t nnz, const int32_t *segptr, int nseg, double *out, void *workspace,
                       hipStream_t st)
{
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX && nseg >= 0 && nseg < INT_MAX && nw >= 0, "mxd_segment_dot: bad size");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_NONE, "mxd_segment_dot: unsupported value dtype %d",
               value_dtype);
    if (nseg == 0) return 0;
    MX_REQUIRE(segptr && out, "mxd_segment_dot: null pointer");
    const bool has_values = value_dtype == MX_F64;
    MX_REQUIRE(nnz == 0 || (key && w && workspace && (!has_values || values)), "mxd_segment_dot: null pointer");
    MX_REQUIRE(nnz == 0 || nw > 0, "mxd_segment_dot: entries without a vector to multiply");
    const ReduceLayout L(workspace, nnz);
    MX_REQUIRE(L.bytes <= 4 * mxd_compact_workspace_bytes(nnz), "mxd_segment_dot: the tile carries outgrew the workspace");
    if (reduce_fill_empty(segptr, nseg, nnz, out, nullptr, st)) return 1;
    if (nnz == 0) return 0;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)rd_ntiles(nnz)), dim3(RD_BLOCK), 0, st, (const double *)values, perm,
                           key, w, nw, nnz, segptr, nseg, out, L.head, L.tail, L.head_cnt, L.tail_cnt);
    };
    if (has_values) {
        if (perm) launch(td_tile_kernel<true, true>); else launch(td_tile_kernel<true, false>);
    } else {
        if (perm) launch(td_tile_kernel<false, true>); else launch(td_tile_kernel<false, false>);
    }
    MX_LAUNCH_CHECK();
    return reduce_combine(nnz, segptr, nseg, 0, L.head, L.tail, L.head_cnt, L.tail_cnt, out, nullptr, st);
}

static int csr_transpose_by_order(int m, int64_t nnz, const int32_t *indptr, const void *values, int value_dtype,
                                  const int32_t *perm, int32_t *out_rows, void *out_values, hipStream_t st)
{
    MX_REQUIRE(m >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_transpose_by_order: bad size");
    MX_REQUIRE(m > 0 || nnz == 0, "mxd_csr_transpose_by_order: entries without rows");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_csr_transpose_by_order: unsupported value dtype %d", value_dtype);
    const bool gather = value_dtype != MX_NONE && out_values;
    if (nnz == 0 || (!out_rows && !gather)) return 0;
    MX_REQUIRE(perm && (!out_rows || indptr) && (!gather || values), "mxd_csr_transpose_by_order: null pointer");
    return dispatch_values("mxd_csr_transpose_by_order", gather ? value_dtype : MX_NONE, [&](auto kind) {
        using K = decltype(kind);
        using VT = typename K::VT;
        hipLaunchKernelGGL((tb_gather_kernel<VT, K::has_values>), dim3((unsigned)ceil_div(nnz, 256)), dim3(256), 0, st, m,
                           nnz, indptr, K::has_values ? (const VT *)values : nullptr, perm, out_rows,
                           K::has_values ? (VT *)out_values : nullptr);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

}  // namespace mx

extern "C" int mxd_segment_dot(const void *values, int value_dtype, const int32_t *perm, const int32_t *key,
                               const double *w, int64_t nw, int64_t nnz, const int32_t *segptr, int nseg, double *out,
                               void *workspace, void *stream)
{
    return mx::segment_dot(values, value_dtype, perm, key, w, nw, nnz, segptr, nseg, out, workspace,
                           mx::as_stream(stream));
}

extern "C" int mxd_csr_transpose_by_order(int m, int64_t nnz, const int32_t *indptr, const void *values, int value_dtype,
                                          const int32_t *perm, int32_t *out_rows, void *out_values, void *stream)
{
    return mx::csr_transpose_by_order(m, nnz, indptr, values, value_dtype, perm, out_rows, out_values,
                                      mx::as_stream(stream));
}

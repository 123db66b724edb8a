// bind.hip — cbind / rbind of CSR matrices for gfx950.
//
// Replaces:
//   cbind_csr<>          src/cbind.cpp:4-99     per-row interleave of two CSR operands
//   concat_indptr2       src/rbind.cpp:9-21
//   concat_csr_batch     src/rbind.cpp:24-173   bulk copy + indptr offset (+ value-type conversion)
// Pure bandwidth copies: 2*12 bytes per entry + 8 bytes per row.  The output row offsets of cbind are
// indptrX[r] + indptrY[r] — no scan is needed.
#include "mx_dispatch.h"

namespace mx {

constexpr int BIND_BLOCK = 256;

template <int G, typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(BIND_BLOCK)
void cbind_kernel(int nX, int nY, const int32_t *__restrict__ Xp, const int32_t *__restrict__ Xj, const VT *__restrict__ Xx,
                  const int32_t *__restrict__ Yp, const int32_t *__restrict__ Yj, const VT *__restrict__ Yx, int y_shift,
                  int32_t *__restrict__ indptr, int32_t *__restrict__ indices, VT *__restrict__ values)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (BIND_BLOCK / G) + threadIdx.x / G;
    const int nrows = max(nX, nY);
    if (row >= nrows) return;
    // rows past the end of an operand contribute nothing and sit after all of its entries
    const int xs = Xp[min((long long)nX, row)], xe = Xp[min((long long)nX, row + 1)];
    const int ys = Yp[min((long long)nY, row)], ye = Yp[min((long long)nY, row + 1)];
    const int o = xs + ys, lx = xe - xs, ly = ye - ys;
    if (lg == 0) {
        indptr[row + 1] = xe + ye;
        if (row == 0) indptr[0] = 0;
    }
    for (int k = lg; k < lx; k += G) {
        indices[o + k] = Xj[xs + k];
        if constexpr (HAS_VALUES) values[o + k] = Xx[xs + k];
    }
    for (int k = lg; k < ly; k += G) {
        indices[o + lx + k] = Yj[ys + k] + y_shift;
        if constexpr (HAS_VALUES) values[o + lx + k] = Yx[ys + k];
    }
}

__global__ __launch_bounds__(256)
void indptr_offset_kernel(const int32_t *__restrict__ src, int n, int offset, int32_t *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = offset + src[i];
}

// the one indptr entry behind a sparse vector's row: written on the stream, so that the append needs no host copy
__global__ void indptr_end_kernel(int32_t *__restrict__ dst, int32_t end)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = end;
}

// value conversion of concat_csr_batch (rbind.cpp:72-166), one entry.  IN: 0 f64, 1 R logical, 2 none, 4 R integer;
// OUT: 0 f64, 1 R logical, 2 none.  `vec` says the input is a sparse vector (an lsparseVector's TRUE becomes 1.0, an
// lgRMatrix's value is widened as it is).  This is the one statement of the table: every concat kernel calls it.
template <int IN, int OUT>
__device__ __forceinline__ void concat_value(const void *__restrict__ val_in, int64_t i, bool vec,
                                             void *__restrict__ val_out, int64_t o)
{
    if constexpr (OUT == 0) {
        double v;
        if constexpr (IN == 0) v = ((const double *)val_in)[i];
        else if constexpr (IN == 1) { const int l = ((const int32_t *)val_in)[i]; v = l == MX_NA_INT ? na_real() : (vec ? (double)(l != 0) : (double)l); }
        else if constexpr (IN == 4) { const int l = ((const int32_t *)val_in)[i]; v = l == MX_NA_INT ? na_real() : (double)l; }
        else v = 1.0;
        ((double *)val_out)[o] = v;
    } else if constexpr (OUT == 1) {
        int v;
        if constexpr (IN == 0) { const double d = ((const double *)val_in)[i]; v = d != d ? MX_NA_INT : (d != 0.0); }
        else if constexpr (IN == 1) v = ((const int32_t *)val_in)[i];
        else if constexpr (IN == 4) { const int l = ((const int32_t *)val_in)[i]; v = l == MX_NA_INT ? MX_NA_INT : (l != 0); }
        else v = 1;
        ((int32_t *)val_out)[o] = v;
    }
}

// value kind of an operand kind (0 dgR, 1 lgR, 2 ngR / dgT, lgT, ngT, 3 d, 4 i, 5 l, 6 n sparseVector)
__host__ __device__ __forceinline__ int concat_value_kind(int in_kind)
{
    return (in_kind == 0 || in_kind == 3) ? 0 : (in_kind == 1 || in_kind == 5) ? 1 : (in_kind == 4) ? 4 : 2;
}

// the same with the input's value kind known only at run time (a tile that spans operands of several kinds)
template <int OUT>
__device__ __forceinline__ void concat_value_any(int vin, const void *__restrict__ val_in, int64_t i, bool vec,
                                                 void *__restrict__ val_out, int64_t o)
{
    switch (vin) {
        case 0: concat_value<0, OUT>(val_in, i, vec, val_out, o); break;
        case 1: concat_value<1, OUT>(val_in, i, vec, val_out, o); break;
        case 4: concat_value<4, OUT>(val_in, i, vec, val_out, o); break;
        default: concat_value<2, OUT>(val_in, i, vec, val_out, o); break;
    }
}

template <int IN, int OUT>
__global__ __launch_bounds__(256)
void concat_entries_kernel(int64_t n, const int32_t *__restrict__ idx_in, const void *__restrict__ val_in, int add,
                           int32_t *__restrict__ idx_out, void *__restrict__ val_out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        idx_out[i] = idx_in[i] + add;
        concat_value<IN, OUT>(val_in, i, add != 0, val_out, i);
    }
}

// ---- the batched row concat: a device-resident table of mx_rbind_item drives two launches, whatever the operand
// count.  Offsets are non-decreasing along the table and operands without rows (without entries) share theirs with
// the next one, so "the operand of row r (entry e)" is the LAST item whose offset is <= r (e): of a run of equal
// offsets only the last can own anything.
constexpr int RBIND_BLOCK = 256;
constexpr int RBIND_TILE = 1024;          // output entries per workgroup
constexpr int RBIND_STAGE = 2048;         // entry offsets of a spanning tile kept in LDS

// last k in [lo, hi] with off(k) <= key; off(lo) <= key is the caller's guarantee
template <typename Off>
__device__ __forceinline__ int last_not_above(int lo, int hi, int64_t key, Off &&off)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off(mid) <= key) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(RBIND_BLOCK)
void rbind_indptr_kernel(const mx_rbind_item *__restrict__ items, int n_items, int nrows_out,
                         int32_t *__restrict__ out_indptr)
{
    const int64_t row = (int64_t)blockIdx.x * RBIND_BLOCK + threadIdx.x;
    if (row == 0) out_indptr[0] = 0;
    if (row >= nrows_out) return;
    const int k = last_not_above(0, n_items - 1, row, [&](int m) { return (int64_t)items[m].row_offset; });
    const mx_rbind_item &it = items[k];
    const int64_t end = it.kind >= 3 ? it.nnz : (int64_t)it.indptr[row - it.row_offset + 1];
    out_indptr[row + 1] = (int32_t)(it.entry_offset + end);
}

template <int OUT>
__device__ __forceinline__ void rbind_entry(const mx_rbind_item &it, int64_t e, int32_t *__restrict__ idx_out,
                                            void *__restrict__ val_out)
{
    const int64_t i = e - it.entry_offset;
    const bool vec = it.kind >= 3;
    idx_out[e] = it.indices[i] - (vec ? 1 : 0);
    concat_value_any<OUT>(concat_value_kind(it.kind), it.values, i, vec, val_out, e);
}

template <int IN, int OUT>
__device__ __forceinline__ void rbind_copy_tile(const mx_rbind_item &it, int64_t t0, int64_t t1,
                                                int32_t *__restrict__ idx_out, void *__restrict__ val_out)
{
    const bool vec = it.kind >= 3;
    const int add = vec ? -1 : 0;
    const int32_t *__restrict__ idx_in = it.indices;
    const void *__restrict__ val_in = it.values;
    const int64_t base = it.entry_offset;
    for (int64_t e = t0 + threadIdx.x; e < t1; e += RBIND_BLOCK) {
        idx_out[e] = idx_in[e - base] + add;
        concat_value<IN, OUT>(val_in, e - base, vec, val_out, e);
    }
}

template <int OUT>
__global__ __launch_bounds__(RBIND_BLOCK)
void rbind_entries_kernel(const mx_rbind_item *__restrict__ items, int n_items, int64_t nnz_out,
                          int32_t *__restrict__ idx_out, void *__restrict__ val_out)
{
    __shared__ int32_t s_off[RBIND_STAGE];
    const int64_t t0 = (int64_t)blockIdx.x * RBIND_TILE;
    const int64_t t1 = t0 + RBIND_TILE < nnz_out ? t0 + RBIND_TILE : nnz_out;
    if (t0 >= t1) return;
    auto off = [&](int m) { return items[m].entry_offset; };
    // block-uniform: the operands of the tile's first and last entry (items[0].entry_offset == 0 <= t0)
    const int k0 = last_not_above(0, n_items - 1, t0, off);
    const int k1 = last_not_above(k0, n_items - 1, t1 - 1, off);
    if (k0 == k1) {                       // inside one operand: a straight copy
        const mx_rbind_item &it = items[k0];
        switch (concat_value_kind(it.kind)) {
            case 0: rbind_copy_tile<0, OUT>(it, t0, t1, idx_out, val_out); break;
            case 1: rbind_copy_tile<1, OUT>(it, t0, t1, idx_out, val_out); break;
            case 4: rbind_copy_tile<4, OUT>(it, t0, t1, idx_out, val_out); break;
            default: rbind_copy_tile<2, OUT>(it, t0, t1, idx_out, val_out); break;
        }
        return;
    }
    const int span = k1 - k0 + 1;
    const bool staged = span <= RBIND_STAGE;                           // nnz_out <= INT_MAX: offsets fit int32
    if (staged) {
        for (int m = threadIdx.x; m < span; m += RBIND_BLOCK) s_off[m] = (int32_t)items[k0 + m].entry_offset;
        __syncthreads();
    }
    for (int64_t e = t0 + threadIdx.x; e < t1; e += RBIND_BLOCK) {
        const int k = staged ? k0 + last_not_above(0, span - 1, e, [&](int m) { return (int64_t)s_off[m]; })
                             : last_not_above(k0, k1, e, off);
        rbind_entry<OUT>(items[k], e, idx_out, val_out);
    }
}

// ---- COO concat: the twin of the entry pass.  A matrix operand's rows move down by row_offset; a sparse vector is
// the one row `row_offset` with its 1-based indices as columns.
template <int IN, int OUT>
__global__ __launch_bounds__(256)
void coo_append_kernel(int64_t n, const int32_t *__restrict__ i_in, const int32_t *__restrict__ j_in,
                       const void *__restrict__ val_in, bool vec, int row_offset, int32_t *__restrict__ i_out,
                       int32_t *__restrict__ j_out, void *__restrict__ val_out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        i_out[k] = vec ? row_offset : i_in[k] + row_offset;
        j_out[k] = vec ? j_in[k] - 1 : j_in[k];
        concat_value<IN, OUT>(val_in, k, vec, val_out, k);
    }
}

// ---- a sparse vector as one more column of a CSR: cbind_kernel with the second operand given as sorted 1-based
// (idx, values).  Row r gains one entry iff r + 1 is in idx, so its output offset is Xp[r] + lower_bound(idx, r + 1).
template <int OUT>
__global__ __launch_bounds__(BIND_BLOCK)
void cbind_svec_kernel(int nX, int nrows, const int32_t *__restrict__ Xp, const int32_t *__restrict__ Xj,
                       const void *__restrict__ Xx, int x_vin, int ncolX, const int32_t *__restrict__ vi,
                       const void *__restrict__ vx, int v_vin, int nv, int first, int32_t *__restrict__ indptr,
                       int32_t *__restrict__ indices, void *__restrict__ values)
{
    constexpr int G = 8;
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (BIND_BLOCK / G) + threadIdx.x / G;
    if (row >= nrows) return;
    const int xs = Xp[min((long long)nX, row)], xe = Xp[min((long long)nX, row + 1)];
    const int lb = lower_bound_dev(vi, nv, (int)row + 1);
    const int has = lb < nv && vi[lb] == (int)row + 1;
    const int64_t o = (int64_t)xs + lb;
    const int lx = xe - xs;
    if (lg == 0) {
        indptr[row + 1] = xe + lb + has;
        if (row == 0) indptr[0] = 0;
        if (has) {
            const int64_t at = first ? o : o + lx;
            indices[at] = first ? 0 : ncolX;
            concat_value_any<OUT>(v_vin, vx, lb, true, values, at);
        }
    }
    const int64_t ox = o + (first ? has : 0);
    for (int k = lg; k < lx; k += G) {
        indices[ox + k] = Xj[xs + k] + (first ? 1 : 0);
        concat_value_any<OUT>(x_vin, Xx, (int64_t)xs + k, false, values, ox + k);
    }
}

}  // namespace mx

static int csr_cbind(const char *what, int nX, int nY, const int32_t *Xp, const int32_t *Xj, const void *Xx,
                     const int32_t *Yp, const int32_t *Yj, const void *Yx, int y_shift, int value_dtype,
                     int64_t nnz_total, int32_t *indptr, int32_t *indices, void *values, void *stream)
{
    MX_REQUIRE(nX >= 0 && nY >= 0 && y_shift >= 0, "%s: negative size", what);
    const int nrows = nX > nY ? nX : nY;
    hipStream_t st = mx::as_stream(stream);
    if (nrows == 0) { MX_HIP(hipMemsetAsync(indptr, 0, sizeof(int32_t), st)); return 0; }
    const int G = mx::pick_group(0.5 * (double)nnz_total / (double)nrows);
    return mx::dispatch_values(what, value_dtype, [&](auto vk) {
        using VT = typename decltype(vk)::VT;
        return mx::launch_rows(mx::lane_groups{}, what, G, nrows, mx::BIND_BLOCK,
                               [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::cbind_kernel<g(), VT, vk.has_values>), grid, block, 0, st, nX, nY, Xp, Xj,
                               (const VT *)Xx, Yp, Yj, (const VT *)Yx, y_shift, indptr, indices, (VT *)values);
        });
    });
}

extern "C" int mxd_csr_cbind(int nX, int nY, const int32_t *Xp, const int32_t *Xj, const void *Xx, const int32_t *Yp,
                             const int32_t *Yj_plus_ncol, const void *Yx, int value_dtype, int64_t nnz_total,
                             int32_t *indptr, int32_t *indices, void *values, void *stream)
{
    return csr_cbind("mxd_csr_cbind", nX, nY, Xp, Xj, Xx, Yp, Yj_plus_ncol, Yx, 0, value_dtype, nnz_total, indptr,
                     indices, values, stream);
}

// the same with Y's column ids as they are: the kernel adds ncolX to them
extern "C" int mxd_csr_cbind_shift(int nX, int nY, int ncolX, const int32_t *Xp, const int32_t *Xj, const void *Xx,
                                   const int32_t *Yp, const int32_t *Yj, const void *Yx, int value_dtype,
                                   int64_t nnz_total, int32_t *indptr, int32_t *indices, void *values, void *stream)
{
    return csr_cbind("mxd_csr_cbind_shift", nX, nY, Xp, Xj, Xx, Yp, Yj, Yx, ncolX, value_dtype, nnz_total, indptr,
                     indices, values, stream);
}

// Appends one operand of an rbind at (row_offset, entry_offset) of the output arrays.
// in_kind: 0 dgRMatrix, 1 lgRMatrix, 2 ngRMatrix, 3 dsparseVector, 4 isparseVector, 5 lsparseVector,
// 6 nsparseVector (vectors: 1-based indices, one row, indptr_in ignored); out_kind 0 dgR, 1 lgR, 2 ngR.
// out_indptr[row_offset] must already hold entry_offset (out_indptr[0] = 0 is written when row_offset == 0).
extern "C" int mxd_csr_rbind_append(int in_kind, const int32_t *indptr_in, const int32_t *indices_in, const void *values_in,
                                    int nrows_in, int64_t nnz_in, int out_kind, int row_offset, int64_t entry_offset,
                                    int32_t *out_indptr, int32_t *out_indices, void *out_values, void *stream)
{
    MX_REQUIRE(in_kind >= 0 && in_kind <= 6 && out_kind >= 0 && out_kind <= 2, "mxd_csr_rbind_append: bad kind");
    MX_REQUIRE(entry_offset + nnz_in <= (int64_t)INT_MAX, "rbind result exceeds R's int32 index range");
    hipStream_t st = mx::as_stream(stream);
    const bool vec = in_kind >= 3;
    if (row_offset == 0) MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t), st));
    if (vec) {
        hipLaunchKernelGGL(mx::indptr_end_kernel, dim3(1), dim3(1), 0, st, out_indptr + row_offset + 1,
                           (int32_t)(entry_offset + nnz_in));
        MX_LAUNCH_CHECK();
    } else if (nrows_in > 0) {
        hipLaunchKernelGGL(mx::indptr_offset_kernel, dim3((unsigned)mx::ceil_div(nrows_in, 256)), dim3(256), 0, st,
                           indptr_in + 1, nrows_in, (int)entry_offset, out_indptr + row_offset + 1);
        MX_LAUNCH_CHECK();
    }
    if (nnz_in == 0) return 0;
    const unsigned grid = (unsigned)(mx::ceil_div(nnz_in, 256) < 4096 ? mx::ceil_div(nnz_in, 256) : 4096);
    int32_t *jo = out_indices + entry_offset;
    const int add = vec ? -1 : 0;
    const int vin = mx::concat_value_kind(in_kind);
    void *vo = out_kind == 0 ? (void *)((double *)out_values + entry_offset)
             : out_kind == 1 ? (void *)((int32_t *)out_values + entry_offset) : nullptr;
    const char *what = "mxd_csr_rbind_append";
    return mx::dispatch_int(mx::int_list<0, 1, 2>{}, what, "output kind", out_kind, [&](auto out) {
        return mx::dispatch_int(mx::int_list<0, 1, 4, 2>{}, what, "input value kind", vin, [&](auto in) {
            hipLaunchKernelGGL((mx::concat_entries_kernel<in(), out()>), dim3(grid), dim3(256), 0, st, nnz_in,
                               indices_in, values_in, add, jo, vo);
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
}

// The whole rbind in two launches: items_dev[n_items] (device memory) holds every operand with its offsets, which
// the caller has summed (row_offset / entry_offset are exclusive prefix sums of the rows / entries, in order).
extern "C" int mxd_csr_rbind_batch(const mx_rbind_item *items_dev, int n_items, int out_kind, int nrows_out,
                                   int64_t nnz_out, int32_t *out_indptr, int32_t *out_indices, void *out_values,
                                   void *stream)
{
    const char *what = "mxd_csr_rbind_batch";
    MX_REQUIRE(n_items >= 0 && nrows_out >= 0 && nnz_out >= 0 && out_indptr, "%s: bad arguments", what);
    MX_REQUIRE(n_items > 0 || (nrows_out == 0 && nnz_out == 0), "%s: rows or entries without operands", what);
    MX_REQUIRE(n_items == 0 || items_dev, "%s: null table", what);
    MX_REQUIRE(nnz_out == 0 || out_indices, "%s: null output", what);
    MX_REQUIRE(nnz_out <= (int64_t)INT_MAX, "rbind result exceeds R's int32 index range");
    hipStream_t st = mx::as_stream(stream);
    hipLaunchKernelGGL(mx::rbind_indptr_kernel, dim3(mx::grid_for(nrows_out, mx::RBIND_BLOCK)), dim3(mx::RBIND_BLOCK),
                       0, st, items_dev, n_items, nrows_out, out_indptr);
    MX_LAUNCH_CHECK();
    if (nnz_out == 0) return 0;
    return mx::dispatch_int(mx::int_list<0, 1, 2>{}, what, "output kind", out_kind, [&](auto out) {
        hipLaunchKernelGGL((mx::rbind_entries_kernel<out()>), dim3(mx::grid_for(nnz_out, mx::RBIND_TILE)),
                           dim3(mx::RBIND_BLOCK), 0, st, items_dev, n_items, nnz_out, out_indices, out_values);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

// Appends one operand of a COO rbind at entry_offset of the output triplets.  in_kind: 0 dgT, 1 lgT, 2 ngT
// (i_in / j_in 0-based), 3 / 4 / 5 / 6 d / i / l / n sparseVector (i_in ignored, j_in 1-based, the one row
// row_offset); out_kind 0 dgT, 1 lgT, 2 ngT.
extern "C" int mxd_coo_rbind_append(int in_kind, const int32_t *i_in, const int32_t *j_in, const void *values_in,
                                    int64_t nnz_in, int out_kind, int row_offset, int64_t entry_offset,
                                    int32_t *out_i, int32_t *out_j, void *out_values, void *stream)
{
    const char *what = "mxd_coo_rbind_append";
    MX_REQUIRE(in_kind >= 0 && in_kind <= 6 && out_kind >= 0 && out_kind <= 2, "%s: bad kind", what);
    MX_REQUIRE(nnz_in >= 0 && entry_offset >= 0 && row_offset >= 0, "%s: negative size", what);
    MX_REQUIRE(entry_offset + nnz_in <= (int64_t)INT_MAX, "rbind result exceeds R's int32 index range");
    if (nnz_in == 0) return 0;
    hipStream_t st = mx::as_stream(stream);
    void *vo = out_kind == 0 ? (void *)((double *)out_values + entry_offset)
             : out_kind == 1 ? (void *)((int32_t *)out_values + entry_offset) : nullptr;
    return mx::dispatch_int(mx::int_list<0, 1, 2>{}, what, "output kind", out_kind, [&](auto out) {
        return mx::dispatch_int(mx::int_list<0, 1, 4, 2>{}, what, "input value kind", mx::concat_value_kind(in_kind),
                                [&](auto in) {
            hipLaunchKernelGGL((mx::coo_append_kernel<in(), out()>), dim3(mx::grid_for(nnz_in, 256, 4096)), dim3(256), 0,
                               st, nnz_in, i_in, j_in, values_in, in_kind >= 3, row_offset, out_i + entry_offset,
                               out_j + entry_offset, vo);
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
}

// cbind of a CSR (x_kind 0 dgR, 1 lgR, 2 ngR; nX rows, ncolX columns) and a sparse vector (v_kind 3 / 4 / 5 / 6,
// nv sorted 1-based indices below `length`) as one column: appended behind X's columns (first = 0) or put in front
// of them (first = 1).  max(nX, length) rows, Xp[nX] + nv entries, values converted as the rbind does.
extern "C" int mxd_csr_cbind_svec(int nX, int ncolX, const int32_t *Xp, const int32_t *Xj, const void *Xx, int x_kind,
                                  const int32_t *vi, const void *vx, int v_kind, int nv, int length, int first,
                                  int out_kind, int32_t *indptr, int32_t *indices, void *values, void *stream)
{
    const char *what = "mxd_csr_cbind_svec";
    MX_REQUIRE(nX >= 0 && ncolX >= 0 && nv >= 0 && length >= 0 && nv <= length, "%s: bad size", what);
    MX_REQUIRE(x_kind >= 0 && x_kind <= 2 && v_kind >= 3 && v_kind <= 6, "%s: bad kind", what);
    MX_REQUIRE(ncolX < INT_MAX, "cbind result exceeds R's int32 index range");
    hipStream_t st = mx::as_stream(stream);
    const int nrows = nX > length ? nX : length;
    if (nrows == 0) { MX_HIP(hipMemsetAsync(indptr, 0, sizeof(int32_t), st)); return 0; }
    return mx::dispatch_int(mx::int_list<0, 1, 2>{}, what, "output kind", out_kind, [&](auto out) {
        hipLaunchKernelGGL((mx::cbind_svec_kernel<out()>), dim3(mx::grid_for(nrows, mx::BIND_BLOCK / 8)),
                           dim3(mx::BIND_BLOCK), 0, st, nX, nrows, Xp, Xj, Xx, mx::concat_value_kind(x_kind), ncolX, vi,
                           vx, mx::concat_value_kind(v_kind), nv, first, indptr, indices, values);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

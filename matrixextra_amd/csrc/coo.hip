// coo.hip — CSR (.) COO elementwise product and logical AND, values from the CSR looked up per COO entry.
//
// Replaces:
//   multiply_csr_by_coo_elemwise<>     src/operators.cpp:572-671
//   multiply_csr_by_coo_elemwise       src/operators.cpp:673-696   (f64)
//   logicaland_csr_by_coo_elemwise     src/operators.cpp:698-720   (R logicals)
// One lane per COO entry.  An entry is considered when its value is non-zero or NaN (logical: non-zero, so NA
// counts) and its row and column fall inside X; then X[row, col] is found by binary search of X's row (rows
// sorted ascending, as the R caller establishes, R/operators.R:81-95).  The entry is kept when that value is
// non-zero or NaN, with x * y (or R's 3-valued AND) as its value.  Kept entries are compacted in COO input order
// by count -> scan -> fill, so a duplicated COO entry gives one output entry per occurrence.
// The reference tests only `row < nrow(X)` and `col < ncol(X)`; a negative index is skipped here as well, so no
// index is used to read outside X.
#include "mx_workspace.h"

namespace mx {

constexpr int CB_BLOCK = 256;

template <bool LOGICAL>
__device__ __forceinline__ bool cb_match(int m, int ncol, const int32_t *__restrict__ indptr,
                                         const int32_t *__restrict__ indices, const void *__restrict__ xvals,
                                         int r, int c, const void *__restrict__ yvals, int64_t k, double &xd, int &xl)
{
    if ((unsigned)r >= (unsigned)m || (unsigned)c >= (unsigned)ncol) return false;
    if (LOGICAL) {
        if (((const int32_t *)yvals)[k] == 0) return false;
    } else {
        const double y = ((const double *)yvals)[k];
        if (!(isnan(y) || y != 0)) return false;
    }
    const int s = indptr[r], e = indptr[r + 1];
    const int pos = s + lower_bound_dev(indices + s, e - s, c);
    if (pos >= e || indices[pos] != c) return false;
    if (LOGICAL) {
        xl = ((const int32_t *)xvals)[pos];
        return xl != 0;
    }
    xd = ((const double *)xvals)[pos];
    return isnan(xd) || xd != 0;
}

// counts[k] = 1 when COO entry k is kept
template <bool LOGICAL>
__global__ __launch_bounds__(CB_BLOCK)
void csr_by_coo_count_kernel(int m, int ncol, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                             const void *__restrict__ xvals, const int32_t *__restrict__ yrows,
                             const int32_t *__restrict__ ycols, const void *__restrict__ yvals, int64_t nnz_y,
                             int32_t *__restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz_y) return;
    double xd;
    int xl;
    counts[k] = cb_match<LOGICAL>(m, ncol, indptr, indices, xvals, yrows[k], ycols[k], yvals, k, xd, xl) ? 1 : 0;
}

// kept entries go to pos[k] (pos = exclusive scan of the counts, so pos[k+1] > pos[k] marks them)
template <bool LOGICAL>
__global__ __launch_bounds__(CB_BLOCK)
void csr_by_coo_fill_kernel(int m, int ncol, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                            const void *__restrict__ xvals, const int32_t *__restrict__ yrows,
                            const int32_t *__restrict__ ycols, const void *__restrict__ yvals, int64_t nnz_y,
                            const int32_t *__restrict__ pos, int32_t *__restrict__ out_rows,
                            int32_t *__restrict__ out_cols, void *__restrict__ out_vals)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz_y) return;
    const int q = pos[k];
    if (pos[k + 1] == q) return;
    const int r = yrows[k], c = ycols[k];
    double xd = 0;
    int xl = 0;
    (void)cb_match<LOGICAL>(m, ncol, indptr, indices, xvals, r, c, yvals, k, xd, xl);
    out_rows[q] = r;
    out_cols[q] = c;
    if (LOGICAL) ((int32_t *)out_vals)[q] = r_logical_and(xl, ((const int32_t *)yvals)[k]);
    else ((double *)out_vals)[q] = xd * ((const double *)yvals)[k];
}

using CbLayout = CountOffsetsLayout;         // per entry of y: its count, then its position in the output

}  // namespace mx

extern "C" size_t mxd_csr_by_coo_workspace_bytes(int64_t nnz_y) { return mx::CbLayout(nullptr, nnz_y).bytes; }

extern "C" int mxd_csr_by_coo_count(int logical, int m, int ncol, const int32_t *indptr, const int32_t *indices,
                                    const void *x_values, const int32_t *y_rows, const int32_t *y_cols,
                                    const void *y_values, int64_t nnz_y, void *workspace, int64_t *nnz_out_host,
                                    void *stream)
{
    MX_REQUIRE(m >= 0 && ncol >= 0 && nnz_y >= 0 && nnz_y <= INT_MAX, "mxd_csr_by_coo_count: bad size");
    MX_REQUIRE(nnz_out_host && (nnz_y == 0 || (y_rows && y_cols && y_values && workspace)),
               "mxd_csr_by_coo_count: null pointer");
    MX_REQUIRE(m == 0 || indptr, "mxd_csr_by_coo_count: null pointer");
    if (nnz_y == 0) { *nnz_out_host = 0; return 0; }
    hipStream_t st = mx::as_stream(stream);
    const mx::CbLayout L(workspace, nnz_y);
    int32_t *counts = L.counts;
    const unsigned g = (unsigned)mx::ceil_div(nnz_y, mx::CB_BLOCK);
    if (logical)
        hipLaunchKernelGGL(mx::csr_by_coo_count_kernel<true>, dim3(g), dim3(mx::CB_BLOCK), 0, st, m, ncol, indptr,
                           indices, x_values, y_rows, y_cols, y_values, nnz_y, counts);
    else
        hipLaunchKernelGGL(mx::csr_by_coo_count_kernel<false>, dim3(g), dim3(mx::CB_BLOCK), 0, st, m, ncol, indptr,
                           indices, x_values, y_rows, y_cols, y_values, nnz_y, counts);
    MX_LAUNCH_CHECK();
    return mx::finish_count(nnz_y, L.counts, L.offsets, nnz_out_host, st);
}

extern "C" int mxd_csr_by_coo_fill(int logical, int m, int ncol, const int32_t *indptr, const int32_t *indices,
                                   const void *x_values, const int32_t *y_rows, const int32_t *y_cols,
                                   const void *y_values, int64_t nnz_y, const void *workspace, int32_t *out_rows,
                                   int32_t *out_cols, void *out_values, void *stream)
{
    MX_REQUIRE(m >= 0 && ncol >= 0 && nnz_y >= 0 && nnz_y <= INT_MAX, "mxd_csr_by_coo_fill: bad size");
    if (nnz_y == 0) return 0;
    MX_REQUIRE(y_rows && y_cols && y_values && workspace, "mxd_csr_by_coo_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const int32_t *pos = mx::CbLayout(workspace, nnz_y).offsets;
    const unsigned g = (unsigned)mx::ceil_div(nnz_y, mx::CB_BLOCK);
    if (logical)
        hipLaunchKernelGGL(mx::csr_by_coo_fill_kernel<true>, dim3(g), dim3(mx::CB_BLOCK), 0, st, m, ncol, indptr,
                           indices, x_values, y_rows, y_cols, y_values, nnz_y, pos, out_rows, out_cols, out_values);
    else
        hipLaunchKernelGGL(mx::csr_by_coo_fill_kernel<false>, dim3(g), dim3(mx::CB_BLOCK), 0, st, m, ncol, indptr,
                           indices, x_values, y_rows, y_cols, y_values, nnz_y, pos, out_rows, out_cols, out_values);
    MX_LAUNCH_CHECK();
    return 0;
}

// CSR (op) dense vector with R's recycling rules — values-only transforms (second half).
//
// Replaces:
//   multiply_csr_by_dvec_no_NAs<>            src/operators.cpp:1604-2140   (* ^ / %% %/% with X on either side)
//   multiply_csr_by_dvec_no_NAs_numeric      src/operators.cpp:2142-2175
//   logicaland_csr_by_dvec_internal          src/operators.cpp:2177-2200
// The reference has four branches for the length of the vector (== nrows :1640, >= nrows*ncols :1773,
// divides nrows :1870, anything else :2033); all four read dvec[(row + col*nrows) mod length]
// (`recyle_pos`, :1478), which is what the kernel computes — per row when the position does not depend on the
// column, without the modulo when the vector covers the whole matrix, with a 64-bit modulo otherwise.
// R's arithmetic (R_pow, R_modulus = %%, R_intdiv = %/%, :1482-1590) is restated for the device; where the
// reference carries an intermediate in `long double` (x87, 64-bit mantissa) the device uses one fused
// multiply-add (exact product, one rounding): results agree to the last bit or two, not always bit for bit.
// The structure-changing route (multiply_csr_by_dvec_with_NAs, :2258-) is dvecna.hip; the arithmetic both share is
// mx_rarith.h.
//
// The COO twin (multiply_coo_by_dense_ignore_NAs_{numeric,logical}, :2856-3425, same four branches) runs the
// same arithmetic and the same recycling position with the row read from i[k]: one lane per entry.
#include "mx_dispatch.h"
#include "mx_rarith.h"

namespace mx {

constexpr int DV_BLOCK = 256;

// recycling position of entry (row, col): MODE 0 rowpos, 1 row + col*nrows, 2 (row + col*nrows) mod len
__device__ __forceinline__ unsigned long long dv_pos(int mode, unsigned long long row, unsigned long long col,
                                                    unsigned long long nr, unsigned long long len,
                                                    unsigned long long rowpos)
{
    if (mode == 1) return row + nr * col;
    if (mode == 2) return (row + nr * col) % len;
    return rowpos;
}

template <bool LOGICAL>
__device__ __forceinline__ void dv_store(int op, bool lhs, const void *__restrict__ values, const void *__restrict__ dvec,
                                         unsigned long long at, int64_t k, void *__restrict__ out)
{
    if constexpr (LOGICAL)
        ((int32_t *)out)[k] = r_logical_and(((const int32_t *)values)[k], ((const int32_t *)dvec)[at]);
    else
        ((double *)out)[k] = dv_apply(op, lhs, ((const double *)values)[k], ((const double *)dvec)[at]);
}

// MODE 0: position depends on the row only (length == nrows, or length divides nrows); 1: the vector covers the
// matrix (row + col*nrows, no wrap); 2: general recycling, 64-bit modulo per entry.
template <int G, bool LOGICAL>
__global__ __launch_bounds__(DV_BLOCK)
void csr_by_dvec_kernel(int m, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                        const void *__restrict__ values, const void *__restrict__ dvec, unsigned long long len,
                        int mode, int op, int lhs, void *__restrict__ out)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (DV_BLOCK / G) + threadIdx.x / G;
    if (row >= m) return;
    const int s = indptr[row], e = indptr[row + 1];
    const unsigned long long nr = (unsigned long long)m;
    const unsigned long long rowpos = mode == 0 ? (unsigned long long)row % len : 0ULL;
    for (int k = s + lg; k < e; k += G) {
        const unsigned long long at = mode == 0 ? rowpos
                                                : dv_pos(mode, (unsigned long long)row, (unsigned long long)indices[k],
                                                         nr, len, rowpos);
        dv_store<LOGICAL>(op, lhs != 0, values, dvec, at, k, out);
    }
}

// COO: one lane per entry.  Indices are read as unsigned and a position past the vector wraps, so an entry outside
// the matrix never reads outside dvec (the R caller passes valid triplets).
template <bool LOGICAL>
__global__ __launch_bounds__(DV_BLOCK)
void coo_by_dvec_kernel(int m, int64_t nnz, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                        const void *__restrict__ values, const void *__restrict__ dvec, unsigned long long len,
                        int mode, int op, int lhs, void *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (k >= nnz) return;
    const unsigned long long row = (unsigned)rows[k];
    unsigned long long at = dv_pos(mode, row, (unsigned)cols[k], (unsigned long long)m, len, row % len);
    if (at >= len) at %= len;
    dv_store<LOGICAL>(op, lhs != 0, values, dvec, at, k, out);
}

// the reference's length branches (operators.cpp:1640,1773,1870,2033 / :2903-) reduce to three position rules
static int dv_mode(int m, int ncols, unsigned long long len)
{
    if (len == (unsigned long long)m || (len < (unsigned long long)m && (unsigned long long)m % len == 0)) return 0;
    if (len >= (unsigned long long)m * (unsigned long long)ncols) return 1;
    return 2;
}

}  // namespace mx

extern "C" int mxd_csr_by_dvec(int m, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                               const void *values, const void *dvec, int64_t dvec_len, int op, int x_is_lhs,
                               void *values_out, void *stream)
{
    MX_REQUIRE(m >= 0 && ncols >= 0 && dvec_len >= 0, "mxd_csr_by_dvec: negative size");
    MX_REQUIRE(op >= MX_DV_MULTIPLY && op <= MX_DV_LOGICAL_AND, "mxd_csr_by_dvec: unknown operation %d", op);
    if (m == 0 || nnz == 0) return 0;
    MX_REQUIRE(dvec_len > 0, "mxd_csr_by_dvec: empty vector");       // the R caller returns early (R/operators.R:961-966)
    MX_REQUIRE(indptr && indices && values && dvec && values_out, "mxd_csr_by_dvec: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const unsigned long long len = (unsigned long long)dvec_len;
    const int mode = mx::dv_mode(m, ncols, len);
    const int G = nnz < 0 ? 32 : mx::pick_group((double)nnz / (double)m);
    return mx::dispatch_int(mx::int_list<1, 0>{}, "mxd_csr_by_dvec", "logical", op == MX_DV_LOGICAL_AND, [&](auto lgl) {
        return mx::launch_rows(mx::lane_groups{}, "mxd_csr_by_dvec", G, m, mx::DV_BLOCK,
                               [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::csr_by_dvec_kernel<g(), lgl() != 0>), grid, block, 0, st, m, indptr, indices,
                               values, dvec, len, mode, op, x_is_lhs, values_out);
        });
    });
}

extern "C" int mxd_coo_by_dvec(int m, int ncols, int64_t nnz, const int32_t *rows, const int32_t *cols,
                               const void *values, const void *dvec, int64_t dvec_len, int op, int x_is_lhs,
                               void *values_out, void *stream)
{
    MX_REQUIRE(m >= 0 && ncols >= 0 && nnz >= 0 && dvec_len >= 0, "mxd_coo_by_dvec: negative size");
    MX_REQUIRE(op >= MX_DV_MULTIPLY && op <= MX_DV_LOGICAL_AND, "mxd_coo_by_dvec: unknown operation %d", op);
    if (nnz == 0) return 0;
    MX_REQUIRE(dvec_len > 0, "mxd_coo_by_dvec: empty vector");
    MX_REQUIRE(rows && cols && values && dvec && values_out, "mxd_coo_by_dvec: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const unsigned long long len = (unsigned long long)dvec_len;
    const int mode = mx::dv_mode(m, ncols, len);
    const unsigned g = (unsigned)mx::ceil_div(nnz, mx::DV_BLOCK);
    if (op == MX_DV_LOGICAL_AND)
        hipLaunchKernelGGL(mx::coo_by_dvec_kernel<true>, dim3(g), dim3(mx::DV_BLOCK), 0, st, m, nnz, rows, cols,
                           values, dvec, len, mode, op, x_is_lhs, values_out);
    else
        hipLaunchKernelGGL(mx::coo_by_dvec_kernel<false>, dim3(g), dim3(mx::DV_BLOCK), 0, st, m, nnz, rows, cols,
                           values, dvec, len, mode, op, x_is_lhs, values_out);
    MX_LAUNCH_CHECK();
    return 0;
}

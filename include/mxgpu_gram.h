/* mxgpu_gram.h — the one-triangle sparse x sparse product of libmxgpu.so's C-ABI: the upper or the lower triangle of
 * C = A B for two CSR matrices, and on it the Gram products X X^T and X^T X as a symmetric matrix that stores one
 * triangle.
 *
 * Same two layers and the same rules as mxgpu.h (mx_* export level on HOST pointers, synchronous; mxd_* device level on
 * DEVICE pointers and a caller-supplied stream, passed last as void*; 0 on success, the message through
 * mx_last_error()).  The family has a header of its own so that the sets of prototypes in mxgpu.h, mxgpu_reduce.h,
 * mxgpu_sym.h, mxgpu_tprod.h and mxgpu_spgemm.h stay what they are; matrixextra_amd/_lib.py reads all of them with the
 * same parser and binds them on the one library.
 *
 * What it stands for in the reference: crossprod(X) and tcrossprod(X) of a sparse X, which MatrixExtra leaves to Matrix
 * and Matrix answers with a dsCMatrix.
 *
 * The product is that of mxgpu_spgemm.h, restricted to a triangle.  `uplo` is an mx_uplo
 * (mxgpu_sym.h); any other value is refused.
 *   keep     MX_UPLO_UPPER keeps the product for cell (i, j) when j >= i, MX_UPLO_LOWER when j <= i, for any m x n:
 *            nothing requires a square result.  A product outside the triangle is never inserted, so the result is the
 *            triangle of the full product bit for bit: every cell is folded on its own, in the order mxgpu_spgemm.h
 *            defines.
 *   window   row i can hold w_i = max(0, n - i) (upper) or min(i + 1, n) (lower) columns; its bound is
 *            ub_i = min(f_i, w_i), and the bins of mxd_csr_spgemm_limits are chosen from that bound.
 *   b_sorted a promise by the caller that every row of B is ascending.  With it the row of B behind each entry of A is
 *            trimmed to the window by a binary search before any of it is read (upper: from the first column >= i,
 *            lower: up to the last column <= i), a step without a column in the window is skipped, and f_i counts the
 *            trimmed lengths.  Without it (b_sorted = 0) nothing is trimmed and the keep rule alone decides.  When B is
 *            in fact sorted both give the same bits.  A promise that does not hold loses entries; it stays in bounds.
 * Values, explicit zeros, the sorted unique rows of C, columns out of range and the operands' rules are those of
 * mxd_csr_spgemm_count / _fill.  The workspace is mxd_csr_spgemm_workspace_bytes(m, n), the bin edges
 * mxd_csr_spgemm_limits(m, n).  No atomic touches a value; the operands are never written.
 */
#ifndef MXGPU_GRAM_H
#define MXGPU_GRAM_H

#include "mxgpu_spgemm.h"
#include "mxgpu_sym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ========================================================================== */
/* device level                                                               */
/* ========================================================================== */

/* The count pass of the triangle `uplo` of C = A B: out_indptr[0 .. m] (out_indptr[m] = nnz_out), nnz_out in
 * *nnz_out_host and in *products_host what the bounds pass counted: every product of the rows when b_sorted = 0, the
 * products inside the window when b_sorted != 0 (either may be null; without both nothing is read back).  A row whose
 * window is empty, or none of whose products lies in the triangle, gets count 0.  A result with more than INT32_MAX
 * entries is an error, reported here; both totals are set all the same.  Every out_indptr cell is written.  The
 * workspace keeps the bins for the fill.
 * One synchronisation: the two totals are read back together. */
int mxd_csr_spgemm_tri_count(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, int64_t nnzA, const int32_t *Bp,
                             const int32_t *Bj, int64_t nnzB, int uplo, int b_sorted, int32_t *out_indptr,
                             void *workspace, int64_t *products_host, int64_t *nnz_out_host, void *stream);

/* The fill pass, behind mxd_csr_spgemm_tri_count on the same operands, uplo, b_sorted, out_indptr and workspace (assumed,
 * not checked): out_indices and out_values[nnz_out], rows sorted.  a_dtype / b_dtype: MX_F64, MX_LGL or MX_NONE
 * (Ax / Bx unread).
 * Enqueues and returns: no synchronisation. */
int mxd_csr_spgemm_tri_fill(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, const void *Ax, int a_dtype,
                            const int32_t *Bp, const int32_t *Bj, const void *Bx, int b_dtype, int uplo, int b_sorted,
                            const int32_t *out_indptr, int32_t *out_indices, double *out_values, void *workspace,
                            void *stream);

/* ========================================================================== */
/* export level                                                               */
/* ========================================================================== */

/* The triangle `uplo` of the Gram product of an nrow x ncol CSR X on host pointers: X X^T (nrow x nrow) for trans = 0,
 * X^T X (ncol x ncol) otherwise.  One upload and one transpose on the device (mxd_csr_column_order +
 * mxd_csr_transpose_by_order), which is the right-hand operand for trans = 0 (sorted by construction: b_sorted = 1) and
 * the left-hand one otherwise (b_sorted then comes from mxd_csr_rows_sorted on the upload); count, fill; the result is
 * taken with mx_result_finish (f64 values).  X must not repeat a cell inside a row.  With sorted rows of X the result is
 * the stored triangle of a symmetric matrix whose other triangle the full product holds bit for bit. */
int mx_csr_gram_begin(const int32_t *indptr, int nrow, int ncol, const int32_t *indices, const void *values,
                      int value_dtype, int trans, int uplo, mx_result **res, mx_result_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_GRAM_H */

/* mxgpu_spgemm.h — the sparse x sparse product family of libmxgpu.so's C-ABI: C = A B for two CSR matrices, by rows
 * (Gustavson), as a count pass and a fill pass.
 *
 * Same two layers and the same rules as mxgpu.h (mx_* export level on HOST pointers, synchronous; mxd_* device level on
 * DEVICE pointers and a caller-supplied stream, passed last as void*; 0 on success, the message through
 * mx_last_error()).  The family has a header of its own so that the sets of prototypes in mxgpu.h, mxgpu_reduce.h,
 * mxgpu_sym.h and mxgpu_tprod.h stay what they are; matrixextra_amd/_lib.py reads all of them with the same parser and
 * binds them on the one library.
 *
 * What it stands for in the reference: X %*% Y, crossprod(X), crossprod(X, Y) and tcrossprod(X, Y) with both operands
 * sparse, which MatrixExtra leaves to Matrix (R/matmul.R registers none of these signatures).
 *
 * The product.  A is m x K, B is K x n, both CSR with int32 indptr / indices.
 *   values   a_dtype / b_dtype, per operand: MX_F64 is read as is, MX_LGL as a double (NA_LOGICAL -> NA_real_, FALSE
 *            -> 0, anything else -> 1), MX_NONE reads every entry as 1.0.  The result's values are f64.
 *   pattern  row i of C stores column j exactly when some entry (i, k) of A and some entry (k, j) of B are stored.
 *            Nothing is dropped: a sum that cancels to 0, and a product with a stored 0 or FALSE, stay as explicit
 *            entries.  The rows of C are sorted ascending and their columns unique.
 *   order    for q = Ap[i] .. Ap[i + 1] - 1 in storage order, k = Aj[q], every stored (k, j, b) of B gives
 *            t = fl(a_q * b), rounded on its own (never fused into an addition).  C[i, j] is the first such t as it is
 *            (a lone -0.0 stays -0.0), then C[i, j] = fl(C[i, j] + t) for every later one.  NaN and Inf propagate.
 *   operands A's rows may be unsorted and may repeat a column: repeats are further terms, in storage order.  B's rows
 *            must have unique columns, in any order (assumed, not checked).  An A column outside [0, K) contributes
 *            nothing and a B column outside [0, n) is skipped; both stay in bounds.
 * No atomic touches a value (integer atomics on hash keys, bitmaps and list lengths only): repeated calls give the same
 * bits.  The operands are never written.
 */
#ifndef MXGPU_SPGEMM_H
#define MXGPU_SPGEMM_H

#include "mxgpu_tprod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ========================================================================== */
/* device level                                                               */
/* ========================================================================== */

/* Bytes of the workspace both passes share: the count block, a header (totals, entry counts, list lengths), the
 * per-row bounds, one row list per bin and the dense accumulators (dense_groups x (n f64 cells + a ceil(n / 32)-word
 * bitmap)), which are reserved only when n is above the lds_ub of mxd_csr_spgemm_limits: a row's bound never exceeds n,
 * so no row reaches the dense bin otherwise.  m, n >= 0. */
size_t mxd_csr_spgemm_workspace_bytes(int m, int n);

/* The bin edges for an m x n result: with f_i the number of products of row i and ub_i = min(f_i, n), a row with
 * 0 < ub_i <= *group_ub is taken by a lane group with a table of its own in LDS, one with ub_i <= *lds_ub by a
 * workgroup with one LDS table, any other by one of *dense_groups workgroups with a dense accumulator in the
 * workspace (*dense_groups >= 1).  Any of the three pointers may be null.  Host only: no synchronisation. */
int mxd_csr_spgemm_limits(int m, int n, int *group_ub, int *lds_ub, int *dense_groups);

/* The count pass: out_indptr[0 .. m] of C = A B (out_indptr[m] = nnz_out), the number of products in *products_host
 * and nnz_out in *nnz_out_host (either may be null; without both nothing is read back).  The per-row product counts
 * and their total are 64-bit and cannot wrap.  A result with more than INT32_MAX entries is an error, reported here,
 * before anything is allocated for the fill; *products_host and *nnz_out_host are set all the same.  m = 0, nnzA = 0
 * and nnzB = 0 give an empty result; every out_indptr cell is written.  The workspace keeps the bins for the fill.
 * One synchronisation: the two totals are read back together. */
int mxd_csr_spgemm_count(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, int64_t nnzA, const int32_t *Bp,
                         const int32_t *Bj, int64_t nnzB, int32_t *out_indptr, void *workspace, int64_t *products_host,
                         int64_t *nnz_out_host, void *stream);

/* The fill pass, behind mxd_csr_spgemm_count on the same operands, out_indptr and workspace: out_indices and
 * out_values[nnz_out], rows sorted.  a_dtype / b_dtype: MX_F64, MX_LGL or MX_NONE (Ax / Bx unread).
 * Enqueues and returns: no synchronisation. */
int mxd_csr_spgemm_fill(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, const void *Ax, int a_dtype,
                        const int32_t *Bp, const int32_t *Bj, const void *Bx, int b_dtype, const int32_t *out_indptr,
                        int32_t *out_indices, double *out_values, void *workspace, void *stream);

/* ========================================================================== */
/* export level                                                               */
/* ========================================================================== */

/* C = op(A) op(B) for an m x K CSR A and a K2 x n CSR B on host pointers, op(X) = X^T where trans_a / trans_b is
 * non-zero: one upload, the transposes on the device (mxd_csr_column_order + mxd_csr_transpose_by_order: rows sorted,
 * no second sort), count, fill; the result is taken with mx_result_finish (f64 values).  The inner dimensions are
 * checked after the transposes.  An operand that is transposed must not repeat a cell when it is the right-hand one. */
int mx_csr_spgemm_begin(const int32_t *Ap, int m, int K, const int32_t *Aj, const void *Ax, int a_dtype, int trans_a,
                        const int32_t *Bp, int K2, int n, const int32_t *Bj, const void *Bx, int b_dtype, int trans_b,
                        mx_result **res, mx_result_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_SPGEMM_H */

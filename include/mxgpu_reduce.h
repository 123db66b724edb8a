/* mxgpu_reduce.h — the reduction family of libmxgpu.so's C-ABI: row and column
 * sums and means, norm() and diag() of a CSR / CSC matrix.
 *
 * Same two layers and the same rules as mxgpu.h (mx_* export level on HOST
 * pointers, synchronous; mxd_* device level on DEVICE pointers and a
 * caller-supplied stream, passed last as void*; 0 on success, the message
 * through mx_last_error()).  The family has a header of its own so that the
 * set of prototypes in mxgpu.h, which the .Call shim and its generated fake
 * are built from, stays what it is; matrixextra_amd/_lib.py reads both files
 * with the same parser and binds both on the one library.
 *
 * What it stands for in the reference:
 *   colMeans(X * v), the gradient of vignettes/Introducing_MatrixExtra.Rmd:454-470
 *   norm / diag of an RsparseMatrix, R/csr_linalg.R (norm_csr :13-31)
 *   rowSums / colSums / rowMeans / colMeans, which MatrixExtra leaves to Matrix
 */
#ifndef MXGPU_REDUCE_H
#define MXGPU_REDUCE_H

#include "mxgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what a segment is reduced with; f is applied to each entry first */
typedef enum {
    MX_RED_SUM = 0,      /* sum of x                      rowSums / colSums          */
    MX_RED_ABS_SUM = 1,  /* sum of |x|                    norm "O" / "I" (margins)   */
    MX_RED_SQ_SUM = 2,   /* sum of x * x                  norm "F" (before the sqrt) */
    MX_RED_ABS_MAX = 3   /* largest |x|, NaN if any is    norm "M", last step of O/I */
} mx_reduce_op;

/* ========================================================================== */
/* device level                                                               */
/* ========================================================================== */

/* Segmented reduction over entries:
 *   out[s] = OP over q in [segptr[s], segptr[s + 1]) of f(values[perm ? perm[q] : q]),  s in [0, nseg)
 * values: nnz entries of value_dtype MX_F64, MX_LGL (TRUE = 1, a stored FALSE = 0, NA_LOGICAL = NA) or MX_NONE (unread:
 * every entry is 1); perm: nnz int32 positions in [0, nnz), or null; segptr: nseg + 1 non-decreasing int32 offsets
 * (a CSR indptr for the rows, the colptr of mxd_csr_column_order with its perm for the columns, {0, n} for a whole
 * array).  The part of a segment outside [0, nnz) is ignored.
 * The work is cut into tiles of 4096 entries, never by segment: a tile reduces the segments that lie inside it and
 * leaves the partial results of the segment it starts in the middle of and of the one it ends in the middle of in
 * `workspace`; a second launch adds those in tile order.  No atomics on values: repeated calls give the same bits.
 * Every out[s] is written; a segment without entries gives 0.  Totals are f64 whatever the values are.
 * NaN / NA: with na_rm = 0 any NaN or NA entry makes its segment NaN (MX_RED_ABS_MAX included); with na_rm != 0 such
 * entries are left out and, when skipped_out is not null, skipped_out[s] (int32[nseg]) receives how many were.  With
 * na_rm = 0 skipped_out, when given, is written with zeros.
 * workspace: 4 * mxd_compact_workspace_bytes(nnz) bytes (that function gives one slot per 4096-entry tile; a tile
 * carries two f64 partial results and two int32 counts).  Enqueues and returns: no synchronisation. */
int mxd_segment_reduce(int op, const void *values, int value_dtype, const int32_t *perm, int64_t nnz,
                       const int32_t *segptr, int nseg, int na_rm, double *out, int32_t *skipped_out,
                       void *workspace, void *stream);

/* Column order of a CSR pattern (m x n, nnz entries): perm_out[q] (int32[nnz]) is the row-major position of the q-th
 * entry in column-major order, rows ascending inside a column (the order is stable), and colptr_out (int32[n + 1])
 * the column pointer, so that column c is perm_out[colptr_out[c] .. colptr_out[c + 1]).  These are the radix passes of
 * mxd_csr_transpose without its gather of rows and values; values are not read, and the result serves every matrix
 * with the same indptr and indices.  A column index outside [0, n) fails the call as the transpose does (it is replaced
 * by 0 before it is used, so nothing is written out of bounds).  One synchronisation (the error flag).
 * workspace: mxd_csr_transpose_workspace_bytes(nnz). */
int mxd_csr_column_order(int m, int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int32_t *perm_out,
                         int32_t *colptr_out, void *workspace, void *stream);

/* diag(X) of an m x n CSR (R/csr_linalg.R, diag of an RsparseMatrix): out[k], k < min(m, n), is the value of the
 * first stored entry (k, k) in storage order, or 0 if there is none.  One lane group per row: a binary search of the
 * row when rows_sorted != 0 (pass it only when that is known, e.g. from mxd_csr_rows_sorted), a strided scan otherwise.
 * out: f64 for MX_F64; int32 R logicals for MX_LGL (NA_LOGICAL kept) and for MX_NONE (0 / 1).
 * Enqueues and returns: no synchronisation. */
int mxd_csr_diag(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values, int value_dtype,
                 int64_t nnz, int rows_sorted, void *out, void *stream);

/* ========================================================================== */
/* export level                                                               */
/* ========================================================================== */

/* rowSums / colSums / rowMeans / colMeans of an nrow x ncol CSR (value_dtype MX_F64, MX_LGL or MX_NONE; a CSC's
 * (p, i, x) with nrow and ncol swapped gives the other margin).  axis 0: one result per row, out f64[nrow]; axis 1:
 * one per column, out f64[ncol] (the column order is built first).  op is an mx_reduce_op.  mean != 0 divides each
 * result by the number of cells of its row (ncol) or column (nrow), less the entries na_rm skipped there: cells that
 * are not stored are zeros, not NAs, and a row in which every cell is a stored NA gives NaN. */
int mx_csr_margin_reduce(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                         int value_dtype, int axis, int op, int na_rm, int mean, double *out);

/* norm(X, type) of an nrow x ncol CSR, norm_csr of R/csr_linalg.R:13-31: type 'O' the largest column sum of |x|,
 * 'I' the largest row sum of |x|, 'F' sqrt(sum of x * x), 'M' the largest |x| (the mirror maps the other spellings
 * onto these four; "2" stays with Matrix).  The maximum over the margin sums is the same segmented reduction run as
 * one MX_RED_ABS_MAX segment.  A matrix without entries, or with a zero dimension, has norm 0; any NaN / NA that
 * contributes makes the result NaN.  *out receives the result. */
int mx_csr_norm(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                int value_dtype, int type, double *out);

/* diag(X) of an nrow x ncol CSR into out[min(nrow, ncol)]: f64 for MX_F64, int32 for MX_LGL and MX_NONE, as
 * mxd_csr_diag writes them.  Whether the rows are sorted is found on the device first (mxd_csr_rows_sorted). */
int mx_csr_diag(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                int value_dtype, void *out);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_REDUCE_H */

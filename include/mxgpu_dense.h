/* mxgpu_dense.h — the dense <-> compressed sparse conversions of libmxgpu.so's C-ABI: a dense matrix as CSR or CSC
 * arrays, and CSR or CSC arrays as a dense matrix.
 *
 * Same two layers and the same rules as mxgpu.h (mx_* export level on HOST pointers, synchronous; mxd_* device level on
 * DEVICE pointers and a caller-supplied stream, passed last as void*; 0 on success, the message through
 * mx_last_error()).  The family has a header of its own so that the sets of prototypes in mxgpu.h, mxgpu_reduce.h,
 * mxgpu_sym.h, mxgpu_tprod.h, mxgpu_spgemm.h and mxgpu_gram.h stay what they are; matrixextra_amd/_lib.py reads all of
 * them with the same parser and binds them on the one library.
 *
 * What it stands for in the reference: as.csr.matrix / as.csc.matrix / as.coo.matrix of a dense matrix
 * (R/conversions.R:180-295), which go through Matrix's coercions, and as.matrix() of a sparse matrix.
 *
 * The dense side is m x n, column-major, with leading dimension ld >= m counted in elements; the
 * cells of the padding rows [m, ld) of a column are never read and never written.  Every cell offset is 64-bit.
 *   by_col = 1   the compressed side is the CSC arrays: indptr[n + 1], index = row.  A segment (a column) is contiguous
 *                in the dense matrix.
 *   by_col = 0   the CSR arrays: indptr[m + 1], index = column.  A segment (a row) is strided by ld.
 * The CSR arrays of a ROW-major matrix are the CSC arrays of its transpose, which is column-major: both directions
 * serve a row-major matrix as the call with by_col = 1 and the roles of m and n swapped.
 *
 * dense -> compressed.  dense_dtype: MX_F64, MX_F32, MX_I32 or MX_LGL.
 *   keep     a cell is kept when it is not zero: x != 0, under which -0.0 is dropped and NaN, NA_real_, +-Inf,
 *            NA_integer_ and NA (logical) are kept.
 *   values   out_dtype MX_F64: an f64 keeps its bits (a NaN's payload included), an f32 is widened ((double)x), an
 *            integer or logical is (double)x with NA -> NA_real_.  MX_LGL: NaN / NA -> NA_LOGICAL, any other kept cell
 *            -> 1, and a logical input is copied.  MX_NONE: no values (a pattern).
 *   order    segments ascending, and inside a segment the index ascending: rows sorted, no cell twice.
 * No atomic is used and every write position comes from scanned counts: the same bits on every call.
 *
 * compressed -> dense.  value_dtype: MX_F64, MX_LGL or MX_NONE; out_dtype: MX_F64 (NA_LOGICAL -> NA_real_, a pattern
 * entry -> 1.0) or MX_LGL (int32; a NaN -> NA_LOGICAL, another f64 -> x != 0, a pattern entry -> 1).  Every cell of the
 * m x n output is stored exactly once, zero where the matrix stores nothing: one launch, no memset, no atomic.
 *   requires   the indices of every segment strictly ascending and inside [0, nother).  Every entry is checked against
 *              its predecessor and the bound in the same kernel; an offending entry is never used to write, *flag_dev
 *              becomes 1 and the content of `out` is then unspecified (inside its m x n cells).  The kernel never
 *              clears the flag: the caller zeroes it.
 *
 * col_splits (by_col = 0 only): the workgroups that share the columns of one panel of 64 rows, each sweeping a range
 * of 64-column chunks.  0 lets the library choose from the shape; a positive value (at most 4096) is taken as given.
 * The count and the fill of one conversion, and the workspace they share, take the same value.
 */
#ifndef MXGPU_DENSE_H
#define MXGPU_DENSE_H

#include "mxgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ========================================================================== */
/* device level                                                               */
/* ========================================================================== */

/* Bytes of the workspace that mxd_dense_to_csr_count fills and mxd_dense_to_csr_fill reads (0 for bad arguments).
 * Host arithmetic only: no device work, no synchronisation. */
size_t mxd_dense_to_csr_workspace_bytes(int m, int n, int by_col, int col_splits);

/* The count pass: out_indptr[0 .. nseg] with nseg = n (by_col) or m, out_indptr[nseg] = the number of kept cells, which
 * is also written to *nnz_host.  More than INT32_MAX kept cells is an error, reported here.  Every out_indptr cell is
 * written; with by_col = 1, or more than one split, the last kernel that writes it is enqueued behind the read-back, so
 * out_indptr is complete in stream order, not on return.  The workspace keeps the offsets for the fill.
 * One synchronisation: the total is read back. */
int mxd_dense_to_csr_count(int m, int n, const void *dense, int64_t ld, int dense_dtype, int by_col, int col_splits,
                           int32_t *out_indptr, void *workspace, int64_t *nnz_host, void *stream);

/* The fill pass, behind mxd_dense_to_csr_count on the same operand, by_col, col_splits, out_indptr and workspace
 * (assumed, not checked; a write position outside [0, out_indptr[nseg]) is skipped): out_indices and, unless out_dtype
 * is MX_NONE, out_values (double for MX_F64, int32 for MX_LGL), out_indptr[nseg] entries each.
 * Enqueues and returns: no synchronisation. */
int mxd_dense_to_csr_fill(int m, int n, const void *dense, int64_t ld, int dense_dtype, int by_col, int col_splits,
                          const int32_t *out_indptr, const void *workspace, int32_t *out_indices, void *out_values,
                          int out_dtype, void *stream);

/* Compressed -> dense: nseg segments (indptr[nseg + 1], entries indptr[nseg]) with indices in [0, nother); the output
 * is nother x nseg (by_col = 1) or nseg x nother (by_col = 0), column-major at `ld` (double for MX_F64, int32 for
 * MX_LGL).  flag_dev: one int32 on the device, zeroed by the caller, set to 1 when an entry offends (see above).
 * indices and values may be null only when there are no entries.  CSR -> row-major dense is this routine called with
 * by_col = 1 and the roles of m and n swapped (nseg = rows, nother = columns, ld = the row stride).
 * Enqueues and returns: no synchronisation. */
int mxd_csr_to_dense(int nseg, int nother, const int32_t *indptr, const int32_t *indices, const void *values,
                     int value_dtype, int by_col, int col_splits, void *out, int64_t ld, int out_dtype,
                     int32_t *flag_dev, void *stream);

/* ========================================================================== */
/* export level                                                               */
/* ========================================================================== */

/* A dense m x n column-major matrix (ld = m) on host pointers as CSR (by_col = 0) or CSC (by_col = 1) arrays: upload,
 * count, fill; the result is taken with mx_result_finish (values of out_dtype, none for MX_NONE). */
int mx_dense_to_csr_begin(const void *dense, int m, int n, int dense_dtype, int by_col, int out_dtype, mx_result **res,
                          mx_result_info *info);

/* CSR (by_col = 0) or CSC (by_col = 1) arrays on host pointers as a dense column-major matrix in out (ld = its row
 * count; nseg x nother, or nother x nseg with by_col).  When the kernel flags the arrays (unsorted or repeated indices)
 * they are normalised on the device through mxd_csr_to_coo + mxd_coo_to_csr, which merges repeated cells by that
 * routine's rules (f64 summed in storage order, logicals by R's `|`, a pattern once), and scattered again.  An index
 * outside [0, nother) fails the call. */
int mx_csr_to_dense(const int32_t *indptr, int nseg, int nother, const int32_t *indices, const void *values,
                    int value_dtype, int by_col, void *out, int out_dtype);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_DENSE_H */

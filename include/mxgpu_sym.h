/* mxgpu_sym.h — the structured-matrix family of libmxgpu.so's C-ABI: a symmetric CSR that stores one triangle, or a
 * unit-triangular CSR that leaves its diagonal out, expanded into the general CSR every other routine takes.
 *
 * Same two layers and the same rules as mxgpu.h (mx_* export level on HOST pointers, synchronous; mxd_* device level
 * on DEVICE pointers and a caller-supplied stream, passed last as void*; 0 on success, the message through
 * mx_last_error()).  Like mxgpu_reduce.h the family has a header of its own, so that the set of prototypes in mxgpu.h
 * stays what it is; matrixextra_amd/_lib.py reads it with the same parser and binds it on the one library.
 *
 * What it stands for in the reference: as.csr.matrix / as.csc.matrix / as.coo.matrix of a dsR / lsR / nsR / dtR / ltR /
 * ntR / dsC / dtC operand (R/conversions.R:180-295), which hand the expansion to Matrix's as(x, "generalMatrix").
 * Copies only, no arithmetic: every result is defined bit for bit.
 */
#ifndef MXGPU_SYM_H
#define MXGPU_SYM_H

#include "mxgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which triangle an operand stores (Matrix's `uplo` slot) */
typedef enum {
    MX_UPLO_UPPER = 0,   /* "U": every stored (r, c) has c >= r */
    MX_UPLO_LOWER = 1    /* "L": every stored (r, c) has c <= r */
} mx_uplo;

/* ========================================================================== */
/* device level                                                               */
/* ========================================================================== */

/* How many of the nnz entries of an n x n CSR lie outside the triangle `uplo` names (an mx_uplo); with strict != 0
 * entries on the diagonal count as well, as a unit-triangular operand (diag = "U") needs.  One lane group per row, an
 * integer counter in the workspace.  *outside_host receives the count.  One synchronisation (the read-back).
 * workspace: 16 bytes (any workspace of this family serves). */
int mxd_csr_triangle_check(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int uplo, int strict,
                           void *workspace, int64_t *outside_host, void *stream);

/* Symmetric expansion, count -> scan -> fill.  The input is an n x n CSR that stores the triangle `uplo`; the output is
 * the general CSR of the same symmetric matrix:
 *   uplo U: output row r = the MIRRORED segment, then the STORED row r in its storage order
 *   uplo L: output row r = the STORED row r, then the MIRRORED segment
 * where the mirrored segment of row r is every stored (c, r) with c != r, as (r, c), in ascending c and repeats in
 * storage order.  Sorted input rows give sorted output rows; explicit zeros, NaN payloads, -0.0, NA_LOGICAL and
 * repeated entries are copied as they are.
 *
 * _count writes out_indptr[0..n] (len[r] = row length + column length - stored (r, r) entries, scanned with
 * mxd_exclusive_scan_i32) and leaves in `workspace` what _fill reads: the column order of the pattern
 * (mxd_csr_column_order) and the row of every entry (the ids mxd_csr_to_coo gives, written by the pass over the rows
 * that counts).  *nnz_out_host receives out_indptr[n].  An entry in the wrong triangle fails the call ("... outside
 * the stored triangle"), as does a column outside [0, n) or a result of more than INT32_MAX entries; out_indptr is
 * then not to be used.
 * Two synchronisations: the column order's error flag, then one read-back of the wrong-triangle count and nnz_out.
 * workspace: mxd_csr_sym_workspace_bytes(n, nnz), untouched between _count and _fill. */
size_t mxd_csr_sym_workspace_bytes(int n, int64_t nnz);
int mxd_csr_symmetric_to_general_count(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int uplo,
                                       int32_t *out_indptr, void *workspace, int64_t *nnz_out_host, void *stream);

/* _fill writes out_indices[0..nnz_out) and, for value_dtype MX_F64 / MX_LGL, out_values[0..nnz_out) (MX_NONE: values
 * and out_values are not touched).  One lane group per output row, its width from the output's average row length:
 * the mirrored segment is gathered through the column order straight into place, the stored row is a contiguous copy.
 * The column's stored (r, r) entries are its last (U) or first (L) ones, because the column order is stable; how many
 * there are follows from out_indptr.  Nothing is written outside [0, nnz_out).  No atomics.
 * Enqueues and returns: no synchronisation. */
int mxd_csr_symmetric_to_general_fill(int n, const int32_t *indptr, const int32_t *indices, const void *values,
                                      int value_dtype, int64_t nnz, int uplo, const int32_t *out_indptr,
                                      int64_t nnz_out, int32_t *out_indices, void *out_values, const void *workspace,
                                      void *stream);

/* Unit-triangular expansion (diag = "U"): the n x n CSR stores the strict triangle `uplo`, the output gains (r, r) in
 * every row, in front of the stored row (U) or behind it (L), valued 1.0 (MX_F64) / TRUE (MX_LGL) / nothing
 * (MX_NONE).  out_indptr[r] = indptr[r] + r, out_indptr[n] = nnz + n: out_indptr has n + 1 entries, out_indices and
 * out_values nnz + n.  The input is not checked (mxd_csr_triangle_check with strict = 1 does that).
 * Enqueues and returns: no synchronisation. */
int mxd_csr_unit_triangular_to_general(int n, const int32_t *indptr, const int32_t *indices, const void *values,
                                       int value_dtype, int64_t nnz, int uplo, int32_t *out_indptr,
                                       int32_t *out_indices, void *out_values, void *stream);

/* ========================================================================== */
/* export level                                                               */
/* ========================================================================== */

/* as(x, "generalMatrix") of a dsR / lsR / nsR matrix (a dsC's (p, i, x) with uplo flipped): n x n, value_dtype MX_F64 /
 * MX_LGL / MX_NONE (or n_values 0: a pattern), the triangle `uplo`.  The result (n + 1 index pointers, nnz_out indices
 * and values) is taken with mx_result_finish. */
int mx_csr_symmetric_to_general_begin(const int32_t *indptr, int n, const int32_t *indices, const void *values,
                                      int value_dtype, int64_t n_values, int uplo, mx_result **res,
                                      mx_result_info *info);

/* as(x, "generalMatrix") of a dtR / ltR / ntR matrix with diag = "U": the strict triangle is checked first (an entry
 * on the diagonal or in the other triangle fails the call), then every row gains its unit diagonal. */
int mx_csr_unit_triangular_to_general_begin(const int32_t *indptr, int n, const int32_t *indices, const void *values,
                                            int value_dtype, int64_t n_values, int uplo, mx_result **res,
                                            mx_result_info *info);

/* *outside receives how many entries of the n x n CSR lie outside the triangle `uplo` (strict != 0: or on the
 * diagonal). */
int mx_csr_triangle_check(const int32_t *indptr, int n, const int32_t *indices, int uplo, int strict, int64_t *outside);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_SYM_H */

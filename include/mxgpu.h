/* mxgpu.h — C-ABI of libmxgpu.so, the MI355X (gfx950) backend for MatrixExtra's
 * CSR hot path.
 *
 * Two layers, both plain C (pointers + sizes, no torch / Rcpp / R types):
 *
 *  (1) mx_*   "export level": one entry point per Rcpp-exported routine of the
 *             reference's hot path (src/RcppExports.cpp CallEntries[] :2233-2242,
 *             :2290-2291, :2297-2298, :2333-2334, :2341-2343).  Arguments are
 *             HOST pointers with exactly the meaning of the reference's
 *             IntegerVector / NumericVector / NumericMatrix views; outputs are
 *             caller-allocated (fixed-size results) or obtained through a
 *             begin/finish pair (variable-size results, so that the caller —
 *             the R .Call shim — can allocate R vectors of the right length
 *             and have the D2H copy land directly in them).  Synchronous at
 *             return, as the reference is (SURVEY §8b "Threading").
 *
 *  (2) mxd_*  "device level": the same operations on DEVICE pointers, enqueued
 *             on a caller-supplied hipStream_t (passed as void*), no
 *             allocation, no synchronisation (graph-capture safe) except where
 *             a size must come back to the host.  This is what bench.py, the
 *             multi-GPU path and layer (1) drive.
 *
 * Every function returns 0 on success, non-zero on failure; the message for the
 * calling thread is read with mx_last_error() (the .Call shim turns it into
 * Rf_error, mirroring BEGIN_RCPP/END_RCPP at src/RcppExports.cpp:16,24).
 *
 * Index type is int32 (R INTSXP) throughout, as in the reference.
 * R's NA_INTEGER / NA_LOGICAL = INT_MIN; NA_REAL = NaN with low word 1954.
 */
#ifndef MXGPU_H
#define MXGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXGPU_ABI_VERSION 1

/* ---- status / device management ------------------------------------------ */
const char *mx_last_error(void);
int  mx_abi_version(void);
int  mx_device_count(int *count);
int  mx_set_device(int device);
int  mx_device_name(char *buf, size_t buflen);
/* raw device memory for callers that do not bring their own allocator */
int  mx_dev_malloc(void **dptr, size_t bytes);
int  mx_dev_free(void *dptr);
int  mx_dev_memset(void *dptr, int value, size_t bytes, void *stream);
int  mx_memcpy_h2d(void *dptr, const void *hptr, size_t bytes, void *stream);
int  mx_memcpy_d2h(void *hptr, const void *dptr, size_t bytes, void *stream);
int  mx_stream_sync(void *stream);
int  mx_host_register(void *hptr, size_t bytes);   /* pin caller memory for async H2D/D2H */
int  mx_host_unregister(void *hptr);

/* ---- element types --------------------------------------------------------- */
typedef enum {
    MX_F64 = 0,      /* double (R numeric)                                   */
    MX_F32 = 1,      /* float  (float32@Data INTSXP reinterpreted)           */
    MX_I32 = 2,      /* R integer, NA_INTEGER = INT_MIN                      */
    MX_LGL = 3,      /* R logical, {0,1,NA_LOGICAL}                          */
    MX_NONE = 4      /* no values (ngRMatrix)                                */
} mx_dtype;

typedef enum {
    MX_OP_ADD = 0,   /* add_csr_elemwise(substract=false)   operators.cpp:539 */
    MX_OP_SUB = 1,   /* add_csr_elemwise(substract=true)                      */
    MX_OP_MUL = 2,   /* multiply_csr_elemwise               operators.cpp:209 */
    MX_OP_OR  = 3,   /* logicalor_csr_elemwise(xor=false)   operators.cpp:556 */
    MX_OP_XOR = 4,   /* logicalor_csr_elemwise(xor=true)                      */
    MX_OP_AND = 5    /* logicaland_csr_elemwise             operators.cpp:224 */
} mx_merge_op;

/* ========================================================================== */
/* (2) device level                                                           */
/* ========================================================================== */

/* SpMM  C = A * B,  A CSR m x K (int32 indptr[m+1], indices[nnz], f64 values),
 * B row-major K x n with leading dimension ldb (elements), C m x n.
 *   colmajor_out = 0 : C row-major, leading dim ldc  (gemm_csr_drm_as_drm,
 *                      src/matmul.cpp:118-142; exports start from zeroed C so
 *                      "C += A*B" == "C = A*B")
 *   colmajor_out = 1 : C column-major, leading dim ldc (gemm_csr_drm_as_dcm,
 *                      src/matmul.cpp:150-185)
 * dense_dtype MX_F64 or MX_F32; CSR values are f64 in both (narrowed per
 * nonzero for MX_F32 as at src/matmul.cpp:53-57).  Column indices need not be
 * sorted; duplicates accumulate.  Rows with no entries give zeros. */
int mxd_spmm_csr_dense(int m, int n,
                       const int32_t *indptr, const int32_t *indices, const double *values,
                       const void *B, size_t ldb,
                       void *C, size_t ldc,
                       int dense_dtype, int colmajor_out, void *stream);

/* Same product with an explicit kernel choice.  K = number of rows of B (= ncol A).
 *   algo MX_SPMM_ROWWAVE : one wavefront per row x 1-KiB column chunk (any operands)
 *   algo MX_SPMM_SLAB    : 128-byte column slabs dealt to the XCDs + column panels sized to one XCD's L2,
 *                          accumulators in registers (needs 16-B aligned rows of B; npanels > 1 needs
 *                          rows sorted by column — pass rows_sorted = 1 only when that is known, e.g. from
 *                          mxd_csr_rows_sorted)
 *   algo MX_SPMM_PLANNED : build a plan (see mxd_spmm_plan_create below) and run the planned panel-sweep kernel;
 *                          the plan is rebuilt on every call here — hold a plan yourself to amortise it
 *   algo MX_SPMM_AUTO    : PLANNED when B is larger than an XCD's L2, the operands qualify and there is enough
 *                          work to fill the chip, else ROWWAVE
 * npanels <= 0 / wg_per_cu <= 0 pick defaults.  ROWWAVE and SLAB enqueue and return; PLANNED, and AUTO when it picks
 * PLANNED, synchronises once with the stream's work up to the plan's sizing pass, as mxd_spmm_plan_create does. */
typedef enum { MX_SPMM_AUTO = 0, MX_SPMM_ROWWAVE = 1, MX_SPMM_SLAB = 2, MX_SPMM_PLANNED = 3 } mx_spmm_algo;
int mxd_spmm_csr_dense_ex(int m, int n, int K,
                          const int32_t *indptr, const int32_t *indices, const double *values,
                          const void *B, size_t ldb, void *C, size_t ldc,
                          int dense_dtype, int colmajor_out, int algo, int rows_sorted,
                          int npanels, int wg_per_cu, void *stream);

/* Planned SpMM (v3): a device-resident regrouping of A's entries by (row bundle, column panel), wave-interleaved,
 * so that the panel-sweep kernel reads every entry once, coalesced, while B's current slab-panel stays in L2.
 * The plan depends on A and npanels only; build it once per matrix and run it against any number of B.
 * mxd_spmm_plan_create: *plan = NULL creates, a previous plan re-uses its buffers (grow-only); one internal
 * stream sync (the padded size comes back to the host).  npanels <= 0 picks K*128 B / 1.6 MB.
 * mxd_spmm_plan_run: sync_mode 0 = free running, 1 = the waves of a CU's workgroup meet at every panel boundary,
 * 2 = 1 + one timing barrier per generation among the workgroups of an XCD group; -1 = default (1).
 * Needs 16-B aligned rows of B (and of C when C is row-major).  wg_per_cu 1 / 2 / 4 = that many workgroups of
 * 16 / 8 / 4 wavefronts per CU (1024 / 512 / 256 rows per generation); any other value picks the default (1).
 * mxd_spmm_csr_dense_ex runs its plans with the defaults (wg_per_cu and sync_mode).
 * Streams: a plan's arrays are written on the stream given to mxd_spmm_plan_create, and the call returns once the sizes
 * are back, possibly before the fill has run: the plan is bound to the stream order of its creation.  Run it on that
 * stream, or on another one only after the creating stream has been synchronised.  mxd_spmm_plan_run itself enqueues
 * and returns; it packs B into scratch of the calling thread (see mxd_release_workspaces). */
typedef struct mx_spmm_plan mx_spmm_plan;
int mxd_spmm_plan_create(int m, int K, const int32_t *indptr, const int32_t *indices, const double *values,
                         int npanels, void *stream, mx_spmm_plan **plan);
int mxd_spmm_plan_destroy(mx_spmm_plan *plan);
int mxd_spmm_plan_info(const mx_spmm_plan *plan, int *npanels, int64_t *padded_entries);
/* Read-only copy of a built plan to host memory (tests): step_off[noct * npanels + 1] with noct = ceil(m / 64),
 * pcol[padded_entries + 512] (column | row inside the bundle << 27) and pval[padded_entries + 512]; synchronises. */
int mxd_spmm_plan_copy_to_host(const mx_spmm_plan *plan, int32_t *step_off, int32_t *pcol, double *pval, void *stream);
int mxd_spmm_plan_run(const mx_spmm_plan *plan, int n, const void *B, size_t ldb, void *C, size_t ldc,
                      int dense_dtype, int colmajor_out, int wg_per_cu, int sync_mode, void *stream);

/* AUTO's plan and the slab-major copy of B live in grow-only per-thread device buffers between calls; this frees them.
 * That scratch (the packed copy of B, the timing barrier's counters, AUTO's plan buffers, the ring of timing events)
 * is per host thread and per device, not per stream: every stream of one thread shares it.  So the SpMM calls of one
 * thread (mxd_spmm_csr_dense_ex, mxd_spmm_plan_run) must be ordered on one stream, or separated by a synchronisation;
 * two of them in flight on two streams of one thread would share the packed B and the plan.  Growth alone is safe:
 * every buffer grows through hipFree + hipMalloc, and hipFree waits for the whole device, so no kernel still reads a
 * buffer that is freed (a call that grows scratch is therefore not asynchronous; one of the same sizes before it is).
 * Different host threads never share scratch. */
int mxd_release_workspaces(void);

/* HIP-event timing of the dominant kernel of every SpMM launch of this thread (events recorded on the launch stream
 * right around that kernel): enable, run, then read the per-launch milliseconds (the read synchronises). */
int mxd_spmm_kernel_timing(int enable);
int mxd_spmm_kernel_times(float *out_ms, int max_out, int *count);

/* name of the SpMM kernel the last mxd_spmm_csr_dense_ex call of this thread launched (reporting only) */
const char *mxd_spmm_last_kernel(void);

/* label and lane-group width G (4, 8, 16, 32 or 64 lanes per row) of the last row-group kernel this thread launched:
 * SpMV, merge, gather, sort, column slices, cbind, CSR x / (.) vector.  "none" and 0 before the first one.  Either
 * pointer may be null (reporting only). */
int mxd_last_row_launch(const char **what, int *G);

/* SpMV  y = A * v  (matmul_csr_dvec<>, src/matmul.cpp:381-419).
 * v_dtype MX_F64 / MX_I32 / MX_LGL -> y f64[m];  MX_F32 -> y f32[m]
 * (float accumulate).  NA_INTEGER / NA_LOGICAL entries contribute NA_REAL. */
int mxd_spmv_csr_dvec(int m, int64_t nnz /* lanes-per-row hint, -1 = unknown */,
                      const int32_t *indptr, const int32_t *indices, const double *values,
                      const void *v, int v_dtype, void *y, void *stream);

/* CSR (+) CSR, pass 1: per-row output lengths (union for ADD/SUB/OR/XOR,
 * intersection for MUL/AND) then exclusive scan into out_indptr[m+1].
 * Rows must be sorted ascending with unique column ids (precondition the R
 * callers establish, R/operators.R:58,64,748,754).  workspace: mxd_merge_workspace_bytes(m).
 * *nnz_out_host (pinned or pageable host int64) is written after an internal
 * stream sync — the one host round trip of the operation.  nnz1 / nnz2 only
 * steer the lanes-per-row choice (pass -1 when unknown). */
size_t mxd_merge_workspace_bytes(int m);
int mxd_csr_merge_count(int op, int m,
                        const int32_t *indptr1, const int32_t *indices1, int64_t nnz1,
                        const int32_t *indptr2, const int32_t *indices2, int64_t nnz2,
                        int32_t *out_indptr, void *workspace,
                        int64_t *nnz_out_host, void *stream);
/* pass 2: fill out_indices / out_values (f64 for ADD/SUB/MUL, int32 R logical
 * for OR/XOR/AND) at the offsets in out_indptr. */
int mxd_csr_merge_fill(int op, int m,
                       const int32_t *indptr1, const int32_t *indices1, const void *values1, int64_t nnz1,
                       const int32_t *indptr2, const int32_t *indices2, const void *values2, int64_t nnz2,
                       const int32_t *out_indptr, int32_t *out_indices, void *out_values,
                       void *stream);
/* identical-pattern fast path (operators.cpp:104-132, :343-395): values only */
int mxd_values_elemwise(int op, int64_t nnz, const void *values1, const void *values2,
                        void *out_values, void *stream);

/* Row gather  out = A[rows_take, :]  (copy_csr_rows_template, src/slice.cpp:225-274)
 * pass 1: new_indptr[r+1] + total, *nnz_out_host written after an internal stream sync;  pass 2: copy.
 * value_dtype MX_F64 / MX_LGL / MX_NONE. */
size_t mxd_gather_workspace_bytes(int r);
int mxd_csr_gather_count(int r, const int32_t *indptr, const int32_t *rows_take,
                         int32_t *new_indptr, void *workspace,
                         int64_t *nnz_out_host, void *stream);
int mxd_csr_gather_fill(int r, const int32_t *indptr, const int32_t *indices, const void *values,
                        const int32_t *rows_take, const int32_t *new_indptr,
                        int32_t *new_indices, void *new_values, int value_dtype,
                        int64_t nnz_out /* lanes-per-row hint, -1 = unknown */, void *stream);

/* Column-filtering slices.  Same count -> scan -> fill shape as the row gather (each count
 * synchronises the stream once, for *nnz_out_host; the fills and mxd_colmap_build do not); workspace of
 * mxd_gather_workspace_bytes(r).  avg_row_len (mean entries per source row) only steers the lanes-per-row choice.
 *   colrange: keep min_col <= col <= max_col, re-based to min_col, input order kept; values come out as f64
 *             whatever the input kind (copy_csr_rows_col_seq_template, src/slice.cpp:326-383)
 *   colmap:   arbitrary selector through a dense map built by mxd_colmap_build: start[ncol_map+1], pos[n] with
 *             pos[start[c] .. start[c+1]) = ascending positions of column c in cols_take
 *             (copy_csr_arbitrary_template, src/slice.cpp:449-578; re-order rows afterwards with mxd_csr_sort_rows
 *             unless cols_take is non-decreasing) */
int mxd_csr_colrange_count(int r, const int32_t *indptr, const int32_t *indices, const int32_t *rows_take,
                           int min_col, int max_col, double avg_row_len, int32_t *new_indptr,
                           void *workspace, int64_t *nnz_out_host, void *stream);
int mxd_csr_colrange_fill(int r, const int32_t *indptr, const int32_t *indices, const void *values,
                          int value_dtype, const int32_t *rows_take, int min_col, int max_col,
                          double avg_row_len, const int32_t *new_indptr, int32_t *new_indices,
                          double *new_values, void *stream);
size_t mxd_colmap_workspace_bytes(int ncol_map);
int mxd_colmap_build(const int32_t *cols_take, int64_t n, int ncol_map, int32_t *start, int32_t *pos,
                     void *workspace, void *stream);
int mxd_csr_colmap_count(int r, const int32_t *indptr, const int32_t *indices, const int32_t *rows_take,
                         int ncol_map, const int32_t *start, double avg_row_len, int32_t *new_indptr,
                         void *workspace, int64_t *nnz_out_host, void *stream);
int mxd_csr_colmap_fill(int r, const int32_t *indptr, const int32_t *indices, const void *values,
                        int value_dtype, const int32_t *rows_take, int ncol_map, const int32_t *start,
                        const int32_t *pos, double avg_row_len, const int32_t *new_indptr,
                        int32_t *new_indices, void *new_values, void *stream);
/* col -> ncol-1-col and each row reversed, in place (reverse_columns_inplace, src/slice.cpp:142-170) */
int mxd_csr_reverse_columns(int m, int64_t nnz, const int32_t *indptr, int32_t *indices, void *values,
                            int value_dtype, int ncol, void *stream);
int mxd_reversed_iota(int n, int32_t *out, void *stream);   /* out[i] = n-1-i: row list of reverse_rows */

/* cbind / rbind.
 * cbind: out row r = X row r followed by Y row r (Y's column ids already shifted by ncol X), rows past the end of
 * the shorter operand come from the longer one only (cbind_csr<>, src/cbind.cpp:4-99).  Outputs hold
 * max(nX, nY)+1 / nnzX+nnzY entries; no scan needed (offsets are Xp[r] + Yp[r]). */
int mxd_csr_cbind(int nX, int nY, const int32_t *Xp, const int32_t *Xj, const void *Xx, const int32_t *Yp,
                  const int32_t *Yj_plus_ncol, const void *Yx, int value_dtype, int64_t nnz_total,
                  int32_t *indptr, int32_t *indices, void *values, void *stream);
/* the same for device-resident operands whose column ids nobody has shifted: Y's ids + ncolX */
int mxd_csr_cbind_shift(int nX, int nY, int ncolX, const int32_t *Xp, const int32_t *Xj, const void *Xx,
                        const int32_t *Yp, const int32_t *Yj, const void *Yx, int value_dtype, int64_t nnz_total,
                        int32_t *indptr, int32_t *indices, void *values, void *stream);
/* rbind: append one operand at (row_offset, entry_offset) with the value conversions of concat_csr_batch
 * (src/rbind.cpp:24-173).  in_kind 0 dgR, 1 lgR, 2 ngR, 3/4/5/6 d/i/l/n sparseVector (1-based indices, one row);
 * out_kind 0 dgR, 1 lgR, 2 ngR.  No synchronisation, for a vector as for a matrix. */
int mxd_csr_rbind_append(int in_kind, const int32_t *indptr_in, const int32_t *indices_in, const void *values_in,
                         int nrows_in, int64_t nnz_in, int out_kind, int row_offset, int64_t entry_offset,
                         int32_t *out_indptr, int32_t *out_indices, void *out_values, void *stream);
/* The whole rbind at once: mxd_csr_rbind_batch, declared with its table record beside mx_rbind_input below.
 * COO rbind: append one operand's triplets at entry_offset.  in_kind 0 dgT, 1 lgT, 2 ngT (0-based i_in / j_in,
 * rows moved down by row_offset), 3/4/5/6 d/i/l/n sparseVector (i_in ignored, j_in 1-based: the one row
 * row_offset); out_kind 0 dgT, 1 lgT, 2 ngT; values converted as mxd_csr_rbind_append converts them. */
int mxd_coo_rbind_append(int in_kind, const int32_t *i_in, const int32_t *j_in, const void *values_in,
                         int64_t nnz_in, int out_kind, int row_offset, int64_t entry_offset,
                         int32_t *out_i, int32_t *out_j, void *out_values, void *stream);
/* cbind of a CSR and a sparse vector as one column: X (x_kind 0 dgR, 1 lgR, 2 ngR; nX rows, ncolX columns), the
 * vector as nv SORTED 1-based indices <= length with values of v_kind 3/4/5/6 (d/i/l/n sparseVector).  first = 0:
 * the entry of row r follows X's row r with column ncolX; first = 1: it comes first with column 0 and X's columns
 * move up by one.  Outputs: indptr[max(nX, length) + 1], indices / values[Xp[nX] + nv] of out_kind 0 dgR, 1 lgR,
 * 2 ngR; no scan, no workspace. */
int mxd_csr_cbind_svec(int nX, int ncolX, const int32_t *Xp, const int32_t *Xj, const void *Xx, int x_kind,
                       const int32_t *vi, const void *vx, int v_kind, int nv, int length, int first,
                       int out_kind, int32_t *indptr, int32_t *indices, void *values, void *stream);

/* SURVEY §8f rank 4.
 * CSR x sparse vector (matmul_csr_svec<>, src/matmul.cpp:486-641): y given as sorted 1-based indices + values;
 *   kind 0 numeric (f64), 1 integer, 2 logical, 3 binary (no values), 4 float32; out f64[m].
 * CSR (.) dense (multiply_csr_by_dense_elemwise<>, src/operators.cpp:239-334): dense column-major m x ncol;
 *   kind 0 double, 1 float32, 2 integer, 3 logical (f64 values in/out), 4 logical AND (int32 values in/out). */
int mxd_spmv_csr_svec(int m, int64_t nnz, const int32_t *indptr, const int32_t *indices, const double *values,
                      const int32_t *y_indices_base1, int ny, const void *y_values, int kind, double *out,
                      void *stream);
int mxd_csr_by_dense_elemwise(int m, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                              const void *values, const void *dense_colmajor, int kind, void *values_out,
                              void *stream);

/* CSC (.) dense (multiply_csc_by_dense_{ignore,keep}_NAs_*, src/operators.cpp:1061-1460).  X is
 * nrows x ncols in CSC (indptr[ncols+1], row indices, f64 values; kind 4: int32 R logicals); the dense operand is
 * column-major nrows x ncols.  kind / dense_kind: 0 double, 1 float32, 2 R integer, 3 R logical, 4 (values only) R's
 * three-valued & of R logicals.
 * mxd_csc_by_dense_elemwise: values only, out[k] = x[k] (op) dense[indices[k] + nrows*col(k)] with the arithmetic of
 *   mxd_csr_by_dense_elemwise (svec.hip's kernel with CSC addressing): f64 / float32 x * d, integer / logical NA ->
 *   NA_real_.
 * NA-keeping route, for a CSC whose rows are sorted inside each column: output column c holds the stored rows (a
 *   repeated row once, with the first entry's value) and every row whose dense cell is NA (any NaN; NA_INTEGER) and
 *   not stored, with value NA_real_; rows ascending.  count: *nnz_out_host = output entries (64-bit; above INT32_MAX
 *   the call fails), *na_outside_host = 1 when some NA cell lies outside the pattern, else 0 (one synchronise).  When
 *   that is 0 and the count equals nnz the structure is unchanged, and mxd_csc_by_dense_elemwise gives the values.  fill: out_indptr[ncols+1],
 *   out_indices / out_values (that many entries).  workspace: mxd_csc_dense_na_workspace_bytes(nrows, ncols), holding
 *   a 1-bit-per-cell NA mask; shared by both passes. */
int mxd_csc_by_dense_elemwise(int ncols, int nrows, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                              const void *values, const void *dense_colmajor, int kind, void *values_out,
                              void *stream);
size_t mxd_csc_dense_na_workspace_bytes(int nrows, int ncols);
int mxd_csc_dense_na_count(int nrows, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                           const void *dense_colmajor, int dense_kind, void *workspace, int64_t *nnz_out_host,
                           int64_t *na_outside_host, void *stream);
int mxd_csc_dense_na_fill(int nrows, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                          const double *values, const void *dense_colmajor, int dense_kind, const void *workspace,
                          int32_t *out_indptr, int32_t *out_indices, double *out_values, void *stream);

/* CSR * sparse vector, the masked row scaling (multiply_csr_by_svec_no_NAs / _keep_NAs, src/operators.cpp:3426-3697;
 * DESIGN.md §4.11).  X is m x ncol in CSR with f64 values and sorted rows; the vector is vi_base1[nv] (sorted 1-based
 * positions), vx[nv] f64 values (NULL: an nsparseVector) and its length, recycled down the rows: output row r is
 * ruled by position r mod length.  Not stored: no entries, or with keep_na the row's NaN / +-Inf entries (NaN as it
 * is, +-Inf as the default NaN).  Stored: the row times the value (copied without values); with keep_na a NaN / +-Inf
 * value fills all ncol columns (NaN: the value everywhere; +-Inf: the default NaN, and value * x at the stored
 * columns, the last entry of a repeated column winning).
 * count: out_indptr[m+1] (the scanned counts), *nnz_out_host = output entries (64-bit; above INT32_MAX the call
 *   fails, which the reference does not check), *x_na_host = 1 when a row that the vector does not store holds a NaN
 *   / +-Inf (only looked for under keep_na), else 0; one synchronise.  It stands in for the reference's
 *   contains_any_nas_or_inf(values) where that flag matters (rows the vector drops): with 0 the dropped rows left
 *   nothing behind.  It is information for the caller; the result does not depend on it and mx_* does not use it.  fill: out_indices / out_values of that many
 *   entries.  workspace: mxd_csr_by_svec_workspace_bytes(m); the count leaves each row's position in the vector
 *   there for the fill. */
size_t mxd_csr_by_svec_workspace_bytes(int m);
int mxd_csr_by_svec_count(int m, int ncol, int64_t nnz, const int32_t *indptr, const double *values,
                          const int32_t *vi_base1, int64_t nv, const double *vx, int length, int keep_na,
                          void *workspace, int32_t *out_indptr, int64_t *nnz_out_host, int64_t *x_na_host,
                          void *stream);
int mxd_csr_by_svec_fill(int m, int ncol, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                         const double *values, const int32_t *vi_base1, int64_t nv, const double *vx, int length,
                         int keep_na, const void *workspace, const int32_t *out_indptr, int32_t *out_indices,
                         double *out_values, void *stream);

/* Dense matrix * sparse vector (multiply_elemwise_dense_by_svec_template<>, src/operators.cpp:3699-4303; densevec.hip;
 * DESIGN.md §4.15).  X is nrows x ncols, column-major, of dense_kind 0 double, 1 float32, 2 R integer, 3 R logical;
 * the vector is vi_base1[nv] (1-based positions), vx[nv] f64 values and its length.  A stored cell holds X * value
 * (float32 widened per cell; NA_INTEGER gives C's NAN, and NA_real_ on the CSR route with length == nrows and
 * keep_na == 0, :3803).  A position outside 1..length is ignored here; the export level refuses it.
 * mxd_dense_by_svec_dense (routes A and D, :3720-3763 and :4235-4300): out_colmajor[nrows * ncols], the vector
 *   recycled over the flat column-major cell index; cells it does not cover hold 0, or under keep_na the fill of a
 *   special cell (an f64 NaN unchanged; an f64 +-Inf or a float32 NaN / +-Inf as C's NAN; NA_INTEGER as NA_real_).  Of a
 *   repeated position the last entry rules.  Cell indices >= nrows * ncols are never written (:4273 writes one).
 * mxd_dense_by_svec_count / _fill (routes B and C, :3765-4233): a CSR result, length dividing nrows, the vector
 *   recycled down the rows.  A row whose position is stored is a full row of products; the others are empty, or
 *   under keep_na hold their special cells in column order with the fill above (NA_real_ also where :4113-4120
 *   pushes (double)NA_INTEGER).  Of a repeated position the first entry rules.  With length < nrows, an f64 X and
 *   keep_na == 0 the product is daxpy's: +0.0 for a value of 0, else 0.0 + value * X (:4005-4015).
 *   count: out_indptr[nrows+1], *nnz_out_host = entries (64-bit; above INT32_MAX the call fails; one synchronise).
 *   fill: out_indices / out_values of that many entries.  workspace: mxd_dense_by_svec_workspace_bytes(nrows,
 *   length); the count leaves the position map there for the fill.  _dense takes the same workspace (nrows may be 0). */
size_t mxd_dense_by_svec_workspace_bytes(int nrows, int length);
int mxd_dense_by_svec_dense(int nrows, int ncols, const void *dense_colmajor, int dense_kind,
                            const int32_t *vi_base1, int64_t nv, const double *vx, int length, int keep_na,
                            void *workspace, double *out_colmajor, void *stream);
int mxd_dense_by_svec_count(int nrows, int ncols, const void *dense_colmajor, int dense_kind,
                            const int32_t *vi_base1, int64_t nv, int length, int keep_na, void *workspace,
                            int32_t *out_indptr, int64_t *nnz_out_host, void *stream);
int mxd_dense_by_svec_fill(int nrows, int ncols, const void *dense_colmajor, int dense_kind, const double *vx,
                           int length, int keep_na, const void *workspace, const int32_t *out_indptr,
                           int32_t *out_indices, double *out_values, void *stream);
/* COO * dense matrix, values only (multiply_coo_by_dense<>, src/operators.cpp:721-770; densevec.hip): out[k] =
 * xx[k] * dense[ii[k] + jj[k] * nrows] for kind 0 double, 1 float32, 2 R integer, 3 R logical (read as bool), with
 * NA_INTEGER / NA_LOGICAL giving NA_real_; kind 4: xx, dense and out are R logicals, R's three-valued and.  An entry
 * outside the matrix reads nothing and gives NA here; the export level refuses it. */
int mxd_coo_by_dense(int64_t nnz, const int32_t *ii, const int32_t *jj, const void *xx, const void *dense_colmajor,
                     int nrows, int ncols, int kind, void *out, void *stream);

/* The outer products of `%*%` with a one-column CSR, and the float32 row vector x CSC product (outer.hip; DESIGN.md
 * §4.14).  X is the CSR triple of a one-column matrix with m rows: row r is non-empty when indptr[r] < indptr[r+1]
 * and its value is values[indptr[r]], the first stored entry; the column indices are never read.
 * Dense outer (matmul_colvec_by_scolvecascsr{,_f32}, src/matmul.cpp:686-781): a CSR with m rows, every non-empty row
 *   holding columns 0..dim-1 with value * colvec[c].  colvec_dtype MX_F64: 0.0 + a*v, the product rounded on its own
 *   (daxpy into a zeroed slot: a product of -0 comes out as +0; a == 0 leaves the zeros).  MX_F32: a narrowed to float
 *   (:53-57), 0.0f + a*v in float, widened for the output.  count: out_indptr[m+1], *nnz_out_host = output entries
 *   (64-bit; above INT32_MAX the call fails); one synchronise.  workspace: mxd_csr_outer_dense_workspace_bytes(m).
 * Sparse outer (matmul_spcolvec_by_scolvecascsr_*, :783-938): a CSC with y_length columns; column
 *   y_indices_base1[k]-1 holds every non-empty row of X, ascending, with value y_values[k] * a (value_dtype MX_F64;
 *   MX_I32 / MX_LGL: NA gives NA_real_, other values multiply as ints promoted to double; MX_NONE: a copied, y_values
 *   NULL); every other column is empty.  y's positions sorted and unique; those outside [1, y_length] are skipped.
 *   count: compacts the non-empty rows into the workspace (*nonempty_host of them) and scans out_indptr[y_length+1];
 *   *nnz_out_host = nonempty * ny, refused above INT32_MAX; two synchronises.  fill: out_indices / out_values of that
 *   many entries.  workspace: mxd_csr_outer_svec_workspace_bytes(m, y_length), shared by both passes.
 * Deviations from the reference: (1) its output arrays have length(indices) * dim entries, which leaves a zero tail
 *   when a row stores more than one entry; here they have out_indptr[m] entries.  (2) The entry count is checked
 *   against INT32_MAX, which the reference does not check.  (3) Known defect, not copied: :808 reads y_values[col]
 *   where it means y_values[ix], an out-of-bounds read whenever y stores fewer positions than its length;
 *   y_values[k] is used here.
 * Row vector (matmul_rowvec_by_csc / _cscbin, :643-684): out[col] = sum of values[ix] * rowvec[indices[ix]] over the
 *   compressed column, each product in double, accumulated into a float (SpMV's float32 kind on the CSC arrays; the
 *   lane-group reduction reorders the float sum).  values NULL: the sum of rowvec[indices[ix]]. */
size_t mxd_csr_outer_dense_workspace_bytes(int m);
int mxd_csr_outer_dense_count(int m, int dim, const int32_t *indptr, void *workspace, int32_t *out_indptr,
                              int64_t *nnz_out_host, void *stream);
int mxd_csr_outer_dense_fill(int m, int dim, int64_t nnz, const int32_t *indptr, const double *values,
                             const void *colvec, int colvec_dtype, const int32_t *out_indptr, int32_t *out_indices,
                             double *out_values, void *stream);
size_t mxd_csr_outer_svec_workspace_bytes(int m, int y_length);
int mxd_csr_outer_svec_count(int m, int64_t nnz, const int32_t *indptr, const double *values,
                             const int32_t *y_indices_base1, int64_t ny, int y_length, void *workspace,
                             int32_t *out_indptr, int64_t *nonempty_host, int64_t *nnz_out_host, void *stream);
int mxd_csr_outer_svec_fill(int m, const int32_t *y_indices_base1, int64_t ny, const void *y_values, int value_dtype,
                            int y_length, int64_t nonempty, const void *workspace, const int32_t *out_indptr,
                            int32_t *out_indices, double *out_values, void *stream);
int mxd_rowvec_by_csc(int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices, const double *values,
                      const float *rowvec, float *out, void *stream);

/* sort_sparse_indices of a sparse vector (sort_vector_indices_*, src/misc.cpp:460-527): ii[n] (non-negative) and
 * its values xx[n] (MX_F64, MX_I32 / MX_LGL, or MX_NONE with xx NULL) sorted by ii in place, stably, by the LSD
 * radix passes of the transpose.  One reduction first: *was_sorted_host = 1 and nothing is
 * written when ii is already non-decreasing.  One synchronise (after the reduction).
 * workspace: mxd_sort_vector_indices_workspace_bytes(n). */
size_t mxd_sort_vector_indices_workspace_bytes(int64_t n);
int mxd_sort_vector_indices(int32_t *ii, void *xx, int64_t n, int value_dtype, void *workspace,
                            int *was_sorted_host, void *stream);

/* sort_sparse_indices of a TsparseMatrix (sort_coo_indices<T>, src/misc.cpp:387-457): the triplets
 * ii[nnz], jj[nnz] (non-negative, below INT32_MAX) and their values xx[nnz] (MX_F64, MX_LGL, or MX_NONE with xx NULL)
 * sorted by (ii, jj) in place.  The sort is stable: entries of one cell stay adjacent and in input order, one of the
 * orders the reference's std::sort may give.  One reduction first: *was_sorted = 1 and nothing else is launched or
 * written when the triplets are already non-decreasing; a negative index fails with all three arrays untouched.
 * Otherwise the transpose's radix passes run on jj and then on ii, carrying the entry index through both, and the
 * values are gathered once.  One synchronise (after the reduction).  workspace: mxd_coo_sort_workspace_bytes(nnz). */
size_t mxd_coo_sort_workspace_bytes(int64_t nnz);
int mxd_coo_sort(int32_t *ii, int32_t *jj, void *xx, int64_t nnz, int value_dtype, void *workspace, int *was_sorted,
                 void *stream);

/* CSR (op) dense vector with R's recycling (multiply_csr_by_dvec_no_NAs<>, src/operators.cpp:1604-2140): a
 * values-only transform, out[k] = values[k] op dvec[(row + col*m) mod dvec_len] (`recyle_pos`, :1478; the reference's
 * four length branches :1640,1773,1870,2033 all reduce to it).  op: R's * ^ / %% %/% on f64 values with the sparse
 * matrix on the left (x_is_lhs) or right, or R's 3-valued & on int32 logicals (MX_DV_LOGICAL_AND; values, dvec and out
 * int32).  ^ %% %/% follow R_pow / R_modulus / R_intdiv (:1482-1601).  nnz < 0 = unknown (launch shape only). */
typedef enum { MX_DV_MULTIPLY = 0, MX_DV_POWERTO = 1, MX_DV_DIVIDE = 2, MX_DV_DIVREST = 3, MX_DV_INTDIV = 4,
               MX_DV_LOGICAL_AND = 5 } mx_dvec_op;
int mxd_csr_by_dvec(int m, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                    const void *values, const void *dvec, int64_t dvec_len, int op, int x_is_lhs,
                    void *values_out, void *stream);

/* CSR (op) dense vector keeping R's NA cells (multiply_csr_by_dvec_with_NAs, src/operators.cpp:2258-2852; DESIGN.md
 * §4.12).  X is m x ncols in CSR, f64 values, rows sorted by column; op is one of the five arithmetic mx_dvec_op,
 * applied with X on the left.
 *
 * Row-ruled regime (:2314-2513), dvec_len <= m and m % dvec_len == 0: row r is ruled by val = dvec[r % dvec_len].  A
 * plain row keeps its entries with x op val; a filled row has all ncols columns: under * a NaN val (NA_real_ for an
 * NA val, else the default NaN, everywhere) or a +-Inf val (the default NaN, x * val where stored); under / %% %/% a
 * zero val (the default NaN, x op val where stored) or a NaN val (val everywhere); under ^ a NaN val (val), a zero
 * val (1) or a negative val (+Inf), R_pow(x, val) where stored.  The last entry of a repeated column wins.
 * count: out_indptr[m+1] from indptr and dvec alone, *nnz_out_host = output entries (64-bit; above INT32_MAX the call
 * fails, which the reference does not check); one synchronise.  fill: out_indices / out_values of that many entries.
 * workspace: mxd_csr_by_dvec_na_rows_workspace_bytes(m), used by the count only. */
size_t mxd_csr_by_dvec_na_rows_workspace_bytes(int m);
int mxd_csr_by_dvec_na_rows_count(int m, int ncols, int64_t nnz, const int32_t *indptr, const double *dvec,
                                  int64_t dvec_len, int op, void *workspace, int32_t *out_indptr,
                                  int64_t *nnz_out_host, void *stream);
int mxd_csr_by_dvec_na_rows_fill(int m, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                 const double *values, const double *dvec, int64_t dvec_len, int op,
                                 const int32_t *out_indptr, int32_t *out_indices, double *out_values, void *stream);
/* Flat regime (:2515-2841), any other dvec_len <= m * ncols (and <= INT32_MAX here): the stored entries get
 * mxd_csr_by_dvec's values; a position ix of the vector is special when dvec[ix] is NaN, 0 under / %% %/% ^, negative
 * under ^ or +-Inf under *, and every flat cell ix + rep * dvec_len < m * ncols of a special position (row = flat % m,
 * col = flat / m) outside X's pattern is a new entry: the default NaN for an NA or a zero divisor, 1 for a zero
 * exponent, +Inf for a negative one, NA_real_ for anything else (:2618-2636).
 * mxd_dvec_na_special: flags, scans and compacts the special positions into special_ws
 *   (mxd_dvec_na_special_workspace_bytes(dvec_len)); *nspecial_host = their number, *candidates_host = the closed-form
 *   number of their cells, sum of ceil((m * ncols - ix) / dvec_len).  INT32_MAX candidates or more fail with the
 *   reference's message (:2654-2660), since every candidate is a new entry or one of X's.  Two read-backs.
 * mxd_dvec_na_cells_count: one lane per candidate cell searches its row of X; *new_host = the new entries (one
 *   read-back); new + nnz >= INT32_MAX fails with the same message.  cells_ws:
 *   mxd_dvec_na_cells_workspace_bytes(candidates), shared with the fill.
 * mxd_dvec_na_cells_fill: the new entries as COO triplets (row, col, value), *new_host of them, in no particular
 *   order and without repeats; mxd_coo_to_csr sorts them.
 * mxd_csr_join_disjoint: the union of two CSR matrices with disjoint patterns and sorted rows, here X's transformed
 *   values and the new entries: out_indptr = indptr1 + indptr2, values copied bit for bit (mxd_csr_merge_fill places
 *   them); out_indices / out_values hold nnz1 + nnz2 entries.  No synchronise. */
size_t mxd_dvec_na_special_workspace_bytes(int64_t dvec_len);
int mxd_dvec_na_special(int m, int ncols, const double *dvec, int64_t dvec_len, int op, void *special_ws,
                        int64_t *nspecial_host, int64_t *candidates_host, void *stream);
size_t mxd_dvec_na_cells_workspace_bytes(int64_t candidates);
int mxd_dvec_na_cells_count(int m, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                            int64_t dvec_len, const void *special_ws, int64_t nspecial, int64_t candidates,
                            void *cells_ws, int64_t *new_host, void *stream);
int mxd_dvec_na_cells_fill(int m, int ncols, const double *dvec, int64_t dvec_len, int op, const void *special_ws,
                           int64_t nspecial, int64_t candidates, const void *cells_ws, int32_t *out_rows,
                           int32_t *out_cols, double *out_values, void *stream);
int mxd_csr_join_disjoint(int m, const int32_t *indptr1, const int32_t *indices1, const double *values1, int64_t nnz1,
                          const int32_t *indptr2, const int32_t *indices2, const double *values2, int64_t nnz2,
                          int32_t *out_indptr, int32_t *out_indices, double *out_values, void *stream);

/* check_is_seq / check_is_rev_seq (src/slice.cpp:25-47) on a device vector.
 * *flag_host receives 0/1 after an internal stream sync. */
int mxd_check_is_seq(const int32_t *idx, int64_t n, int reversed, int32_t *workspace4,
                     int *flag_host, void *stream);

/* exclusive scan of int32 counts[n] -> out[n+1] (out[n] = total); total also
 * returned as int64 in *total_dev (device int64).  workspace: mxd_scan_workspace_bytes(n). */
size_t mxd_scan_workspace_bytes(int64_t n);
int mxd_exclusive_scan_i32(const int32_t *counts, int64_t n, int32_t *out,
                           int64_t *total_dev, void *workspace, void *stream);

/* Next-row components: per-row sortedness check and
 * per-row index sort (check_is_sorted / sort_sparse_indices_known_ncol,
 * src/misc.cpp:118-128, :261-298).  *flag_host is written after an internal stream sync. */
int mxd_csr_rows_sorted(int m, const int32_t *indptr, const int32_t *indices,
                        int32_t *workspace4, int *flag_host, void *stream);
/* sorts every row by column id (stable), in place; tmp_indices / tmp_values are
 * caller scratch of nnz entries each (tmp_values unused for MX_NONE). */
int mxd_csr_sort_rows(int m, int64_t nnz, const int32_t *indptr, int32_t *indices, void *values,
                      int value_dtype, int32_t *tmp_indices, void *tmp_values, void *stream);

/* Device transpose of a CSR structure (transpose.hip), replacing t_deep_internal's coercion chain
 * (R/trans.R:46-56: as(x, "TsparseMatrix") -> t_shallow -> as(x, "RsparseMatrix" / "CsparseMatrix")) and the
 * Matrix coercions that as.csr.matrix / as.csc.matrix call for a CSC / CSR input (R/conversions.R).  The CSC
 * arrays of a matrix are the CSR arrays of its transpose, so this serves CSR -> CSR of X^T, CSR -> CSC and
 * CSC -> CSR alike.  Input: m x n CSR with nnz = indptr[m] entries (nnz passed by the caller); value_dtype
 * MX_F64 / MX_LGL / MX_NONE.  Output: out_indptr[n+1]; output row c lists, in strictly ascending order, the
 * source rows of the entries in column c (stable over the input's row order, whatever the order inside a
 * row); values are copied bit for bit.  Repeated (row, col) pairs inside one input row are merged as Matrix's
 * triplet coercion does: f64 summed in source order, logical by R's `|`, pattern kept once.  out_indices /
 * out_values hold nnz entries; *nnz_out_host (after an internal stream sync) is the count after merging.
 * A column index outside [0, n) fails the call; nothing is written out of bounds.
 * workspace: mxd_csr_transpose_workspace_bytes(nnz). */
size_t mxd_csr_transpose_workspace_bytes(int64_t nnz);
int mxd_csr_transpose(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values,
                      int value_dtype, int64_t nnz, int32_t *out_indptr, int32_t *out_indices,
                      void *out_values, void *workspace, int64_t *nnz_out_host, void *stream);

/* COO -> CSR (coo.hip / transpose.hip), replacing Matrix's TsparseMatrix -> RsparseMatrix coercion that
 * as.csr.matrix calls (R/conversions.R:180-295) and the route of t_deep_internal (R/trans.R:46-56).  Input: nnz
 * triplets (rows[k], cols[k], values[k]) of an m x n matrix, 0-based, any order, duplicates allowed; value_dtype
 * MX_F64 / MX_LGL / MX_NONE.  Output: canonical CSR, out_indptr[m+1], each row's columns strictly ascending,
 * values copied bit for bit.  Repeated (row, col) pairs are merged as mxd_csr_transpose merges them (f64 summed
 * in input order, logical by R's `|`, pattern kept once); explicit zeros stay.  out_indices / out_values hold nnz
 * entries; *nnz_out_host (after an internal stream sync) is the count after merging.  A row outside [0, m) or a
 * column outside [0, n) fails the call and is never used to write; nnz > INT32_MAX is refused up front.
 * COO -> CSC is the same call with the roles swapped: (n, m, cols, rows) gives the CSC arrays.
 * workspace: mxd_coo_to_csr_workspace_bytes(nnz, n) with n the column count passed to the call. */
size_t mxd_coo_to_csr_workspace_bytes(int64_t nnz, int n);
int mxd_coo_to_csr(int m, int n, const int32_t *rows, const int32_t *cols, const void *values, int value_dtype,
                   int64_t nnz, int32_t *out_indptr, int32_t *out_indices, void *out_values, void *workspace,
                   int64_t *nnz_out_host, void *stream);
/* CSR / CSC -> COO: out_rows[k] = the row of entry k (the column, for a CSC), storage order kept; the COO's
 * other index vector and its values are the input's indices and values as they are.  nnz = indptr[m]. */
int mxd_csr_to_coo(int m, int64_t nnz, const int32_t *indptr, int32_t *out_rows, void *stream);
/* CSR (.) COO (multiply_csr_by_coo_elemwise / logicaland_csr_by_coo_elemwise, src/operators.cpp:572-720):
 * X is m x ncol with rows sorted ascending and unique (f64 values, or int32 R logicals when logical != 0); the
 * COO Y is given as nnz_y triplets.  Entry k of Y is kept when y_k is non-zero or NaN (logical: non-zero, NA
 * included), its row is in [0, m) and its column in [0, ncol), and X[row, col] is non-zero or NaN; its value is
 * x * y (logical: R's 3-valued AND).  Kept entries come out in Y's input order, one per occurrence.
 * pass 1 counts and scans (one host read-back of the count into *nnz_out_host); pass 2 fills out_rows / out_cols
 * / out_values with that many entries.  workspace: mxd_csr_by_coo_workspace_bytes(nnz_y), shared by both passes. */
size_t mxd_csr_by_coo_workspace_bytes(int64_t nnz_y);
int mxd_csr_by_coo_count(int logical, int m, int ncol, const int32_t *indptr, const int32_t *indices,
                         const void *x_values, const int32_t *y_rows, const int32_t *y_cols, const void *y_values,
                         int64_t nnz_y, void *workspace, int64_t *nnz_out_host, void *stream);
int mxd_csr_by_coo_fill(int logical, int m, int ncol, const int32_t *indptr, const int32_t *indices,
                        const void *x_values, const int32_t *y_rows, const int32_t *y_cols, const void *y_values,
                        int64_t nnz_y, const void *workspace, int32_t *out_rows, int32_t *out_cols,
                        void *out_values, void *stream);
/* COO (op) dense vector, the COO twin of mxd_csr_by_dvec (multiply_coo_by_dense_ignore_NAs_template,
 * src/operators.cpp:2856-3425): out[k] = values[k] op dvec[(rows[k] + cols[k]*m) mod dvec_len], same ops and
 * arithmetic as mxd_csr_by_dvec. */
int mxd_coo_by_dvec(int m, int ncols, int64_t nnz, const int32_t *rows, const int32_t *cols, const void *values,
                    const void *dvec, int64_t dvec_len, int op, int x_is_lhs, void *values_out, void *stream);
/* X[i, j] of a COO (cooslice.hip), replacing slice_coo_arbitrary_template (src/slice_coo.cpp:123-706).  Each
 * axis is described by an mx_coo_axis:
 *   MX_AXIS_AFFINE  all / seq / rev-seq selector: index r in [lo, hi] has the one position r - lo (reversed = 0)
 *                   or hi - r (reversed = 1); other indices are not selected.  0 <= lo <= hi < the axis length.
 *   MX_AXIS_MAP     arbitrary selector, through the dense map that mxd_colmap_build makes of the 1-based
 *                   selector (ncol_map = nmap = max + 1): index r's positions are pos[start[r+1] .. start[r+2]),
 *                   ascending; r + 1 >= nmap is not selected.
 * Triplet k = (rows[k], cols[k], values[k]) gives one output (a, b, values[k]) for every position a of rows[k]
 * (outer loop, ascending) and every position b of cols[k] (inner loop, ascending), triplets in storage order;
 * values are copied bit for bit and keep their type (MX_F64 / MX_LGL / MX_NONE); nothing is merged.
 * count: one lane per triplet, multiplicities in 64 bits; the total (one host read-back into *nnz_out_host) and any
 * single triplet above INT32_MAX fail the call, as does a row outside [0, nrow) or a column outside [0, ncol),
 * which is never used to read a map.  fill writes out_rows / out_cols / out_values (that many entries).
 * workspace: mxd_coo_slice_workspace_bytes(nnz), shared by both passes. */
typedef enum { MX_AXIS_AFFINE = 0, MX_AXIS_MAP = 1 } mx_coo_axis_kind;
typedef struct {
    int kind;                  /* mx_coo_axis_kind */
    int lo, hi, reversed;      /* MX_AXIS_AFFINE */
    int nmap;                  /* MX_AXIS_MAP: start has nmap + 1 entries */
    const int32_t *start;      /* device pointers */
    const int32_t *pos;
} mx_coo_axis;
size_t mxd_coo_slice_workspace_bytes(int64_t nnz);
int mxd_coo_slice_count(int nrow, int ncol, const int32_t *rows, const int32_t *cols, int64_t nnz,
                        const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, void *workspace,
                        int64_t *nnz_out_host, void *stream);
int mxd_coo_slice_fill(int nrow, int ncol, const int32_t *rows, const int32_t *cols, const void *values,
                       int value_dtype, int64_t nnz, const mx_coo_axis *axis_i, const mx_coo_axis *axis_j,
                       const void *workspace, int32_t *out_rows, int32_t *out_cols, void *out_values, void *stream);
/* X[i, j] with scalar i, j of a COO (slice_coo_single_template, src/slice_coo.cpp:3-71): *k_host = the smallest k
 * with (rows[k], cols[k]) == (r, c), or -1; on a hit value_host (when non-null) receives values[k] (8 bytes for
 * MX_F64, 4 for MX_LGL, nothing for MX_NONE).  One host read-back.  workspace: mxd_coo_single_workspace_bytes(). */
size_t mxd_coo_single_workspace_bytes(void);
int mxd_coo_single(const int32_t *rows, const int32_t *cols, const void *values, int value_dtype, int64_t nnz,
                   int r, int c, void *workspace, int64_t *k_host, void *value_host, void *stream);
/* NA rows / columns injected into a COO (coona.hip), replacing inject_NAs_inplace_coo_template
 * (src/slice_coo.cpp:708-946).  rows_na[n_rna] / cols_na[n_cna]: device arrays of 0-based indices, ascending and
 * distinct (which(is.na(.)) - 1L); a list that is not, or that leaves [0, nrow) / [0, ncol), fails the count.
 * Output, bit for bit the reference's: the kept triplets in storage order (a triplet is dropped when its row is an
 * NA row / its column an NA column, and when both lists are given only when both hold), then the NA block, every
 * value NA_real_ (MX_F64) or NA_LOGICAL (MX_LGL):
 *   n_rna > n_cna:  (r, 0 .. ncol-1) per r of rows_na, then (rem[k], c), k < nrow - n_rna, per c of cols_na
 *   otherwise:      (0 .. nrow-1, c) per c of cols_na, then (r, rem[k]), k < ncol - n_cna, per r of rows_na
 * where rem is what the reference's swap loop (:729-739) leaves of 0 .. n-1 over the major axis.
 * count: *nnz_out_host = kept + n_rna*ncol + n_cna*(nrow - n_rna) in 64 bits after one read-back; a total above
 * INT32_MAX fails the call.  fill writes that many entries.  value_dtype MX_F64 or MX_LGL.
 * Two caller-allocated regions, shared by both passes: workspace, mxd_compact_workspace_bytes(nnz) bytes (the kept
 * pass is the tiled compaction of compact.hip), and maps, int32[4 + nrow + ncol + max(nrow, ncol)] (the list
 * flags, the two membership maps and rem). */
int mxd_coo_inject_na_count(int nrow, int ncol, const int32_t *rows, const int32_t *cols, int64_t nnz,
                            const int32_t *rows_na, int64_t n_rna, const int32_t *cols_na, int64_t n_cna,
                            void *workspace, int32_t *maps, int64_t *nnz_out_host, void *stream);
int mxd_coo_inject_na_fill(int nrow, int ncol, const int32_t *rows, const int32_t *cols, const void *values,
                           int value_dtype, int64_t nnz, const int32_t *rows_na, int64_t n_rna,
                           const int32_t *cols_na, int64_t n_cna, const void *workspace, const int32_t *maps,
                           int32_t *out_rows, int32_t *out_cols, void *out_values, void *stream);
/* X[i, j] with scalar i, j of a CSR (extract_single_val_csr with is_sorted = false, src/slice.cpp:661-785):
 * *k_host = the first k of [indptr[r], indptr[r+1]), in storage order, with indices[k] == c, or -1 (an empty row is
 * no hit); value_host as for mxd_coo_single.  One wavefront, one host read-back.  workspace: 16 bytes. */
int mxd_csr_single(int nrows, const int32_t *indptr, const int32_t *indices, const void *values, int value_dtype,
                   int64_t nnz, int r, int c, void *workspace, int64_t *k_host, void *value_host, void *stream);
/* repeat_indices_n_times (src/slice.cpp:636-659): out[t + n_indices*rep] = indices[t] + ix_length*rep for
 * rep < desired_length / ix_length, then out[n_indices*full + t] = remainder[t] + ix_length*full; out holds
 * n_indices * (desired_length / ix_length) + n_remainder entries. */
int mxd_repeat_indices(const int32_t *indices, int64_t n_indices, const int32_t *remainder, int64_t n_remainder,
                       int ix_length, int desired_length, int32_t *out, void *stream);
/* The dense vector of n entries at distinct 0-based positions (drop_slice's as.vector(), R/slice.R:210-236):
 * out[len] (out_dtype MX_F64, or MX_LGL for int32 R logicals) is zero-filled, then out[pos[k]] = values[k], or 1
 * when value_dtype is MX_NONE; otherwise value_dtype equals out_dtype.  Positions outside [0, len) are skipped. */
int mxd_entries_to_dense_vector(const int32_t *pos, const void *values, int value_dtype, int64_t n, void *out,
                                int out_dtype, int64_t len, void *stream);

/* X[i, j] <- scalar and X[i, ] <- CSR of a CSR with f64 values (assign.hip): count -> scan -> fill
 * with one lane group per row, chosen from avg_row_len as for mxd_csr_colrange_*.  Both selectors are mx_coo_axis
 * values without duplicates (MX_AXIS_MAP as mxd_colmap_build makes it of the 1-based selector); nsel_i / nsel_j are
 * their lengths.  workspace: mxd_gather_workspace_bytes(nrows).
 *   scalar, is_const = 0: a selected row drops the entries whose column is selected, in order
 *   scalar, is_const = 1: a selected row becomes the ascending merge of its kept entries and one (col, value) per
 *                         selected column; rows must be sorted and free of duplicates; `value` is written bit for bit
 *   count:  new_indptr[nrows + 1], *nnz_out_host = the 64-bit total, *hits_out_host = the selected cells the matrix
 *           stores; one host read-back.  A total above INT32_MAX fails with the reference's message
 *           (src/assignment.cpp:380-382) and nothing has been written but the workspace and new_indptr.  When the
 *           column axis is all columns, indices is not read.
 *   fill:   cols_sorted[nsel_j] = the selected columns ascending, read only for an MX_AXIS_MAP column axis on the
 *           const route; new_indices may be NULL when the structure does not change (total = nnz on the const route)
 *   replace_rows: selected row r becomes row k of the value CSR (nvalue_rows rows), k = r's position in the selector;
 *           every other row is copied */
int mxd_csr_assign_count(int nrows, int ncols, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                         const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, int64_t nsel_i, int64_t nsel_j,
                         int is_const, double avg_row_len, int32_t *new_indptr, void *workspace,
                         int64_t *nnz_out_host, int64_t *hits_out_host, void *stream);
int mxd_csr_assign_fill(int nrows, int ncols, const int32_t *indptr, const int32_t *indices, const double *values,
                        const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, const int32_t *cols_sorted,
                        int64_t nsel_j, int is_const, double value, double avg_row_len, const int32_t *new_indptr,
                        int32_t *new_indices, double *new_values, void *stream);
int mxd_csr_replace_rows_count(int nrows, const int32_t *indptr, const mx_coo_axis *axis_i, int nvalue_rows,
                               const int32_t *v_indptr, int32_t *new_indptr, void *workspace, int64_t *nnz_out_host,
                               void *stream);
int mxd_csr_replace_rows_fill(int nrows, const int32_t *indptr, const int32_t *indices, const double *values,
                              const mx_coo_axis *axis_i, int nvalue_rows, const int32_t *v_indptr,
                              const int32_t *v_indices, const double *v_values, double avg_row_len,
                              const int32_t *new_indptr, int32_t *new_indices, double *new_values, void *stream);

/* X[, c] <- vector and the pattern of X[r, ] <- vector of a CSR with f64 values (assignvec.hip).
 * A pattern is (ii, xx, n_xx, length): 0-based positions ii[0..n_xx) inside [0, length) and their values; ii == NULL
 * is the dense pattern 0..length-1 (n_xx == length).  A sparse pattern without entries passes n_xx = 0.
 *   col_count / col_fill: set_single_col_to_colvec (src/assignment.cpp:839-913) and set_single_col_to_svec
 *           (:1009-1133) with their per-row insert_col_into_row (:8-117) / remove_col_from_row (:119-180): row r ends
 *           up holding (col, xx[.]) when the pattern stores r % length (ii ascending), and without col otherwise.
 *           Rows must be sorted.  count -> scan -> fill as mxd_csr_assign_*; workspace:
 *           mxd_gather_workspace_bytes(nrows); one host synchronisation.  *changed_out_host = the rows whose structure
 *           changes (0: new_indices may be NULL in the fill, which then writes values only).  A total above INT32_MAX
 *           fails with the reference's message (:380-382).
 *   expand_pattern_row: the recycling loops of set_single_row_to_rowvec (:771-837) and set_single_row_to_svec
 *           (:915-1007): row_indices[t] = ii[t % n_xx] + length * (t / n_xx) (t when dense), row_values[t] =
 *           xx[t % n_xx] for t < n_xx * n_repeats, row_indptr = {0, n_xx * n_repeats}: a one-row CSR for
 *           mxd_csr_replace_rows_*.  row_indptr and row_indices may be NULL (values only). */
int mxd_csr_assign_col_count(int nrows, int ncols, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                             int col, const int32_t *ii, int64_t n_xx, int length, double avg_row_len,
                             int32_t *new_indptr, void *workspace, int64_t *nnz_out_host, int64_t *changed_out_host,
                             void *stream);
int mxd_csr_assign_col_fill(int nrows, int ncols, const int32_t *indptr, const int32_t *indices, const double *values,
                            int col, const int32_t *ii, const double *xx, int64_t n_xx, int length,
                            double avg_row_len, const int32_t *new_indptr, int32_t *new_indices, double *new_values,
                            void *stream);
int mxd_csr_expand_pattern_row(const int32_t *ii, const double *xx, int64_t n_xx, int length, int n_repeats,
                               int32_t *row_indptr, int32_t *row_indices, double *row_values, void *stream);

/* Stable compaction of sparse entries (compact.hip), the core of remove_sparse_zeros and filterSparse
 * (remove_zero_valued_{csr,coo,svec}_*, src/misc.cpp:553-968; rebuild_indptr_after_filter, :1099-1116).
 * Entry k of n is kept by `rule`, evaluated on values[k] (value_dtype MX_F64, MX_LGL or MX_I32) or on mask[k]:
 *   MX_KEEP_NONZERO        x != 0 (a NaN / NA value is kept)
 *   MX_KEEP_NONZERO_NOT_NA x != 0 and x is not NaN (f64) / NA_INTEGER (int32)
 *   MX_KEEP_NOT_NA         x is not NaN / NA_INTEGER (zeros are kept)
 *   MX_KEEP_MASK           mask[k] != 0 (R logical; NA keeps the entry and writes the kind's NA as its value:
 *                          NA_real_ or NA_LOGICAL).  values may then be absent (value_dtype MX_NONE).
 * count: kept entries per tile, scanned; *kept_host (one 8-byte read-back) = entries kept.
 * fill: kept entries in input order: out_idx0[q] = idx0[k], out_idx1[q] = idx1[k], out_values[q] = values[k]
 * (each output skipped when null).  With out_indptr (m + 1 entries; indptr[m] = n, non-decreasing), out_indptr[r]
 * = kept entries before indptr[r], so a CSR / CSC (indptr, idx0) comes out as a CSR / CSC.  Same arguments in
 * both passes.  workspace: mxd_compact_workspace_bytes(n), shared by both passes. */
typedef enum { MX_KEEP_NONZERO = 0, MX_KEEP_NONZERO_NOT_NA = 1, MX_KEEP_NOT_NA = 2, MX_KEEP_MASK = 3 } mx_keep_rule;
size_t mxd_compact_workspace_bytes(int64_t n);
int mxd_compact_count(int64_t n, const void *values, int value_dtype, int rule, const int32_t *mask,
                      void *workspace, int64_t *kept_host, void *stream);
int mxd_compact_fill(int64_t n, const void *values, int value_dtype, int rule, const int32_t *mask,
                     const int32_t *idx0, const int32_t *idx1, int m, const int32_t *indptr, const void *workspace,
                     int32_t *out_idx0, int32_t *out_idx1, void *out_values, int32_t *out_indptr, void *stream);
/* A dense R vector (dtype MX_F64 numeric, MX_I32 integer, MX_LGL logical; n < INT_MAX cells) as a dsparseVector, by
 * the same two passes: a cell is kept when it is not zero or is NA / NaN; out_indices_base1 receives the kept
 * cells' 1-based positions in order, out_values their values as f64 (NA_integer_ / NA -> NA_real_, TRUE -> 1).
 * workspace: mxd_compact_workspace_bytes(n), the same tiles.  The count reads the total back (one synchronisation);
 * the fill needs the workspace the count left. */
int mxd_dense_to_svec_count(int64_t n, const void *dense, int dtype, void *workspace, int64_t *kept_host,
                            void *stream);
int mxd_dense_to_svec_fill(int64_t n, const void *dense, int dtype, const void *workspace,
                           int32_t *out_indices_base1, double *out_values, void *stream);
/* Index validation of check_sparse_matrix (check_valid_{csr,coo}_matrix, check_valid_svec, src/misc.cpp:970-1097):
 * *flags_host (one read-back) ORs MX_BAD_NEGATIVE / MX_BAD_BOUND / MX_BAD_NA over indices[0..n) against [0, bound),
 * MX_BAD_PTR_NA over indptr[0..n_ptr) and MX_BAD_PTR_ORDER for some r < n_mono with indptr[r] > indptr[r+1]
 * (n_mono < n_ptr, or 0).  workspace4: 4 device bytes. */
typedef enum { MX_BAD_NEGATIVE = 1, MX_BAD_BOUND = 2, MX_BAD_NA = 4, MX_BAD_PTR_NA = 8, MX_BAD_PTR_ORDER = 16 } mx_bad_flag;
int mxd_validate_indices(const int32_t *indices, int64_t n, int bound, const int32_t *indptr, int64_t n_ptr,
                         int64_t n_mono, int32_t *workspace4, int *flags_host, void *stream);

/* ========================================================================== */
/* (1) export level — host pointers, names follow the Rcpp exports            */
/* ========================================================================== */

/* tcrossprod_csr_dense_numeric  src/matmul.cpp:345-359  (RcppExports.cpp:547)
 * X CSR with nrows_X rows; Y_colmajor is nrow_Y x ncol_Y column-major (so it
 * is ncol_Y x nrow_Y row-major == B of the SpMM); out is nrows_X x nrow_Y
 * column-major, fully written.  nthreads is accepted and ignored. */
int mx_tcrossprod_csr_dense_numeric(const int32_t *X_indptr, const int32_t *X_indices,
                                    const double *X_values, int nrows_X,
                                    const double *Y_colmajor, int nrow_Y, int ncol_Y,
                                    int nthreads, double *out_colmajor);
/* tcrossprod_csr_dense_float32  src/matmul.cpp:361-375  (RcppExports.cpp:561) */
int mx_tcrossprod_csr_dense_float32(const int32_t *X_indptr, const int32_t *X_indices,
                                    const double *X_values, int nrows_X,
                                    const float *Y_colmajor, int nrow_Y, int ncol_Y,
                                    int nthreads, float *out_colmajor);
/* matmul_dense_csc_numeric  src/matmul.cpp:221-235  (RcppExports.cpp:489)
 * X_colmajor nrows_X x ncols_X; Y CSC with ncols_Y columns; out nrows_X x ncols_Y col-major. */
int mx_matmul_dense_csc_numeric(const double *X_colmajor, int nrows_X, int ncols_X,
                                const int32_t *Y_indptr, const int32_t *Y_indices,
                                const double *Y_values, int ncols_Y,
                                int nthreads, double *out_colmajor);
int mx_matmul_dense_csc_float32(const float *X_colmajor, int nrows_X, int ncols_X,
                                const int32_t *Y_indptr, const int32_t *Y_indices,
                                const double *Y_values, int ncols_Y,
                                int nthreads, float *out_colmajor);
/* tcrossprod_dense_csr_numeric  src/matmul.cpp:283-297  (RcppExports.cpp:517)
 * out is nrows_X x nrows_Y col-major; ncols_Y is unused by the reference too. */
int mx_tcrossprod_dense_csr_numeric(const double *X_colmajor, int nrows_X, int ncols_X,
                                    const int32_t *Y_indptr, const int32_t *Y_indices,
                                    const double *Y_values, int nrows_Y,
                                    int nthreads, int ncols_Y, double *out_colmajor);
int mx_tcrossprod_dense_csr_float32(const float *X_colmajor, int nrows_X, int ncols_X,
                                    const int32_t *Y_indptr, const int32_t *Y_indices,
                                    const double *Y_values, int nrows_Y,
                                    int nthreads, int ncols_Y, float *out_colmajor);

/* matmul_csr_dvec_{numeric,integer,logical,float32}  src/matmul.cpp:421-483
 * (RcppExports.cpp:575,589,603,617).  len_y = ncol(X). */
int mx_matmul_csr_dvec_numeric(const int32_t *X_indptr, const int32_t *X_indices,
                               const double *X_values, int nrows_X,
                               const double *y_dense, int len_y, int nthreads, double *out);
int mx_matmul_csr_dvec_integer(const int32_t *X_indptr, const int32_t *X_indices,
                               const double *X_values, int nrows_X,
                               const int32_t *y_dense, int len_y, int nthreads, double *out);
int mx_matmul_csr_dvec_logical(const int32_t *X_indptr, const int32_t *X_indices,
                               const double *X_values, int nrows_X,
                               const int32_t *y_dense, int len_y, int nthreads, double *out);
int mx_matmul_csr_dvec_float32(const int32_t *X_indptr, const int32_t *X_indices,
                               const double *X_values, int nrows_X,
                               const float *y_dense, int len_y, int nthreads, float *out);

/* Variable-size results: begin computes on the device and reports the sizes,
 * finish copies into caller-allocated vectors and releases the handle
 * (mx_result_discard releases without copying). */
typedef struct mx_result mx_result;
typedef struct {
    int64_t indptr_len;    /* length of the indptr vector to allocate           */
    int64_t nnz;           /* length of indices                                 */
    int64_t values_len;    /* length of values (nnz, or 0 when there are none)  */
    int     values_dtype;  /* MX_F64 / MX_LGL / MX_NONE                         */
    int     alias_structure; /* 1: reference returns the INPUT indptr1/indices1
                                objects themselves (operators.cpp:127-131,:390-394);
                                finish then fills only values                   */
} mx_result_info;

/* add_csr_elemwise / logicalor_csr_elemwise / multiply_csr_elemwise /
 * logicaland_csr_elemwise  (RcppExports.cpp:1287,1303,1192,1207).
 * op selects the export and its flag (substract / xor_op). nrows = len(indptr)-1. */
int mx_csr_elemwise_begin(int op, int nrows,
                          const int32_t *indptr1, const int32_t *indptr2,
                          const int32_t *indices1, const int32_t *indices2,
                          const void *values1, const void *values2,
                          int64_t nnz1, int64_t nnz2,
                          mx_result **res, mx_result_info *info);
/* copy_csr_rows_{numeric,logical,binary}  src/slice.cpp:276-324 (RcppExports.cpp:1886,1899,1912)
 * value_dtype MX_F64 / MX_LGL / MX_NONE; n_values = length of the values vector
 * (0 => no values copied, slice.cpp:246,257). */
int mx_copy_csr_rows_begin(const int32_t *indptr, int nrows,
                           const int32_t *indices, const void *values, int value_dtype,
                           int64_t n_values,
                           const int32_t *rows_take, int64_t n_take,
                           mx_result **res, mx_result_info *info);
/* copy_csr_rows_col_seq_{numeric,logical,binary}  src/slice.cpp:385-447 (RcppExports.cpp:1924,1939,1954):
 * cols_take is only used for its min / max (minus index1), as in the reference.  Result values are f64. */
int mx_copy_csr_rows_col_seq_begin(const int32_t *indptr, int nrows,
                                   const int32_t *indices, const void *values, int value_dtype, int64_t n_values,
                                   const int32_t *rows_take, int64_t n_take,
                                   const int32_t *cols_take, int64_t n_cols_take, int index1,
                                   mx_result **res, mx_result_info *info);
/* copy_csr_arbitrary_{numeric,logical,binary}  src/slice.cpp:580-634: rows_take, cols_take 0-based */
int mx_copy_csr_arbitrary_begin(const int32_t *indptr, int nrows,
                                const int32_t *indices, const void *values, int value_dtype, int64_t n_values,
                                const int32_t *rows_take, int64_t n_take,
                                const int32_t *cols_take, int64_t n_cols_take,
                                mx_result **res, mx_result_info *info);
/* reverse_rows_{numeric,logical,binary}  src/slice.cpp:98-140 */
int mx_reverse_rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                          int value_dtype, int64_t n_values, mx_result **res, mx_result_info *info);
/* reverse_columns_inplace_{numeric,logical,binary}  src/slice.cpp:172-221: modifies indices / values */
int mx_reverse_columns_inplace(const int32_t *indptr, int nrows, int32_t *indices, void *values,
                               int value_dtype, int64_t n_values, int ncol);
/* matmul_csr_svec_{numeric,integer,logical,binary,float32}  src/matmul.cpp:555-641 (kind as mxd_spmv_csr_svec) */
int mx_matmul_csr_svec(const int32_t *X_indptr, const int32_t *X_indices, const double *X_values, int nrows_X,
                       const int32_t *y_indices_base1, int64_t ny, const void *y_values, int kind, int nthreads,
                       double *out);
/* multiply_csr_by_dense_elemwise_{double,float32,int,bool} + logicaland_csr_by_dense_cpp  src/operators.cpp:289-334:
 * dense_mat column-major nrows x ncols; values_out has nnz entries (f64, or int32 for kind 4). */
int mx_multiply_csr_by_dense_elemwise(const int32_t *indptr, const int32_t *indices, const void *values, int nrows,
                                      const void *dense_mat, int64_t ncols, int kind, void *values_out);
/* multiply_csc_by_dense_ignore_NAs_{numeric,float32,integer,logical}  src/operators.cpp:1125-1189 and
 * logicaland_csc_by_dense_ignore_NAs  :1191-1206 (RcppExports.cpp:2310-2314): X CSC with ncols columns
 * (indptr[ncols+1]), dense column-major nrows x ncols; values_out has nnz entries (f64; int32 R logicals for the
 * logicaland), in storage order. */
int mx_multiply_csc_by_dense_ignore_NAs_numeric(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const double *dense, int nrows,
                                                double *values_out);
int mx_multiply_csc_by_dense_ignore_NAs_float32(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const float *dense, int nrows,
                                                double *values_out);
int mx_multiply_csc_by_dense_ignore_NAs_integer(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const int32_t *dense, int nrows,
                                                double *values_out);
int mx_multiply_csc_by_dense_ignore_NAs_logical(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const int32_t *dense, int nrows,
                                                double *values_out);
int mx_logicaland_csc_by_dense_ignore_NAs(const int32_t *indptr, int ncols, const int32_t *indices,
                                          const int32_t *values, const int32_t *dense, int nrows,
                                          int32_t *values_out);
/* multiply_csc_by_dense_keep_NAs_{numeric,integer,logical,float32}  src/operators.cpp:1388-1458
 * (RcppExports.cpp:2315-2318), through mxd_csc_dense_na_count / _fill: a new indptr (ncols + 1), indices and f64
 * values; rows must be sorted inside each column (the R caller sorts, R/operators.R:626-630).  A result of more than
 * INT32_MAX entries fails before anything is allocated for it.  logicaland_csc_by_dense_keep_NAs (:1460-) is not
 * provided. */
int mx_multiply_csc_by_dense_keep_NAs_numeric(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const double *dense, int nrows,
                                              mx_result **res, mx_result_info *info);
int mx_multiply_csc_by_dense_keep_NAs_integer(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const int32_t *dense, int nrows,
                                              mx_result **res, mx_result_info *info);
int mx_multiply_csc_by_dense_keep_NAs_logical(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const int32_t *dense, int nrows,
                                              mx_result **res, mx_result_info *info);
int mx_multiply_csc_by_dense_keep_NAs_float32(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const float *dense, int nrows,
                                              mx_result **res, mx_result_info *info);
/* multiply_csr_by_dvec_no_NAs_numeric  src/operators.cpp:2142-2175: exactly one of the five flags is set (as the R
 * caller passes them, R/operators.R:1134-1137); values_out f64[nnz].  The structure-changing NA route is
 * mx_multiply_csr_by_dvec_with_NAs_begin below. */
int mx_multiply_csr_by_dvec_no_NAs_numeric(const int32_t *indptr, const int32_t *indices, const double *values,
                                           int nrows, const double *dvec, int64_t dvec_len, int ncols, int multiply,
                                           int powerto, int divide, int divrest, int intdiv, int X_is_LHS,
                                           double *values_out);
/* multiply_csr_by_dvec_with_NAs  src/operators.cpp:2258-2852 (RcppExports.cpp:1628-1645): the
 * route the R caller takes when the vector makes cells outside X's pattern NA / NaN / 1 / Inf (R/operators.R:981-988).
 * Rows of X sorted by column (the R caller sorts, :1113); 1 <= dvec_len <= nrows * ncols; exactly one of the five
 * flags set; ^ / %% with X_is_LHS = 0 fail as the reference's throw_internal_err does (:2275).  Result: a new indptr
 * (nrows + 1), indices and f64 values, rows sorted.  When the flat regime adds no entry, info->alias_structure = 1:
 * the reference returns the INPUT indptr / indices objects (:2643-2651) and finish fills only the values.  Too many
 * entries fail before the result is allocated: the row-ruled regime through the count's int32 check (the reference
 * does not check there), the flat regime with the reference's message (:2654-2660). */
int mx_multiply_csr_by_dvec_with_NAs_begin(const int32_t *indptr, const int32_t *indices, const double *values,
                                           int nrows, const double *dvec, int64_t dvec_len, int ncols, int multiply,
                                           int powerto, int divide, int divrest, int intdiv, int X_is_LHS,
                                           mx_result **res, mx_result_info *info);
/* logicaland_csr_by_dvec_internal  src/operators.cpp:2177-2200: R logicals (int32), values_out int32[nnz] */
int mx_logicaland_csr_by_dvec_internal(const int32_t *indptr, const int32_t *indices, const int32_t *values,
                                       int nrows, const int32_t *dvec, int64_t dvec_len, int ncols,
                                       int32_t *values_out);
/* cbind_csr_{numeric,logical,binary}  src/cbind.cpp:101-157 (value_dtype MX_F64 / MX_LGL / MX_NONE) */
int mx_cbind_csr_begin(const int32_t *X_indptr, int nrows_X, const int32_t *X_indices, const void *X_values,
                       int64_t n_values_X, const int32_t *Y_indptr, int nrows_Y,
                       const int32_t *Y_indices_plus_ncol, const void *Y_values, int64_t n_values_Y,
                       int value_dtype, mx_result **res, mx_result_info *info);
/* concat_csr_batch  src/rbind.cpp:24-173 over plain arrays instead of S4 objects */
typedef struct {
    int kind;                  /* 0 dgR, 1 lgR, 2 ngR, 3 dsparseVector, 4 isparseVector, 5 lsparseVector, 6 nsparseVector */
    const int32_t *indptr;     /* matrices only */
    const int32_t *indices;    /* @j (0-based) or @i of a sparse vector (1-based) */
    const void *values;        /* f64 / int32 / NULL */
    int nrows;                 /* matrices: Dim[1]; vectors: ignored (one row) */
    int64_t nnz;
} mx_rbind_input;
int mx_concat_csr_batch_begin(const mx_rbind_input *objects, int n_inputs, int out_kind,
                              mx_result **res, mx_result_info *info);
/* The device-level form of the same concat (declared here, beside mx_rbind_input, whose members it repeats): one
 * record per operand in DEVICE memory, pointers to device arrays, with the operand's place in the output.
 * row_offset / entry_offset are the exclusive prefix sums of the operands' rows (a vector counts one) and entries,
 * in table order; operands without rows or without entries are allowed anywhere.  Two launches whatever n_items is,
 * no workspace, no synchronisation.  Outputs: out_indptr[nrows_out + 1], out_indices / out_values[nnz_out]
 * (f64 for out_kind 0, int32 for 1, unused for 2). */
typedef struct {
    int kind;                  /* as mx_rbind_input.kind */
    int nrows;                 /* matrices: rows; vectors: ignored (one row) */
    const int32_t *indptr;     /* matrices only */
    const int32_t *indices;
    const void *values;
    int64_t nnz;
    int64_t entry_offset;      /* where the operand's entries start in the output */
    int row_offset;            /* where its rows start */
} mx_rbind_item;
int mxd_csr_rbind_batch(const mx_rbind_item *items_dev, int n_items, int out_kind, int nrows_out, int64_t nnz_out,
                        int32_t *out_indptr, int32_t *out_indices, void *out_values, void *stream);
/* rbind2_coo / rbind2_coo_vec  R/rbind.R:405-520 over plain arrays: the operands' triplets one after the other, a
 * matrix's rows moved down by the rows before it, a sparse vector as one row.  objects as for the CSR batch with
 * kinds 0 / 1 / 2 = dgT / lgT / ngT, whose `indptr` member holds the ROW ids (nnz of them); out_kind 0 dgT, 1 lgT,
 * 2 ngT.  row_offsets[n_inputs] gives each operand's first output row; NULL places them one below the other in
 * table order (rbind2_coo_vec with the vector first stores the matrix's triplets first all the same, :497-498).
 * The result is a COO held in the mx_result as mx_multiply_csr_by_coo_begin's is: the indptr vector holds
 * the row ids (info.indptr_len = info.nnz). */
int mx_rbind_coo_begin(const mx_rbind_input *objects, int n_inputs, const int32_t *row_offsets, int out_kind,
                       mx_result **res, mx_result_info *info);
/* cbind2(RsparseMatrix, sparseVector) / cbind2(sparseVector, RsparseMatrix): X (x_kind 0 dgR, 1 lgR, 2 ngR) with
 * the vector (v_kind 3 / 4 / 5 / 6 d / i / l / n sparseVector, 1-based indices, any order, below `length`) as one
 * more column, last (first = 0) or first (first = 1).  max(nrows_X, length) rows; out_kind 0 dgR, 1 lgR, 2 ngR. */
int mx_cbind_csr_svec_begin(const int32_t *X_indptr, int nrows_X, int ncols_X, const int32_t *X_indices,
                            const void *X_values, int x_kind, const int32_t *v_indices, const void *v_values,
                            int v_kind, int nv, int length, int first, int out_kind,
                            mx_result **res, mx_result_info *info);
/* A dense vector bound to a sparse matrix becomes a dsparseVector first (mxd_dense_to_svec_*): dtype MX_F64 /
 * MX_I32 / MX_LGL.  The result holds no indptr (info.indptr_len = 0), the 1-based positions as indices and f64
 * values. */
int mx_dense_to_svec_begin(const void *dense, int64_t n, int dtype, mx_result **res, mx_result_info *info);
/* t_deep / as.csc.matrix / as.csr.matrix(dgCMatrix): replaces t_deep_internal (R/trans.R:46-56) and the Matrix
 * coercions that R/conversions.R's as.csr.matrix / as.csc.matrix call, through mxd_csr_transpose.  indptr has
 * nrows + 1 entries starting at 0; value_dtype MX_F64 / MX_LGL / MX_NONE; n_values = length of the values vector
 * (0 => pattern).  info.indptr_len = ncols + 1; info.nnz = entries after duplicates are merged. */
int mx_csr_transpose_begin(const int32_t *indptr, int nrows, int ncols, const int32_t *indices,
                           const void *values, int value_dtype, int64_t n_values,
                           mx_result **res, mx_result_info *info);
/* as.csr.matrix / as.csc.matrix of a TsparseMatrix (Matrix's T -> R / T -> C coercion, R/conversions.R:180-295)
 * through mxd_coo_to_csr: nrows x ncols COO with n_entries triplets; value_dtype MX_F64 / MX_LGL / MX_NONE.
 * Pass (ncols, nrows, cols, rows) for the CSC.  info.indptr_len = nrows + 1; info.nnz = entries after merging. */
int mx_coo_to_csr_begin(const int32_t *rows, const int32_t *cols, const void *values, int value_dtype,
                        int64_t n_entries, int nrows, int ncols, mx_result **res, mx_result_info *info);
/* as.coo.matrix of a CSR / CSC (R/conversions.R:515-590): out_rows[indptr[nrows]] receives the row (CSC: column)
 * of every entry in storage order. */
int mx_csr_to_coo(const int32_t *indptr, int nrows, int32_t *out_rows);
/* multiply_csr_by_coo_elemwise / logicaland_csr_by_coo_elemwise  src/operators.cpp:572-720 (RcppExports.cpp:1319,
 * 1336): logical = 0 f64, 1 R logicals.  X_indptr has max_row_X + 1 entries.  The result is a COO held in the
 * mx_result: the indptr vector holds the row ids (info.indptr_len = info.nnz), indices the column ids, values
 * the values. */
int mx_multiply_csr_by_coo_begin(int logical, const int32_t *X_indptr, const int32_t *X_indices,
                                 const void *X_values, const int32_t *Y_rows, const int32_t *Y_cols,
                                 const void *Y_values, int64_t nnz_Y, int max_row_X, int max_col_X,
                                 mx_result **res, mx_result_info *info);
/* multiply_coo_by_dense_ignore_NAs_numeric  src/operators.cpp:3363-3394: flags as for
 * mx_multiply_csr_by_dvec_no_NAs_numeric; values_out f64[nnz]. */
int mx_multiply_coo_by_dense_ignore_NAs_numeric(const int32_t *ii, const int32_t *jj, const double *xx, int64_t nnz,
                                                const double *dvec, int64_t dvec_len, int nrows, int ncols,
                                                int multiply, int powerto, int divide, int divrest, int intdiv,
                                                int X_is_LHS, double *values_out);
/* multiply_coo_by_dense_ignore_NAs_logical  src/operators.cpp:3396-3418: R logicals, values_out int32[nnz] */
int mx_multiply_coo_by_dense_ignore_NAs_logical(const int32_t *ii, const int32_t *jj, const int32_t *xx, int64_t nnz,
                                                const int32_t *dvec, int64_t dvec_len, int nrows, int ncols,
                                                int32_t *values_out);
/* slice_coo_arbitrary_{numeric,logical,binary}  src/slice_coo.cpp:123-706 (RcppExports.cpp:2103-2167), through
 * mxd_coo_slice_count / _fill: ii / jj / xx hold nnz 0-based triplets (value_dtype MX_F64 / MX_LGL / MX_NONE);
 * rows_take_base1 / cols_take_base1 are the 1-based selectors and the six flags are get_ij_properties' (R/slice.R:
 * 59-143).  The result is a COO held in the mx_result, as for mx_multiply_csr_by_coo_begin: the indptr vector
 * holds the row ids (info.indptr_len = info.nnz), indices the column ids, values the values.  An empty selector
 * or nnz = 0 gives an empty result. */
int mx_slice_coo_arbitrary_begin(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype,
                                 int64_t nnz, const int32_t *rows_take_base1, int64_t n_rows_take,
                                 const int32_t *cols_take_base1, int64_t n_cols_take, int all_i, int all_j,
                                 int i_is_seq, int j_is_seq, int i_is_rev_seq, int j_is_rev_seq, int nrows,
                                 int ncols, mx_result **res, mx_result_info *info);
/* slice_coo_single_{numeric,logical,binary}  src/slice_coo.cpp:3-71 (RcppExports.cpp:2061-2101): i, j 0-based;
 * *found = 1 when some triplet matches, and value_out (when non-null; f64 for MX_F64, int32 for MX_LGL) receives
 * the value of the first one in storage order. */
int mx_slice_coo_single(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype, int64_t nnz, int i,
                        int j, int *found, void *value_out);
/* inject_NAs_inplace_coo_{numeric,logical}  src/slice_coo.cpp:902-946 (R/slice.R:177-194), through
 * mxd_coo_inject_na_count / _fill: value_dtype MX_F64 or MX_LGL; rows_na / cols_na 0-based, ascending, distinct.
 * The result is a COO held in the mx_result, as for mx_slice_coo_arbitrary_begin.  Both lists empty gives an empty
 * result (the reference returns an empty list there, and R then leaves the matrix alone). */
int mx_inject_NAs_inplace_coo_begin(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype,
                                    int64_t nnz, const int32_t *rows_na, int64_t n_rows_na, const int32_t *cols_na,
                                    int64_t n_cols_na, int nrows, int ncols, mx_result **res, mx_result_info *info);
/* extract_single_val_csr_{numeric,logical,binary}  src/slice.cpp:737-785: row, col 0-based; *found = 1 when the row
 * stores the column, and value_out (when non-null; f64 for MX_F64, int32 for MX_LGL) receives the value of the first
 * such entry in storage order. */
int mx_extract_single_val_csr(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                              int value_dtype, int row, int col, int *found, void *value_out);
/* repeat_indices_n_times  src/slice.cpp:636-659; out holds n_indices * (desired_length / ix_length) + n_remainder
 * entries. */
int mx_repeat_indices_n_times(const int32_t *indices, int64_t n_indices, const int32_t *remainder,
                              int64_t n_remainder, int ix_length, int desired_length, int32_t *out);
/* as.vector() of a one-row / one-column slice (drop_slice, R/slice.R:210-236) through mxd_entries_to_dense_vector:
 * out[len] of out_dtype (MX_F64, or MX_LGL for int32 R logicals); pos are distinct 0-based positions inside
 * [0, len). */
int mx_entries_to_dense_vector(const int32_t *pos, const void *values, int value_dtype, int64_t n, void *out,
                               int out_dtype, int64_t len);
/* remove_sparse_zeros (R/utils.R:255-346) through mxd_compact_count / _fill.  remove_NAs is the na.rm flag; the
 * keep rule of each export is the reference's loop, quirks included.  When every entry is kept,
 * info.alias_structure = MX_ALIAS_ALL: the reference returns the input vectors themselves (src/misc.cpp:586-590,
 * :735-739, :864-867); nothing is allocated and finish copies nothing.  Otherwise the result is new vectors:
 *   CSR / CSC  indptr (nrows + 1), indices, values
 *   COO        the indptr vector holds ii (info.indptr_len = info.nnz), indices jj, values xx
 *   svec       indptr is empty (info.indptr_len = 0), indices ii, values xx */
#define MX_ALIAS_ALL 2
/* remove_zero_valued_csr_numeric / _logical  src/misc.cpp:667-699 (indptr has nrows + 1 entries; a CSC passes
 * (p, i) and ncol): keep x != 0 (numeric, na.rm: and not NaN; logical: FALSE removed, na.rm: only NA removed) */
int mx_remove_zero_valued_csr_numeric(const int32_t *indptr, const int32_t *indices, const double *values, int nrows,
                                      int remove_NAs, mx_result **res, mx_result_info *info);
int mx_remove_zero_valued_csr_logical(const int32_t *indptr, const int32_t *indices, const int32_t *values,
                                      int nrows, int remove_NAs, mx_result **res, mx_result_info *info);
/* remove_zero_valued_coo_numeric / _logical  src/misc.cpp:790-822: keep x != 0 (na.rm: and not NaN / NA) */
int mx_remove_zero_valued_coo_numeric(const int32_t *ii, const int32_t *jj, const double *xx, int64_t nnz,
                                      int remove_NAs, mx_result **res, mx_result_info *info);
int mx_remove_zero_valued_coo_logical(const int32_t *ii, const int32_t *jj, const int32_t *xx, int64_t nnz,
                                      int remove_NAs, mx_result **res, mx_result_info *info);
/* remove_zero_valued_svec_numeric / _integer / _logical  src/misc.cpp:925-968: keep x != 0 (numeric, na.rm: NaN
 * still kept; integer / logical, na.rm: and not NA) */
int mx_remove_zero_valued_svec_numeric(const int32_t *ii, const double *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info);
int mx_remove_zero_valued_svec_integer(const int32_t *ii, const int32_t *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info);
int mx_remove_zero_valued_svec_logical(const int32_t *ii, const int32_t *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info);
/* filterSparse's x[mask] with the indices taken along (R/utils.R:608-674), through the same compaction:
 * layout 0 CSR / CSC (indptr with nrows + 1 entries, idx0), 1 COO (idx0 = i, idx1 = j), 2 svec (idx0); mask is
 * nnz R logicals: FALSE drops the entry, NA keeps it with the kind's NA as its value.  value_dtype MX_F64 / MX_LGL /
 * MX_I32.  Results are laid out as for the remove_zero_valued_* exports and are always new vectors. */
int mx_filter_sparse_begin(int layout, const int32_t *indptr, int nrows, const int32_t *idx0, const int32_t *idx1,
                           const void *values, int value_dtype, int64_t nnz, const int32_t *mask, mx_result **res,
                           mx_result_info *info);
/* rebuild_indptr_after_filter  src/misc.cpp:1099-1116: out_indptr[indptr_len]; filter has indptr[indptr_len - 1]
 * R logicals (0 removes, anything else, NA included, keeps); indptr[0] must be 0. */
int mx_rebuild_indptr_after_filter(const int32_t *indptr, int64_t indptr_len, const int32_t *filter,
                                   int32_t *out_indptr);
/* check_valid_csr_matrix  src/misc.cpp:970-1017: *err receives the reference's message of the first failing check,
 * or NULL.  indptr has indptr_len entries (all checked for NA); monotonicity is checked over the first
 * min(nrows, indptr_len - 1) pointers; indices are checked against ncols.  nnz = 0 passes the index checks. */
int mx_check_valid_csr_matrix(const int32_t *indptr, int64_t indptr_len, const int32_t *indices, int64_t nnz,
                              int nrows, int ncols, const char **err);
/* check_valid_coo_matrix  src/misc.cpp:1018-1068: ii against nrows, then jj against ncols */
int mx_check_valid_coo_matrix(const int32_t *ii, const int32_t *jj, int64_t nnz, int nrows, int ncols,
                              const char **err);
/* check_valid_svec  src/misc.cpp:1069-1097: ii against nrows (the R caller passes 1-based ii and the length) */
int mx_check_valid_svec(const int32_t *ii, int64_t nnz, int nrows, const char **err);
/* `[<-` of a dgRMatrix (R/assignment.R:37-513; api_assign.hip, through mxd_csr_assign_* / mxd_csr_replace_rows_*).
 * A selector is a kind and 0-based indices: MX_SEL_ALL, MX_SEL_SINGLE (lo), MX_SEL_RANGE (lo..hi) or
 * MX_SEL_ARBITRARY (set[0..n_set), any order, no duplicates).  info.alias_structure follows the reference export by
 * export: MX_ALIAS_ALL where it returns the input vectors themselves (nothing to remove), 1 where it returns the
 * input indptr / indices with new values (the diff == 0 branches of the const routes), else 0. */
typedef enum { MX_SEL_ALL = 0, MX_SEL_SINGLE = 1, MX_SEL_RANGE = 2, MX_SEL_ARBITRARY = 3 } mx_sel_kind;
/* X[i, j] <- value: the twenty set_*_to_zero / set_*_to_const exports of src/assignment.cpp:384-769 (single row /
 * col / val), :1135-1364 (rowseq, colseq), :1366-1793 (arbitrary rows, arbitrary cols) and :1795-2476 (arbitrary rows
 * x single col, single row x arbitrary cols, arbitrary x arbitrary).  The zero route is value == 0 (-0.0 included);
 * anything else, NaN and NA included, is the const route, whose rows must be sorted. */
int mx_assign_csr_scalar_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                               int ncols, int i_kind, int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set,
                               int j_kind, int j_lo, int j_hi, const int32_t *cols_set, int64_t n_cols_set,
                               double value, mx_result **res, mx_result_info *info);
/* X[i, ] <- value, value a CSR of v_nrows = length(i) rows: set_rowseq_to_smat and set_arbitrary_rows_to_smat,
 * src/assignment.cpp:2478-2598, without the latter's tail defect (:2554) and in any order of the selector: row
 * set[k] (or lo + k) becomes row k of the value. */
int mx_assign_csr_rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                             int i_kind, int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set,
                             const int32_t *v_indptr, int64_t v_nrows, const int32_t *v_indices,
                             const double *v_values, mx_result **res, mx_result_info *info);
/* X[row, ] <- vector: set_single_row_to_rowvec (src/assignment.cpp:771-837; ii == NULL, length == n_xx) and
 * set_single_row_to_svec (:915-1007; ii as stored, any order).  The row becomes the pattern recycled ncols / length
 * times, every other row is copied.  info.alias_structure = 1 when the row's indices already equal the recycled
 * pattern element for element (only values are made); the fast path of :939-966 is taken on that condition alone, so
 * its two defects (a read past ii, values written past a shorter row) are not copied.  An ii without entries empties
 * the row.  A full row that is not sorted gives three new vectors (the reference returns its indptr, :800-808). */
int mx_assign_csr_row_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                int ncols, int row, const int32_t *ii, const double *xx, int64_t n_xx, int length,
                                mx_result **res, mx_result_info *info);
/* X[, col] <- vector: set_single_col_to_colvec (src/assignment.cpp:839-913; ii == NULL, length == n_xx) and
 * set_single_col_to_svec (:1009-1133; ii strictly ascending), recycled nrows / length times.  Rows that are not sorted
 * are sorted in the device copy first.  info.alias_structure = 1 for a dense vector when every row already stores
 * the column and no row had to be sorted; a sparse vector never aliases, as in the reference. */
int mx_assign_csr_col_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                int ncols, int col, const int32_t *ii, const double *xx, int64_t n_xx, int length,
                                mx_result **res, mx_result_info *info);
int mx_result_finish(mx_result *res, int32_t *out_indptr, int32_t *out_indices, void *out_values);
int mx_result_discard(mx_result *res);

/* check_is_seq / check_is_rev_seq  src/slice.cpp:25-47 (RcppExports.cpp:1795,1805) */
int mx_check_is_seq(const int32_t *indices, int64_t n, int *result);
int mx_check_is_rev_seq(const int32_t *indices, int64_t n, int *result);

/* §8(f)-1: sort_sparse_indices (R/utils.R:22-161 -> src/misc.cpp:261-298,333-347) and
 * check_is_sorted (src/misc.cpp:118-128) for a CSR held in host memory; sorts in place. */
int mx_check_indices_are_sorted(const int32_t *indptr, const int32_t *indices, int nrows, int *result);
int mx_sort_sparse_indices(const int32_t *indptr, int32_t *indices, void *values,
                           int value_dtype, int nrows);
/* sort_vector_indices_{numeric,integer,logical,binary}  src/misc.cpp:460-527 (R/utils.R:126-155): a sparse vector's
 * ii (and xx; MX_NONE with NULL for an nsparseVector) in host memory, sorted in place; left alone when sorted. */
int mx_sort_vector_indices(int32_t *ii, void *xx, int64_t n, int value_dtype);
/* sort_coo_indices_{numeric,logical,binary}  src/misc.cpp:387-457 (R/utils.R:85-124): a TsparseMatrix's ii, jj (and
 * xx: MX_F64, MX_LGL, or MX_NONE with NULL for an ngTMatrix) in host memory, sorted by (ii, jj) in place through
 * mxd_coo_sort.  The caller's arrays are written only on success and only when they were not already sorted; more
 * than INT32_MAX entries fail before anything is allocated. */
int mx_sort_coo_indices(int32_t *ii, int32_t *jj, void *xx, int64_t nnz, int value_dtype);
/* multiply_csr_by_svec_no_NAs (keep_NAs = 0) and multiply_csr_by_svec_keep_NAs  src/operators.cpp:3426-3697,
 * through mxd_csr_by_svec_count / _fill: a new indptr (nrows + 1), indices and f64 values.  ii_base1 sorted, xx NULL
 * for an nsparseVector, length dividing nrows.  A result above INT32_MAX entries (dense-filled rows) fails before
 * anything is allocated for it; the reference does not check. */
int mx_multiply_csr_by_svec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                  const int32_t *ii_base1, const double *xx, int64_t nnz_v, int ncols, int length,
                                  int keep_NAs, mx_result **res, mx_result_info *info);

/* matmul_colvec_by_scolvecascsr (colvec_dtype MX_F64) / _f32 (MX_F32, the float32@Data bits)  src/matmul.cpp:686-781,
 * through mxd_csr_outer_dense_count / _fill: a CSR of nrows rows (indptr nrows + 1), indices and f64 values of
 * out_indptr[nrows] entries (the reference pads to length(indices) * dim).  `indices` is not read.  (non-empty rows) *
 * dim above INT32_MAX fails before anything is allocated; the reference does not check. */
int mx_matmul_colvec_by_scolvecascsr_begin(const void *colvec, int colvec_dtype, int dim, const int32_t *indptr,
                                           int nrows, const int32_t *indices, const double *values,
                                           mx_result **res, mx_result_info *info);
/* matmul_spcolvec_by_scolvecascsr_{numeric,integer,logical,binary}  src/matmul.cpp:783-938 (value_dtype MX_F64 /
 * MX_I32 / MX_LGL / MX_NONE with y_values NULL), through mxd_csr_outer_svec_count / _fill: a CSC of y_length columns
 * (indptr y_length + 1), row indices and f64 values.  Uses y_values[k] where the reference reads y_values[col]
 * (:808, out of bounds for a vector that stores fewer positions than its length).  (non-empty rows) * nnz_y above
 * INT32_MAX fails before anything is allocated. */
int mx_matmul_spcolvec_by_scolvecascsr_begin(const int32_t *X_indptr, int nrows, const int32_t *X_indices,
                                             const double *X_values, const int32_t *y_indices_base1,
                                             const void *y_values, int value_dtype, int64_t nnz_y, int y_length,
                                             mx_result **res, mx_result_info *info);
/* matmul_rowvec_by_csc / matmul_rowvec_by_cscbin (values NULL)  src/matmul.cpp:643-684: out[ncols] float32; every
 * index must lie in [0, len_rowvec), which is checked here and not in the reference */
int mx_matmul_rowvec_by_csc(const float *rowvec, int64_t len_rowvec, const int32_t *indptr, int ncols,
                            const int32_t *indices, const double *values, float *out);

/* multiply_elemwise_dense_by_svec_{numeric,float32,integer,logical}  src/operators.cpp:3699-4379 (kind 0, 1, 2, 3 as
 * for the csc (.) dense entries; X_colmajor holds nrows * ncols doubles, float32 values or R integers / logicals).
 * mx_dense_by_svec_route is the reference's choice of route (:3720, :3765, :3984, :4235), taken in that order:
 *   MX_DSV_ROUTE_A  length == nrows * ncols                    dense result
 *   MX_DSV_ROUTE_B  length == nrows                            CSR result
 *   MX_DSV_ROUTE_C  length < nrows and nrows % length == 0     CSR result, the vector recycled down the rows
 *   MX_DSV_ROUTE_D  anything else                              dense result, the vector recycled over the cells
 * or -1 for a negative argument, or a vector without length next to a matrix with cells.
 * _begin serves routes B and C through mxd_dense_by_svec_count / _fill: a new indptr (nrows + 1), indices and f64
 * values; _dense serves routes A and D through mxd_dense_by_svec_dense and writes out_colmajor[nrows * ncols].  Either
 * fails on the other's routes.  Refused before any launch, where the reference checks nothing: a position outside
 * 1..length, nnz_v > length, and (through the count) a CSR result above INT32_MAX entries.  ii_base1 sorted when
 * keep_NAs is set, as the R side makes it. */
typedef enum { MX_DSV_ROUTE_A = 0, MX_DSV_ROUTE_B = 1, MX_DSV_ROUTE_C = 2, MX_DSV_ROUTE_D = 3 } mx_dsv_route;
int mx_dense_by_svec_route(int nrows, int ncols, int length);
int mx_multiply_elemwise_dense_by_svec_begin(const void *X_colmajor, int kind, int nrows, int ncols,
                                             const int32_t *ii_base1, const double *xx, int64_t nnz_v, int length,
                                             int keep_NAs, mx_result **res, mx_result_info *info);
int mx_multiply_elemwise_dense_by_svec_dense(const void *X_colmajor, int kind, int nrows, int ncols,
                                             const int32_t *ii_base1, const double *xx, int64_t nnz_v, int length,
                                             int keep_NAs, double *out_colmajor);
/* multiply_coo_by_dense_{numeric,integer,logical,float32}  src/operators.cpp:772-838, and
 * logicaland_coo_by_dense_logical  :840-855, through mxd_coo_by_dense: values_out[nnz] (f64; R logicals for the
 * and); the row and column vectors of the result are the caller's (the reference copies them, :763-769).  X_colmajor
 * is nrows x ncols.  An entry with ii outside [0, nrows) or jj outside [0, ncols) is refused before any launch; the
 * reference does not check. */
int mx_multiply_coo_by_dense_numeric(const double *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out);
int mx_multiply_coo_by_dense_integer(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out);
int mx_multiply_coo_by_dense_logical(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out);
int mx_multiply_coo_by_dense_float32(const float *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out);
int mx_logicaland_coo_by_dense_logical(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                       const int32_t *jj, const int32_t *xx, int64_t nnz, int32_t *values_out);

#ifdef __cplusplus
}
#endif
#endif /* MXGPU_H */

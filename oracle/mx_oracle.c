/* mx_oracle.c — CPU restatement of MatrixExtra's CSR hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  This file is the checker the HIP kernels are
 * compared against and the timed "cpu_baseline" of bench.py.  Nothing under
 * matrixextra_amd/ may import, link or call it; the product path has no CPU
 * fallback.
 *
 * Parity status: pinned by reference-run outputs.  The reference's own
 * translation units compile behind the R / Rcpp / BLAS stand-in of
 * oracle/refshim into oracle/_ref/libmxref.so (`make ref`), and
 * tests/test_reference_pin.py holds this file to them: against the committed
 * reference-run fixture tests/golden/reference_golden.npz always, and against
 * the live library on a wider sweep where it is built.  The non-FMA variant
 * here equals the reference bit for bit, SpMM and SpMV included.
 * The older pins stay as well: the literal known answers of the reference tree
 * and the dense numpy / scipy evaluation of tests/test_oracle.py.
 *
 * Each function cites the reference lines it follows.  BLAS daxpy/dcopy
 * (matmul.cpp:45,50,72) are replaced by the plain loops the reference itself
 * uses for float (matmul.cpp:17-40).  `use_fma` selects fused multiply-add in
 * the axpy (what an FMA-enabled BLAS and the GPU do) or separate mul+add.
 *
 * Build: see oracle/Makefile  (gcc -O3 -march=native -fopenmp -ffp-contract=off).
 */
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define NA_INT INT_MIN /* R: NA_INTEGER == NA_LOGICAL == INT_MIN */

static double na_real(void)
{
    /* R's NA_real_: quiet NaN whose low word is 1954 (arithmetic.c R_NaReal) */
    union { uint64_t u; double d; } x;
    x.u = 0x7FF00000000007A2ULL;
    return x.d;
}

int mxo_max_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ---- axpy helpers (matmul.cpp:17-67) ------------------------------------- */
static inline void axpy_f64(int n, double a, const double *x, double *y, int use_fma)
{
    if (use_fma) for (int i = 0; i < n; i++) y[i] = fma(a, x[i], y[i]);
    else         for (int i = 0; i < n; i++) y[i] += a * x[i];
}
/* float path: alpha narrowed to float first (matmul.cpp:53-57), and saxpy's
 * alpha == 1 branch adds without the multiply (matmul.cpp:23-27: identical value). */
static inline void axpy_f32(int n, double a, const float *x, float *y, int use_fma)
{
    const float af = (float)a;
    if (use_fma) for (int i = 0; i < n; i++) y[i] = fmaf(af, x[i], y[i]);
    else         for (int i = 0; i < n; i++) y[i] += af * x[i];
}

/* ---- gemm_csr_drm_as_drm (matmul.cpp:118-142) ---------------------------- */
/* X <- A*B + X, A CSR m x k, B row-major (ldb), X row-major (ldc) */
#define DEF_DRM(NAME, T, AXPY)                                                      \
void NAME(int m, int n, const int *indptr, const int *indices, const double *values, \
          const T *B, size_t ldb, T *C, size_t ldc, int nthreads, int use_fma)       \
{                                                                                    \
    if (m <= 0 || indptr[0] == indptr[m]) return;                                    \
    if (nthreads < 1) nthreads = 1;                                                  \
    _Pragma("omp parallel for schedule(dynamic) num_threads(nthreads)")              \
    for (int row = 0; row < m; row++) {                                              \
        T *row_ptr = C + (size_t)row * ldc;                                          \
        for (int ix = indptr[row]; ix < indptr[row + 1]; ix++)                       \
            AXPY(n, values[ix], B + (size_t)indices[ix] * ldb, row_ptr, use_fma);    \
    }                                                                                \
}
DEF_DRM(mxo_gemm_csr_drm_as_drm_f64, double, axpy_f64)
DEF_DRM(mxo_gemm_csr_drm_as_drm_f32, float, axpy_f32)

/* ---- gemm_csr_drm_as_dcm (matmul.cpp:150-185) ---------------------------- */
/* X <- A*B, X column-major with leading dim ldc.  Per-thread scratch row, then
 * strided copy.  The reference sizes the scratch by ldc (=m) but uses ldb (=n)
 * entries (matmul.cpp:176,179): an overflow when n > m.  Sized by max(n, ldb) here. */
#define DEF_DCM(NAME, T, AXPY)                                                      \
void NAME(int m, int n, const int *indptr, const int *indices, const double *values, \
          const T *B, size_t ldb, T *C, int ldc, int nthreads, int use_fma)          \
{                                                                                    \
    if (m <= 0 || indptr[0] == indptr[m]) return;                                    \
    if (nthreads < 1) nthreads = 1;                                                  \
    if (nthreads > m) nthreads = m;                                                  \
    _Pragma("omp parallel num_threads(nthreads)")                                    \
    {                                                                                \
        T *scratch = NULL;                                                           \
        _Pragma("omp for schedule(dynamic)")                                         \
        for (int row = 0; row < m; row++) {                                          \
            if (indptr[row] < indptr[row + 1]) {                                     \
                if (!scratch) scratch = (T *)malloc(sizeof(T) * (ldb > (size_t)n ? ldb : (size_t)n)); \
                memset(scratch, 0, ldb * sizeof(T));                                 \
                for (int ix = indptr[row]; ix < indptr[row + 1]; ix++)               \
                    AXPY(n, values[ix], B + (size_t)indices[ix] * ldb, scratch, use_fma); \
                for (int c = 0; c < n; c++) C[(size_t)row + (size_t)c * (size_t)ldc] = scratch[c]; \
            }                                                                        \
        }                                                                            \
        free(scratch);                                                               \
    }                                                                                \
}
DEF_DCM(mxo_gemm_csr_drm_as_dcm_f64, double, axpy_f64)
DEF_DCM(mxo_gemm_csr_drm_as_dcm_f32, float, axpy_f32)

/* ---- matmul_csr_dvec (matmul.cpp:381-419) -------------------------------- */
/* kind: 0 numeric (f64 y), 1 integer, 2 logical, 3 float32 (y and out float) */
void mxo_matmul_csr_dvec(int nrows, const int *indptr, const int *indices, const double *values,
                         const void *y_dense, int kind, void *out, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    const double NA = na_real();
    #pragma omp parallel for schedule(dynamic) num_threads(nthreads)
    for (int row = 0; row < nrows; row++) {
        if (kind == 3) {
            const float *y = (const float *)y_dense;
            float val = 0; /* OutputDType val: float accumulate, double product (matmul.cpp:403,413) */
            for (int ix = indptr[row]; ix < indptr[row + 1]; ix++)
                val += values[ix] * y[indices[ix]];
            ((float *)out)[row] = val;
        } else {
            double val = 0;
            for (int ix = indptr[row]; ix < indptr[row + 1]; ix++) {
                if (kind == 1) {
                    const int yv = ((const int *)y_dense)[indices[ix]];
                    val += (yv == NA_INT) ? NA : values[ix] * yv;
                } else if (kind == 2) {
                    const int yv = ((const int *)y_dense)[indices[ix]];
                    val += (yv == NA_INT) ? NA : values[ix] * (double)(yv != 0);
                } else {
                    val += values[ix] * ((const double *)y_dense)[indices[ix]];
                }
            }
            ((double *)out)[row] = val;
        }
    }
}

/* ---- R logical tables (operators.cpp:17-25 / :28-93) --------------------- */
static inline int r_or(int x, int y)
{
    if (x == NA_INT) return (y == NA_INT) ? NA_INT : (y ? 1 : NA_INT);
    if (y == NA_INT) return x ? 1 : NA_INT;
    return (x != 0) || (y != 0);
}
static inline int r_and(int x, int y)
{
    if (x == NA_INT) return (y == NA_INT) ? NA_INT : (y ? NA_INT : 0);
    if (y == NA_INT) return x ? NA_INT : 0;
    return (x != 0) && (y != 0);
}
static inline int r_xor(int x, int y)
{
    if (x == NA_INT || y == NA_INT) return NA_INT;
    return (x != 0) != (y != 0);
}
int mxo_r_logical(int which, int x, int y)
{
    return which == 0 ? r_or(x, y) : which == 1 ? r_and(x, y) : r_xor(x, y);
}

static const int *lower_bound_int(const int *first, const int *last, int value)
{
    size_t count = (size_t)(last - first);
    while (count > 0) {
        size_t step = count / 2;
        const int *it = first + step;
        if (*it < value) { first = it + 1; count -= step + 1; }
        else count = step;
    }
    return first;
}

/* ---- multiply_csr_elemwise (operators.cpp:99-207) ------------------------ */
/* logical==0: f64 product; logical==1: R_logical_and on int values.
 * Outputs must hold min(nnz1,nnz2) entries (operators.cpp:139-143).
 * Returns nnz_out.  The identical-pattern fast path (pointer identity,
 * operators.cpp:104-132) is restated in oracle.py (it aliases R objects). */
size_t mxo_multiply_csr_elemwise(int nrows, const int *indptr1, const int *indptr2,
                                 const int *indices1, const int *indices2,
                                 const void *values1, const void *values2, int logical,
                                 int *indptr_out, int *indices_out, void *values_out)
{
    size_t curr = 0;
    indptr_out[0] = 0;
    for (int row = 0; row < nrows; row++) {
        if (indptr1[row] == indptr1[row + 1] || indptr2[row] == indptr2[row + 1]) goto next_row;
        if (indices1[indptr1[row + 1] - 1] < indices2[indptr2[row]] ||
            indices2[indptr2[row + 1] - 1] < indices1[indptr1[row]]) goto next_row;
        {
            const int *ptr1 = indices1 + indptr1[row], *end1 = indices1 + indptr1[row + 1];
            const int *ptr2 = indices2 + indptr2[row], *end2 = indices2 + indptr2[row + 1];
            while (1) {
                if (ptr1 >= end1 || ptr2 >= end2) goto next_row;
                else if (*ptr1 == *ptr2) {
                    indices_out[curr] = *ptr1;
                    if (!logical)
                        ((double *)values_out)[curr] = ((const double *)values1)[ptr1 - indices1] *
                                                       ((const double *)values2)[ptr2 - indices2];
                    else
                        ((int *)values_out)[curr] = r_and(((const int *)values1)[ptr1 - indices1],
                                                          ((const int *)values2)[ptr2 - indices2]);
                    ptr1++; ptr2++; curr++;
                }
                else if (*ptr1 > *ptr2) ptr2 = lower_bound_int(ptr2, end2, *ptr1);
                else                    ptr1 = lower_bound_int(ptr1, end1, *ptr2);
            }
        }
        next_row:
        indptr_out[row + 1] = (int)curr;
    }
    return curr;
}

/* ---- add_csr_elemwise (operators.cpp:337-537) ---------------------------- */
/* mode 0: f64 add/sub (substract flag); mode 1: logical or; mode 2: logical xor.
 * Outputs must hold nnz1+nnz2 entries (operators.cpp:402-406).  Returns nnz_out. */
size_t mxo_add_csr_elemwise(int nrows, const int *indptr1, const int *indptr2,
                            const int *indices1, const int *indices2,
                            const void *values1_, const void *values2_,
                            int mode, int substract,
                            int *indptr_out, int *indices_out, void *values_out_)
{
    const double *v1d = (const double *)values1_, *v2d = (const double *)values2_;
    const int *v1i = (const int *)values1_, *v2i = (const int *)values2_;
    double *vod = (double *)values_out_;
    int *voi = (int *)values_out_;
    const int lgl = mode != 0;
    size_t curr = 0;
    indptr_out[0] = 0;
#define PUT1(pos) do { indices_out[curr] = indices1[pos]; \
        if (lgl) voi[curr] = v1i[pos]; else vod[curr] = v1d[pos]; curr++; } while (0)
#define PUT2(pos) do { indices_out[curr] = indices2[pos]; \
        if (lgl) voi[curr] = v2i[pos]; else vod[curr] = substract ? -v2d[pos] : v2d[pos]; curr++; } while (0)
    for (int row = 0; row < nrows; row++) {
        int p1 = indptr1[row], e1 = indptr1[row + 1];
        int p2 = indptr2[row], e2 = indptr2[row + 1];
        if (p1 == e1 && p2 == e2) goto next_row;
        else if (p1 == e1) { for (; p2 < e2; p2++) PUT2(p2); goto next_row; }
        else if (p2 == e2) { for (; p1 < e1; p1++) PUT1(p1); goto next_row; }
        while (1) {
            if (p1 >= e1 || p2 >= e2) {
                for (; p1 < e1; p1++) PUT1(p1);
                for (; p2 < e2; p2++) PUT2(p2);
                goto next_row;
            }
            else if (indices1[p1] == indices2[p2]) {
                indices_out[curr] = indices1[p1];
                if (!lgl) vod[curr] = v1d[p1] + (substract ? (-v2d[p2]) : v2d[p2]);
                else      voi[curr] = (mode == 2) ? r_xor(v1i[p1], v2i[p2]) : r_or(v1i[p1], v2i[p2]);
                curr++; p1++; p2++;
            }
            else if (indices1[p1] > indices2[p2]) {
                do { PUT2(p2); p2++; } while (p2 < e2 && indices2[p2] < indices1[p1]);
            }
            else {
                do { PUT1(p1); p1++; } while (p1 < e1 && indices1[p1] < indices2[p2]);
            }
        }
        next_row:
        indptr_out[row + 1] = (int)curr;
    }
#undef PUT1
#undef PUT2
    return curr;
}

/* ---- copy_csr_rows_template (slice.cpp:225-274) -------------------------- */
/* value_bytes: 8 (numeric), 4 (logical), 0 (binary / empty values vector).
 * Returns total nnz; when it is 0 the reference returns three EMPTY vectors
 * (slice.cpp:236-240) — the caller models that; nothing is written here then. */
size_t mxo_copy_csr_rows_size(const int *indptr, const int *rows_take, size_t n_take)
{
    size_t total = 0;
    for (size_t ix = 0; ix < n_take; ix++) total += (size_t)(indptr[rows_take[ix] + 1] - indptr[rows_take[ix]]);
    return total;
}
void mxo_copy_csr_rows(const int *indptr, const int *indices, const void *values, int value_bytes,
                       const int *rows_take, size_t n_take,
                       int *new_indptr, int *new_indices, void *new_values)
{
    size_t curr = 0;
    new_indptr[0] = 0;
    for (size_t ix = 0; ix < n_take; ix++) {
        const int row = rows_take[ix];
        const size_t n_copy = (size_t)(indptr[row + 1] - indptr[row]);
        new_indptr[ix + 1] = new_indptr[ix] + (int)n_copy;
        if (n_copy) {
            memcpy(new_indices + curr, indices + indptr[row], n_copy * sizeof(int));
            if (value_bytes)
                memcpy((char *)new_values + curr * (size_t)value_bytes,
                       (const char *)values + (size_t)indptr[row] * (size_t)value_bytes,
                       n_copy * (size_t)value_bytes);
        }
        curr += n_copy;
    }
}

/* ---- check_is_seq / check_is_rev_seq (slice.cpp:25-47) ------------------- */
int mxo_check_is_seq(const int *indices, size_t n)
{
    if (n < 2) return 1;
    if ((indices[n - 1] - indices[0]) != (int)n - 1) return 0;
    for (size_t ix = 1; ix < n; ix++) if (indices[ix] != indices[ix - 1] + 1) return 0;
    return 1;
}
int mxo_check_is_rev_seq(const int *indices, size_t n)
{
    if (n < 2) return 1;
    if ((indices[0] - indices[n - 1]) != (int)n - 1) return 0;
    for (size_t ix = 1; ix < n; ix++) if (indices[ix] != indices[ix - 1] - 1) return 0;
    return 1;
}

/* ---- check_is_sorted / sort_sparse_indices_known_ncol (misc.cpp:118-128, 261-298) */
int mxo_check_indices_are_sorted(const int *indptr, const int *indices, int nrows)
{
    for (int row = 0; row < nrows; row++)
        for (int ix = indptr[row] + 1; ix < indptr[row + 1]; ix++)
            if (indices[ix] < indices[ix - 1]) return 0;
    return 1;
}
/* Rows already non-decreasing are left alone (misc.cpp:283).  The reference
 * argsorts with a non-stable std::sort, so the relative order of EQUAL column
 * ids is unspecified there; this restatement (insertion sort) is stable. */
void mxo_sort_sparse_indices(const int *indptr, int *indices, void *values, int value_bytes, int nrows)
{
    for (int row = 0; row < nrows; row++) {
        const int s = indptr[row], e = indptr[row + 1];
        for (int i = s + 1; i < e; i++) {
            const int key = indices[i];
            double vd = 0; int vi = 0;
            if (value_bytes == 8) vd = ((double *)values)[i];
            else if (value_bytes == 4) vi = ((int *)values)[i];
            int k = i - 1;
            while (k >= s && indices[k] > key) {
                indices[k + 1] = indices[k];
                if (value_bytes == 8) ((double *)values)[k + 1] = ((double *)values)[k];
                else if (value_bytes == 4) ((int *)values)[k + 1] = ((int *)values)[k];
                k--;
            }
            indices[k + 1] = key;
            if (value_bytes == 8) ((double *)values)[k + 1] = vd;
            else if (value_bytes == 4) ((int *)values)[k + 1] = vi;
        }
    }
}

/* ==== §8(f) rank 2: column-filtering slices =================================================== */

/* ---- copy_csr_rows_col_seq_template (slice.cpp:326-383) ------------------ */
/* rows_take 0-based; keeps entries with min_col <= col <= max_col, re-based to min_col, input order kept.
 * value_kind: 0 none, 1 f64, 2 int32 (R logical) — output values are ALWAYS double (the reference builds an
 * Rcpp::NumericVector, slice.cpp:363).  Pass NULL outputs to only size the result.  Returns total entries;
 * new_indptr[n_take+1] is always written. */
size_t mxo_copy_csr_rows_col_seq(const int *indptr, const int *indices, const void *values, int value_kind,
                                 const int *rows_take, size_t n_take, int min_col, int max_col,
                                 int *new_indptr, int *new_indices, double *new_values)
{
    size_t total = 0;
    new_indptr[0] = 0;
    for (size_t row = 0; row < n_take; row++) {
        for (int ix = indptr[rows_take[row]]; ix < indptr[rows_take[row] + 1]; ix++) {
            if (indices[ix] >= min_col && indices[ix] <= max_col) {
                if (new_indices) {
                    new_indices[total] = indices[ix] - min_col;
                    if (value_kind == 1) new_values[total] = ((const double *)values)[ix];
                    else if (value_kind == 2) new_values[total] = (double)((const int *)values)[ix];
                }
                total++;
            }
        }
        new_indptr[row + 1] = (int)total;
    }
    return total;
}

/* ---- copy_csr_arbitrary_template (slice.cpp:449-578) --------------------- */
/* rows_take, cols_take 0-based.  A kept entry of column c goes to every position of c in cols_take
 * (ascending position; a non-repeated column: its only position).  Rows are then ordered by new column id
 * unless cols_take is non-decreasing (slice.cpp:487-493, 540-560).  value_bytes 0/4/8.
 * Pass NULL outputs to only size the result.  ncol = number of columns of the matrix (dense map instead of
 * the reference's hash map).  Returns total entries, or (size_t)-1 on allocation failure. */
static int cmp_pair_key(const void *a, const void *b)
{
    const int ka = ((const int *)a)[0], kb = ((const int *)b)[0];
    return (ka > kb) - (ka < kb);
}
size_t mxo_copy_csr_arbitrary(const int *indptr, const int *indices, const void *values, int value_bytes,
                              const int *rows_take, size_t n_take, const int *cols_take, size_t n_cols_take,
                              int ncol, int *new_indptr, int *new_indices, void *new_values)
{
    int *start = (int *)calloc((size_t)ncol + 2, sizeof(int));
    int *pos = (int *)malloc((n_cols_take ? n_cols_take : 1) * sizeof(int));
    if (!start || !pos) { free(start); free(pos); return (size_t)-1; }
    for (size_t c = 0; c < n_cols_take; c++) start[cols_take[c] + 2]++;
    for (int c = 0; c < ncol; c++) start[c + 2] += start[c + 1];           /* start[c+1] = first slot of column c */
    for (size_t c = 0; c < n_cols_take; c++) pos[start[cols_take[c] + 1]++] = (int)c;   /* ascending positions */
    /* now start[c] .. start[c+1] delimit column c's positions */
    int cols_sorted = 1;
    for (size_t c = 1; c < n_cols_take; c++) if (cols_take[c] < cols_take[c - 1]) { cols_sorted = 0; break; }
    size_t total = 0;
    new_indptr[0] = 0;
    for (size_t r = 0; r < n_take; r++) {
        const int row = rows_take[r];
        const size_t row_begin = total;
        for (int ix = indptr[row]; ix < indptr[row + 1]; ix++) {
            const int c = indices[ix];
            if (c < 0 || c >= ncol) continue;
            for (int q = start[c]; q < start[c + 1]; q++) {
                if (new_indices) {
                    new_indices[total] = pos[q];
                    if (value_bytes == 8) ((double *)new_values)[total] = ((const double *)values)[ix];
                    else if (value_bytes == 4) ((int *)new_values)[total] = ((const int *)values)[ix];
                }
                total++;
            }
        }
        new_indptr[r + 1] = (int)total;
        if (new_indices && !cols_sorted && total > row_begin + 1) {
            /* order the row by new column id (keys are unique inside a row of a valid matrix) */
            const size_t len = total - row_begin;
            int *tmp = (int *)malloc(len * 2 * sizeof(int));
            if (!tmp) { free(start); free(pos); return (size_t)-1; }
            for (size_t k = 0; k < len; k++) { tmp[2 * k] = new_indices[row_begin + k]; tmp[2 * k + 1] = (int)k; }
            qsort(tmp, len, 2 * sizeof(int), cmp_pair_key);
            if (value_bytes) {
                char *vt = (char *)malloc(len * (size_t)value_bytes);
                if (!vt) { free(tmp); free(start); free(pos); return (size_t)-1; }
                memcpy(vt, (char *)new_values + row_begin * (size_t)value_bytes, len * (size_t)value_bytes);
                for (size_t k = 0; k < len; k++)
                    memcpy((char *)new_values + (row_begin + k) * (size_t)value_bytes,
                           vt + (size_t)tmp[2 * k + 1] * (size_t)value_bytes, (size_t)value_bytes);
                free(vt);
            }
            for (size_t k = 0; k < len; k++) new_indices[row_begin + k] = tmp[2 * k];
            free(tmp);
        }
    }
    free(start); free(pos);
    return total;
}

/* ---- reverse_rows_template (slice.cpp:49-95) ------------------------------ */
void mxo_reverse_rows(const int *indptr, const int *indices, const void *values, int value_bytes, int nrows,
                      int *indptr_new, int *indices_new, void *values_new)
{
    indptr_new[0] = 0;
    for (int row = 0; row < nrows; row++) {
        const int rev = nrows - row - 1;
        const int n_this = indptr[rev + 1] - indptr[rev];
        indptr_new[row + 1] = indptr_new[row] + n_this;
        memcpy(indices_new + indptr_new[row], indices + indptr[rev], (size_t)n_this * sizeof(int));
        if (value_bytes)
            memcpy((char *)values_new + (size_t)indptr_new[row] * (size_t)value_bytes,
                   (const char *)values + (size_t)indptr[rev] * (size_t)value_bytes, (size_t)n_this * (size_t)value_bytes);
    }
}

/* ---- reverse_columns_inplace (slice.cpp:142-170) -------------------------- */
void mxo_reverse_columns_inplace(const int *indptr, int *indices, void *values, int value_bytes, int nrows, int ncol)
{
    for (int row = 0; row < nrows; row++) {
        const int s = indptr[row], e = indptr[row + 1];
        for (int ix = s; ix < e; ix++) indices[ix] = ncol - indices[ix] - 1;
        for (int a = s, b = e - 1; a < b; a++, b--) {
            const int t = indices[a]; indices[a] = indices[b]; indices[b] = t;
            if (value_bytes == 8) { double *v = (double *)values; const double tv = v[a]; v[a] = v[b]; v[b] = tv; }
            else if (value_bytes == 4) { int *v = (int *)values; const int tv = v[a]; v[a] = v[b]; v[b] = tv; }
        }
    }
}

/* ==== §8(f) rank 3: cbind / rbind of CSR ====================================================== */

/* ---- cbind_csr (cbind.cpp:4-99) ------------------------------------------- */
/* Y's column ids arrive already shifted by ncol(X) (R/cbind.R:87-97).  value_bytes 0/4/8 (0 when BOTH value
 * vectors are empty).  indptr[nrows+1], indices[nnzX+nnzY], values likewise.  nX / nY = number of rows. */
void mxo_cbind_csr(const int *Xp, const int *Xj, const void *Xx, int nX, const int *Yp, const int *Yj, const void *Yx,
                   int nY, int value_bytes, int *indptr, int *indices, void *values)
{
    const int nrows = nX > nY ? nX : nY, nmin = nX < nY ? nX : nY;
    indptr[0] = 0;
    for (int row = 0; row < nrows; row++) {
        const int lx = row < nX ? Xp[row + 1] - Xp[row] : 0;
        const int ly = row < nY ? Yp[row + 1] - Yp[row] : 0;
        indptr[row + 1] = indptr[row] + lx + ly;
        if (lx) memcpy(indices + indptr[row], Xj + Xp[row], (size_t)lx * sizeof(int));
        if (ly) memcpy(indices + indptr[row] + lx, Yj + Yp[row], (size_t)ly * sizeof(int));
        if (value_bytes) {
            if (lx) memcpy((char *)values + (size_t)indptr[row] * value_bytes, (const char *)Xx + (size_t)Xp[row] * value_bytes, (size_t)lx * value_bytes);
            if (ly) memcpy((char *)values + (size_t)(indptr[row] + lx) * value_bytes, (const char *)Yx + (size_t)Yp[row] * value_bytes, (size_t)ly * value_bytes);
        }
    }
    (void)nmin;
}

/* ---- concat_indptr2 (rbind.cpp:9-21) --------------------------------------- */
void mxo_concat_indptr2(const int *ptr1, int n1, const int *ptr2, int n2, int *out)
{
    memcpy(out, ptr1, (size_t)n1 * sizeof(int));
    const int offset = ptr1[n1 - 1];
    for (int row = 1; row < n2; row++) out[n1 + row - 1] = offset + ptr2[row];
}

/* ---- concat_csr_batch (rbind.cpp:24-173): one input appended at (curr_row, curr_pos) ---------------
 * in_kind: 0 dgRMatrix (f64), 1 lgRMatrix (int32), 2 ngRMatrix (no values),
 *          3 dsparseVector, 4 isparseVector, 5 lsparseVector, 6 nsparseVector (1-based `i`, one row)
 * out_kind: 0 dgRMatrix, 1 lgRMatrix, 2 ngRMatrix.  Returns the number of rows appended. */
int mxo_concat_csr_append(int in_kind, const int *indptr_obj, const int *indices_obj, const void *values_obj,
                          int nrows_add, int nnz_add, int out_kind, int curr_row, int curr_pos,
                          int *indptr_out, int *indices_out, void *values_out)
{
    const double NA = na_real();
    double *vd = (double *)values_out;
    int *vl = (int *)values_out;
    if (in_kind <= 2) {
        for (int row = 0; row < nrows_add; row++) indptr_out[row + curr_row + 1] = indptr_out[curr_row] + indptr_obj[row + 1];
        memcpy(indices_out + curr_pos, indices_obj, (size_t)nnz_add * sizeof(int));
    } else {
        indptr_out[curr_row + 1] = indptr_out[curr_row] + nnz_add;
        for (int el = 0; el < nnz_add; el++) indices_out[el + curr_pos] = indices_obj[el] - 1;
        nrows_add = 1;
    }
    const double *xd = (const double *)values_obj;
    const int *xi = (const int *)values_obj;
    for (int el = 0; el < nnz_add; el++) {
        if (out_kind == 0) {
            if (in_kind == 0 || in_kind == 3) vd[el + curr_pos] = xd[el];
            else if (in_kind == 1) vd[el + curr_pos] = xi[el] == NA_INT ? NA : xi[el];               /* rbind.cpp:76 */
            else if (in_kind == 4) vd[el + curr_pos] = xi[el] == NA_INT ? NA : xi[el];
            else if (in_kind == 5) vd[el + curr_pos] = xi[el] == NA_INT ? NA : (double)(xi[el] != 0);
            else vd[el + curr_pos] = 1.0;
        } else if (out_kind == 1) {
            if (in_kind == 1 || in_kind == 5) vl[el + curr_pos] = xi[el];
            else if (in_kind == 0 || in_kind == 3) vl[el + curr_pos] = isnan(xd[el]) ? NA_INT : (xd[el] != 0);
            else if (in_kind == 4) vl[el + curr_pos] = xi[el] == NA_INT ? NA_INT : (xi[el] != 0);
            else vl[el + curr_pos] = 1;
        }
    }
    return nrows_add;
}

/* ==== §8(f) rank 4: CSR x sparse vector, CSR (.) dense elementwise ============================== */

/* ---- matmul_csr_svec (matmul.cpp:486-551) --------------------------------- */
/* kind: 0 numeric, 1 integer, 2 logical, 3 binary (no y values), 4 float32 (y float).  y_indices 1-based sorted. */
void mxo_matmul_csr_svec(int nrows, const int *indptr, const int *indices, const double *values,
                         const int *y_indices_base1, size_t ny, const void *y_values, int kind, double *out, int nthreads)
{
    for (int r = 0; r < nrows; r++) out[r] = 0;
    if (!ny) return;
    if (nthreads < 1) nthreads = 1;
    const double NA = na_real();
    #pragma omp parallel for schedule(dynamic) num_threads(nthreads)
    for (int row = 0; row < nrows; row++) {
        const int *ptr1 = indices + indptr[row], *end1 = indices + indptr[row + 1];
        const int *ptr2 = y_indices_base1, *end_y = y_indices_base1 + ny;
        while (1) {
            if (ptr1 >= end1 || ptr2 >= end_y) break;
            else if (*ptr1 == (*ptr2) - 1) {
                const size_t iy = (size_t)(ptr2 - y_indices_base1), ix = (size_t)(ptr1 - indices);
                if (kind == 1) { const int yv = ((const int *)y_values)[iy]; out[row] += yv == NA_INT ? NA : values[ix] * yv; }
                else if (kind == 2) { const int yv = ((const int *)y_values)[iy]; out[row] += yv == NA_INT ? NA : values[ix] * (double)(yv != 0); }
                else if (kind == 3) out[row] += values[ix];
                else if (kind == 4) out[row] += values[ix] * ((const float *)y_values)[iy];
                else out[row] += values[ix] * ((const double *)y_values)[iy];
                ptr1++; ptr2++;
            }
            else if (*ptr2 - 1 > *ptr1) ptr1 = lower_bound_int(ptr1, end1, *ptr2 - 1);
            else ptr2 = lower_bound_int(ptr2, end_y, *ptr1 + 1);
        }
    }
}

/* ---- multiply_csr_by_dense_elemwise (operators.cpp:239-334) ---------------- */
/* dense_mat column-major nrows x ncol.  kind: 0 double, 1 float32, 2 integer, 3 logical (values f64, out f64);
 * kind 4: logical values AND logical dense (R_logical_and), out int32. */
void mxo_multiply_csr_by_dense_elemwise(int nrows, const int *indptr, const int *indices, const void *values,
                                        const void *dense_mat, int kind, void *values_out)
{
    const double NA = na_real();
    const size_t nr = (size_t)nrows;
    for (size_t row = 0; row < nr; row++) {
        for (int el = indptr[row]; el < indptr[row + 1]; el++) {
            const size_t at = row + nr * (size_t)indices[el];
            if (kind == 4) {
                ((int *)values_out)[el] = r_and(((const int *)values)[el], ((const int *)dense_mat)[at]);
                continue;
            }
            const double v = ((const double *)values)[el];
            double o;
            if (kind == 0) o = v * ((const double *)dense_mat)[at];
            else if (kind == 1) o = v * ((const float *)dense_mat)[at];
            else if (kind == 2) { const int d = ((const int *)dense_mat)[at]; o = d == NA_INT ? NA : v * d; }
            else { const int d = ((const int *)dense_mat)[at]; o = d == NA_INT ? NA : v * (double)(d != 0); }
            ((double *)values_out)[el] = o;
        }
    }
}

/* ---- CSR (op) dense vector, values only (operators.cpp:1604-2200) ------------ */
/* R's arithmetic as the reference restates it: R_intdiv :1500-1513, R_modulus :1526-1540 (both with a long double
 * intermediate, as compiled on x86), R_pow = R's C API function whose body is quoted at :1555-1601. */
#include <float.h>
static double r_modulus_o(double x1, double x2)
{
    if (x2 == 0.0) return NAN;
    if (fabs(x2) * LDBL_EPSILON > 1 && isfinite(x1) && fabs(x1) <= fabs(x2))
        return (fabs(x1) == fabs(x2)) ? 0 : (((x1 < 0 && x2 > 0) || (x2 < 0 && x1 > 0)) ? x1 + x2 : x1);
    double q = x1 / x2;
    long double tmp = (long double)x1 - floor(q) * (long double)x2;
    return (double)(tmp - floorl(tmp / x2) * x2);
}
static double r_intdiv_o(double x1, double x2)
{
    double q = x1 / x2;
    if (x2 == 0.0 || fabs(q) * LDBL_EPSILON > 1 || !isfinite(q)) return q;
    if (fabs(q) < 1) return (q < 0) ? -1 : (((x1 < 0 && x2 > 0) || (x1 > 0 && x2 < 0)) ? -1 : 0);
    long double tmp = (long double)x1 - floor(q) * (long double)x2;
    return (double)(floor(q) + floorl(tmp / x2));
}
static double r_pow_o(double x, double y)
{
    if (y == 2.0) return x * x;
    if (x == 1. || y == 0.) return 1.;
    if (x == 0.) {
        if (y > 0.) return 0.;
        else if (y < 0) return INFINITY;
        else return y;
    }
    if (isfinite(x) && isfinite(y)) return pow(x, y);
    if (isnan(x) || isnan(y)) return x + y;
    if (!isfinite(x)) {
        if (x > 0) return (y < 0.) ? 0. : INFINITY;
        else if (isfinite(y) && y == floor(y)) return (y < 0.) ? 0. : (r_modulus_o(y, 2.) != 0 ? x : -x);
    }
    if (!isfinite(y)) {
        if (x >= 0) {
            if (y > 0) return (x >= 1) ? INFINITY : 0.;
            else return (x < 1) ? INFINITY : 0.;
        }
    }
    return NAN;
}
/* op: 0 multiply, 1 powerto, 2 divide, 3 divrest, 4 intdiv, 5 logical AND (int32 values / dvec / out).
 * The four length branches of the reference (:1640 == nrows, :1773 >= nrows*ncols, :1870 divides nrows, :2033 general)
 * are kept as written, not folded into one formula, so that the device's single formula is checked against them. */
void mxo_csr_by_dvec(int nrows, int ncols, const int *indptr, const int *indices, const void *values,
                     const void *dvec, size_t len, int op, int x_is_lhs, void *values_out)
{
    const size_t nr = (size_t)nrows;
    for (size_t row = 0; row < nr; row++) {
        for (int ix = indptr[row]; ix < indptr[row + 1]; ix++) {
            size_t at;
            if (len == nr) at = row;
            else if ((unsigned long long)len >= (unsigned long long)nr * (unsigned long long)ncols) at = row + (size_t)indices[ix] * nr;
            else if (len < nr && (nr % len) == 0) at = row % len;
            else at = (size_t)(((unsigned long long)row + (unsigned long long)indices[ix] * (unsigned long long)nr) % (unsigned long long)len);
            if (op == 5) {
                ((int *)values_out)[ix] = r_and(((const int *)values)[ix], ((const int *)dvec)[at]);
                continue;
            }
            const double x = ((const double *)values)[ix], d = ((const double *)dvec)[at];
            double o;
            switch (op) {
                case 0: o = x * d; break;
                case 2: o = x_is_lhs ? x / d : d / x; break;
                case 3: o = x_is_lhs ? r_modulus_o(x, d) : r_modulus_o(d, x); break;
                case 4: o = x_is_lhs ? r_intdiv_o(x, d) : r_intdiv_o(d, x); break;
                default: o = x_is_lhs ? r_pow_o(x, d) : r_pow_o(d, x); break;
            }
            ((double *)values_out)[ix] = o;
        }
    }
}

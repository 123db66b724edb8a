// r_shim.cpp — thin `.Call` translation unit between R and libmxgpu's C-ABI.
//
// Exports, for the 19 hot-path routines (+ 12 column-slice / reversal routines of SURVEY §8f rank 2), exactly the native-routine names and arities that the
// reference registers in CallEntries[] (src/RcppExports.cpp:2233-2242, 2290-2291, 2297-2298, 2333-2334,
// 2341-2343), so R code written as `.Call("_MatrixExtra_<fn>", ...)` (R/RcppExports.R) dispatches
// unchanged, plus mxgpu_register() to add them to a DllInfo.  It also exports mxgpu_csr_transpose, the device
// transpose behind the overlay's t_deep_internal, and mxgpu_coo_to_csr, the device COO sort behind its
// as.csr.matrix / as.csc.matrix of a TsparseMatrix.  Written against the plain R C API
// (no Rcpp): INTEGER()/REAL(), Rf_allocMatrix, Rf_error.
//
// This file is NOT part of libmxgpu.so: it is built on a machine that has R with
//     R CMD SHLIB -o mxgpu_r.so r_shim.cpp -L<repo>/matrixextra_amd -lmxgpu -I<repo>/include
// No R has compiled or run it yet.  What does compile and run it is the project's own build: `make rshim` builds it
// with -Wall -Wextra -Werror against the stand-in for R's C API under tests/rstub, once linked to libmxgpu.so and once
// to a generated fake of the C-ABI, and tests/test_rshim_host.py / tests/test_gpu_rshim.py call every routine below
// through it (registration, handle lifecycle, PROTECT balance under a gctorture-like mode, result types and names,
// and the reference-run records on the device).
// See INTEGRATION.md.  Everything numerically meaningful lives behind the C-ABI and is tested through it;
// what is left here is mechanical marshalling:
//   * inputs are borrowed (no copies unless the SEXP type differs, as Rcpp's input_parameter<> does);
//   * outputs are fresh R objects; variable-size results use the begin/finish pair so that the D2H copy
//     lands directly in R-allocated vectors (SURVEY §8b "Ownership");
//   * identical-structure merges return the INPUT indptr/indices SEXPs (operators.cpp:127-131, :390-394);
//   * a non-zero status becomes Rf_error(mx_last_error()) after the device handle is released.
#if defined(__has_include)
#  if __has_include(<Rinternals.h>)
#    define MXGPU_HAVE_R 1
#  endif
#endif

#ifdef MXGPU_HAVE_R
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include "mxgpu.h"

namespace {

struct Protect {          // PROTECT counter that unwinds on scope exit (normal returns only; Rf_error long-jumps
    int n = 0;            // and R unprotects everything above the .Call frame itself)
    SEXP operator()(SEXP s) { PROTECT(s); ++n; return s; }
    ~Protect() { if (n) UNPROTECT(n); }
};

inline SEXP as_type(SEXP x, SEXPTYPE t, Protect &p) { return (SEXPTYPE)TYPEOF(x) == t ? x : p(Rf_coerceVector(x, t)); }
inline void fail() { Rf_error("%s", mx_last_error()); }

// float32@Data is an INTSXP matrix carrying binary32 bit patterns (R/matmul.R:260,276; matmul.cpp:213)
inline const float *f32(SEXP x) { return reinterpret_cast<const float *>(INTEGER(x)); }
inline float *f32w(SEXP x) { return reinterpret_cast<float *>(INTEGER(x)); }

SEXP named_list3(SEXP indptr, SEXP indices, SEXP values, Protect &p)
{
    SEXP out = p(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, indptr);
    SET_VECTOR_ELT(out, 1, indices);
    SET_VECTOR_ELT(out, 2, values);
    SEXP nm = p(Rf_allocVector(STRSXP, 3));
    SET_STRING_ELT(nm, 0, Rf_mkChar("indptr"));
    SET_STRING_ELT(nm, 1, Rf_mkChar("indices"));
    SET_STRING_ELT(nm, 2, Rf_mkChar("values"));
    Rf_setAttrib(out, R_NamesSymbol, nm);
    return out;
}

// mx_result_finish owns the handle from the moment it is entered and deletes it on every return, failure included:
// `res` is cleared before the call, so that no cleanup releases it a second time
SEXP finish_list(mx_result *&res, const mx_result_info &info, SEXP alias_p, SEXP alias_j, Protect &p)
{
    // doubles, logicals, or the integers of an isparseVector; no values at all is an empty double vector
    const SEXPTYPE vt = info.values_dtype == MX_LGL ? LGLSXP : (info.values_dtype == MX_I32 ? INTSXP : REALSXP);
    const R_xlen_t nv = info.values_dtype == MX_NONE ? 0 : (R_xlen_t)info.values_len;
    SEXP values = p(Rf_allocVector(vt, nv));           // may long-jump on allocation failure:
    void *vptr = vt == REALSXP ? (void *)REAL(values)
               : vt == LGLSXP  ? (void *)LOGICAL(values) : (void *)INTEGER(values);
    SEXP indptr = alias_p, indices = alias_j;
    if (!info.alias_structure) {
        indptr = p(Rf_allocVector(INTSXP, (R_xlen_t)info.indptr_len));
        indices = p(Rf_allocVector(INTSXP, (R_xlen_t)info.nnz));
    }
    mx_result *handle = res;
    res = nullptr;
    if (mx_result_finish(handle, info.alias_structure ? nullptr : INTEGER(indptr),
                         info.alias_structure ? nullptr : INTEGER(indices), nv ? vptr : nullptr))
        fail();
    return named_list3(indptr, indices, values, p);
}

// R allocation can long-jump; run it with the device handle guarded so it is never leaked
struct FinishArgs { mx_result *res; mx_result_info info; SEXP alias_p, alias_j; SEXP out; };
void finish_body(void *d)
{
    FinishArgs *a = static_cast<FinishArgs *>(d);
    Protect p;
    a->out = finish_list(a->res, a->info, a->alias_p, a->alias_j, p);     // consumes a->res
    R_PreserveObject(a->out);              // survives p's UNPROTECT; released by the caller
}
void finish_cleanup(void *d)
{
    FinishArgs *a = static_cast<FinishArgs *>(d);
    if (a->res) mx_result_discard(a->res);
}
SEXP finish_guarded(mx_result *res, const mx_result_info &info, SEXP alias_p, SEXP alias_j)
{
    FinishArgs a{res, info, alias_p, alias_j, R_NilValue};
    R_ExecWithCleanup([](void *d) -> SEXP { finish_body(d); return R_NilValue; }, &a, finish_cleanup, &a);
    SEXP out = a.out;
    PROTECT(out);
    R_ReleaseObject(out);
    UNPROTECT(1);
    return out;
}

SEXP elemwise(int op, SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, SEXPTYPE vt)
{
    Protect p;
    p1 = as_type(p1, INTSXP, p); p2 = as_type(p2, INTSXP, p);
    j1 = as_type(j1, INTSXP, p); j2 = as_type(j2, INTSXP, p);
    x1 = as_type(x1, vt, p);     x2 = as_type(x2, vt, p);
    const void *v1 = vt == REALSXP ? (const void *)REAL(x1) : (const void *)LOGICAL(x1);
    const void *v2 = vt == REALSXP ? (const void *)REAL(x2) : (const void *)LOGICAL(x2);
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_csr_elemwise_begin(op, (int)XLENGTH(p1) - 1, INTEGER(p1), INTEGER(p2), INTEGER(j1), INTEGER(j2), v1, v2,
                              (int64_t)XLENGTH(j1), (int64_t)XLENGTH(j2), &res, &info))
        fail();
    return finish_guarded(res, info, p1, j1);
}

SEXP copy_rows(SEXP indptr, SEXP indices, SEXP values, SEXP rows_take, int dtype)
{
    Protect p;
    indptr = as_type(indptr, INTSXP, p); indices = as_type(indices, INTSXP, p);
    rows_take = as_type(rows_take, INTSXP, p);
    const void *v = nullptr;
    int64_t nv = 0;
    if (dtype == MX_F64) { values = as_type(values, REALSXP, p); v = REAL(values); nv = XLENGTH(values); }
    else if (dtype == MX_LGL) { values = as_type(values, LGLSXP, p); v = LOGICAL(values); nv = XLENGTH(values); }
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_copy_csr_rows_begin(INTEGER(indptr), (int)XLENGTH(indptr) - 1, INTEGER(indices), v, dtype, nv,
                               INTEGER(rows_take), (int64_t)XLENGTH(rows_take), &res, &info))
        fail();
    if (dtype != MX_NONE) info.values_dtype = dtype;     // empty values keep their R type (slice.cpp:246)
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}

}  // namespace

extern "C" {

// ---- CSR x dense --------------------------------------------------------------------------------
SEXP _MatrixExtra_tcrossprod_csr_dense_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP Y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); Y = as_type(Y, REALSXP, p);
    const int m = (int)XLENGTH(p_) - 1, n = Rf_nrows(Y), K = Rf_ncols(Y);
    SEXP out = p(Rf_allocMatrix(REALSXP, m, n));
    if (mx_tcrossprod_csr_dense_numeric(INTEGER(p_), INTEGER(j_), REAL(x_), m, REAL(Y), n, K, Rf_asInteger(nthreads), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_tcrossprod_csr_dense_float32(SEXP p_, SEXP j_, SEXP x_, SEXP Y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); Y = as_type(Y, INTSXP, p);
    const int m = (int)XLENGTH(p_) - 1, n = Rf_nrows(Y), K = Rf_ncols(Y);
    SEXP out = p(Rf_allocMatrix(INTSXP, m, n));
    if (mx_tcrossprod_csr_dense_float32(INTEGER(p_), INTEGER(j_), REAL(x_), m, f32(Y), n, K, Rf_asInteger(nthreads), f32w(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_dense_csc_numeric(SEXP X, SEXP p_, SEXP i_, SEXP x_, SEXP nthreads)
{
    Protect p;
    X = as_type(X, REALSXP, p); p_ = as_type(p_, INTSXP, p); i_ = as_type(i_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    const int nr = Rf_nrows(X), nc = Rf_ncols(X), ncY = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocMatrix(REALSXP, nr, ncY));
    if (mx_matmul_dense_csc_numeric(REAL(X), nr, nc, INTEGER(p_), INTEGER(i_), REAL(x_), ncY, Rf_asInteger(nthreads), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_dense_csc_float32(SEXP X, SEXP p_, SEXP i_, SEXP x_, SEXP nthreads)
{
    Protect p;
    X = as_type(X, INTSXP, p); p_ = as_type(p_, INTSXP, p); i_ = as_type(i_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    const int nr = Rf_nrows(X), nc = Rf_ncols(X), ncY = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocMatrix(INTSXP, nr, ncY));
    if (mx_matmul_dense_csc_float32(f32(X), nr, nc, INTEGER(p_), INTEGER(i_), REAL(x_), ncY, Rf_asInteger(nthreads), f32w(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_tcrossprod_dense_csr_numeric(SEXP X, SEXP p_, SEXP j_, SEXP x_, SEXP nthreads, SEXP ncols_Y)
{
    Protect p;
    X = as_type(X, REALSXP, p); p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    const int nr = Rf_nrows(X), nc = Rf_ncols(X), nrY = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocMatrix(REALSXP, nr, nrY));
    if (mx_tcrossprod_dense_csr_numeric(REAL(X), nr, nc, INTEGER(p_), INTEGER(j_), REAL(x_), nrY, Rf_asInteger(nthreads),
                                        Rf_asInteger(ncols_Y), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_tcrossprod_dense_csr_float32(SEXP X, SEXP p_, SEXP j_, SEXP x_, SEXP nthreads, SEXP ncols_Y)
{
    Protect p;
    X = as_type(X, INTSXP, p); p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    const int nr = Rf_nrows(X), nc = Rf_ncols(X), nrY = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocMatrix(INTSXP, nr, nrY));
    if (mx_tcrossprod_dense_csr_float32(f32(X), nr, nc, INTEGER(p_), INTEGER(j_), REAL(x_), nrY, Rf_asInteger(nthreads),
                                        Rf_asInteger(ncols_Y), f32w(out)))
        fail();
    return out;
}

// ---- CSR x dense vector ---------------------------------------------------------------------------
SEXP _MatrixExtra_matmul_csr_dvec_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); y = as_type(y, REALSXP, p);
    const int m = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocVector(REALSXP, m));
    if (mx_matmul_csr_dvec_numeric(INTEGER(p_), INTEGER(j_), REAL(x_), m, REAL(y), (int)XLENGTH(y), Rf_asInteger(nthreads), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_csr_dvec_integer(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); y = as_type(y, INTSXP, p);
    const int m = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocVector(REALSXP, m));
    if (mx_matmul_csr_dvec_integer(INTEGER(p_), INTEGER(j_), REAL(x_), m, INTEGER(y), (int)XLENGTH(y), Rf_asInteger(nthreads), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_csr_dvec_logical(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); y = as_type(y, LGLSXP, p);
    const int m = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocVector(REALSXP, m));
    if (mx_matmul_csr_dvec_logical(INTEGER(p_), INTEGER(j_), REAL(x_), m, LOGICAL(y), (int)XLENGTH(y), Rf_asInteger(nthreads), REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_csr_dvec_float32(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); y = as_type(y, INTSXP, p);
    const int m = (int)XLENGTH(p_) - 1;
    SEXP out = p(Rf_allocVector(INTSXP, m));
    if (mx_matmul_csr_dvec_float32(INTEGER(p_), INTEGER(j_), REAL(x_), m, f32(y), (int)XLENGTH(y), Rf_asInteger(nthreads), f32w(out)))
        fail();
    return out;
}

// ---- CSR (+) CSR --------------------------------------------------------------------------------------
SEXP _MatrixExtra_multiply_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2)
{ return elemwise(MX_OP_MUL, p1, p2, j1, j2, x1, x2, REALSXP); }
SEXP _MatrixExtra_logicaland_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2)
{ return elemwise(MX_OP_AND, p1, p2, j1, j2, x1, x2, LGLSXP); }
SEXP _MatrixExtra_add_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, SEXP substract)
{ return elemwise(Rf_asLogical(substract) ? MX_OP_SUB : MX_OP_ADD, p1, p2, j1, j2, x1, x2, REALSXP); }
SEXP _MatrixExtra_logicalor_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, SEXP xor_op)
{ return elemwise(Rf_asLogical(xor_op) ? MX_OP_XOR : MX_OP_OR, p1, p2, j1, j2, x1, x2, LGLSXP); }

// ---- X[rows, ] -------------------------------------------------------------------------------------------
SEXP _MatrixExtra_copy_csr_rows_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows) { return copy_rows(p_, j_, x_, rows, MX_F64); }
SEXP _MatrixExtra_copy_csr_rows_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows) { return copy_rows(p_, j_, x_, rows, MX_LGL); }
SEXP _MatrixExtra_copy_csr_rows_binary(SEXP p_, SEXP j_, SEXP rows) { return copy_rows(p_, j_, R_NilValue, rows, MX_NONE); }

// ---- X[rows, cols] (§8f rank 2) -----------------------------------------------------------------------------
static SEXP col_seq(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, SEXP index1, int dtype)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); rows = as_type(rows, INTSXP, p); cols = as_type(cols, INTSXP, p);
    const void *v = nullptr; int64_t nv = 0;
    if (dtype == MX_F64) { x_ = as_type(x_, REALSXP, p); v = REAL(x_); nv = XLENGTH(x_); }
    else if (dtype == MX_LGL) { x_ = as_type(x_, LGLSXP, p); v = LOGICAL(x_); nv = XLENGTH(x_); }
    mx_result *res = nullptr; mx_result_info info;
    if (mx_copy_csr_rows_col_seq_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), v, dtype, nv, INTEGER(rows),
                                       (int64_t)XLENGTH(rows), INTEGER(cols), (int64_t)XLENGTH(cols),
                                       Rf_asLogical(index1), &res, &info))
        fail();
    return finish_guarded(res, info, R_NilValue, R_NilValue);         // values: numeric vector (slice.cpp:363)
}
SEXP _MatrixExtra_copy_csr_rows_col_seq_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, x_, rows, cols, index1, MX_F64); }
SEXP _MatrixExtra_copy_csr_rows_col_seq_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, x_, rows, cols, index1, MX_LGL); }
SEXP _MatrixExtra_copy_csr_rows_col_seq_binary(SEXP p_, SEXP j_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, R_NilValue, rows, cols, index1, MX_NONE); }

static SEXP arbitrary(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, int dtype)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); rows = as_type(rows, INTSXP, p); cols = as_type(cols, INTSXP, p);
    const void *v = nullptr; int64_t nv = 0;
    if (dtype == MX_F64) { x_ = as_type(x_, REALSXP, p); v = REAL(x_); nv = XLENGTH(x_); }
    else if (dtype == MX_LGL) { x_ = as_type(x_, LGLSXP, p); v = LOGICAL(x_); nv = XLENGTH(x_); }
    mx_result *res = nullptr; mx_result_info info;
    if (mx_copy_csr_arbitrary_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), v, dtype, nv, INTEGER(rows),
                                    (int64_t)XLENGTH(rows), INTEGER(cols), (int64_t)XLENGTH(cols), &res, &info))
        fail();
    const bool no_values = info.values_dtype == MX_NONE;
    SEXP out = p(finish_guarded(res, info, R_NilValue, R_NilValue));
    if (!no_values) return out;
    // the reference's list has no `values` element when the matrix has none (slice.cpp:565)
    SEXP two = p(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(two, 0, VECTOR_ELT(out, 0));
    SET_VECTOR_ELT(two, 1, VECTOR_ELT(out, 1));
    SEXP nm = p(Rf_allocVector(STRSXP, 2));
    SET_STRING_ELT(nm, 0, Rf_mkChar("indptr"));
    SET_STRING_ELT(nm, 1, Rf_mkChar("indices"));
    Rf_setAttrib(two, R_NamesSymbol, nm);
    return two;
}
SEXP _MatrixExtra_copy_csr_arbitrary_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, x_, rows, cols, MX_F64); }
SEXP _MatrixExtra_copy_csr_arbitrary_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, x_, rows, cols, MX_LGL); }
SEXP _MatrixExtra_copy_csr_arbitrary_binary(SEXP p_, SEXP j_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, R_NilValue, rows, cols, MX_NONE); }

static SEXP reverse_rows(SEXP p_, SEXP j_, SEXP x_, int dtype)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p);
    const void *v = nullptr; int64_t nv = 0;
    if (dtype == MX_F64) { x_ = as_type(x_, REALSXP, p); v = REAL(x_); nv = XLENGTH(x_); }
    else if (dtype == MX_LGL) { x_ = as_type(x_, LGLSXP, p); v = LOGICAL(x_); nv = XLENGTH(x_); }
    mx_result *res = nullptr; mx_result_info info;
    if (mx_reverse_rows_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), v, dtype, nv, &res, &info)) fail();
    if (dtype == MX_LGL) info.values_dtype = info.values_len ? MX_LGL : info.values_dtype;
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}
SEXP _MatrixExtra_reverse_rows_numeric(SEXP p_, SEXP j_, SEXP x_) { return reverse_rows(p_, j_, x_, MX_F64); }
SEXP _MatrixExtra_reverse_rows_logical(SEXP p_, SEXP j_, SEXP x_) { return reverse_rows(p_, j_, x_, MX_LGL); }
SEXP _MatrixExtra_reverse_rows_binary(SEXP p_, SEXP j_) { return reverse_rows(p_, j_, R_NilValue, MX_NONE); }

// in place on the caller's vectors, like the reference (the R glue only passes freshly created results here)
static SEXP reverse_cols(SEXP p_, SEXP j_, SEXP x_, SEXP ncol, int dtype)
{
    void *v = nullptr; int64_t nv = 0;
    if (dtype == MX_F64 && TYPEOF(x_) == REALSXP) { v = REAL(x_); nv = XLENGTH(x_); }
    else if (dtype == MX_LGL && TYPEOF(x_) == LGLSXP) { v = LOGICAL(x_); nv = XLENGTH(x_); }
    if (TYPEOF(p_) != INTSXP || TYPEOF(j_) != INTSXP) Rf_error("reverse_columns_inplace: integer index vectors required");
    if (mx_reverse_columns_inplace(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), v, nv ? dtype : MX_NONE, nv,
                                   Rf_asInteger(ncol)))
        fail();
    return R_NilValue;
}
SEXP _MatrixExtra_reverse_columns_inplace_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_F64); }
SEXP _MatrixExtra_reverse_columns_inplace_logical(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_LGL); }
SEXP _MatrixExtra_reverse_columns_inplace_binary(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_NONE); }

SEXP _MatrixExtra_check_is_seq(SEXP idx)
{
    Protect p;
    idx = as_type(idx, INTSXP, p);
    int r = 0;
    if (mx_check_is_seq(INTEGER(idx), (int64_t)XLENGTH(idx), &r)) fail();
    return Rf_ScalarLogical(r);
}
SEXP _MatrixExtra_check_is_rev_seq(SEXP idx)
{
    Protect p;
    idx = as_type(idx, INTSXP, p);
    int r = 0;
    if (mx_check_is_rev_seq(INTEGER(idx), (int64_t)XLENGTH(idx), &r)) fail();
    return Rf_ScalarLogical(r);
}

// values-only CSR (op) vector  (src/operators.cpp:2142-2200; glue src/RcppExports.cpp `_MatrixExtra_multiply_csr_by_dvec_no_NAs_numeric`, 11 arguments)
SEXP _MatrixExtra_multiply_csr_by_dvec_no_NAs_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols, SEXP multiply,
                                                      SEXP powerto, SEXP divide, SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); dvec = as_type(dvec, REALSXP, p);
    SEXP out = p(Rf_allocVector(REALSXP, XLENGTH(x_)));
    if (mx_multiply_csr_by_dvec_no_NAs_numeric(INTEGER(p_), INTEGER(j_), REAL(x_), (int)XLENGTH(p_) - 1, REAL(dvec),
                                               (int64_t)XLENGTH(dvec), Rf_asInteger(ncols), Rf_asLogical(multiply),
                                               Rf_asLogical(powerto), Rf_asLogical(divide), Rf_asLogical(divrest),
                                               Rf_asLogical(intdiv), Rf_asLogical(lhs), REAL(out)))
        fail();
    return out;
}
// CSR (op) vector keeping R's NA cells  (src/operators.cpp:2258-2852; glue src/RcppExports.cpp:1628-1645, 11
// arguments): list(indptr, indices, values); when the flat regime adds no entry, indptr / indices are the arguments
// themselves, as the reference returns them (:2643-2651)
SEXP _MatrixExtra_multiply_csr_by_dvec_with_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols, SEXP multiply,
                                                SEXP powerto, SEXP divide, SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); dvec = as_type(dvec, REALSXP, p);
    if (XLENGTH(x_) != XLENGTH(j_)) Rf_error("multiply_csr_by_dvec_with_NAs: indices and values have different length");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_multiply_csr_by_dvec_with_NAs_begin(INTEGER(p_), INTEGER(j_), REAL(x_), (int)XLENGTH(p_) - 1, REAL(dvec),
                                               (int64_t)XLENGTH(dvec), Rf_asInteger(ncols), Rf_asLogical(multiply),
                                               Rf_asLogical(powerto), Rf_asLogical(divide), Rf_asLogical(divrest),
                                               Rf_asLogical(intdiv), Rf_asLogical(lhs), &res, &info))
        fail();
    return finish_guarded(res, info, p_, j_);
}
SEXP _MatrixExtra_logicaland_csr_by_dvec_internal(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, LGLSXP, p); dvec = as_type(dvec, LGLSXP, p);
    SEXP out = p(Rf_allocVector(LGLSXP, XLENGTH(x_)));
    if (mx_logicaland_csr_by_dvec_internal(INTEGER(p_), INTEGER(j_), LOGICAL(x_), (int)XLENGTH(p_) - 1, LOGICAL(dvec),
                                           (int64_t)XLENGTH(dvec), Rf_asInteger(ncols), LOGICAL(out)))
        fail();
    return out;
}

// Device transpose behind the overlay's t_deep_internal (R/trans.R:46-56): the CSR (or CSC) slots of x^T.
// values: a double vector (dg*), a logical vector (lg*) or NULL (ng*); ncol: columns of the CSR view (ncol(x) for
// an RsparseMatrix, nrow(x) for a CsparseMatrix).  Returns list(indptr=, indices=, values=).
SEXP mxgpu_csr_transpose(SEXP p_, SEXP idx, SEXP x_, SEXP ncol)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); idx = as_type(idx, INTSXP, p);
    int dtype = MX_NONE;
    const void *v = nullptr;
    int64_t nv = 0;
    if (TYPEOF(x_) == REALSXP) { dtype = MX_F64; v = REAL(x_); nv = XLENGTH(x_); }
    else if (TYPEOF(x_) == LGLSXP) { dtype = MX_LGL; v = LOGICAL(x_); nv = XLENGTH(x_); }
    else if (x_ != R_NilValue) Rf_error("mxgpu_csr_transpose: values must be double, logical or NULL");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_csr_transpose_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, Rf_asInteger(ncol), INTEGER(idx), v, dtype, nv,
                               &res, &info))
        fail();
    if (dtype != MX_NONE) info.values_dtype = dtype;     // an empty result keeps the values' R type
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}

// COO -> CSR behind the overlay's as.csr.matrix / as.csc.matrix of a general d/l/n TsparseMatrix: i, j 0-based
// (the @i / @j slots), values as for mxgpu_csr_transpose.  Call with (j, i, x, ncol, nrow) for the CSC slots.
// Returns list(indptr=, indices=, values=) with repeated (i, j) merged as Matrix's coercion merges them.
SEXP mxgpu_coo_to_csr(SEXP i_, SEXP j_, SEXP x_, SEXP nrow, SEXP ncol)
{
    Protect p;
    i_ = as_type(i_, INTSXP, p); j_ = as_type(j_, INTSXP, p);
    if (XLENGTH(i_) != XLENGTH(j_)) Rf_error("mxgpu_coo_to_csr: row and column indices have different length");
    int dtype = MX_NONE;
    const void *v = nullptr;
    if (TYPEOF(x_) == REALSXP) { dtype = MX_F64; v = REAL(x_); }
    else if (TYPEOF(x_) == LGLSXP) { dtype = MX_LGL; v = LOGICAL(x_); }
    else if (x_ != R_NilValue) Rf_error("mxgpu_coo_to_csr: values must be double, logical or NULL");
    if (v && XLENGTH(x_) != XLENGTH(i_)) Rf_error("mxgpu_coo_to_csr: values and indices have different length");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_coo_to_csr_begin(INTEGER(i_), INTEGER(j_), v, dtype, (int64_t)XLENGTH(i_), Rf_asInteger(nrow),
                            Rf_asInteger(ncol), &res, &info))
        fail();
    if (dtype != MX_NONE) info.values_dtype = dtype;
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}

// CSR (.) COO  (src/operators.cpp:673-720; glue src/RcppExports.cpp:1317-1350, 8 arguments): list(row, col, val)
static SEXP csr_by_coo(int logical, SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yj, SEXP yx, SEXP max_row, SEXP max_col)
{
    Protect p;
    const SEXPTYPE vt = logical ? LGLSXP : REALSXP;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, vt, p);
    yi = as_type(yi, INTSXP, p); yj = as_type(yj, INTSXP, p); yx = as_type(yx, vt, p);
    const int m = Rf_asInteger(max_row);
    if (XLENGTH(p_) != (R_xlen_t)m + 1) Rf_error("multiply_csr_by_coo: indptr does not match max_row_X");
    if (XLENGTH(yi) != XLENGTH(yj) || XLENGTH(yi) != XLENGTH(yx)) Rf_error("multiply_csr_by_coo: bad COO lengths");
    const void *xv = logical ? (const void *)LOGICAL(x_) : (const void *)REAL(x_);
    const void *yv = logical ? (const void *)LOGICAL(yx) : (const void *)REAL(yx);
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_multiply_csr_by_coo_begin(logical, INTEGER(p_), INTEGER(j_), xv, INTEGER(yi), INTEGER(yj), yv,
                                     (int64_t)XLENGTH(yi), m, Rf_asInteger(max_col), &res, &info))
        fail();
    SEXP out = PROTECT(finish_guarded(res, info, R_NilValue, R_NilValue));
    SEXP nm = PROTECT(Rf_allocVector(STRSXP, 3));
    SET_STRING_ELT(nm, 0, Rf_mkChar("row"));
    SET_STRING_ELT(nm, 1, Rf_mkChar("col"));
    SET_STRING_ELT(nm, 2, Rf_mkChar("val"));
    Rf_setAttrib(out, R_NamesSymbol, nm);
    UNPROTECT(2);
    return out;
}
SEXP _MatrixExtra_multiply_csr_by_coo_elemwise(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yj, SEXP yx, SEXP mr, SEXP mc)
{ return csr_by_coo(0, p_, j_, x_, yi, yj, yx, mr, mc); }
SEXP _MatrixExtra_logicaland_csr_by_coo_elemwise(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yj, SEXP yx, SEXP mr, SEXP mc)
{ return csr_by_coo(1, p_, j_, x_, yi, yj, yx, mr, mc); }

// values-only COO (op) vector  (src/operators.cpp:3363-3418; 12 and 6 arguments)
SEXP _MatrixExtra_multiply_coo_by_dense_ignore_NAs_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP dvec, SEXP nrows,
                                                           SEXP ncols, SEXP multiply, SEXP powerto, SEXP divide,
                                                           SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p); xx = as_type(xx, REALSXP, p);
    dvec = as_type(dvec, REALSXP, p);
    SEXP out = p(Rf_allocVector(REALSXP, XLENGTH(xx)));
    if (mx_multiply_coo_by_dense_ignore_NAs_numeric(INTEGER(ii), INTEGER(jj), REAL(xx), (int64_t)XLENGTH(xx),
                                                    REAL(dvec), (int64_t)XLENGTH(dvec), Rf_asInteger(nrows),
                                                    Rf_asInteger(ncols), Rf_asLogical(multiply),
                                                    Rf_asLogical(powerto), Rf_asLogical(divide),
                                                    Rf_asLogical(divrest), Rf_asLogical(intdiv), Rf_asLogical(lhs),
                                                    REAL(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_multiply_coo_by_dense_ignore_NAs_logical(SEXP ii, SEXP jj, SEXP xx, SEXP dvec, SEXP nrows,
                                                           SEXP ncols)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p); xx = as_type(xx, LGLSXP, p);
    dvec = as_type(dvec, LGLSXP, p);
    SEXP out = p(Rf_allocVector(LGLSXP, XLENGTH(xx)));
    if (mx_multiply_coo_by_dense_ignore_NAs_logical(INTEGER(ii), INTEGER(jj), LOGICAL(xx), (int64_t)XLENGTH(xx),
                                                    LOGICAL(dvec), (int64_t)XLENGTH(dvec), Rf_asInteger(nrows),
                                                    Rf_asInteger(ncols), LOGICAL(out)))
        fail();
    return out;
}

// X[i, j] of a COO  (src/slice_coo.cpp:3-706; glue src/RcppExports.cpp:2061-2167): the single-element routines
// take 5 / 5 / 4 arguments and return a double / bool / bool; the arbitrary ones take 13 / 13 / 12 and return
// list(ii, jj, xx) (pattern: xx is an empty double vector here, the reference leaves it unset and R never reads it)
static SEXP slice_coo_single(int dtype, SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p);
    if (XLENGTH(ii) != XLENGTH(jj)) Rf_error("slice_coo_single: row and column indices have different length");
    const void *xv = nullptr;
    if (dtype == MX_F64) { xx = as_type(xx, REALSXP, p); xv = REAL(xx); }
    if (dtype == MX_LGL) { xx = as_type(xx, LGLSXP, p); xv = LOGICAL(xx); }
    if (xv && XLENGTH(xx) != XLENGTH(ii)) Rf_error("slice_coo_single: values and indices have different length");
    int found = 0;
    double vd = 0;
    int vl = 0;
    void *value_out = dtype == MX_F64 ? (void *)&vd : dtype == MX_LGL ? (void *)&vl : nullptr;     // a pattern has none
    if (mx_slice_coo_single(INTEGER(ii), INTEGER(jj), xv, dtype, (int64_t)XLENGTH(ii), Rf_asInteger(i),
                            Rf_asInteger(j), &found, value_out))
        fail();
    if (dtype == MX_F64) return Rf_ScalarReal(found ? vd : 0.0);
    return Rf_ScalarLogical(found && (dtype == MX_NONE || vl != 0));       // C++ bool: NA reads as TRUE
}
SEXP _MatrixExtra_slice_coo_single_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{ return slice_coo_single(MX_F64, ii, jj, xx, i, j); }
SEXP _MatrixExtra_slice_coo_single_logical(SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{ return slice_coo_single(MX_LGL, ii, jj, xx, i, j); }
SEXP _MatrixExtra_slice_coo_single_binary(SEXP ii, SEXP jj, SEXP i, SEXP j)
{ return slice_coo_single(MX_NONE, ii, jj, R_NilValue, i, j); }

static SEXP slice_coo_arbitrary(int dtype, SEXP ii, SEXP jj, SEXP xx, SEXP rows, SEXP cols, SEXP all_i, SEXP all_j,
                                SEXP i_seq, SEXP j_seq, SEXP i_rev, SEXP j_rev, SEXP nrows, SEXP ncols)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p);
    rows = as_type(rows, INTSXP, p); cols = as_type(cols, INTSXP, p);
    if (XLENGTH(ii) != XLENGTH(jj)) Rf_error("slice_coo_arbitrary: row and column indices have different length");
    const void *xv = nullptr;
    if (dtype == MX_F64) { xx = as_type(xx, REALSXP, p); xv = REAL(xx); }
    if (dtype == MX_LGL) { xx = as_type(xx, LGLSXP, p); xv = LOGICAL(xx); }
    if (xv && XLENGTH(xx) != XLENGTH(ii)) Rf_error("slice_coo_arbitrary: values and indices have different length");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_slice_coo_arbitrary_begin(INTEGER(ii), INTEGER(jj), xv, dtype, (int64_t)XLENGTH(ii), INTEGER(rows),
                                     (int64_t)XLENGTH(rows), INTEGER(cols), (int64_t)XLENGTH(cols),
                                     Rf_asLogical(all_i), Rf_asLogical(all_j), Rf_asLogical(i_seq),
                                     Rf_asLogical(j_seq), Rf_asLogical(i_rev), Rf_asLogical(j_rev),
                                     Rf_asInteger(nrows), Rf_asInteger(ncols), &res, &info))
        fail();
    SEXP out = PROTECT(finish_guarded(res, info, R_NilValue, R_NilValue));
    SEXP nm = PROTECT(Rf_allocVector(STRSXP, 3));
    SET_STRING_ELT(nm, 0, Rf_mkChar("ii"));
    SET_STRING_ELT(nm, 1, Rf_mkChar("jj"));
    SET_STRING_ELT(nm, 2, Rf_mkChar("xx"));
    Rf_setAttrib(out, R_NamesSymbol, nm);
    UNPROTECT(2);
    return out;
}
SEXP _MatrixExtra_slice_coo_arbitrary_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP rows, SEXP cols, SEXP all_i,
                                              SEXP all_j, SEXP i_seq, SEXP j_seq, SEXP i_rev, SEXP j_rev,
                                              SEXP nrows, SEXP ncols)
{ return slice_coo_arbitrary(MX_F64, ii, jj, xx, rows, cols, all_i, all_j, i_seq, j_seq, i_rev, j_rev, nrows, ncols); }
SEXP _MatrixExtra_slice_coo_arbitrary_logical(SEXP ii, SEXP jj, SEXP xx, SEXP rows, SEXP cols, SEXP all_i,
                                              SEXP all_j, SEXP i_seq, SEXP j_seq, SEXP i_rev, SEXP j_rev,
                                              SEXP nrows, SEXP ncols)
{ return slice_coo_arbitrary(MX_LGL, ii, jj, xx, rows, cols, all_i, all_j, i_seq, j_seq, i_rev, j_rev, nrows, ncols); }
SEXP _MatrixExtra_slice_coo_arbitrary_binary(SEXP ii, SEXP jj, SEXP rows, SEXP cols, SEXP all_i, SEXP all_j,
                                             SEXP i_seq, SEXP j_seq, SEXP i_rev, SEXP j_rev, SEXP nrows, SEXP ncols)
{
    return slice_coo_arbitrary(MX_NONE, ii, jj, R_NilValue, rows, cols, all_i, all_j, i_seq, j_seq, i_rev, j_rev,
                               nrows, ncols);
}

// remove_sparse_zeros / filterSparse / check_sparse_matrix  (src/misc.cpp:553-1116; glue src/RcppExports.cpp
// CallEntries :2279-2289).  The zero removers return list(indptr, indices, values) / list(ii, jj, xx) / list(ii, xx)
// and, when nothing is removed, the input vectors themselves (misc.cpp:586-590, :735-739, :864-867).
static SEXP named(SEXP out, const char *a, const char *b, const char *c)
{
    PROTECT(out);
    const int n = (int)XLENGTH(out);
    SEXP nm = PROTECT(Rf_allocVector(STRSXP, n));
    SET_STRING_ELT(nm, 0, Rf_mkChar(a));
    SET_STRING_ELT(nm, 1, Rf_mkChar(b));
    if (n > 2) SET_STRING_ELT(nm, 2, Rf_mkChar(c));
    Rf_setAttrib(out, R_NamesSymbol, nm);
    UNPROTECT(2);
    return out;
}

static SEXP compacted(mx_result *res, const mx_result_info &info, SEXP a, SEXP b, SEXP x, int layout)
{
    if (info.alias_structure == MX_ALIAS_ALL) {
        mx_result_discard(res);
        SEXP out = PROTECT(Rf_allocVector(VECSXP, layout == 2 ? 2 : 3));
        if (layout == 2) { SET_VECTOR_ELT(out, 0, b); SET_VECTOR_ELT(out, 1, x); }
        else { SET_VECTOR_ELT(out, 0, a); SET_VECTOR_ELT(out, 1, b); SET_VECTOR_ELT(out, 2, x); }
        UNPROTECT(1);
        return out;
    }
    SEXP l = PROTECT(finish_guarded(res, info, R_NilValue, R_NilValue));   // (indptr-or-ii, indices, values)
    SEXP out = l;
    if (layout == 2) {
        out = PROTECT(Rf_allocVector(VECSXP, 2));
        SET_VECTOR_ELT(out, 0, VECTOR_ELT(l, 1));
        SET_VECTOR_ELT(out, 1, VECTOR_ELT(l, 2));
        UNPROTECT(1);
    }
    UNPROTECT(1);
    return out;
}

static SEXP rz_csr(int dtype, SEXP p_, SEXP j_, SEXP x_, SEXP na_rm)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p);
    x_ = as_type(x_, dtype == MX_F64 ? REALSXP : LGLSXP, p);
    if (XLENGTH(x_) != XLENGTH(j_)) Rf_error("remove_zero_valued_csr: indices and values have different length");
    mx_result *res = nullptr;
    mx_result_info info;
    const int rc = dtype == MX_F64
        ? mx_remove_zero_valued_csr_numeric(INTEGER(p_), INTEGER(j_), REAL(x_), (int)XLENGTH(p_) - 1,
                                            Rf_asLogical(na_rm), &res, &info)
        : mx_remove_zero_valued_csr_logical(INTEGER(p_), INTEGER(j_), LOGICAL(x_), (int)XLENGTH(p_) - 1,
                                            Rf_asLogical(na_rm), &res, &info);
    if (rc) fail();
    return named(compacted(res, info, p_, j_, x_, 0), "indptr", "indices", "values");
}
SEXP _MatrixExtra_remove_zero_valued_csr_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP na_rm)
{ return rz_csr(MX_F64, p_, j_, x_, na_rm); }
SEXP _MatrixExtra_remove_zero_valued_csr_logical(SEXP p_, SEXP j_, SEXP x_, SEXP na_rm)
{ return rz_csr(MX_LGL, p_, j_, x_, na_rm); }

static SEXP rz_coo(int dtype, SEXP ii, SEXP jj, SEXP xx, SEXP na_rm)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p);
    xx = as_type(xx, dtype == MX_F64 ? REALSXP : LGLSXP, p);
    if (XLENGTH(ii) != XLENGTH(jj) || XLENGTH(ii) != XLENGTH(xx)) Rf_error("remove_zero_valued_coo: bad lengths");
    mx_result *res = nullptr;
    mx_result_info info;
    const int rc = dtype == MX_F64
        ? mx_remove_zero_valued_coo_numeric(INTEGER(ii), INTEGER(jj), REAL(xx), (int64_t)XLENGTH(ii),
                                            Rf_asLogical(na_rm), &res, &info)
        : mx_remove_zero_valued_coo_logical(INTEGER(ii), INTEGER(jj), LOGICAL(xx), (int64_t)XLENGTH(ii),
                                            Rf_asLogical(na_rm), &res, &info);
    if (rc) fail();
    return named(compacted(res, info, ii, jj, xx, 1), "ii", "jj", "xx");
}
SEXP _MatrixExtra_remove_zero_valued_coo_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP na_rm)
{ return rz_coo(MX_F64, ii, jj, xx, na_rm); }
SEXP _MatrixExtra_remove_zero_valued_coo_logical(SEXP ii, SEXP jj, SEXP xx, SEXP na_rm)
{ return rz_coo(MX_LGL, ii, jj, xx, na_rm); }

static SEXP rz_svec(int dtype, SEXP ii, SEXP xx, SEXP na_rm)
{
    Protect p;
    ii = as_type(ii, INTSXP, p);
    xx = as_type(xx, dtype == MX_F64 ? REALSXP : dtype == MX_LGL ? LGLSXP : INTSXP, p);
    if (XLENGTH(ii) != XLENGTH(xx)) Rf_error("remove_zero_valued_svec: indices and values have different length");
    mx_result *res = nullptr;
    mx_result_info info;
    const int64_t n = (int64_t)XLENGTH(ii);
    const int na = Rf_asLogical(na_rm);
    int rc;
    if (dtype == MX_F64) rc = mx_remove_zero_valued_svec_numeric(INTEGER(ii), REAL(xx), n, na, &res, &info);
    else if (dtype == MX_LGL) rc = mx_remove_zero_valued_svec_logical(INTEGER(ii), LOGICAL(xx), n, na, &res, &info);
    else rc = mx_remove_zero_valued_svec_integer(INTEGER(ii), INTEGER(xx), n, na, &res, &info);
    if (rc) fail();
    // the integer kind reports MX_I32 and finish_list keeps it an INTSXP; every kind goes through the guarded finish
    return named(compacted(res, info, R_NilValue, ii, xx, 2), "ii", "xx", nullptr);
}
SEXP _MatrixExtra_remove_zero_valued_svec_numeric(SEXP ii, SEXP xx, SEXP na_rm) { return rz_svec(MX_F64, ii, xx, na_rm); }
SEXP _MatrixExtra_remove_zero_valued_svec_integer(SEXP ii, SEXP xx, SEXP na_rm) { return rz_svec(MX_I32, ii, xx, na_rm); }
SEXP _MatrixExtra_remove_zero_valued_svec_logical(SEXP ii, SEXP xx, SEXP na_rm) { return rz_svec(MX_LGL, ii, xx, na_rm); }

static SEXP err_list(const char *err)
{
    if (!err) return Rf_allocVector(VECSXP, 0);                     // Rcpp::List()
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 1));
    SET_VECTOR_ELT(out, 0, Rf_mkString(err));
    SEXP nm = PROTECT(Rf_mkString("err"));
    Rf_setAttrib(out, R_NamesSymbol, nm);
    UNPROTECT(2);
    return out;
}
SEXP _MatrixExtra_check_valid_csr_matrix(SEXP p_, SEXP j_, SEXP nrows, SEXP ncols)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p);
    const char *err = nullptr;
    if (mx_check_valid_csr_matrix(INTEGER(p_), (int64_t)XLENGTH(p_), INTEGER(j_), (int64_t)XLENGTH(j_),
                                  Rf_asInteger(nrows), Rf_asInteger(ncols), &err))
        fail();
    return err_list(err);
}
SEXP _MatrixExtra_check_valid_coo_matrix(SEXP ii, SEXP jj, SEXP nrows, SEXP ncols)
{
    Protect p;
    ii = as_type(ii, INTSXP, p); jj = as_type(jj, INTSXP, p);
    if (XLENGTH(ii) != XLENGTH(jj)) Rf_error("check_valid_coo_matrix: row and column indices have different length");
    const char *err = nullptr;
    if (mx_check_valid_coo_matrix(INTEGER(ii), INTEGER(jj), (int64_t)XLENGTH(ii), Rf_asInteger(nrows),
                                  Rf_asInteger(ncols), &err))
        fail();
    return err_list(err);
}
SEXP _MatrixExtra_check_valid_svec(SEXP ii, SEXP nrows)
{
    Protect p;
    ii = as_type(ii, INTSXP, p);
    const char *err = nullptr;
    if (mx_check_valid_svec(INTEGER(ii), (int64_t)XLENGTH(ii), Rf_asInteger(nrows), &err)) fail();
    return err_list(err);
}
SEXP _MatrixExtra_rebuild_indptr_after_filter(SEXP p_, SEXP filter)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); filter = as_type(filter, LGLSXP, p);
    SEXP out = p(Rf_allocVector(INTSXP, XLENGTH(p_)));
    if (mx_rebuild_indptr_after_filter(INTEGER(p_), (int64_t)XLENGTH(p_), LOGICAL(filter), INTEGER(out))) fail();
    return out;
}

// CSC (.) dense  (src/operators.cpp:1061-1458; glue src/RcppExports.cpp:1464-1580, 4 arguments each): dense_ is the
// matrix (float32: the float32@Data INTSXP bit patterns), its row count nrow(dense_).  The ignore_NAs routines return
// the values vector, the keep_NAs ones list(indptr, indices, values).
static SEXP csc_dense(int kind, bool keep, SEXP p_, SEXP i_, SEXP x_, SEXP dense_)
{
    Protect p;
    const int nrows = Rf_nrows(dense_);
    p_ = as_type(p_, INTSXP, p); i_ = as_type(i_, INTSXP, p);
    x_ = as_type(x_, kind == 4 ? LGLSXP : REALSXP, p);
    dense_ = as_type(dense_, kind == 0 ? REALSXP : kind == 3 || kind == 4 ? LGLSXP : INTSXP, p);
    const int ncols = (int)XLENGTH(p_) - 1;
    if (XLENGTH(x_) != XLENGTH(i_)) Rf_error("multiply_csc_by_dense: indices and values have different length");
    if ((R_xlen_t)nrows * ncols != XLENGTH(dense_)) Rf_error("multiply_csc_by_dense: dense matrix does not match");
    const int32_t *ip = INTEGER(p_), *ii = INTEGER(i_);
    if (keep) {
        mx_result *res = nullptr;
        mx_result_info info;
        int rc;
        switch (kind) {
            case 0: rc = mx_multiply_csc_by_dense_keep_NAs_numeric(ip, ncols, ii, REAL(x_), REAL(dense_), nrows, &res, &info); break;
            case 1: rc = mx_multiply_csc_by_dense_keep_NAs_float32(ip, ncols, ii, REAL(x_), f32(dense_), nrows, &res, &info); break;
            case 2: rc = mx_multiply_csc_by_dense_keep_NAs_integer(ip, ncols, ii, REAL(x_), INTEGER(dense_), nrows, &res, &info); break;
            default: rc = mx_multiply_csc_by_dense_keep_NAs_logical(ip, ncols, ii, REAL(x_), LOGICAL(dense_), nrows, &res, &info); break;
        }
        if (rc) fail();
        return finish_guarded(res, info, R_NilValue, R_NilValue);
    }
    SEXP out = p(Rf_allocVector(kind == 4 ? LGLSXP : REALSXP, XLENGTH(x_)));
    int rc;
    switch (kind) {
        case 0: rc = mx_multiply_csc_by_dense_ignore_NAs_numeric(ip, ncols, ii, REAL(x_), REAL(dense_), nrows, REAL(out)); break;
        case 1: rc = mx_multiply_csc_by_dense_ignore_NAs_float32(ip, ncols, ii, REAL(x_), f32(dense_), nrows, REAL(out)); break;
        case 2: rc = mx_multiply_csc_by_dense_ignore_NAs_integer(ip, ncols, ii, REAL(x_), INTEGER(dense_), nrows, REAL(out)); break;
        case 3: rc = mx_multiply_csc_by_dense_ignore_NAs_logical(ip, ncols, ii, REAL(x_), LOGICAL(dense_), nrows, REAL(out)); break;
        default: rc = mx_logicaland_csc_by_dense_ignore_NAs(ip, ncols, ii, LOGICAL(x_), LOGICAL(dense_), nrows, LOGICAL(out)); break;
    }
    if (rc) fail();
    return out;
}
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_numeric(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(0, false, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_float32(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(1, false, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_integer(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(2, false, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_logical(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(3, false, p_, i_, x_, d); }
SEXP _MatrixExtra_logicaland_csc_by_dense_ignore_NAs(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(4, false, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_numeric(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(0, true, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_integer(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(2, true, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_logical(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(3, true, p_, i_, x_, d); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_float32(SEXP p_, SEXP i_, SEXP x_, SEXP d) { return csc_dense(1, true, p_, i_, x_, d); }

// RsparseMatrix * sparseVector  (src/operators.cpp:3426-3697; 6 and 7 arguments): ii_base1 sorted, an empty xx is an
// nsparseVector.  Both return list(indptr, indices, values).
static SEXP csr_by_svec(int keep, SEXP p_, SEXP j_, SEXP x_, SEXP ii, SEXP xx, int ncols, SEXP length)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    ii = as_type(ii, INTSXP, p); xx = as_type(xx, REALSXP, p);
    if (XLENGTH(x_) != XLENGTH(j_)) Rf_error("multiply_csr_by_svec: indices and values have different length");
    if (XLENGTH(xx) && XLENGTH(xx) != XLENGTH(ii)) Rf_error("multiply_csr_by_svec: vector indices and values differ");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_multiply_csr_by_svec_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), REAL(x_), INTEGER(ii),
                                      XLENGTH(xx) ? REAL(xx) : nullptr, (int64_t)XLENGTH(ii), ncols,
                                      Rf_asInteger(length), keep, &res, &info))
        fail();
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}
SEXP _MatrixExtra_multiply_csr_by_svec_no_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP ii, SEXP xx, SEXP length)
{
    return csr_by_svec(0, p_, j_, x_, ii, xx, 0, length);
}
SEXP _MatrixExtra_multiply_csr_by_svec_keep_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP ii, SEXP xx, SEXP ncols, SEXP length)
{
    return csr_by_svec(1, p_, j_, x_, ii, xx, Rf_asInteger(ncols), length);
}

// outer products with a one-column CSR and float32 row vector x CSC  (src/matmul.cpp:643-938; outer.hip)
static SEXP outer_dense(int dtype, SEXP colvec, SEXP p_, SEXP j_, SEXP x_)
{
    Protect p;
    colvec = as_type(colvec, dtype == MX_F32 ? INTSXP : REALSXP, p);
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    if (XLENGTH(p_) < 1 || XLENGTH(x_) < INTEGER(p_)[XLENGTH(p_) - 1])
        Rf_error("matmul_colvec_by_scolvecascsr: values shorter than the index pointer says");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_matmul_colvec_by_scolvecascsr_begin(dtype == MX_F32 ? (const void *)f32(colvec) : (const void *)REAL(colvec),
                                               dtype, (int)XLENGTH(colvec), INTEGER(p_), (int)XLENGTH(p_) - 1,
                                               INTEGER(j_), REAL(x_), &res, &info))
        fail();
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}
SEXP _MatrixExtra_matmul_colvec_by_scolvecascsr(SEXP v, SEXP p_, SEXP j_, SEXP x_) { return outer_dense(MX_F64, v, p_, j_, x_); }
SEXP _MatrixExtra_matmul_colvec_by_scolvecascsr_f32(SEXP v, SEXP p_, SEXP j_, SEXP x_) { return outer_dense(MX_F32, v, p_, j_, x_); }

static SEXP outer_svec(int dtype, int ytype, SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP length)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p); yi = as_type(yi, INTSXP, p);
    const void *yv = nullptr;
    if (dtype != MX_NONE) {
        yx = as_type(yx, ytype, p);
        if (XLENGTH(yx) != XLENGTH(yi)) Rf_error("matmul_spcolvec_by_scolvecascsr: vector indices and values differ");
        yv = ytype == REALSXP ? (const void *)REAL(yx) : ytype == LGLSXP ? (const void *)LOGICAL(yx) : (const void *)INTEGER(yx);
    }
    if (XLENGTH(p_) < 1 || XLENGTH(x_) < INTEGER(p_)[XLENGTH(p_) - 1])
        Rf_error("matmul_spcolvec_by_scolvecascsr: values shorter than the index pointer says");
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_matmul_spcolvec_by_scolvecascsr_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), REAL(x_), INTEGER(yi), yv,
                                                 dtype, (int64_t)XLENGTH(yi), Rf_asInteger(length), &res, &info))
        fail();
    return finish_guarded(res, info, R_NilValue, R_NilValue);
}
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_F64, REALSXP, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_integer(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_I32, INTSXP, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_logical(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_LGL, LGLSXP, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_binary(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP n)
{ return outer_svec(MX_NONE, NILSXP, p_, j_, x_, yi, R_NilValue, n); }

// a 1 x ncol integer matrix holding the float32 bits, as Rcpp::IntegerMatrix(1, ncols_Y)
static SEXP rowvec_csc(SEXP v, SEXP p_, SEXP i_, SEXP x_)
{
    Protect p;
    v = as_type(v, INTSXP, p); p_ = as_type(p_, INTSXP, p); i_ = as_type(i_, INTSXP, p);
    const bool has = x_ != R_NilValue;
    if (has) x_ = as_type(x_, REALSXP, p);
    const int ncols = (int)XLENGTH(p_) - 1;
    if (ncols < 0 || XLENGTH(i_) < INTEGER(p_)[ncols] || (has && XLENGTH(x_) < INTEGER(p_)[ncols]))
        Rf_error("matmul_rowvec_by_csc: indices / values shorter than the index pointer says");
    SEXP out = p(Rf_allocMatrix(INTSXP, 1, ncols));
    if (mx_matmul_rowvec_by_csc(f32(v), (int64_t)XLENGTH(v), INTEGER(p_), ncols, INTEGER(i_), has ? REAL(x_) : nullptr,
                                f32w(out)))
        fail();
    return out;
}
SEXP _MatrixExtra_matmul_rowvec_by_csc(SEXP v, SEXP p_, SEXP i_, SEXP x_) { return rowvec_csc(v, p_, i_, x_); }
SEXP _MatrixExtra_matmul_rowvec_by_cscbin(SEXP v, SEXP p_, SEXP i_) { return rowvec_csc(v, p_, i_, R_NilValue); }

// sort_vector_indices_*  (src/misc.cpp:489-527): the caller's vectors are sorted where they are, so no coercion
static SEXP sort_svec(SEXP ii, SEXP xx, int xtype, int dtype)
{
    if (TYPEOF(ii) != INTSXP) Rf_error("sort_vector_indices: indices must be an integer vector");
    void *xv = nullptr;
    if (dtype != MX_NONE) {
        if (TYPEOF(xx) != xtype || XLENGTH(xx) != XLENGTH(ii)) Rf_error("sort_vector_indices: values do not match");
        xv = xtype == REALSXP ? (void *)REAL(xx) : xtype == LGLSXP ? (void *)LOGICAL(xx) : (void *)INTEGER(xx);
    }
    if (mx_sort_vector_indices(INTEGER(ii), xv, (int64_t)XLENGTH(ii), dtype)) fail();
    return R_NilValue;
}
SEXP _MatrixExtra_sort_vector_indices_numeric(SEXP ii, SEXP xx) { return sort_svec(ii, xx, REALSXP, MX_F64); }
SEXP _MatrixExtra_sort_vector_indices_integer(SEXP ii, SEXP xx) { return sort_svec(ii, xx, INTSXP, MX_I32); }
SEXP _MatrixExtra_sort_vector_indices_logical(SEXP ii, SEXP xx) { return sort_svec(ii, xx, LGLSXP, MX_LGL); }
SEXP _MatrixExtra_sort_vector_indices_binary(SEXP ii) { return sort_svec(ii, R_NilValue, NILSXP, MX_NONE); }

// sort_coo_indices_*  (src/misc.cpp:430-457): the caller's triplets are sorted where they are, so no coercion
static SEXP sort_coo(SEXP ii, SEXP jj, SEXP xx, int xtype, int dtype)
{
    if (TYPEOF(ii) != INTSXP || TYPEOF(jj) != INTSXP) Rf_error("sort_coo_indices: indices must be integer vectors");
    if (XLENGTH(jj) != XLENGTH(ii)) Rf_error("sort_coo_indices: indices do not match");
    void *xv = nullptr;
    if (dtype != MX_NONE) {
        if (TYPEOF(xx) != xtype || XLENGTH(xx) != XLENGTH(ii)) Rf_error("sort_coo_indices: values do not match");
        xv = xtype == REALSXP ? (void *)REAL(xx) : (void *)LOGICAL(xx);
    }
    if (mx_sort_coo_indices(INTEGER(ii), INTEGER(jj), xv, (int64_t)XLENGTH(ii), dtype)) fail();
    return R_NilValue;
}
SEXP _MatrixExtra_sort_coo_indices_numeric(SEXP ii, SEXP jj, SEXP xx) { return sort_coo(ii, jj, xx, REALSXP, MX_F64); }
SEXP _MatrixExtra_sort_coo_indices_logical(SEXP ii, SEXP jj, SEXP xx) { return sort_coo(ii, jj, xx, LGLSXP, MX_LGL); }
SEXP _MatrixExtra_sort_coo_indices_binary(SEXP ii, SEXP jj) { return sort_coo(ii, jj, R_NilValue, NILSXP, MX_NONE); }

// `[<-` of a dgRMatrix: the set_* routines of src/assignment.cpp (glue: src/RcppExports.cpp, one CallEntries line
// each) over mx_assign_csr_scalar_begin / mx_assign_csr_rows_begin.  A selector is (kind, lo, hi, set); where the
// reference returns its input vectors (MX_ALIAS_ALL) or its input indptr / indices with new values (alias 1), so
// does this.  The zero-route routines of the reference receive no ncol; INT_MAX stands for "not needed".
struct Sel { int kind, lo, hi; SEXP set; };
static Sel sel_all() { return Sel{MX_SEL_ALL, 0, 0, R_NilValue}; }
static Sel sel_one(SEXP k) { const int v = Rf_asInteger(k); return Sel{MX_SEL_SINGLE, v, v, R_NilValue}; }
static Sel sel_seq(SEXP a, SEXP b) { return Sel{MX_SEL_RANGE, Rf_asInteger(a), Rf_asInteger(b), R_NilValue}; }
static Sel sel_set(SEXP v) { return Sel{MX_SEL_ARBITRARY, 0, 0, v}; }

static SEXP assigned(mx_result *res, const mx_result_info &info, SEXP p_, SEXP j_, SEXP x_)
{
    if (info.alias_structure == MX_ALIAS_ALL) {
        mx_result_discard(res);
        Protect p;
        return named_list3(p_, j_, x_, p);
    }
    return finish_guarded(res, info, p_, j_);
}

static SEXP assign_scalar(SEXP p_, SEXP j_, SEXP x_, int ncols, Sel si, Sel sj, double value)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    if (XLENGTH(x_) != XLENGTH(j_)) Rf_error("assignment: indices and values have different length");
    if (si.kind == MX_SEL_ARBITRARY) si.set = as_type(si.set, INTSXP, p);
    if (sj.kind == MX_SEL_ARBITRARY) sj.set = as_type(sj.set, INTSXP, p);
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_assign_csr_scalar_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), REAL(x_), ncols,
                                   si.kind, si.lo, si.hi, si.kind == MX_SEL_ARBITRARY ? INTEGER(si.set) : nullptr,
                                   si.kind == MX_SEL_ARBITRARY ? (int64_t)XLENGTH(si.set) : 0,
                                   sj.kind, sj.lo, sj.hi, sj.kind == MX_SEL_ARBITRARY ? INTEGER(sj.set) : nullptr,
                                   sj.kind == MX_SEL_ARBITRARY ? (int64_t)XLENGTH(sj.set) : 0, value, &res, &info))
        fail();
    return assigned(res, info, p_, j_, x_);
}

static SEXP assign_rows(SEXP p_, SEXP j_, SEXP x_, Sel si, SEXP vp, SEXP vj, SEXP vx)
{
    Protect p;
    p_ = as_type(p_, INTSXP, p); j_ = as_type(j_, INTSXP, p); x_ = as_type(x_, REALSXP, p);
    vp = as_type(vp, INTSXP, p); vj = as_type(vj, INTSXP, p); vx = as_type(vx, REALSXP, p);
    if (XLENGTH(x_) != XLENGTH(j_) || XLENGTH(vx) != XLENGTH(vj) || XLENGTH(vp) < 1)
        Rf_error("assignment: indices and values have different length");
    if (si.kind == MX_SEL_ARBITRARY) si.set = as_type(si.set, INTSXP, p);
    mx_result *res = nullptr;
    mx_result_info info;
    if (mx_assign_csr_rows_begin(INTEGER(p_), (int)XLENGTH(p_) - 1, INTEGER(j_), REAL(x_), si.kind, si.lo, si.hi,
                                 si.kind == MX_SEL_ARBITRARY ? INTEGER(si.set) : nullptr,
                                 si.kind == MX_SEL_ARBITRARY ? (int64_t)XLENGTH(si.set) : 0, INTEGER(vp),
                                 (int64_t)XLENGTH(vp) - 1, INTEGER(vj), REAL(vx), &res, &info))
        fail();
    return assigned(res, info, p_, j_, x_);
}

#define MX_NCOL_UNKNOWN 2147483647
SEXP _MatrixExtra_set_single_row_to_zero(SEXP p, SEXP j, SEXP x, SEXP row)
{ return assign_scalar(p, j, x, MX_NCOL_UNKNOWN, sel_one(row), sel_all(), 0.0); }
SEXP _MatrixExtra_set_single_col_to_zero(SEXP p, SEXP j, SEXP x, SEXP col)
{ return assign_scalar(p, j, x, MX_NCOL_UNKNOWN, sel_all(), sel_one(col), 0.0); }
SEXP _MatrixExtra_set_single_row_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP row, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_all(), Rf_asReal(val)); }
SEXP _MatrixExtra_set_single_col_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP col, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_one(col), Rf_asReal(val)); }
SEXP _MatrixExtra_set_single_val_to_zero(SEXP p, SEXP j, SEXP x, SEXP row, SEXP col)
{ return assign_scalar(p, j, x, MX_NCOL_UNKNOWN, sel_one(row), sel_one(col), 0.0); }
SEXP _MatrixExtra_set_single_val_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP row, SEXP col, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_one(col), Rf_asReal(val)); }
SEXP _MatrixExtra_set_rowseq_to_zero(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end)
{ return assign_scalar(p, j, x, MX_NCOL_UNKNOWN, sel_seq(st, end), sel_all(), 0.0); }
SEXP _MatrixExtra_set_rowseq_to_const(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_seq(st, end), sel_all(), Rf_asReal(val)); }
SEXP _MatrixExtra_set_colseq_to_zero(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_seq(st, end), 0.0); }
SEXP _MatrixExtra_set_colseq_to_const(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_seq(st, end), Rf_asReal(val)); }
SEXP _MatrixExtra_set_arbitrary_rows_to_zero(SEXP p, SEXP j, SEXP x, SEXP rows)
{ return assign_scalar(p, j, x, MX_NCOL_UNKNOWN, sel_set(rows), sel_all(), 0.0); }
SEXP _MatrixExtra_set_arbitrary_rows_to_const(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_set(rows), sel_all(), Rf_asReal(val)); }
SEXP _MatrixExtra_set_arbitrary_cols_to_zero(SEXP p, SEXP j, SEXP x, SEXP cols, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_set(cols), 0.0); }
SEXP _MatrixExtra_set_arbitrary_cols_to_const(SEXP p, SEXP j, SEXP x, SEXP cols, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_set(cols), Rf_asReal(val)); }
SEXP _MatrixExtra_set_arbitrary_rows_single_col_to_zero(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP col, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_set(rows), sel_one(col), 0.0); }
SEXP _MatrixExtra_set_arbitrary_rows_single_col_to_const(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP col, SEXP val,
                                                         SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_set(rows), sel_one(col), Rf_asReal(val)); }
SEXP _MatrixExtra_set_single_row_arbitrary_cols_to_zero(SEXP p, SEXP j, SEXP x, SEXP row, SEXP cols, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_set(cols), 0.0); }
SEXP _MatrixExtra_set_single_row_arbitrary_cols_to_const(SEXP p, SEXP j, SEXP x, SEXP row, SEXP cols, SEXP ncols,
                                                         SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_set(cols), Rf_asReal(val)); }
SEXP _MatrixExtra_set_arbitrary_rows_arbitrary_cols_to_zero(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP cols, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_set(rows), sel_set(cols), 0.0); }
SEXP _MatrixExtra_set_arbitrary_rows_arbitrary_cols_to_const(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP cols,
                                                             SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_set(rows), sel_set(cols), Rf_asReal(val)); }
SEXP _MatrixExtra_set_rowseq_to_smat(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP vp, SEXP vj, SEXP vx)
{ return assign_rows(p, j, x, sel_seq(st, end), vp, vj, vx); }
SEXP _MatrixExtra_set_arbitrary_rows_to_smat(SEXP p, SEXP j, SEXP x, SEXP rows, SEXP vp, SEXP vj, SEXP vx)
{ return assign_rows(p, j, x, sel_set(rows), vp, vj, vx); }

#define MX_ENTRY(name, n) {"_MatrixExtra_" #name, (DL_FUNC)&_MatrixExtra_##name, n}
static const R_CallMethodDef mxgpu_call_entries[] = {
    MX_ENTRY(matmul_dense_csc_numeric, 5), MX_ENTRY(matmul_dense_csc_float32, 5),
    MX_ENTRY(tcrossprod_dense_csr_numeric, 6), MX_ENTRY(tcrossprod_dense_csr_float32, 6),
    MX_ENTRY(tcrossprod_csr_dense_numeric, 5), MX_ENTRY(tcrossprod_csr_dense_float32, 5),
    MX_ENTRY(matmul_csr_dvec_numeric, 5), MX_ENTRY(matmul_csr_dvec_integer, 5),
    MX_ENTRY(matmul_csr_dvec_logical, 5), MX_ENTRY(matmul_csr_dvec_float32, 5),
    MX_ENTRY(multiply_csr_elemwise, 6), MX_ENTRY(logicaland_csr_elemwise, 6),
    MX_ENTRY(add_csr_elemwise, 7), MX_ENTRY(logicalor_csr_elemwise, 7),
    MX_ENTRY(copy_csr_rows_numeric, 4), MX_ENTRY(copy_csr_rows_logical, 4), MX_ENTRY(copy_csr_rows_binary, 3),
    MX_ENTRY(check_is_seq, 1), MX_ENTRY(check_is_rev_seq, 1),
    MX_ENTRY(copy_csr_rows_col_seq_numeric, 6), MX_ENTRY(copy_csr_rows_col_seq_logical, 6),
    MX_ENTRY(copy_csr_rows_col_seq_binary, 5),
    MX_ENTRY(copy_csr_arbitrary_numeric, 5), MX_ENTRY(copy_csr_arbitrary_logical, 5), MX_ENTRY(copy_csr_arbitrary_binary, 4),
    MX_ENTRY(reverse_rows_numeric, 3), MX_ENTRY(reverse_rows_logical, 3), MX_ENTRY(reverse_rows_binary, 2),
    MX_ENTRY(reverse_columns_inplace_numeric, 4), MX_ENTRY(reverse_columns_inplace_logical, 4),
    MX_ENTRY(reverse_columns_inplace_binary, 4),
    MX_ENTRY(multiply_csr_by_dvec_no_NAs_numeric, 11), MX_ENTRY(logicaland_csr_by_dvec_internal, 5),
    MX_ENTRY(multiply_csr_by_dvec_with_NAs, 11),
    MX_ENTRY(multiply_csr_by_coo_elemwise, 8), MX_ENTRY(logicaland_csr_by_coo_elemwise, 8),
    MX_ENTRY(multiply_coo_by_dense_ignore_NAs_numeric, 12), MX_ENTRY(multiply_coo_by_dense_ignore_NAs_logical, 6),
    MX_ENTRY(slice_coo_single_numeric, 5), MX_ENTRY(slice_coo_single_logical, 5), MX_ENTRY(slice_coo_single_binary, 4),
    MX_ENTRY(slice_coo_arbitrary_numeric, 13), MX_ENTRY(slice_coo_arbitrary_logical, 13),
    MX_ENTRY(slice_coo_arbitrary_binary, 12),
    MX_ENTRY(remove_zero_valued_csr_numeric, 4), MX_ENTRY(remove_zero_valued_csr_logical, 4),
    MX_ENTRY(remove_zero_valued_coo_numeric, 4), MX_ENTRY(remove_zero_valued_coo_logical, 4),
    MX_ENTRY(remove_zero_valued_svec_numeric, 3), MX_ENTRY(remove_zero_valued_svec_integer, 3),
    MX_ENTRY(remove_zero_valued_svec_logical, 3),
    MX_ENTRY(check_valid_csr_matrix, 4), MX_ENTRY(check_valid_coo_matrix, 4), MX_ENTRY(check_valid_svec, 2),
    MX_ENTRY(rebuild_indptr_after_filter, 2),
    MX_ENTRY(multiply_csc_by_dense_ignore_NAs_numeric, 4), MX_ENTRY(multiply_csc_by_dense_ignore_NAs_float32, 4),
    MX_ENTRY(multiply_csc_by_dense_ignore_NAs_integer, 4), MX_ENTRY(multiply_csc_by_dense_ignore_NAs_logical, 4),
    MX_ENTRY(logicaland_csc_by_dense_ignore_NAs, 4),
    MX_ENTRY(multiply_csc_by_dense_keep_NAs_numeric, 4), MX_ENTRY(multiply_csc_by_dense_keep_NAs_integer, 4),
    MX_ENTRY(multiply_csc_by_dense_keep_NAs_logical, 4), MX_ENTRY(multiply_csc_by_dense_keep_NAs_float32, 4),
    MX_ENTRY(multiply_csr_by_svec_no_NAs, 6), MX_ENTRY(multiply_csr_by_svec_keep_NAs, 7),
    MX_ENTRY(sort_vector_indices_numeric, 2), MX_ENTRY(sort_vector_indices_integer, 2),
    MX_ENTRY(sort_vector_indices_logical, 2), MX_ENTRY(sort_vector_indices_binary, 1),
    MX_ENTRY(sort_coo_indices_numeric, 3), MX_ENTRY(sort_coo_indices_logical, 3), MX_ENTRY(sort_coo_indices_binary, 2),
    MX_ENTRY(matmul_rowvec_by_csc, 4), MX_ENTRY(matmul_rowvec_by_cscbin, 3),
    MX_ENTRY(matmul_colvec_by_scolvecascsr_f32, 4), MX_ENTRY(matmul_colvec_by_scolvecascsr, 4),
    MX_ENTRY(matmul_spcolvec_by_scolvecascsr_numeric, 6), MX_ENTRY(matmul_spcolvec_by_scolvecascsr_integer, 6),
    MX_ENTRY(matmul_spcolvec_by_scolvecascsr_logical, 6), MX_ENTRY(matmul_spcolvec_by_scolvecascsr_binary, 5),
    MX_ENTRY(set_single_row_to_zero, 4), MX_ENTRY(set_single_col_to_zero, 4), MX_ENTRY(set_single_val_to_zero, 5),
    MX_ENTRY(set_single_row_to_const, 6), MX_ENTRY(set_single_col_to_const, 6), MX_ENTRY(set_single_val_to_const, 7),
    MX_ENTRY(set_rowseq_to_zero, 5), MX_ENTRY(set_rowseq_to_const, 7),
    MX_ENTRY(set_colseq_to_zero, 6), MX_ENTRY(set_colseq_to_const, 7),
    MX_ENTRY(set_arbitrary_rows_to_zero, 4), MX_ENTRY(set_arbitrary_rows_to_const, 6),
    MX_ENTRY(set_arbitrary_cols_to_zero, 5), MX_ENTRY(set_arbitrary_cols_to_const, 6),
    MX_ENTRY(set_arbitrary_rows_single_col_to_zero, 6), MX_ENTRY(set_arbitrary_rows_single_col_to_const, 7),
    MX_ENTRY(set_single_row_arbitrary_cols_to_zero, 6), MX_ENTRY(set_single_row_arbitrary_cols_to_const, 7),
    MX_ENTRY(set_arbitrary_rows_arbitrary_cols_to_zero, 6), MX_ENTRY(set_arbitrary_rows_arbitrary_cols_to_const, 7),
    MX_ENTRY(set_rowseq_to_smat, 8), MX_ENTRY(set_arbitrary_rows_to_smat, 7),
    {"mxgpu_csr_transpose", (DL_FUNC)&mxgpu_csr_transpose, 4},
    {"mxgpu_coo_to_csr", (DL_FUNC)&mxgpu_coo_to_csr, 5},
    {NULL, NULL, 0}
};

// standalone use: dyn.load("mxgpu_r.so") registers the 19 routines under their reference names
void R_init_mxgpu_r(DllInfo *dll)
{
    R_registerRoutines(dll, NULL, mxgpu_call_entries, NULL, NULL);
    R_useDynamicSymbols(dll, FALSE);
}

}  // extern "C"
#endif  // MXGPU_HAVE_R

// r_shim.cpp — thin `.Call` translation unit between R and libmxgpu's C-ABI.
//
// Exports 103 routines of the reference under exactly the native-routine names and arities it registers in
// CallEntries[] (src/RcppExports.cpp), so R code written as `.Call("_MatrixExtra_<fn>", ...)` (R/RcppExports.R)
// dispatches unchanged, and two of its own: mxgpu_csr_transpose, the device transpose behind the overlay's
// t_deep_internal, and mxgpu_coo_to_csr, the device COO sort behind its as.csr.matrix / as.csc.matrix of a
// TsparseMatrix.  R_init_mxgpu_r registers all 105.  Written against the plain R C API (no Rcpp).
//
// This file is NOT part of libmxgpu.so: it is built on a machine that has R with
//     R CMD SHLIB -o mxgpu_r.so r_shim.cpp -L<repo>/matrixextra_amd -lmxgpu -I<repo>/include
// No R has compiled or run it yet.  What does compile and run it is the project's own build: `make rshim` builds it
// with -Wall -Wextra -Werror against the stand-in for R's C API under tests/rstub, once linked to libmxgpu.so and once
// to a generated fake of the C-ABI, and tests/test_rshim_host.py / test_rshim_refusals.py / test_gpu_rshim.py call
// every routine below through it.  See INTEGRATION.md.  Everything numerically meaningful lives behind the C-ABI and
// is tested through it; what is left here is mechanical marshalling, said once each in four layers:
//   1. argument views: Vec<T> (Ints, Reals, Lgls, F32s), Csr<X> and the optional-values view Vals borrow an input,
//      coercing only when the SEXP type differs (as Rcpp's input_parameter<> does); data_ptr() is the one place that
//      picks REAL / LOGICAL / INTEGER; same_length / not_shorter / covers are the refusals;
//   2. result(): the one begin - fail - finish path of every variable-size result.  The D2H copy lands directly in
//      R-allocated vectors; identical-structure merges return the INPUT indptr / indices SEXPs (operators.cpp:127-131,
//      :390-394); make_list() builds every named list;
//   3. filled(): a fixed-size output is allocated by the caller, filled by one C-ABI call and returned;
//   4. one helper per routine family, and the `SEXP _MatrixExtra_<name>(...)` definitions as forwarders to it.
// A non-zero status becomes Rf_error(mx_last_error()) after the device handle is released.
//
// Rules (they are what the helpers are for):
//   * Rf_error and every R allocation can long-jump, so nothing that owns heap memory may be alive here: no
//     std::vector, std::string or std::function; callables are template parameters.  Protect is the only type with a
//     destructor (it owns no memory, and R resets the protect stack itself after a long-jump);
//   * between a successful *_begin and finish_guarded / mx_result_discard there is no R allocation outside
//     R_ExecWithCleanup;
//   * a coerced copy is protected before the next allocation (as_type);
//   * C++11 only (R's default on older installations), and only the R API that tests/rstub/Rinternals.h declares;
//   * every routine definition is plain text at the start of a line with the reference's parameter count
//     (tests/rshim_registry.py reads them), no macro generates one, and mxgpu_call_entries[] is written by hand.
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
inline void require(bool ok, const char *message) { if (!ok) Rf_error("%s", message); }
inline void same_length(R_xlen_t a, R_xlen_t b, const char *message) { require(a == b, message); }
inline void not_shorter(R_xlen_t a, R_xlen_t b, const char *message) { require(a >= b, message); }

// ---- 1. argument views ----------------------------------------------------------------------------------------
inline void *data_ptr(SEXP s)
{
    switch (TYPEOF(s)) {
        case REALSXP: return REAL(s);
        case LGLSXP: return LOGICAL(s);
        case INTSXP: return INTEGER(s);
        default: return nullptr;
    }
}
// the R vector type that carries an MX_* dtype; no values at all is an empty double vector.  float32@Data is an INTSXP
// matrix carrying binary32 bit patterns (R/matmul.R:260,276; matmul.cpp:213)
inline SEXPTYPE rtype_of(int dtype)
{ return dtype == MX_LGL ? LGLSXP : dtype == MX_I32 || dtype == MX_F32 ? INTSXP : REALSXP; }

template <class T, SEXPTYPE RT> struct Vec {      // x coerced to RT, borrowed as T
    typedef T elem;
    static SEXPTYPE rtype() { return RT; }
    SEXP s; const T *ptr; R_xlen_t n;
    Vec(SEXP x, Protect &p) : s(as_type(x, RT, p)), ptr(static_cast<const T *>(data_ptr(s))), n(XLENGTH(s)) {}
    const T *unless_empty() const { return n ? ptr : nullptr; }
};
typedef Vec<int32_t, INTSXP> Ints;
typedef Vec<double, REALSXP> Reals;
typedef Vec<int32_t, LGLSXP> Lgls;
typedef Vec<float, INTSXP> F32s;

// a values vector that may be absent: MX_NONE with a null pointer and no length.  ptr is writable for the in-place
// routines, the only ones that write through it
struct Vals {
    SEXP s; int dtype; void *ptr; int64_t n;
    // coerced to the R type that `dtype` names
    static Vals coerced(SEXP x, int dtype, Protect &p)
    {
        if (dtype == MX_NONE) return Vals{x, MX_NONE, nullptr, 0};
        x = as_type(x, rtype_of(dtype), p);
        return Vals{x, dtype, data_ptr(x), (int64_t)XLENGTH(x)};
    }
    // the dtype is the vector's own: double, logical or NULL
    static Vals by_type(SEXP x, const char *refusal)
    {
        require(TYPEOF(x) == REALSXP || TYPEOF(x) == LGLSXP || x == R_NilValue, refusal);
        return borrowed(x, TYPEOF(x) == REALSXP ? MX_F64 : TYPEOF(x) == LGLSXP ? MX_LGL : MX_NONE);
    }
    // as it is, for the routines that work in place: a vector of another type than `dtype` names is absent
    static Vals borrowed(SEXP x, int dtype)
    {
        if (dtype == MX_NONE || (SEXPTYPE)TYPEOF(x) != rtype_of(dtype)) return Vals{x, MX_NONE, nullptr, 0};
        return Vals{x, dtype, data_ptr(x), (int64_t)XLENGTH(x)};
    }
};
// an index vector of an in-place routine: never coerced
inline int32_t *borrowed_ints(SEXP x, const char *refusal)
{
    require(TYPEOF(x) == INTSXP, refusal);
    return static_cast<int32_t *>(data_ptr(x));
}

template <class X> struct Csr {                    // (indptr, indices, values) of a CSR or a CSC
    Ints p, j; X x; int nrows;
    Csr(SEXP p_, SEXP j_, SEXP x_, Protect &pr) : p(p_, pr), j(j_, pr), x(x_, pr), nrows((int)p.n - 1) {}
    Csr(SEXP p_, SEXP j_, const X &x_, Protect &pr) : p(p_, pr), j(j_, pr), x(x_), nrows((int)p.n - 1) {}
};
// `n` entries must reach as far as the last element of the index pointer says
inline void covers(const Ints &indptr, R_xlen_t n, const char *message)
{
    not_shorter(indptr.n, 1, message);
    not_shorter(n, indptr.ptr[indptr.n - 1], message);
}

// ---- 2. variable-size results ---------------------------------------------------------------------------------
const char *const CSR_NAMES[3] = {"indptr", "indices", "values"};
const char *const COO_NAMES[3] = {"ii", "jj", "xx"};
const char *const ROW_COL_VAL[3] = {"row", "col", "val"};
const char *const SVEC_NAMES[2] = {"ii", "xx"};

SEXP make_list(int n, const char *const *names, const SEXP *elements, Protect &p)
{
    SEXP out = p(Rf_allocVector(VECSXP, n));
    SEXP nm = p(Rf_allocVector(STRSXP, n));
    for (int k = 0; k < n; ++k) {
        SET_VECTOR_ELT(out, k, elements[k]);
        SET_STRING_ELT(nm, k, Rf_mkChar(names[k]));
    }
    Rf_setAttrib(out, R_NamesSymbol, nm);
    return out;
}

// mx_result_finish owns the handle from the moment it is entered and deletes it on every return, failure included:
// `res` is cleared before the call, so that no cleanup releases it a second time
struct FinishArgs { mx_result *res; mx_result_info info; SEXP alias_p, alias_j; const char *const *names; SEXP out; };
SEXP finish_list(FinishArgs &a, Protect &p)
{
    const mx_result_info &info = a.info;
    const R_xlen_t nv = info.values_dtype == MX_NONE ? 0 : (R_xlen_t)info.values_len;
    SEXP e[3] = {a.alias_p, a.alias_j, p(Rf_allocVector(rtype_of(info.values_dtype), nv))};   // may long-jump
    int32_t *indptr = nullptr, *indices = nullptr;             // an aliased structure is not downloaded
    if (!info.alias_structure) {
        e[0] = p(Rf_allocVector(INTSXP, (R_xlen_t)info.indptr_len));
        e[1] = p(Rf_allocVector(INTSXP, (R_xlen_t)info.nnz));
        indptr = static_cast<int32_t *>(data_ptr(e[0]));
        indices = static_cast<int32_t *>(data_ptr(e[1]));
    }
    mx_result *handle = a.res;
    a.res = nullptr;
    if (mx_result_finish(handle, indptr, indices, nv ? data_ptr(e[2]) : nullptr)) fail();
    return make_list(3, a.names, e, p);
}
// R allocation can long-jump; run it with the device handle guarded so it is never leaked
void finish_body(void *d)
{
    FinishArgs *a = static_cast<FinishArgs *>(d);
    Protect p;
    a->out = finish_list(*a, p);           // consumes a->res
    R_PreserveObject(a->out);              // survives p's UNPROTECT; released by the caller
}
void finish_cleanup(void *d)
{
    FinishArgs *a = static_cast<FinishArgs *>(d);
    if (a->res) mx_result_discard(a->res);
}
SEXP finish_guarded(mx_result *res, const mx_result_info &info, SEXP alias_p, SEXP alias_j, const char *const *names)
{
    FinishArgs a{res, info, alias_p, alias_j, names, R_NilValue};
    R_ExecWithCleanup([](void *d) -> SEXP { finish_body(d); return R_NilValue; }, &a, finish_cleanup, &a);
    SEXP out = a.out;
    PROTECT(out);
    R_ReleaseObject(out);
    UNPROTECT(1);
    return out;
}

// What a routine makes of the library's (indptr-or-ii, indices, values): three elements under `names`; SVEC, the last
// two under the two names of a sparse vector; CSR_OR_PATTERN, no `values` element when the result has none, as the
// reference's list (slice.cpp:565).
enum Shape { TRIPLE, SVEC, CSR_OR_PATTERN };
struct Out {
    const char *const *names; Shape shape;
    SEXP alias_p, alias_j;        // become indptr / indices when the library reports alias_structure == 1
    SEXP inputs[3];               // handed back when it reports MX_ALIAS_ALL: nothing changed
    int force_dtype; bool force_nonempty_only;
    explicit Out(const char *const *names_ = CSR_NAMES, Shape shape_ = TRIPLE)
        : names(names_), shape(shape_), alias_p(R_NilValue), alias_j(R_NilValue),
          inputs{R_NilValue, R_NilValue, R_NilValue}, force_dtype(MX_NONE), force_nonempty_only(false) {}
    Out &aliasing(SEXP p_, SEXP j_) { alias_p = p_; alias_j = j_; return *this; }
    Out &handing_back(SEXP a, SEXP b, SEXP x) { inputs[0] = a; inputs[1] = b; inputs[2] = x; return *this; }
    // the values keep the input's R type where the library cannot know it (an empty result, slice.cpp:246)
    Out &forcing(int dtype, bool nonempty_only = false)
    { force_dtype = dtype; force_nonempty_only = nonempty_only; return *this; }
};

// The one result path: `begin` is int(mx_result **, mx_result_info *), one mx_*_begin call.
template <class Begin> SEXP result(Begin begin, const Out &o)
{
    mx_result *res = nullptr;
    mx_result_info info;
    if (begin(&res, &info)) fail();
    if (info.alias_structure == MX_ALIAS_ALL) {
        mx_result_discard(res);                    // before any R allocation
        Protect p;
        return o.shape == SVEC ? make_list(2, o.names, o.inputs + 1, p) : make_list(3, o.names, o.inputs, p);
    }
    if (o.force_dtype != MX_NONE && (info.values_len || !o.force_nonempty_only)) info.values_dtype = o.force_dtype;
    const bool pattern = o.shape == CSR_OR_PATTERN && info.values_dtype == MX_NONE;
    if (o.shape != SVEC && !pattern) return finish_guarded(res, info, o.alias_p, o.alias_j, o.names);
    Protect p;
    SEXP l = p(finish_guarded(res, info, o.alias_p, o.alias_j, CSR_NAMES));
    const SEXP e[3] = {VECTOR_ELT(l, 0), VECTOR_ELT(l, 1), VECTOR_ELT(l, 2)};
    return make_list(2, o.names, pattern ? e : e + 1, p);
}

// ---- 3. fixed-size results --------------------------------------------------------------------------------------
// `out` is a fresh, protected vector or matrix of T; `call` is int(T *), one C-ABI call that fills it
template <class T, class Call> SEXP filled(SEXP out, Call call)
{
    if (call(static_cast<T *>(data_ptr(out)))) fail();
    return out;
}

// ---- 4. the routine families ------------------------------------------------------------------------------------
// CSR x dense, dense x CSC, dense x t(CSR): D is the dense operand's and the result's view, Reals or F32s; fn here
// and below is the family's C-ABI function
template <class D, class Fn> SEXP csr_times_dense(SEXP p_, SEXP j_, SEXP x_, SEXP Y_, SEXP nthreads, Fn fn)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const D Y(Y_, p);
    const int n = Rf_nrows(Y.s), K = Rf_ncols(Y.s);
    return filled<typename D::elem>(p(Rf_allocMatrix(D::rtype(), A.nrows, n)), [&](typename D::elem *out) {
        return fn(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, Y.ptr, n, K, Rf_asInteger(nthreads), out); });
}
template <class D, class Fn> SEXP dense_times_sparse(SEXP X_, SEXP p_, SEXP i_, SEXP x_, SEXP nthreads, Fn fn)
{
    Protect p;
    const D X(X_, p);
    const Csr<Reals> A(p_, i_, x_, p);
    const int nr = Rf_nrows(X.s), nc = Rf_ncols(X.s);
    return filled<typename D::elem>(p(Rf_allocMatrix(D::rtype(), nr, A.nrows)), [&](typename D::elem *out) {
        return fn(X.ptr, nr, nc, A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, Rf_asInteger(nthreads), out); });
}
// tcrossprod_dense_csr_* is the same call with ncols_Y before the output
template <class D, class Fn>
SEXP dense_times_tcsr(SEXP X, SEXP p_, SEXP j_, SEXP x_, SEXP nthreads, SEXP ncols_Y, Fn fn)
{
    typedef typename D::elem T;
    return dense_times_sparse<D>(X, p_, j_, x_, nthreads,
        [&](const T *X_, int nr, int nc, const int32_t *ip, const int32_t *ij, const double *ix, int nrY, int nth, T *out) {
            return fn(X_, nr, nc, ip, ij, ix, nrY, nth, Rf_asInteger(ncols_Y), out); });
}

// CSR x dense vector: Y the vector's view, O the result's
template <class Y, class O, class Fn> SEXP csr_times_dvec(SEXP p_, SEXP j_, SEXP x_, SEXP y_, SEXP nthreads, Fn fn)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const Y y(y_, p);
    return filled<typename O::elem>(p(Rf_allocVector(O::rtype(), A.nrows)), [&](typename O::elem *out) {
        return fn(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, y.ptr, (int)y.n, Rf_asInteger(nthreads), out); });
}

// CSR (+) CSR: when both have the same structure the result's indptr / indices are the first operand's
SEXP elemwise(int op, SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, int dtype)
{
    Protect p;
    const Ints P1(p1, p), P2(p2, p), J1(j1, p), J2(j2, p);
    const Vals X1 = Vals::coerced(x1, dtype, p), X2 = Vals::coerced(x2, dtype, p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_csr_elemwise_begin(op, (int)P1.n - 1, P1.ptr, P2.ptr, J1.ptr, J2.ptr, X1.ptr, X2.ptr, (int64_t)J1.n,
                                     (int64_t)J2.n, res, info); }, Out().aliasing(P1.s, J1.s));
}

// X[rows, ]: empty values keep their R type
SEXP copy_rows(SEXP p_, SEXP j_, SEXP x_, SEXP rows_, int dtype)
{
    Protect p;
    const Csr<Vals> A(p_, j_, Vals::coerced(x_, dtype, p), p);
    const Ints rows(rows_, p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_copy_csr_rows_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, dtype, A.x.n, rows.ptr, (int64_t)rows.n, res,
                                      info); }, Out().forcing(dtype));
}
// X[rows, a:b]: the values are a numeric vector whatever the input's are (slice.cpp:363)
SEXP col_seq(SEXP p_, SEXP j_, SEXP x_, SEXP rows_, SEXP cols_, SEXP index1, int dtype)
{
    Protect p;
    const Csr<Vals> A(p_, j_, Vals::coerced(x_, dtype, p), p);
    const Ints rows(rows_, p), cols(cols_, p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_copy_csr_rows_col_seq_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, dtype, A.x.n, rows.ptr,
                                              (int64_t)rows.n, cols.ptr, (int64_t)cols.n, Rf_asLogical(index1), res,
                                              info); }, Out());
}
SEXP arbitrary(SEXP p_, SEXP j_, SEXP x_, SEXP rows_, SEXP cols_, int dtype)
{
    Protect p;
    const Csr<Vals> A(p_, j_, Vals::coerced(x_, dtype, p), p);
    const Ints rows(rows_, p), cols(cols_, p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_copy_csr_arbitrary_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, dtype, A.x.n, rows.ptr, (int64_t)rows.n,
                                           cols.ptr, (int64_t)cols.n, res, info); }, Out(CSR_NAMES, CSR_OR_PATTERN));
}
// logical values stay logical unless the result is empty
SEXP reverse_rows(SEXP p_, SEXP j_, SEXP x_, int dtype)
{
    Protect p;
    const Csr<Vals> A(p_, j_, Vals::coerced(x_, dtype, p), p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_reverse_rows_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, dtype, A.x.n, res, info); },
        Out().forcing(dtype == MX_LGL ? MX_LGL : MX_NONE, true));
}
// in place on the caller's vectors, like the reference (the R glue only passes freshly created results here): no
// coercion; only the indices move when the values are of another type, or empty
SEXP reverse_cols(SEXP p_, SEXP j_, SEXP x_, SEXP ncol, int dtype)
{
    const Vals x = Vals::borrowed(x_, dtype);
    const char *refusal = "reverse_columns_inplace: integer index vectors required";
    const int32_t *indptr = borrowed_ints(p_, refusal);
    int32_t *indices = borrowed_ints(j_, refusal);
    if (mx_reverse_columns_inplace(indptr, (int)XLENGTH(p_) - 1, indices, x.ptr, x.n ? dtype : MX_NONE, x.n,
                                   Rf_asInteger(ncol)))
        fail();
    return R_NilValue;
}

SEXP seq_check(SEXP idx_, int (*fn)(const int32_t *, int64_t, int *))
{
    Protect p;
    const Ints idx(idx_, p);
    int r = 0;
    if (fn(idx.ptr, (int64_t)idx.n, &r)) fail();
    return Rf_ScalarLogical(r);
}

// CSR (.) COO  (src/operators.cpp:673-720; glue src/RcppExports.cpp:1317-1350, 8 arguments): list(row, col, val)
SEXP csr_by_coo(int logical, SEXP p_, SEXP j_, SEXP x_, SEXP yi_, SEXP yj_, SEXP yx_, SEXP max_row, SEXP max_col)
{
    Protect p;
    const int dtype = logical ? MX_LGL : MX_F64;
    const Csr<Vals> A(p_, j_, Vals::coerced(x_, dtype, p), p);
    const Ints yi(yi_, p), yj(yj_, p);
    const Vals yx = Vals::coerced(yx_, dtype, p);
    const int m = Rf_asInteger(max_row);
    same_length(A.p.n, (R_xlen_t)m + 1, "multiply_csr_by_coo: indptr does not match max_row_X");
    same_length(yi.n, yj.n, "multiply_csr_by_coo: bad COO lengths");
    same_length(yi.n, yx.n, "multiply_csr_by_coo: bad COO lengths");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_multiply_csr_by_coo_begin(logical, A.p.ptr, A.j.ptr, A.x.ptr, yi.ptr, yj.ptr, yx.ptr, (int64_t)yi.n, m,
                                            Rf_asInteger(max_col), res, info); }, Out(ROW_COL_VAL));
}

// X[i, j] of a COO  (src/slice_coo.cpp:3-706; glue src/RcppExports.cpp:2061-2167): the single-element routines
// take 5 / 5 / 4 arguments and return a double / bool / bool; the arbitrary ones take 13 / 13 / 12 and return
// list(ii, jj, xx) (pattern: xx is an empty double vector here, the reference leaves it unset and R never reads it)
struct Coo {
    Ints i, j; Vals x;
    Coo(SEXP i_, SEXP j_, SEXP x_, int dtype, Protect &p, const char *indices_differ, const char *values_differ)
        : i(i_, p), j(j_, p), x(Vals::coerced(x_, dtype, p))
    {
        same_length(i.n, j.n, indices_differ);
        if (x.ptr) same_length(x.n, i.n, values_differ);
    }
};
SEXP slice_coo_single(int dtype, SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{
    Protect p;
    const Coo X(ii, jj, xx, dtype, p, "slice_coo_single: row and column indices have different length",
                "slice_coo_single: values and indices have different length");
    int found = 0;
    double vd = 0;
    int vl = 0;
    void *value_out = dtype == MX_F64 ? (void *)&vd : dtype == MX_LGL ? (void *)&vl : nullptr;     // a pattern has none
    if (mx_slice_coo_single(X.i.ptr, X.j.ptr, X.x.ptr, dtype, (int64_t)X.i.n, Rf_asInteger(i), Rf_asInteger(j), &found,
                            value_out))
        fail();
    if (dtype == MX_F64) return Rf_ScalarReal(found ? vd : 0.0);
    return Rf_ScalarLogical(found && (dtype == MX_NONE || vl != 0));       // C++ bool: NA reads as TRUE
}
SEXP slice_coo_arbitrary(int dtype, SEXP ii, SEXP jj, SEXP xx, SEXP rows_, SEXP cols_, SEXP all_i, SEXP all_j,
                         SEXP i_seq, SEXP j_seq, SEXP i_rev, SEXP j_rev, SEXP nrows, SEXP ncols)
{
    Protect p;
    const Ints rows(rows_, p), cols(cols_, p);
    const Coo X(ii, jj, xx, dtype, p, "slice_coo_arbitrary: row and column indices have different length",
                "slice_coo_arbitrary: values and indices have different length");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_slice_coo_arbitrary_begin(X.i.ptr, X.j.ptr, X.x.ptr, dtype, (int64_t)X.i.n, rows.ptr, (int64_t)rows.n,
                                            cols.ptr, (int64_t)cols.n, Rf_asLogical(all_i), Rf_asLogical(all_j),
                                            Rf_asLogical(i_seq), Rf_asLogical(j_seq), Rf_asLogical(i_rev),
                                            Rf_asLogical(j_rev), Rf_asInteger(nrows), Rf_asInteger(ncols), res, info); },
        Out(COO_NAMES));
}

// remove_sparse_zeros / filterSparse / check_sparse_matrix  (src/misc.cpp:553-1116; glue src/RcppExports.cpp
// CallEntries :2279-2289).  The zero removers return list(indptr, indices, values) / list(ii, jj, xx) / list(ii, xx)
// and, when nothing is removed, the input vectors themselves (misc.cpp:586-590, :735-739, :864-867).
template <class X, class Fn> SEXP rz_csr(SEXP p_, SEXP j_, SEXP x_, SEXP na_rm, Fn fn)
{
    Protect p;
    const Csr<X> A(p_, j_, x_, p);
    same_length(A.x.n, A.j.n, "remove_zero_valued_csr: indices and values have different length");
    return result([&](mx_result **res, mx_result_info *info) {
        return fn(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, Rf_asLogical(na_rm), res, info); },
        Out().handing_back(A.p.s, A.j.s, A.x.s));
}
template <class X, class Fn> SEXP rz_coo(SEXP ii_, SEXP jj_, SEXP xx_, SEXP na_rm, Fn fn)
{
    Protect p;
    const Ints ii(ii_, p), jj(jj_, p);
    const X xx(xx_, p);
    same_length(ii.n, jj.n, "remove_zero_valued_coo: bad lengths");
    same_length(ii.n, xx.n, "remove_zero_valued_coo: bad lengths");
    return result([&](mx_result **res, mx_result_info *info) {
        return fn(ii.ptr, jj.ptr, xx.ptr, (int64_t)ii.n, Rf_asLogical(na_rm), res, info); },
        Out(COO_NAMES).handing_back(ii.s, jj.s, xx.s));
}
// the integer kind reports MX_I32, which stays an INTSXP
template <class X, class Fn> SEXP rz_svec(SEXP ii_, SEXP xx_, SEXP na_rm, Fn fn)
{
    Protect p;
    const Ints ii(ii_, p);
    const X xx(xx_, p);
    same_length(ii.n, xx.n, "remove_zero_valued_svec: indices and values have different length");
    return result([&](mx_result **res, mx_result_info *info) {
        return fn(ii.ptr, xx.ptr, (int64_t)ii.n, Rf_asLogical(na_rm), res, info); },
        Out(SVEC_NAMES, SVEC).handing_back(R_NilValue, ii.s, xx.s));
}

SEXP err_list(const char *err)
{
    if (!err) return Rf_allocVector(VECSXP, 0);                     // Rcpp::List()
    Protect p;
    const char *const name[1] = {"err"};
    const SEXP message[1] = {p(Rf_mkString(err))};
    return make_list(1, name, message, p);
}

// CSC (.) dense  (src/operators.cpp:1061-1458; glue src/RcppExports.cpp:1464-1580, 4 arguments each): dense_ is the
// matrix (float32: the float32@Data INTSXP bit patterns), its row count nrow(dense_).  The ignore_NAs routines return
// the values vector, the keep_NAs ones list(indptr, indices, values).  X is the view of the values, D of the matrix.
template <class X, class D> struct CscDense {
    int nrows; Csr<X> A; D dense;
    CscDense(SEXP p_, SEXP i_, SEXP x_, SEXP dense_, Protect &p) : nrows(Rf_nrows(dense_)), A(p_, i_, x_, p), dense(dense_, p)
    {
        same_length(A.x.n, A.j.n, "multiply_csc_by_dense: indices and values have different length");
        same_length((R_xlen_t)nrows * A.nrows, dense.n, "multiply_csc_by_dense: dense matrix does not match");
    }
};
template <class X, class D, class Fn> SEXP csc_dense_ignore(SEXP p_, SEXP i_, SEXP x_, SEXP dense_, Fn fn)
{
    Protect p;
    const CscDense<X, D> a(p_, i_, x_, dense_, p);
    return filled<typename X::elem>(p(Rf_allocVector(X::rtype(), a.A.x.n)), [&](typename X::elem *out) {
        return fn(a.A.p.ptr, a.A.nrows, a.A.j.ptr, a.A.x.ptr, a.dense.ptr, a.nrows, out); });
}
template <class D, class Fn> SEXP csc_dense_keep(SEXP p_, SEXP i_, SEXP x_, SEXP dense_, Fn fn)
{
    Protect p;
    const CscDense<Reals, D> a(p_, i_, x_, dense_, p);
    return result([&](mx_result **res, mx_result_info *info) {
        return fn(a.A.p.ptr, a.A.nrows, a.A.j.ptr, a.A.x.ptr, a.dense.ptr, a.nrows, res, info); }, Out());
}

// RsparseMatrix * sparseVector  (src/operators.cpp:3426-3697; 6 and 7 arguments): ii_base1 sorted, an empty xx is an
// nsparseVector and travels as a null pointer.  Both return list(indptr, indices, values).
SEXP csr_by_svec(int keep, SEXP p_, SEXP j_, SEXP x_, SEXP ii_, SEXP xx_, int ncols, SEXP length)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const Ints ii(ii_, p);
    const Reals xx(xx_, p);
    same_length(A.x.n, A.j.n, "multiply_csr_by_svec: indices and values have different length");
    if (xx.n) same_length(xx.n, ii.n, "multiply_csr_by_svec: vector indices and values differ");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_multiply_csr_by_svec_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, ii.ptr, xx.unless_empty(),
                                             (int64_t)ii.n, ncols, Rf_asInteger(length), keep, res, info); }, Out());
}

// outer products with a one-column CSR and float32 row vector x CSC  (src/matmul.cpp:643-938; outer.hip)
SEXP outer_dense(int dtype, SEXP colvec_, SEXP p_, SEXP j_, SEXP x_)
{
    Protect p;
    const Vals colvec = Vals::coerced(colvec_, dtype, p);
    const Csr<Reals> A(p_, j_, x_, p);
    covers(A.p, A.x.n, "matmul_colvec_by_scolvecascsr: values shorter than the index pointer says");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_matmul_colvec_by_scolvecascsr_begin(colvec.ptr, dtype, (int)colvec.n, A.p.ptr, A.nrows, A.j.ptr,
                                                      A.x.ptr, res, info); }, Out());
}
SEXP outer_svec(int dtype, SEXP p_, SEXP j_, SEXP x_, SEXP yi_, SEXP yx_, SEXP length)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const Ints yi(yi_, p);
    const Vals yx = Vals::coerced(yx_, dtype, p);
    if (dtype != MX_NONE) same_length(yx.n, yi.n, "matmul_spcolvec_by_scolvecascsr: vector indices and values differ");
    covers(A.p, A.x.n, "matmul_spcolvec_by_scolvecascsr: values shorter than the index pointer says");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_matmul_spcolvec_by_scolvecascsr_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, yi.ptr, yx.ptr, dtype,
                                                        (int64_t)yi.n, Rf_asInteger(length), res, info); }, Out());
}
// a 1 x ncol integer matrix holding the float32 bits, as Rcpp::IntegerMatrix(1, ncols_Y); x_ is NULL for a pattern
SEXP rowvec_csc(SEXP v_, SEXP p_, SEXP i_, SEXP x_)
{
    Protect p;
    const F32s v(v_, p);
    const Csr<Vals> A(p_, i_, Vals::coerced(x_, x_ != R_NilValue ? MX_F64 : MX_NONE, p), p);
    const char *refusal = "matmul_rowvec_by_csc: indices / values shorter than the index pointer says";
    covers(A.p, A.j.n, refusal);
    if (A.x.dtype != MX_NONE) covers(A.p, A.x.n, refusal);
    return filled<float>(p(Rf_allocMatrix(INTSXP, 1, A.nrows)), [&](float *out) {
        return mx_matmul_rowvec_by_csc(v.ptr, (int64_t)v.n, A.p.ptr, A.nrows, A.j.ptr,
                                       static_cast<const double *>(A.x.ptr), out); });
}

// sort_vector_indices_*  (src/misc.cpp:489-527) and sort_coo_indices_*  (src/misc.cpp:430-457): the caller's vectors
// are sorted where they are, so no coercion: values of another type, or of another length, are refused
SEXP sort_svec(SEXP ii_, SEXP xx_, int dtype)
{
    int32_t *ii = borrowed_ints(ii_, "sort_vector_indices: indices must be an integer vector");
    const Vals xx = Vals::borrowed(xx_, dtype);
    if (dtype != MX_NONE) require(xx.dtype == dtype && xx.n == XLENGTH(ii_), "sort_vector_indices: values do not match");
    if (mx_sort_vector_indices(ii, xx.ptr, (int64_t)XLENGTH(ii_), dtype)) fail();
    return R_NilValue;
}
SEXP sort_coo(SEXP ii_, SEXP jj_, SEXP xx_, int dtype)
{
    int32_t *ii = borrowed_ints(ii_, "sort_coo_indices: indices must be integer vectors");
    int32_t *jj = borrowed_ints(jj_, "sort_coo_indices: indices must be integer vectors");
    same_length(XLENGTH(jj_), XLENGTH(ii_), "sort_coo_indices: indices do not match");
    const Vals xx = Vals::borrowed(xx_, dtype);
    if (dtype != MX_NONE) require(xx.dtype == dtype && xx.n == XLENGTH(ii_), "sort_coo_indices: values do not match");
    if (mx_sort_coo_indices(ii, jj, xx.ptr, (int64_t)XLENGTH(ii_), dtype)) fail();
    return R_NilValue;
}

// `[<-` of a dgRMatrix: the set_* routines of src/assignment.cpp (glue: src/RcppExports.cpp, one CallEntries line
// each) over mx_assign_csr_scalar_begin / mx_assign_csr_rows_begin.  A selector is (kind, lo, hi, set); where the
// reference returns its input vectors (MX_ALIAS_ALL) or its input indptr / indices with new values (alias 1), so
// does this.  The zero-route routines of the reference receive no ncol; NCOL_UNKNOWN stands for "not needed".
struct Sel {
    int kind, lo, hi; SEXP set;
    void coerce(Protect &p) { if (kind == MX_SEL_ARBITRARY) set = as_type(set, INTSXP, p); }
    const int32_t *ptr() const { return kind == MX_SEL_ARBITRARY ? static_cast<const int32_t *>(data_ptr(set)) : nullptr; }
    int64_t n() const { return kind == MX_SEL_ARBITRARY ? (int64_t)XLENGTH(set) : 0; }
};
const int NCOL_UNKNOWN = 2147483647;
Sel sel_all() { return Sel{MX_SEL_ALL, 0, 0, R_NilValue}; }
Sel sel_one(SEXP k) { const int v = Rf_asInteger(k); return Sel{MX_SEL_SINGLE, v, v, R_NilValue}; }
Sel sel_seq(SEXP a, SEXP b) { return Sel{MX_SEL_RANGE, Rf_asInteger(a), Rf_asInteger(b), R_NilValue}; }
Sel sel_set(SEXP v) { return Sel{MX_SEL_ARBITRARY, 0, 0, v}; }

SEXP assign_scalar(SEXP p_, SEXP j_, SEXP x_, int ncols, Sel si, Sel sj, double value)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    same_length(A.x.n, A.j.n, "assignment: indices and values have different length");
    si.coerce(p);
    sj.coerce(p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_assign_csr_scalar_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, ncols, si.kind, si.lo, si.hi, si.ptr(),
                                          si.n(), sj.kind, sj.lo, sj.hi, sj.ptr(), sj.n(), value, res, info); },
        Out().aliasing(A.p.s, A.j.s).handing_back(A.p.s, A.j.s, A.x.s));
}
SEXP assign_rows(SEXP p_, SEXP j_, SEXP x_, Sel si, SEXP vp, SEXP vj, SEXP vx)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p), V(vp, vj, vx, p);
    const char *refusal = "assignment: indices and values have different length";
    same_length(A.x.n, A.j.n, refusal);
    same_length(V.x.n, V.j.n, refusal);
    not_shorter(V.p.n, 1, refusal);
    si.coerce(p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_assign_csr_rows_begin(A.p.ptr, A.nrows, A.j.ptr, A.x.ptr, si.kind, si.lo, si.hi, si.ptr(), si.n(),
                                        V.p.ptr, (int64_t)V.nrows, V.j.ptr, V.x.ptr, res, info); },
        Out().aliasing(A.p.s, A.j.s).handing_back(A.p.s, A.j.s, A.x.s));
}

}  // namespace

extern "C" {

// ---- CSR x dense --------------------------------------------------------------------------------
SEXP _MatrixExtra_tcrossprod_csr_dense_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP Y, SEXP nthreads)
{ return csr_times_dense<Reals>(p_, j_, x_, Y, nthreads, mx_tcrossprod_csr_dense_numeric); }
SEXP _MatrixExtra_tcrossprod_csr_dense_float32(SEXP p_, SEXP j_, SEXP x_, SEXP Y, SEXP nthreads)
{ return csr_times_dense<F32s>(p_, j_, x_, Y, nthreads, mx_tcrossprod_csr_dense_float32); }
SEXP _MatrixExtra_matmul_dense_csc_numeric(SEXP X, SEXP p_, SEXP i_, SEXP x_, SEXP nthreads)
{ return dense_times_sparse<Reals>(X, p_, i_, x_, nthreads, mx_matmul_dense_csc_numeric); }
SEXP _MatrixExtra_matmul_dense_csc_float32(SEXP X, SEXP p_, SEXP i_, SEXP x_, SEXP nthreads)
{ return dense_times_sparse<F32s>(X, p_, i_, x_, nthreads, mx_matmul_dense_csc_float32); }
SEXP _MatrixExtra_tcrossprod_dense_csr_numeric(SEXP X, SEXP p_, SEXP j_, SEXP x_, SEXP nthreads, SEXP ncols_Y)
{ return dense_times_tcsr<Reals>(X, p_, j_, x_, nthreads, ncols_Y, mx_tcrossprod_dense_csr_numeric); }
SEXP _MatrixExtra_tcrossprod_dense_csr_float32(SEXP X, SEXP p_, SEXP j_, SEXP x_, SEXP nthreads, SEXP ncols_Y)
{ return dense_times_tcsr<F32s>(X, p_, j_, x_, nthreads, ncols_Y, mx_tcrossprod_dense_csr_float32); }

// ---- CSR x dense vector ---------------------------------------------------------------------------
SEXP _MatrixExtra_matmul_csr_dvec_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{ return csr_times_dvec<Reals, Reals>(p_, j_, x_, y, nthreads, mx_matmul_csr_dvec_numeric); }
SEXP _MatrixExtra_matmul_csr_dvec_integer(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{ return csr_times_dvec<Ints, Reals>(p_, j_, x_, y, nthreads, mx_matmul_csr_dvec_integer); }
SEXP _MatrixExtra_matmul_csr_dvec_logical(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{ return csr_times_dvec<Lgls, Reals>(p_, j_, x_, y, nthreads, mx_matmul_csr_dvec_logical); }
SEXP _MatrixExtra_matmul_csr_dvec_float32(SEXP p_, SEXP j_, SEXP x_, SEXP y, SEXP nthreads)
{ return csr_times_dvec<F32s, F32s>(p_, j_, x_, y, nthreads, mx_matmul_csr_dvec_float32); }

// ---- CSR (+) CSR --------------------------------------------------------------------------------------
SEXP _MatrixExtra_multiply_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2)
{ return elemwise(MX_OP_MUL, p1, p2, j1, j2, x1, x2, MX_F64); }
SEXP _MatrixExtra_logicaland_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2)
{ return elemwise(MX_OP_AND, p1, p2, j1, j2, x1, x2, MX_LGL); }
SEXP _MatrixExtra_add_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, SEXP substract)
{ return elemwise(Rf_asLogical(substract) ? MX_OP_SUB : MX_OP_ADD, p1, p2, j1, j2, x1, x2, MX_F64); }
SEXP _MatrixExtra_logicalor_csr_elemwise(SEXP p1, SEXP p2, SEXP j1, SEXP j2, SEXP x1, SEXP x2, SEXP xor_op)
{ return elemwise(Rf_asLogical(xor_op) ? MX_OP_XOR : MX_OP_OR, p1, p2, j1, j2, x1, x2, MX_LGL); }

// ---- X[rows, ] -------------------------------------------------------------------------------------------
SEXP _MatrixExtra_copy_csr_rows_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows) { return copy_rows(p_, j_, x_, rows, MX_F64); }
SEXP _MatrixExtra_copy_csr_rows_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows) { return copy_rows(p_, j_, x_, rows, MX_LGL); }
SEXP _MatrixExtra_copy_csr_rows_binary(SEXP p_, SEXP j_, SEXP rows) { return copy_rows(p_, j_, R_NilValue, rows, MX_NONE); }

// ---- X[rows, cols] (§8f rank 2) -----------------------------------------------------------------------------
SEXP _MatrixExtra_copy_csr_rows_col_seq_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, x_, rows, cols, index1, MX_F64); }
SEXP _MatrixExtra_copy_csr_rows_col_seq_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, x_, rows, cols, index1, MX_LGL); }
SEXP _MatrixExtra_copy_csr_rows_col_seq_binary(SEXP p_, SEXP j_, SEXP rows, SEXP cols, SEXP index1)
{ return col_seq(p_, j_, R_NilValue, rows, cols, index1, MX_NONE); }
SEXP _MatrixExtra_copy_csr_arbitrary_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, x_, rows, cols, MX_F64); }
SEXP _MatrixExtra_copy_csr_arbitrary_logical(SEXP p_, SEXP j_, SEXP x_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, x_, rows, cols, MX_LGL); }
SEXP _MatrixExtra_copy_csr_arbitrary_binary(SEXP p_, SEXP j_, SEXP rows, SEXP cols) { return arbitrary(p_, j_, R_NilValue, rows, cols, MX_NONE); }
SEXP _MatrixExtra_reverse_rows_numeric(SEXP p_, SEXP j_, SEXP x_) { return reverse_rows(p_, j_, x_, MX_F64); }
SEXP _MatrixExtra_reverse_rows_logical(SEXP p_, SEXP j_, SEXP x_) { return reverse_rows(p_, j_, x_, MX_LGL); }
SEXP _MatrixExtra_reverse_rows_binary(SEXP p_, SEXP j_) { return reverse_rows(p_, j_, R_NilValue, MX_NONE); }
SEXP _MatrixExtra_reverse_columns_inplace_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_F64); }
SEXP _MatrixExtra_reverse_columns_inplace_logical(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_LGL); }
SEXP _MatrixExtra_reverse_columns_inplace_binary(SEXP p_, SEXP j_, SEXP x_, SEXP ncol) { return reverse_cols(p_, j_, x_, ncol, MX_NONE); }
SEXP _MatrixExtra_check_is_seq(SEXP idx) { return seq_check(idx, mx_check_is_seq); }
SEXP _MatrixExtra_check_is_rev_seq(SEXP idx) { return seq_check(idx, mx_check_is_rev_seq); }

// values-only CSR (op) vector  (src/operators.cpp:2142-2200; glue src/RcppExports.cpp `_MatrixExtra_multiply_csr_by_dvec_no_NAs_numeric`, 11 arguments)
SEXP _MatrixExtra_multiply_csr_by_dvec_no_NAs_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols, SEXP multiply,
                                                      SEXP powerto, SEXP divide, SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const Reals d(dvec, p);
    return filled<double>(p(Rf_allocVector(REALSXP, A.x.n)), [&](double *out) {
        return mx_multiply_csr_by_dvec_no_NAs_numeric(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, d.ptr, (int64_t)d.n,
                                                      Rf_asInteger(ncols), Rf_asLogical(multiply), Rf_asLogical(powerto),
                                                      Rf_asLogical(divide), Rf_asLogical(divrest), Rf_asLogical(intdiv),
                                                      Rf_asLogical(lhs), out); });
}
// CSR (op) vector keeping R's NA cells  (src/operators.cpp:2258-2852; glue src/RcppExports.cpp:1628-1645, 11
// arguments): list(indptr, indices, values); when the flat regime adds no entry, indptr / indices are the arguments
// themselves, as the reference returns them (:2643-2651)
SEXP _MatrixExtra_multiply_csr_by_dvec_with_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols, SEXP multiply,
                                                SEXP powerto, SEXP divide, SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    const Csr<Reals> A(p_, j_, x_, p);
    const Reals d(dvec, p);
    same_length(A.x.n, A.j.n, "multiply_csr_by_dvec_with_NAs: indices and values have different length");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_multiply_csr_by_dvec_with_NAs_begin(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, d.ptr, (int64_t)d.n,
                                                      Rf_asInteger(ncols), Rf_asLogical(multiply), Rf_asLogical(powerto),
                                                      Rf_asLogical(divide), Rf_asLogical(divrest), Rf_asLogical(intdiv),
                                                      Rf_asLogical(lhs), res, info); }, Out().aliasing(A.p.s, A.j.s));
}
SEXP _MatrixExtra_logicaland_csr_by_dvec_internal(SEXP p_, SEXP j_, SEXP x_, SEXP dvec, SEXP ncols)
{
    Protect p;
    const Csr<Lgls> A(p_, j_, x_, p);
    const Lgls d(dvec, p);
    return filled<int32_t>(p(Rf_allocVector(LGLSXP, A.x.n)), [&](int32_t *out) {
        return mx_logicaland_csr_by_dvec_internal(A.p.ptr, A.j.ptr, A.x.ptr, A.nrows, d.ptr, (int64_t)d.n,
                                                  Rf_asInteger(ncols), out); });
}

// Device transpose behind the overlay's t_deep_internal (R/trans.R:46-56): the CSR (or CSC) slots of x^T.
// values: a double vector (dg*), a logical vector (lg*) or NULL (ng*); ncol: columns of the CSR view (ncol(x) for
// an RsparseMatrix, nrow(x) for a CsparseMatrix).  Returns list(indptr=, indices=, values=); an empty result keeps
// the values' R type.
SEXP mxgpu_csr_transpose(SEXP p_, SEXP idx, SEXP x_, SEXP ncol)
{
    Protect p;
    const Csr<Vals> A(p_, idx, Vals::by_type(x_, "mxgpu_csr_transpose: values must be double, logical or NULL"), p);
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_csr_transpose_begin(A.p.ptr, A.nrows, Rf_asInteger(ncol), A.j.ptr, A.x.ptr, A.x.dtype, A.x.n, res,
                                      info); }, Out().forcing(A.x.dtype));
}

// COO -> CSR behind the overlay's as.csr.matrix / as.csc.matrix of a general d/l/n TsparseMatrix: i, j 0-based
// (the @i / @j slots), values as for mxgpu_csr_transpose.  Call with (j, i, x, ncol, nrow) for the CSC slots.
// Returns list(indptr=, indices=, values=) with repeated (i, j) merged as Matrix's coercion merges them.
SEXP mxgpu_coo_to_csr(SEXP i_, SEXP j_, SEXP x_, SEXP nrow, SEXP ncol)
{
    Protect p;
    const Ints i(i_, p), j(j_, p);
    same_length(i.n, j.n, "mxgpu_coo_to_csr: row and column indices have different length");
    const Vals x = Vals::by_type(x_, "mxgpu_coo_to_csr: values must be double, logical or NULL");
    if (x.ptr) same_length(x.n, i.n, "mxgpu_coo_to_csr: values and indices have different length");
    return result([&](mx_result **res, mx_result_info *info) {
        return mx_coo_to_csr_begin(i.ptr, j.ptr, x.ptr, x.dtype, (int64_t)i.n, Rf_asInteger(nrow), Rf_asInteger(ncol),
                                   res, info); }, Out().forcing(x.dtype));
}

SEXP _MatrixExtra_multiply_csr_by_coo_elemwise(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yj, SEXP yx, SEXP mr, SEXP mc)
{ return csr_by_coo(0, p_, j_, x_, yi, yj, yx, mr, mc); }
SEXP _MatrixExtra_logicaland_csr_by_coo_elemwise(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yj, SEXP yx, SEXP mr, SEXP mc)
{ return csr_by_coo(1, p_, j_, x_, yi, yj, yx, mr, mc); }

// values-only COO (op) vector  (src/operators.cpp:3363-3418; 12 and 6 arguments)
SEXP _MatrixExtra_multiply_coo_by_dense_ignore_NAs_numeric(SEXP ii_, SEXP jj_, SEXP xx_, SEXP dvec, SEXP nrows,
                                                           SEXP ncols, SEXP multiply, SEXP powerto, SEXP divide,
                                                           SEXP divrest, SEXP intdiv, SEXP lhs)
{
    Protect p;
    const Ints ii(ii_, p), jj(jj_, p);
    const Reals xx(xx_, p), d(dvec, p);
    return filled<double>(p(Rf_allocVector(REALSXP, xx.n)), [&](double *out) {
        return mx_multiply_coo_by_dense_ignore_NAs_numeric(ii.ptr, jj.ptr, xx.ptr, (int64_t)xx.n, d.ptr, (int64_t)d.n,
                                                           Rf_asInteger(nrows), Rf_asInteger(ncols),
                                                           Rf_asLogical(multiply), Rf_asLogical(powerto),
                                                           Rf_asLogical(divide), Rf_asLogical(divrest),
                                                           Rf_asLogical(intdiv), Rf_asLogical(lhs), out); });
}
SEXP _MatrixExtra_multiply_coo_by_dense_ignore_NAs_logical(SEXP ii_, SEXP jj_, SEXP xx_, SEXP dvec, SEXP nrows,
                                                           SEXP ncols)
{
    Protect p;
    const Ints ii(ii_, p), jj(jj_, p);
    const Lgls xx(xx_, p), d(dvec, p);
    return filled<int32_t>(p(Rf_allocVector(LGLSXP, xx.n)), [&](int32_t *out) {
        return mx_multiply_coo_by_dense_ignore_NAs_logical(ii.ptr, jj.ptr, xx.ptr, (int64_t)xx.n, d.ptr, (int64_t)d.n,
                                                           Rf_asInteger(nrows), Rf_asInteger(ncols), out); });
}

SEXP _MatrixExtra_slice_coo_single_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{ return slice_coo_single(MX_F64, ii, jj, xx, i, j); }
SEXP _MatrixExtra_slice_coo_single_logical(SEXP ii, SEXP jj, SEXP xx, SEXP i, SEXP j)
{ return slice_coo_single(MX_LGL, ii, jj, xx, i, j); }
SEXP _MatrixExtra_slice_coo_single_binary(SEXP ii, SEXP jj, SEXP i, SEXP j)
{ return slice_coo_single(MX_NONE, ii, jj, R_NilValue, i, j); }
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

SEXP _MatrixExtra_remove_zero_valued_csr_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP na_rm)
{ return rz_csr<Reals>(p_, j_, x_, na_rm, mx_remove_zero_valued_csr_numeric); }
SEXP _MatrixExtra_remove_zero_valued_csr_logical(SEXP p_, SEXP j_, SEXP x_, SEXP na_rm)
{ return rz_csr<Lgls>(p_, j_, x_, na_rm, mx_remove_zero_valued_csr_logical); }
SEXP _MatrixExtra_remove_zero_valued_coo_numeric(SEXP ii, SEXP jj, SEXP xx, SEXP na_rm)
{ return rz_coo<Reals>(ii, jj, xx, na_rm, mx_remove_zero_valued_coo_numeric); }
SEXP _MatrixExtra_remove_zero_valued_coo_logical(SEXP ii, SEXP jj, SEXP xx, SEXP na_rm)
{ return rz_coo<Lgls>(ii, jj, xx, na_rm, mx_remove_zero_valued_coo_logical); }
SEXP _MatrixExtra_remove_zero_valued_svec_numeric(SEXP ii, SEXP xx, SEXP na_rm)
{ return rz_svec<Reals>(ii, xx, na_rm, mx_remove_zero_valued_svec_numeric); }
SEXP _MatrixExtra_remove_zero_valued_svec_integer(SEXP ii, SEXP xx, SEXP na_rm)
{ return rz_svec<Ints>(ii, xx, na_rm, mx_remove_zero_valued_svec_integer); }
SEXP _MatrixExtra_remove_zero_valued_svec_logical(SEXP ii, SEXP xx, SEXP na_rm)
{ return rz_svec<Lgls>(ii, xx, na_rm, mx_remove_zero_valued_svec_logical); }

SEXP _MatrixExtra_check_valid_csr_matrix(SEXP p_, SEXP j_, SEXP nrows, SEXP ncols)
{
    Protect p;
    const Ints P(p_, p), J(j_, p);
    const char *err = nullptr;
    if (mx_check_valid_csr_matrix(P.ptr, (int64_t)P.n, J.ptr, (int64_t)J.n, Rf_asInteger(nrows), Rf_asInteger(ncols), &err))
        fail();
    return err_list(err);
}
SEXP _MatrixExtra_check_valid_coo_matrix(SEXP ii_, SEXP jj_, SEXP nrows, SEXP ncols)
{
    Protect p;
    const Ints ii(ii_, p), jj(jj_, p);
    same_length(ii.n, jj.n, "check_valid_coo_matrix: row and column indices have different length");
    const char *err = nullptr;
    if (mx_check_valid_coo_matrix(ii.ptr, jj.ptr, (int64_t)ii.n, Rf_asInteger(nrows), Rf_asInteger(ncols), &err)) fail();
    return err_list(err);
}
SEXP _MatrixExtra_check_valid_svec(SEXP ii_, SEXP nrows)
{
    Protect p;
    const Ints ii(ii_, p);
    const char *err = nullptr;
    if (mx_check_valid_svec(ii.ptr, (int64_t)ii.n, Rf_asInteger(nrows), &err)) fail();
    return err_list(err);
}
SEXP _MatrixExtra_rebuild_indptr_after_filter(SEXP p_, SEXP filter_)
{
    Protect p;
    const Ints P(p_, p);
    const Lgls filter(filter_, p);
    return filled<int32_t>(p(Rf_allocVector(INTSXP, P.n)), [&](int32_t *out) {
        return mx_rebuild_indptr_after_filter(P.ptr, (int64_t)P.n, filter.ptr, out); });
}

SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_numeric(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_ignore<Reals, Reals>(p_, i_, x_, d, mx_multiply_csc_by_dense_ignore_NAs_numeric); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_float32(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_ignore<Reals, F32s>(p_, i_, x_, d, mx_multiply_csc_by_dense_ignore_NAs_float32); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_integer(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_ignore<Reals, Ints>(p_, i_, x_, d, mx_multiply_csc_by_dense_ignore_NAs_integer); }
SEXP _MatrixExtra_multiply_csc_by_dense_ignore_NAs_logical(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_ignore<Reals, Lgls>(p_, i_, x_, d, mx_multiply_csc_by_dense_ignore_NAs_logical); }
SEXP _MatrixExtra_logicaland_csc_by_dense_ignore_NAs(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_ignore<Lgls, Lgls>(p_, i_, x_, d, mx_logicaland_csc_by_dense_ignore_NAs); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_numeric(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_keep<Reals>(p_, i_, x_, d, mx_multiply_csc_by_dense_keep_NAs_numeric); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_integer(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_keep<Ints>(p_, i_, x_, d, mx_multiply_csc_by_dense_keep_NAs_integer); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_logical(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_keep<Lgls>(p_, i_, x_, d, mx_multiply_csc_by_dense_keep_NAs_logical); }
SEXP _MatrixExtra_multiply_csc_by_dense_keep_NAs_float32(SEXP p_, SEXP i_, SEXP x_, SEXP d)
{ return csc_dense_keep<F32s>(p_, i_, x_, d, mx_multiply_csc_by_dense_keep_NAs_float32); }

SEXP _MatrixExtra_multiply_csr_by_svec_no_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP ii, SEXP xx, SEXP length)
{ return csr_by_svec(0, p_, j_, x_, ii, xx, 0, length); }
SEXP _MatrixExtra_multiply_csr_by_svec_keep_NAs(SEXP p_, SEXP j_, SEXP x_, SEXP ii, SEXP xx, SEXP ncols, SEXP length)
{ return csr_by_svec(1, p_, j_, x_, ii, xx, Rf_asInteger(ncols), length); }

SEXP _MatrixExtra_matmul_colvec_by_scolvecascsr(SEXP v, SEXP p_, SEXP j_, SEXP x_) { return outer_dense(MX_F64, v, p_, j_, x_); }
SEXP _MatrixExtra_matmul_colvec_by_scolvecascsr_f32(SEXP v, SEXP p_, SEXP j_, SEXP x_) { return outer_dense(MX_F32, v, p_, j_, x_); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_numeric(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_F64, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_integer(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_I32, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_logical(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP yx, SEXP n)
{ return outer_svec(MX_LGL, p_, j_, x_, yi, yx, n); }
SEXP _MatrixExtra_matmul_spcolvec_by_scolvecascsr_binary(SEXP p_, SEXP j_, SEXP x_, SEXP yi, SEXP n)
{ return outer_svec(MX_NONE, p_, j_, x_, yi, R_NilValue, n); }
SEXP _MatrixExtra_matmul_rowvec_by_csc(SEXP v, SEXP p_, SEXP i_, SEXP x_) { return rowvec_csc(v, p_, i_, x_); }
SEXP _MatrixExtra_matmul_rowvec_by_cscbin(SEXP v, SEXP p_, SEXP i_) { return rowvec_csc(v, p_, i_, R_NilValue); }

SEXP _MatrixExtra_sort_vector_indices_numeric(SEXP ii, SEXP xx) { return sort_svec(ii, xx, MX_F64); }
SEXP _MatrixExtra_sort_vector_indices_integer(SEXP ii, SEXP xx) { return sort_svec(ii, xx, MX_I32); }
SEXP _MatrixExtra_sort_vector_indices_logical(SEXP ii, SEXP xx) { return sort_svec(ii, xx, MX_LGL); }
SEXP _MatrixExtra_sort_vector_indices_binary(SEXP ii) { return sort_svec(ii, R_NilValue, MX_NONE); }
SEXP _MatrixExtra_sort_coo_indices_numeric(SEXP ii, SEXP jj, SEXP xx) { return sort_coo(ii, jj, xx, MX_F64); }
SEXP _MatrixExtra_sort_coo_indices_logical(SEXP ii, SEXP jj, SEXP xx) { return sort_coo(ii, jj, xx, MX_LGL); }
SEXP _MatrixExtra_sort_coo_indices_binary(SEXP ii, SEXP jj) { return sort_coo(ii, jj, R_NilValue, MX_NONE); }

SEXP _MatrixExtra_set_single_row_to_zero(SEXP p, SEXP j, SEXP x, SEXP row)
{ return assign_scalar(p, j, x, NCOL_UNKNOWN, sel_one(row), sel_all(), 0.0); }
SEXP _MatrixExtra_set_single_col_to_zero(SEXP p, SEXP j, SEXP x, SEXP col)
{ return assign_scalar(p, j, x, NCOL_UNKNOWN, sel_all(), sel_one(col), 0.0); }
SEXP _MatrixExtra_set_single_row_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP row, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_all(), Rf_asReal(val)); }
SEXP _MatrixExtra_set_single_col_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP col, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_one(col), Rf_asReal(val)); }
SEXP _MatrixExtra_set_single_val_to_zero(SEXP p, SEXP j, SEXP x, SEXP row, SEXP col)
{ return assign_scalar(p, j, x, NCOL_UNKNOWN, sel_one(row), sel_one(col), 0.0); }
SEXP _MatrixExtra_set_single_val_to_const(SEXP p, SEXP j, SEXP x, SEXP ncols, SEXP row, SEXP col, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_one(row), sel_one(col), Rf_asReal(val)); }
SEXP _MatrixExtra_set_rowseq_to_zero(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end)
{ return assign_scalar(p, j, x, NCOL_UNKNOWN, sel_seq(st, end), sel_all(), 0.0); }
SEXP _MatrixExtra_set_rowseq_to_const(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_seq(st, end), sel_all(), Rf_asReal(val)); }
SEXP _MatrixExtra_set_colseq_to_zero(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_seq(st, end), 0.0); }
SEXP _MatrixExtra_set_colseq_to_const(SEXP p, SEXP j, SEXP x, SEXP st, SEXP end, SEXP ncols, SEXP val)
{ return assign_scalar(p, j, x, Rf_asInteger(ncols), sel_all(), sel_seq(st, end), Rf_asReal(val)); }
SEXP _MatrixExtra_set_arbitrary_rows_to_zero(SEXP p, SEXP j, SEXP x, SEXP rows)
{ return assign_scalar(p, j, x, NCOL_UNKNOWN, sel_set(rows), sel_all(), 0.0); }
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

// standalone use: dyn.load("mxgpu_r.so") registers the routines under their reference names
void R_init_mxgpu_r(DllInfo *dll)
{
    R_registerRoutines(dll, NULL, mxgpu_call_entries, NULL, NULL);
    R_useDynamicSymbols(dll, FALSE);
}

}  // extern "C"
#endif  // MXGPU_HAVE_R

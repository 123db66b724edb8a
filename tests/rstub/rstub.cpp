// rstub.cpp: a stand-in for the part of R's C API that matrixextra_amd/csrc/r_shim.cpp uses, written from R's
// documented behaviour ("Writing R Extensions", R's coercion rules), so that the shim can be compiled and run where
// no R is installed.  Test infrastructure only; it is not R and it does not evaluate R code.
//
// What it adds to the API is observation.  Every object stays allocated until rstub_reset(), so misuse is counted and
// is not undefined behaviour:
//   * the protect stack: its depth, an UNPROTECT below the depth at entry of the call, a depth left changed at return;
//   * the precious list (R_PreserveObject / R_ReleaseObject);
//   * torture mode, as gctorture(TRUE): inside rstub_call() every allocation first marks what is reachable from the
//     protect stack, the precious list and the objects the caller owns (everything made outside a call, so the call's
//     arguments, with their elements and attributes) and poisons every other object: its data is filled with 0xDF and
//     it is flagged dead.  An accessor used on a dead object, or a dead object returned, is logged;
//   * accessor type checks (INTEGER() of a double vector ...; stricter than R in one place: INTEGER() of a logical
//     vector, which R allows, is logged too, since the shim means LOGICAL() there), and a guard band behind every
//     vector's data, checked when the call returns;
//   * allocation failure on request: rstub_fail_allocation(n) makes the nth allocation of the next call long-jump as
//     R's allocVector does when memory is out, so the paths that guard a resource against it can be walked;
//   * a violation log, read with rstub_violations().
// Rf_error formats its message, runs the pending R_ExecWithCleanup cleanups innermost first (each once), resets the
// protect stack to its depth at entry and long-jumps to rstub_call(), which returns 1.
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>

#include <csetjmp>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct SEXPREC {
    int type;
    int dead;
    int mark;
    int pinned;            // owned by the caller of rstub_call (R code holding it in a variable)
    R_xlen_t length;
    unsigned char *data;   // length * element size bytes, then GUARD bytes of 0xC5
    SEXP names, dim;
};

namespace {

constexpr size_t GUARD = 32;
constexpr unsigned char GUARD_BYTE = 0xC5, POISON_BYTE = 0xDF, FRESH_BYTE = 0xAB;

struct Cleanup { void (*fun)(void *); void *data; };
struct Frame { jmp_buf jb; size_t protect_entry, cleanup_entry; };

std::vector<SEXP> g_all, g_protect, g_precious, g_temp;
std::vector<Cleanup> g_cleanups;
Frame *g_frame = nullptr;
bool g_torture = false;
int g_fail_alloc = 0;          // > 0: that allocation of the current call fails, as R's allocVector does when memory is out
int g_allocations = 0;         // allocations since the call began
int g_nviolations = 0;
std::string g_log;
char g_errmsg[4096];
std::vector<R_CallMethodDef> g_registered;
int g_dynamic_symbols = -1;

void violation(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ++g_nviolations;
    g_log += buf;
    g_log += '\n';
}

size_t elem_size(int type)
{
    switch (type) {
        case LGLSXP: case INTSXP: return sizeof(int);
        case REALSXP: return sizeof(double);
        case STRSXP: case VECSXP: return sizeof(SEXP);
        case CHARSXP: return 1;
        default: return 0;
    }
}

const char *type_name(int type)
{
    switch (type) {
        case NILSXP: return "NULL";
        case SYMSXP: return "symbol";
        case CHARSXP: return "char";
        case LGLSXP: return "logical";
        case INTSXP: return "integer";
        case REALSXP: return "double";
        case STRSXP: return "character";
        case VECSXP: return "list";
        default: return "?";
    }
}

SEXP raw_new(int type, R_xlen_t n)
{
    SEXP s = new SEXPREC;
    s->type = type;
    s->dead = s->mark = 0;
    s->pinned = g_frame == nullptr;
    s->length = n;
    const size_t bytes = (size_t)n * elem_size(type) + (type == CHARSXP ? 1 : 0);
    s->data = static_cast<unsigned char *>(malloc(bytes + GUARD));
    if (!s->data) abort();
    memset(s->data, FRESH_BYTE, bytes);
    memset(s->data + bytes, GUARD_BYTE, GUARD);
    s->names = s->dim = nullptr;
    g_all.push_back(s);
    return s;
}

size_t data_bytes(SEXP s) { return (size_t)s->length * elem_size(s->type) + (s->type == CHARSXP ? 1 : 0); }

void mark(SEXP s)
{
    if (!s || s->mark) return;
    s->mark = 1;
    mark(s->names);
    mark(s->dim);
    if (!s->dead && (s->type == VECSXP || s->type == STRSXP)) {
        SEXP *e = reinterpret_cast<SEXP *>(s->data);
        for (R_xlen_t i = 0; i < s->length; ++i) mark(e[i]);
    }
}

// gctorture: whatever no root reaches is gone before the allocation returns
void torture()
{
    if (!g_torture || !g_frame) return;
    for (SEXP s : g_all) s->mark = 0;
    for (SEXP s : g_all) if (s->pinned) mark(s);
    for (SEXP s : g_protect) mark(s);
    for (SEXP s : g_precious) mark(s);
    for (SEXP s : g_temp) mark(s);
    for (SEXP s : g_all)
        if (!s->mark && !s->dead) {
            s->dead = 1;
            memset(s->data, POISON_BYTE, data_bytes(s));
        }
}

SEXP alloc(int type, R_xlen_t n)
{
    if (g_frame) {
        ++g_allocations;
        if (g_fail_alloc > 0 && --g_fail_alloc == 0) Rf_error("cannot allocate vector of length %ld", (long)n);
    }
    torture();
    return raw_new(type, n);
}

struct TempRoot {          // what R's own functions PROTECT while they allocate
    explicit TempRoot(SEXP s) { g_temp.push_back(s); }
    ~TempRoot() { g_temp.pop_back(); }
};

bool alive(SEXP s, const char *who)
{
    if (!s) { violation("%s of a null pointer", who); return false; }
    if (s->dead) { violation("%s of a dead (collected) %s vector of length %ld", who, type_name(s->type), (long)s->length); return false; }
    return true;
}

void check_guards()
{
    for (SEXP s : g_all) {
        const unsigned char *g = s->data + data_bytes(s);
        for (size_t k = 0; k < GUARD; ++k)
            if (g[k] != GUARD_BYTE) {
                violation("write past the end of a %s vector of length %ld (byte %zu behind it)", type_name(s->type),
                          (long)s->length, k);
                memset(s->data + data_bytes(s), GUARD_BYTE, GUARD);
                break;
            }
    }
}

SEXP make_symbol() { SEXP s = raw_new(SYMSXP, 0); s->pinned = 1; return s; }

int int_from_real(double x)
{
    if (x != x || x >= 2147483648.0 || x <= -2147483649.0) return NA_INTEGER;      // R warns and gives NA
    const int v = (int)x;                                                             // truncation toward zero
    return v;
}
double na_real()
{
    const uint64_t bits = 0x7FF00000000007A2ull;
    double d;
    memcpy(&d, &bits, sizeof d);
    return d;
}

}  // namespace

extern "C" {

SEXP R_NilValue = raw_new(NILSXP, 0);
SEXP R_NamesSymbol = make_symbol();
SEXP R_DimSymbol = make_symbol();
double R_NaReal = na_real();

// ---- accessors -------------------------------------------------------------------------------------------------------
int TYPEOF(SEXP x) { alive(x, "TYPEOF"); return x ? x->type : NILSXP; }
R_xlen_t XLENGTH(SEXP x) { alive(x, "XLENGTH"); return x ? x->length : 0; }
int LENGTH(SEXP x) { alive(x, "LENGTH"); return x ? (int)x->length : 0; }
int *INTEGER(SEXP x)
{
    alive(x, "INTEGER()");
    if (x->type != INTSXP) violation("INTEGER() of a %s vector", type_name(x->type));
    return reinterpret_cast<int *>(x->data);
}
int *LOGICAL(SEXP x)
{
    alive(x, "LOGICAL()");
    if (x->type != LGLSXP) violation("LOGICAL() of a %s vector", type_name(x->type));
    return reinterpret_cast<int *>(x->data);
}
double *REAL(SEXP x)
{
    alive(x, "REAL()");
    if (x->type != REALSXP) violation("REAL() of a %s vector", type_name(x->type));
    return reinterpret_cast<double *>(x->data);
}
SEXP VECTOR_ELT(SEXP x, R_xlen_t i)
{
    if (!alive(x, "VECTOR_ELT")) return R_NilValue;
    if (x->type != VECSXP || i < 0 || i >= x->length) { violation("VECTOR_ELT(%s, %ld) out of range", type_name(x->type), (long)i); return R_NilValue; }
    return reinterpret_cast<SEXP *>(x->data)[i];
}
SEXP SET_VECTOR_ELT(SEXP x, R_xlen_t i, SEXP v)
{
    if (!alive(x, "SET_VECTOR_ELT")) return v;
    alive(v, "SET_VECTOR_ELT value");
    if (x->type != VECSXP || i < 0 || i >= x->length) { violation("SET_VECTOR_ELT(%s, %ld) out of range", type_name(x->type), (long)i); return v; }
    reinterpret_cast<SEXP *>(x->data)[i] = v;
    return v;
}
SEXP STRING_ELT(SEXP x, R_xlen_t i)
{
    if (!alive(x, "STRING_ELT")) return R_NilValue;
    if (x->type != STRSXP || i < 0 || i >= x->length) { violation("STRING_ELT(%s, %ld) out of range", type_name(x->type), (long)i); return R_NilValue; }
    return reinterpret_cast<SEXP *>(x->data)[i];
}
void SET_STRING_ELT(SEXP x, R_xlen_t i, SEXP v)
{
    if (!alive(x, "SET_STRING_ELT")) return;
    alive(v, "SET_STRING_ELT value");
    if (x->type != STRSXP || i < 0 || i >= x->length) { violation("SET_STRING_ELT(%s, %ld) out of range", type_name(x->type), (long)i); return; }
    if (v->type != CHARSXP) { violation("SET_STRING_ELT with a %s value", type_name(v->type)); return; }
    reinterpret_cast<SEXP *>(x->data)[i] = v;
}
const char *R_CHAR(SEXP x)
{
    if (!alive(x, "CHAR") || x->type != CHARSXP) return "";
    return reinterpret_cast<const char *>(x->data);
}

// ---- protection ------------------------------------------------------------------------------------------------------
SEXP Rf_protect(SEXP s)
{
    alive(s, "PROTECT");
    g_protect.push_back(s);
    return s;
}
void Rf_unprotect(int n)
{
    const size_t floor = g_frame ? g_frame->protect_entry : 0;
    const size_t mine = g_protect.size() > floor ? g_protect.size() - floor : 0;
    if (n < 0 || (size_t)n > mine) {
        violation("UNPROTECT(%d) with %zu protected since the call began: stack imbalance", n, mine);
        g_protect.resize(g_protect.size() - mine);
        return;
    }
    g_protect.resize(g_protect.size() - (size_t)n);
}
void R_PreserveObject(SEXP s)
{
    alive(s, "R_PreserveObject");
    g_precious.push_back(s);
}
void R_ReleaseObject(SEXP s)
{
    for (size_t k = g_precious.size(); k-- > 0;)
        if (g_precious[k] == s) { g_precious.erase(g_precious.begin() + (long)k); return; }
    violation("R_ReleaseObject of an object that is not on the precious list");
}

// ---- allocation ------------------------------------------------------------------------------------------------------
SEXP Rf_allocVector(SEXPTYPE type, R_xlen_t n)
{
    if (n < 0) Rf_error("negative length vectors are not allowed");
    if (type != LGLSXP && type != INTSXP && type != REALSXP && type != STRSXP && type != VECSXP)
        Rf_error("allocVector: type %u is not implemented in the stand-in", type);
    SEXP s = alloc((int)type, n);
    if (type == VECSXP || type == STRSXP) {
        SEXP *e = reinterpret_cast<SEXP *>(s->data);
        SEXP fill = R_NilValue;
        for (R_xlen_t i = 0; i < n; ++i) e[i] = fill;
        if (type == STRSXP) {
            TempRoot keep(s);
            fill = Rf_mkChar("");
        }
        for (R_xlen_t i = 0; i < n; ++i) e[i] = fill;
    }
    return s;
}
SEXP Rf_allocMatrix(SEXPTYPE type, int nrow, int ncol)
{
    if (nrow < 0 || ncol < 0) Rf_error("negative extents to matrix");
    SEXP s = Rf_allocVector(type, (R_xlen_t)nrow * ncol);
    TempRoot keep(s);
    SEXP dim = Rf_allocVector(INTSXP, 2);
    INTEGER(dim)[0] = nrow;
    INTEGER(dim)[1] = ncol;
    s->dim = dim;
    return s;
}
SEXP Rf_mkChar(const char *str)
{
    const size_t n = strlen(str);
    SEXP s = alloc(CHARSXP, (R_xlen_t)n);
    memcpy(s->data, str, n + 1);
    return s;
}
SEXP Rf_mkString(const char *str)
{
    SEXP s = Rf_allocVector(STRSXP, 1);
    TempRoot keep(s);
    SET_STRING_ELT(s, 0, Rf_mkChar(str));
    return s;
}
SEXP Rf_ScalarLogical(int v)
{
    SEXP s = Rf_allocVector(LGLSXP, 1);
    LOGICAL(s)[0] = v == NA_LOGICAL ? NA_LOGICAL : (v != 0);
    return s;
}
SEXP Rf_ScalarInteger(int v)
{
    SEXP s = Rf_allocVector(INTSXP, 1);
    INTEGER(s)[0] = v;
    return s;
}
SEXP Rf_ScalarReal(double v)
{
    SEXP s = Rf_allocVector(REALSXP, 1);
    REAL(s)[0] = v;
    return s;
}

// ---- coercion (R's IntegerFromReal, LogicalFromInteger, ... of coerce.c) --------------------------------------------------
SEXP Rf_coerceVector(SEXP x, SEXPTYPE type)
{
    if (!alive(x, "coerceVector")) return R_NilValue;
    if ((SEXPTYPE)x->type == type) return x;
    if (type != LGLSXP && type != INTSXP && type != REALSXP)
        Rf_error("coerceVector: target type %u is not implemented in the stand-in", type);
    if (x->type == NILSXP) return Rf_allocVector(type, 0);
    if (x->type != LGLSXP && x->type != INTSXP && x->type != REALSXP)
        Rf_error("cannot coerce type '%s' to vector of type '%s'", type_name(x->type), type_name((int)type));
    TempRoot keep(x);
    SEXP out = Rf_allocVector(type, x->length);
    out->dim = x->dim;
    out->names = x->names;
    const int *xi = reinterpret_cast<const int *>(x->data);
    const double *xd = reinterpret_cast<const double *>(x->data);
    int *oi = reinterpret_cast<int *>(out->data);
    double *od = reinterpret_cast<double *>(out->data);
    for (R_xlen_t k = 0; k < x->length; ++k) {
        if (x->type == REALSXP) {
            if (type == INTSXP) oi[k] = int_from_real(xd[k]);
            else oi[k] = xd[k] != xd[k] ? NA_LOGICAL : (xd[k] != 0);
        } else if (type == REALSXP) {
            od[k] = xi[k] == NA_INTEGER ? NA_REAL : (double)xi[k];
        } else if (type == LGLSXP) {
            oi[k] = xi[k] == NA_INTEGER ? NA_LOGICAL : (xi[k] != 0);
        } else {
            oi[k] = xi[k];                                  // logical -> integer
        }
    }
    return out;
}
int Rf_asInteger(SEXP x)
{
    if (!alive(x, "asInteger") || x->length < 1) return NA_INTEGER;
    if (x->type == INTSXP || x->type == LGLSXP) return reinterpret_cast<const int *>(x->data)[0];
    if (x->type == REALSXP) return int_from_real(reinterpret_cast<const double *>(x->data)[0]);
    return NA_INTEGER;
}
int Rf_asLogical(SEXP x)
{
    if (!alive(x, "asLogical") || x->length < 1) return NA_LOGICAL;
    if (x->type == INTSXP || x->type == LGLSXP) {
        const int v = reinterpret_cast<const int *>(x->data)[0];
        return v == NA_INTEGER ? NA_LOGICAL : (v != 0);
    }
    if (x->type == REALSXP) {
        const double v = reinterpret_cast<const double *>(x->data)[0];
        return v != v ? NA_LOGICAL : (v != 0);
    }
    return NA_LOGICAL;
}
double Rf_asReal(SEXP x)
{
    if (!alive(x, "asReal") || x->length < 1) return NA_REAL;
    if (x->type == INTSXP || x->type == LGLSXP) {
        const int v = reinterpret_cast<const int *>(x->data)[0];
        return v == NA_INTEGER ? NA_REAL : (double)v;
    }
    if (x->type == REALSXP) return reinterpret_cast<const double *>(x->data)[0];
    return NA_REAL;
}

// ---- attributes ------------------------------------------------------------------------------------------------------
int Rf_nrows(SEXP x)
{
    if (!alive(x, "nrows")) return 0;
    if (!x->dim) return (int)x->length;
    return reinterpret_cast<const int *>(x->dim->data)[0];
}
int Rf_ncols(SEXP x)
{
    if (!alive(x, "ncols")) return 0;
    if (!x->dim || x->dim->length < 2) return 1;
    return reinterpret_cast<const int *>(x->dim->data)[1];
}
SEXP Rf_setAttrib(SEXP x, SEXP name, SEXP value)
{
    if (!alive(x, "setAttrib")) return value;
    alive(value, "setAttrib value");
    if (name == R_NamesSymbol) {
        if (value != R_NilValue && (value->type != STRSXP || value->length != x->length))
            violation("names attribute: a %s vector of length %ld for an object of length %ld", type_name(value->type),
                      (long)value->length, (long)x->length);
        x->names = value == R_NilValue ? nullptr : value;
    } else if (name == R_DimSymbol) {
        x->dim = value == R_NilValue ? nullptr : value;
    } else {
        violation("setAttrib: only names and dim exist in the stand-in");
    }
    return value;
}
SEXP Rf_getAttrib(SEXP x, SEXP name)
{
    if (!alive(x, "getAttrib")) return R_NilValue;
    SEXP a = name == R_NamesSymbol ? x->names : name == R_DimSymbol ? x->dim : nullptr;
    return a ? a : R_NilValue;
}

// ---- conditions ------------------------------------------------------------------------------------------------------
SEXP R_ExecWithCleanup(SEXP (*fun)(void *), void *data, void (*cleanfun)(void *), void *cleandata)
{
    g_cleanups.push_back(Cleanup{cleanfun, cleandata});
    SEXP result = fun(data);
    g_cleanups.pop_back();
    cleanfun(cleandata);
    return result;
}
void Rf_error(const char *fmt, ...)
{
    g_fail_alloc = 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_errmsg, sizeof g_errmsg, fmt, ap);
    va_end(ap);
    if (!g_frame) {
        fprintf(stderr, "rstub: Rf_error outside rstub_call: %s\n", g_errmsg);
        abort();
    }
    while (g_cleanups.size() > g_frame->cleanup_entry) {
        const Cleanup c = g_cleanups.back();
        g_cleanups.pop_back();
        c.fun(c.data);
    }
    if (g_protect.size() > g_frame->protect_entry) g_protect.resize(g_frame->protect_entry);
    g_temp.clear();
    longjmp(g_frame->jb, 1);
}

// ---- registration ------------------------------------------------------------------------------------------------------
int R_registerRoutines(DllInfo *, const R_CMethodDef *const, const R_CallMethodDef *const callRoutines,
                       const R_FortranMethodDef *const, const R_ExternalMethodDef *const)
{
    g_registered.clear();
    for (const R_CallMethodDef *e = callRoutines; e && e->name; ++e) g_registered.push_back(*e);
    return 1;
}
Rboolean R_useDynamicSymbols(DllInfo *, Rboolean value)
{
    const int old = g_dynamic_symbols;
    g_dynamic_symbols = (int)value;
    return old == 0 ? FALSE : TRUE;
}

// ==== the interface of the tests (ctypes) ===============================================================================
SEXP rstub_nil(void) { return R_NilValue; }
SEXP rstub_new(int type, long n)
{
    SEXP s = type == NILSXP ? R_NilValue : Rf_allocVector((SEXPTYPE)type, (R_xlen_t)n);
    if (type == LGLSXP || type == INTSXP || type == REALSXP) memset(s->data, 0, data_bytes(s));
    return s;
}
SEXP rstub_new_string(const char *str) { return Rf_mkString(str); }
void *rstub_data(SEXP s) { return s->data; }
long rstub_len(SEXP s) { return (long)s->length; }
int rstub_type(SEXP s) { return s->type; }
int rstub_dead(SEXP s) { return s->dead; }
void rstub_set_dim(SEXP s, int nrow, int ncol)
{
    SEXP dim = Rf_allocVector(INTSXP, 2);
    INTEGER(dim)[0] = nrow;
    INTEGER(dim)[1] = ncol;
    s->dim = dim;
}
int rstub_dim(SEXP s, int *nrow, int *ncol)
{
    if (!s->dim || s->dim->length != 2) return 0;
    *nrow = reinterpret_cast<const int *>(s->dim->data)[0];
    *ncol = reinterpret_cast<const int *>(s->dim->data)[1];
    return 1;
}
// name i of x, or NULL when x has no names attribute (or i is out of range)
const char *rstub_names(SEXP s, long i)
{
    if (!s->names || s->names->dead || i < 0 || i >= s->names->length) return nullptr;
    SEXP c = reinterpret_cast<SEXP *>(s->names->data)[i];
    return c && !c->dead && c->type == CHARSXP ? reinterpret_cast<const char *>(c->data) : nullptr;
}
SEXP rstub_elt(SEXP s, long i)
{
    if (s->type != VECSXP || s->dead || i < 0 || i >= s->length) return nullptr;
    return reinterpret_cast<SEXP *>(s->data)[i];
}
const char *rstub_string(SEXP s, long i)
{
    if (s->type != STRSXP || s->dead || i < 0 || i >= s->length) return nullptr;
    SEXP c = reinterpret_cast<SEXP *>(s->data)[i];
    return c && !c->dead ? reinterpret_cast<const char *>(c->data) : nullptr;
}

typedef SEXP (*F0)(void);
typedef SEXP (*F1)(SEXP);
typedef SEXP (*F2)(SEXP, SEXP);
typedef SEXP (*F3)(SEXP, SEXP, SEXP);
typedef SEXP (*F4)(SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F5)(SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F6)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F7)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F8)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F9)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F10)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F11)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F12)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*F13)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);

static SEXP dispatch(void *fn, int n, SEXP *a)
{
    switch (n) {
        case 0: return reinterpret_cast<F0>(fn)();
        case 1: return reinterpret_cast<F1>(fn)(a[0]);
        case 2: return reinterpret_cast<F2>(fn)(a[0], a[1]);
        case 3: return reinterpret_cast<F3>(fn)(a[0], a[1], a[2]);
        case 4: return reinterpret_cast<F4>(fn)(a[0], a[1], a[2], a[3]);
        case 5: return reinterpret_cast<F5>(fn)(a[0], a[1], a[2], a[3], a[4]);
        case 6: return reinterpret_cast<F6>(fn)(a[0], a[1], a[2], a[3], a[4], a[5]);
        case 7: return reinterpret_cast<F7>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
        case 8: return reinterpret_cast<F8>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
        case 9: return reinterpret_cast<F9>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
        case 10: return reinterpret_cast<F10>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]);
        case 11: return reinterpret_cast<F11>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]);
        case 12: return reinterpret_cast<F12>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11]);
        case 13: return reinterpret_cast<F13>(fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12]);
        default: return nullptr;
    }
}

// .Call(fn, args...): 0 and *out = the result, or 1 after Rf_error (message: rstub_error_message()), or 2 for an
// arity the trampoline does not have.  The result belongs to the caller from here on.
int rstub_call(void *fn, int nargs, SEXP *args, SEXP *out)
{
    if (nargs < 0 || nargs > 13 || g_frame) return 2;
    Frame frame;
    frame.protect_entry = g_protect.size();
    frame.cleanup_entry = g_cleanups.size();
    g_frame = &frame;
    g_allocations = 0;
    g_errmsg[0] = 0;
    *out = nullptr;
    volatile int status = 0;
    if (setjmp(frame.jb) == 0) {
        SEXP r = dispatch(fn, nargs, args);
        if (g_protect.size() != frame.protect_entry) {
            violation("the call returned with the protect stack at depth %zu, entered at %zu", g_protect.size(), frame.protect_entry);
            g_protect.resize(frame.protect_entry);
        }
        if (!r) violation("the call returned a null pointer");
        else if (r->dead) violation("the call returned a dead (collected) %s vector", type_name(r->type));
        else if (r->type == VECSXP)
            for (R_xlen_t i = 0; i < r->length; ++i) {
                SEXP e = reinterpret_cast<SEXP *>(r->data)[i];
                if (!e || e->dead) violation("element %ld of the returned list is dead (collected)", (long)i);
            }
        if (r) r->pinned = 1;
        *out = r;
    } else {
        status = 1;
    }
    g_frame = nullptr;
    g_fail_alloc = 0;
    check_guards();
    return status;
}

const char *rstub_error_message(void) { return g_errmsg; }
int rstub_protect_depth(void) { return (int)g_protect.size(); }
int rstub_precious_count(void) { return (int)g_precious.size(); }
// the number of violations so far; buf receives the log, one line each
int rstub_violations(char *buf, int n)
{
    if (buf && n > 0) {
        strncpy(buf, g_log.c_str(), (size_t)n - 1);
        buf[n - 1] = 0;
    }
    return g_nviolations;
}
void rstub_clear_violations(void) { g_nviolations = 0; g_log.clear(); }
void rstub_torture(int on) { g_torture = on != 0; }
// the nth allocation of the next call ends in Rf_error("cannot allocate ..."), as in R when memory is out; 0 = none
void rstub_fail_allocation(int nth) { g_fail_alloc = nth; }
int rstub_allocations(void) { return g_allocations; }
int rstub_object_count(void) { return (int)g_all.size(); }
int rstub_dynamic_symbols(void) { return g_dynamic_symbols; }
int rstub_registered(int i, const char **name, void **fn, int *nargs)
{
    if (i < 0 || (size_t)i >= g_registered.size()) return 0;
    *name = g_registered[(size_t)i].name;
    *fn = reinterpret_cast<void *>(g_registered[(size_t)i].fun);
    *nargs = g_registered[(size_t)i].numArgs;
    return 1;
}
// frees every object but the three singletons and empties the stacks and the log
void rstub_reset(void)
{
    std::vector<SEXP> keep;
    for (SEXP s : g_all) {
        if (s == R_NilValue || s == R_NamesSymbol || s == R_DimSymbol) { keep.push_back(s); continue; }
        free(s->data);
        delete s;
    }
    g_all.swap(keep);
    g_protect.clear();
    g_precious.clear();
    g_temp.clear();
    g_cleanups.clear();
    rstub_clear_violations();
    g_errmsg[0] = 0;
}

// ==== routines that misuse the API on purpose: the self-checks of tests/test_rshim_host.py call them ====================
SEXP rstub_selftest_unprotect_too_many(SEXP x) { UNPROTECT(1); return x; }
SEXP rstub_selftest_leaves_protected(SEXP x) { PROTECT(x); return x; }
SEXP rstub_selftest_unprotected(SEXP)
{
    SEXP a = Rf_allocVector(INTSXP, 4);
    for (int k = 0; k < 4; ++k) INTEGER(a)[k] = k + 1;
    SEXP b = PROTECT(Rf_allocVector(INTSXP, 1));          // under torture `a` is collected here
    INTEGER(b)[0] = INTEGER(a)[0];
    UNPROTECT(1);
    return b;
}
SEXP rstub_selftest_protected(SEXP)
{
    SEXP a = PROTECT(Rf_allocVector(INTSXP, 4));
    for (int k = 0; k < 4; ++k) INTEGER(a)[k] = k + 1;
    SEXP b = PROTECT(Rf_allocVector(INTSXP, 1));
    INTEGER(b)[0] = INTEGER(a)[0];
    UNPROTECT(2);
    return b;
}
SEXP rstub_selftest_returns_collected(SEXP)
{
    SEXP a = Rf_allocVector(INTSXP, 4);
    Rf_allocVector(INTSXP, 1);
    return a;
}
static SEXP selftest_body(void *d)
{
    if (Rf_asLogical(static_cast<SEXP>(d))) Rf_error("boom %d", 7);
    return R_NilValue;
}
static void selftest_cleanup(void *d) { ++INTEGER(static_cast<SEXP>(d))[0]; }
SEXP rstub_selftest_cleanup(SEXP fail, SEXP counter)
{
    PROTECT(counter);
    PROTECT(counter);
    R_ExecWithCleanup(selftest_body, fail, selftest_cleanup, counter);
    UNPROTECT(2);
    return counter;
}
SEXP rstub_selftest_preserves(SEXP x) { R_PreserveObject(x); return x; }
SEXP rstub_selftest_overrun(SEXP x) { INTEGER(x)[XLENGTH(x)] = 1; return x; }
SEXP rstub_selftest_wrong_accessor(SEXP x) { return Rf_ScalarInteger(INTEGER(x)[0]); }

}  // extern "C"

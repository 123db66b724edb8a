/* Rinternals.h of the R stand-in (tests/rstub): the part of R's C API that matrixextra_amd/csrc/r_shim.cpp uses,
 * declared as "Writing R Extensions" documents it.  Test infrastructure: the definitions are in rstub.cpp, which also
 * watches what a caller does with them (protect stack, precious list, dead objects).  Not R, and not for linking
 * anything but the tests. */
#ifndef RSTUB_RINTERNALS_H
#define RSTUB_RINTERNALS_H

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SEXPREC *SEXP;
typedef unsigned int SEXPTYPE;
typedef ptrdiff_t R_xlen_t;
typedef enum { FALSE = 0, TRUE } Rboolean;

#define NILSXP 0
#define SYMSXP 1
#define CHARSXP 9
#define LGLSXP 10
#define INTSXP 13
#define REALSXP 14
#define STRSXP 16
#define VECSXP 19

extern SEXP R_NilValue;
extern SEXP R_NamesSymbol;
extern SEXP R_DimSymbol;
extern double R_NaReal;                 /* 0x7FF00000000007A2 */
#define NA_INTEGER INT_MIN
#define NA_LOGICAL INT_MIN
#define NA_REAL R_NaReal

int TYPEOF(SEXP x);
R_xlen_t XLENGTH(SEXP x);
int LENGTH(SEXP x);
int *INTEGER(SEXP x);
int *LOGICAL(SEXP x);
double *REAL(SEXP x);
SEXP VECTOR_ELT(SEXP x, R_xlen_t i);
SEXP SET_VECTOR_ELT(SEXP x, R_xlen_t i, SEXP v);
SEXP STRING_ELT(SEXP x, R_xlen_t i);
void SET_STRING_ELT(SEXP x, R_xlen_t i, SEXP v);
const char *R_CHAR(SEXP x);
#define CHAR(x) R_CHAR(x)

SEXP Rf_protect(SEXP s);
void Rf_unprotect(int n);
#define PROTECT(s) Rf_protect(s)
#define UNPROTECT(n) Rf_unprotect(n)
void R_PreserveObject(SEXP s);
void R_ReleaseObject(SEXP s);

SEXP Rf_allocVector(SEXPTYPE type, R_xlen_t n);
SEXP Rf_allocMatrix(SEXPTYPE type, int nrow, int ncol);
SEXP Rf_coerceVector(SEXP x, SEXPTYPE type);
int Rf_asInteger(SEXP x);
int Rf_asLogical(SEXP x);
double Rf_asReal(SEXP x);
int Rf_nrows(SEXP x);
int Rf_ncols(SEXP x);
SEXP Rf_mkChar(const char *s);
SEXP Rf_mkString(const char *s);
SEXP Rf_ScalarLogical(int v);
SEXP Rf_ScalarInteger(int v);
SEXP Rf_ScalarReal(double v);
SEXP Rf_setAttrib(SEXP x, SEXP name, SEXP value);
SEXP Rf_getAttrib(SEXP x, SEXP name);

SEXP R_ExecWithCleanup(SEXP (*fun)(void *), void *data, void (*cleanfun)(void *), void *cleandata);
#if defined(__GNUC__)
void Rf_error(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
#else
void Rf_error(const char *fmt, ...);
#endif

#ifdef __cplusplus
}
#endif
#endif /* RSTUB_RINTERNALS_H */

/* Stand-in for R's <Rinternals.h>: SEXP is a pointer to a tagged, reference-counted object (see Rcpp.h). */
#ifndef MXREF_SHIM_RINTERNALS_H
#define MXREF_SHIM_RINTERNALS_H
#include "R.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef ptrdiff_t R_xlen_t;
struct SEXPREC;
typedef struct SEXPREC *SEXP;

enum { NILSXP = 0, LGLSXP = 10, INTSXP = 13, REALSXP = 14, STRSXP = 16, VECSXP = 19, S4SXP = 25 };

int *INTEGER(SEXP x);
int *LOGICAL(SEXP x);
double *REAL(SEXP x);
R_xlen_t Rf_xlength(SEXP x);
int Rf_length(SEXP x);
int TYPEOF(SEXP x);

#ifdef __cplusplus
}
#endif
#endif

/* Stand-in for <Rcpp/unwindProtect.h>: there is no R longjmp to guard against, so f(arg) is called directly. */
#ifndef MXREF_SHIM_UNWINDPROTECT_H
#define MXREF_SHIM_UNWINDPROTECT_H
#include "../Rcpp.h"
namespace Rcpp {
inline SEXP unwindProtect(SEXP (*f)(void *), void *arg) { return f(arg); }
}
#endif

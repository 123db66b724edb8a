/* Stand-in for <R_ext/RS.h>: Fortran name mangling as gfortran does it. */
#ifndef MXREF_SHIM_RS_H
#define MXREF_SHIM_RS_H
#define F77_NAME(x) x##_
#define F77_CALL(x) x##_
#define F77_SUB(x) x##_
#endif

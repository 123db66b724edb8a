/* Stand-in for <R_ext/BLAS.h>: the two level-1 routines the reference calls, as plain strided loops
 * (one multiply and one add per element, in index order; no FMA when built with -ffp-contract=off). */
#ifndef MXREF_SHIM_BLAS_H
#define MXREF_SHIM_BLAS_H
#ifdef __cplusplus
extern "C" {
#endif

static inline void daxpy_(const int *n, const double *alpha, const double *dx, const int *incx, double *dy,
                          const int *incy)
{
    ptrdiff_t ix = (*incx < 0) ? (ptrdiff_t)(1 - *n) * *incx : 0;
    ptrdiff_t iy = (*incy < 0) ? (ptrdiff_t)(1 - *n) * *incy : 0;
    if (*n <= 0 || *alpha == 0.0) return;
    for (int i = 0; i < *n; i++, ix += *incx, iy += *incy)
        dy[iy] = dy[iy] + (*alpha) * dx[ix];
}

static inline void dcopy_(const int *n, const double *dx, const int *incx, double *dy, const int *incy)
{
    ptrdiff_t ix = (*incx < 0) ? (ptrdiff_t)(1 - *n) * *incx : 0;
    ptrdiff_t iy = (*incy < 0) ? (ptrdiff_t)(1 - *n) * *incy : 0;
    for (int i = 0; i < *n; i++, ix += *incx, iy += *incy)
        dy[iy] = dx[ix];
}

#ifdef __cplusplus
}
#endif
#endif

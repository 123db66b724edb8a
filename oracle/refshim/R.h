/* Stand-in for R's <R.h>: the C-level slice of R's API that the reference's hot files use.
 * Written from R's documented behaviour ("Writing R Extensions"); test infrastructure only. */
#ifndef MXREF_SHIM_R_H
#define MXREF_SHIM_R_H
#include <limits.h>
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <math.h>

#ifdef __cplusplus
extern "C" {
#endif

/* NA_integer_ / NA_logical_ are INT_MIN; NA_real_ is a quiet-free NaN pattern whose low word is 1954. */
#define NA_INTEGER INT_MIN
#define NA_LOGICAL INT_MIN

static inline double mxref_bits_to_double(uint64_t u)
{
    double d;
    memcpy(&d, &u, sizeof d);
    return d;
}
#define R_NaReal (mxref_bits_to_double(UINT64_C(0x7FF00000000007A2)))
#define NA_REAL R_NaReal
#define R_NaN (mxref_bits_to_double(UINT64_C(0x7FF8000000000000)))
#define R_PosInf (mxref_bits_to_double(UINT64_C(0x7FF0000000000000)))
#define R_NegInf (mxref_bits_to_double(UINT64_C(0xFFF0000000000000)))

static inline int R_IsNA(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return (x != x) && ((uint32_t)(u & 0xFFFFFFFFu) == 1954u);
}
static inline int R_IsNaN(double x) { return (x != x) && !R_IsNA(x); }
static inline int mxref_isnan(double x) { return x != x; }
static inline int R_finite(double x) { return (x - x) == 0.0; }

#define ISNA(x) R_IsNA(x)
#define ISNAN(x) mxref_isnan(x)
#define R_FINITE(x) R_finite(x)

/* x ^ y with R's table of special values (R's arithmetic: 1^y and x^0 are 1 even for NaN, 0^y by the sign of y,
 * NaN operands propagate as x + y, infinities by magnitude / parity, everything else NaN). */
double R_pow(double x, double y);

void R_CheckUserInterrupt(void);

#ifdef __cplusplus
}
#endif
#endif

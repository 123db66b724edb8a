/* Out-of-line part of the R / Rcpp stand-in: the object heap, the C accessors and R_pow. */
#include "Rcpp.h"

namespace mxref {

Heap &heap()
{
    static Heap h;
    return h;
}

static void destroy(SEXP s, std::vector<SEXP> &more)
{
    for (SEXP item : s->items)
        if (item && --item->refs <= 0 && !item->parked) {
            item->parked = true;
            more.push_back(item);
        }
    std::free(s->data);
    delete s;
}

void collect()
{
    Heap &h = heap();
    std::lock_guard<std::mutex> g(h.lock);
    std::vector<SEXP> work;
    work.swap(h.parked);
    while (!work.empty()) {
        SEXP s = work.back();
        work.pop_back();
        if (s->refs > 0) {
            s->parked = false;
            continue;
        }
        destroy(s, work);
        h.live--;
    }
}

long live_objects()
{
    Heap &h = heap();
    std::lock_guard<std::mutex> g(h.lock);
    return h.live;
}

}  // namespace mxref

extern "C" {

int *INTEGER(SEXP x)
{
    if (!x || (x->type != INTSXP && x->type != LGLSXP)) throw std::runtime_error("INTEGER() of a non-integer");
    return (int *)x->data;
}

int *LOGICAL(SEXP x)
{
    if (!x || (x->type != LGLSXP && x->type != INTSXP)) throw std::runtime_error("LOGICAL() of a non-logical");
    return (int *)x->data;
}

double *REAL(SEXP x)
{
    if (!x || x->type != REALSXP) throw std::runtime_error("REAL() of a non-numeric");
    return (double *)x->data;
}

R_xlen_t Rf_xlength(SEXP x)
{
    if (!x) return 0;
    return (x->type == VECSXP) ? (R_xlen_t)x->items.size() : x->length;
}

int Rf_length(SEXP x) { return (int)Rf_xlength(x); }
int TYPEOF(SEXP x) { return x ? x->type : NILSXP; }
void R_CheckUserInterrupt(void) {}

/* NOT the reference's code and not pinned by it: R_pow is R's (the reference links it), so this is our reading of R,
 * the same reading as oracle/mx_oracle.c and the device.  Tests that compare `^` against this library pin operand
 * order, recycling and fill cells only ("Not pinned").
 * R's x ^ y, from its documented table (?Arithmetic, "Writing R Extensions" 6.7): squaring is a product;
 * 1 ^ y and x ^ 0 are 1 for every y / x, NaN included; 0 ^ y is 0, Inf or y by the sign of y; finite operands
 * go to the C library; a NaN operand gives x + y; the remaining infinite cases follow IEC 60559 except that
 * (-Inf) ^ y for a finite integral y keeps R's own sign rule, decided with the same %% as R uses. */
static double mod2(double y)
{
    double q = y / 2.0;
    long double tmp = (long double)y - std::floor(q) * (long double)2.0;
    return (double)(tmp - std::floor(tmp / 2.0) * 2.0);
}

double R_pow(double x, double y)
{
    if (y == 2.0) return x * x;
    if (x == 1. || y == 0.) return 1.;
    if (x == 0.) {
        if (y > 0.) return 0.;
        else if (y < 0) return R_PosInf;
        else return y;
    }
    if (R_FINITE(x) && R_FINITE(y)) return std::pow(x, y);
    if (ISNAN(x) || ISNAN(y)) return x + y;
    if (!R_FINITE(x)) {
        if (x > 0) return (y < 0.) ? 0. : R_PosInf;
        if (R_FINITE(y) && y == std::floor(y)) return (y < 0.) ? 0. : (mod2(y) != 0 ? x : -x);
    }
    if (!R_FINITE(y)) {
        if (x >= 0) {
            if (y > 0) return (x >= 1) ? R_PosInf : 0.;
            return (x < 1) ? R_PosInf : 0.;
        }
    }
    return R_NaN;
}

}  /* extern "C" */

/* C entry over the reference's four vector-valued set_* routines (src/assignment.cpp:771-1133), used by
 * make_assign_vec_golden.py alone.  It is compiled with the reference's assignment.cpp and misc.cpp and
 * oracle/refshim into a temporary directory; nothing compiled is kept.  One call runs one routine by name on copies
 * of the flat inputs and keeps the returned list; the accessors read its three vectors and say which of them are the
 * input objects themselves. */
#include <cstring>
#include <exception>
#include <string>

#include "Rcpp.h"

typedef Rcpp::IntegerVector IV;
typedef Rcpp::NumericVector NV;
typedef Rcpp::List RL;

RL set_single_row_to_rowvec(IV, IV, NV, const int, const int, NV);
RL set_single_col_to_colvec(IV, IV, NV, const int, const int, NV);
RL set_single_row_to_svec(IV, IV, NV, const int, const int, IV, NV, const int);
RL set_single_col_to_svec(IV, IV, NV, const int, const int, IV, NV, const int);

static RL g_result;
static SEXP g_inputs[3];
static IV g_p, g_j;
static NV g_x;

extern "C" {

/* status 0, or 1 with the exception's message in msg; `at` is the row or the column */
int asgv_ref_call(const char *name, const int *p, int np, const int *j, const double *x, int nnz, int ncols, int at,
                  const int *ii, int n_ii, const double *xx, int n_xx, int length, char *msg, int msglen)
{
    try {
        g_p = IV(p, p + np);
        g_j = IV(j, j + nnz);
        g_x = NV(x, x + nnz);
        g_inputs[0] = g_p.get__(); g_inputs[1] = g_j.get__(); g_inputs[2] = g_x.get__();
        IV II(ii, ii + n_ii);
        NV XX(xx, xx + n_xx);
        const std::string f(name);
        if (f == "set_single_row_to_rowvec") g_result = set_single_row_to_rowvec(g_p, g_j, g_x, ncols, at, XX);
        else if (f == "set_single_col_to_colvec") g_result = set_single_col_to_colvec(g_p, g_j, g_x, ncols, at, XX);
        else if (f == "set_single_row_to_svec") g_result = set_single_row_to_svec(g_p, g_j, g_x, ncols, at, II, XX, length);
        else if (f == "set_single_col_to_svec") g_result = set_single_col_to_svec(g_p, g_j, g_x, ncols, at, II, XX, length);
        else throw std::runtime_error("unknown routine " + f);
        return 0;
    } catch (const std::exception &e) {
        std::strncpy(msg, e.what(), (size_t)msglen - 1);
        msg[msglen - 1] = 0;
        return 1;
    }
}

static const char *const KEYS[3] = {"indptr", "indices", "values"};

int asgv_ref_len(int k) { return (int)((SEXP)g_result[KEYS[k]])->length; }
int asgv_ref_is_input(int k) { return (SEXP)g_result[KEYS[k]] == g_inputs[k]; }
void asgv_ref_copy(int k, void *dst)
{
    SEXP s = g_result[KEYS[k]];
    std::memcpy(dst, s->data, (size_t)s->length * (k == 2 ? sizeof(double) : sizeof(int)));
}

}

/* C entry over the reference's set_* routines (src/assignment.cpp), used by make_assign_golden.py alone.  It is
 * compiled with the reference's assignment.cpp and misc.cpp and oracle/refshim into a temporary directory; nothing
 * compiled is kept.  One call runs one routine by name on copies of the flat inputs and keeps the returned list;
 * the accessors read its three vectors and say which of them are the input objects themselves. */
#include <cstring>
#include <exception>
#include <string>

#include "Rcpp.h"

typedef Rcpp::IntegerVector IV;
typedef Rcpp::NumericVector NV;
typedef Rcpp::List RL;

RL set_single_row_to_zero(IV, IV, NV, const int);
RL set_single_col_to_zero(IV, IV, NV, const int);
RL set_single_row_to_const(IV, IV, NV, const int, const int, const double);
RL set_single_col_to_const(IV, IV, NV, const int, const int, const double);
RL set_single_val_to_zero(IV, IV, NV, const int, const int);
RL set_single_val_to_const(IV, IV, NV, const int, const int, const int, const double);
RL set_rowseq_to_zero(IV, IV, NV, const int, const int);
RL set_rowseq_to_const(IV, IV, NV, const int, const int, const int, const double);
RL set_colseq_to_zero(IV, IV, NV, const int, const int, const int);
RL set_colseq_to_const(IV, IV, NV, const int, const int, const int, const double);
RL set_arbitrary_rows_to_zero(IV, IV, NV, IV);
RL set_arbitrary_rows_to_const(IV, IV, NV, IV, const int, const double);
RL set_arbitrary_cols_to_zero(IV, IV, NV, IV, const int);
RL set_arbitrary_cols_to_const(IV, IV, NV, IV, const int, const double);
RL set_arbitrary_rows_single_col_to_zero(IV, IV, NV, IV, const int, const int);
RL set_arbitrary_rows_single_col_to_const(IV, IV, NV, IV, const int, const double, const int);
RL set_single_row_arbitrary_cols_to_zero(IV, IV, NV, const int, IV, const int);
RL set_single_row_arbitrary_cols_to_const(IV, IV, NV, const int, IV, const int, const double);
RL set_arbitrary_rows_arbitrary_cols_to_zero(IV, IV, NV, IV, IV, const int);
RL set_arbitrary_rows_arbitrary_cols_to_const(IV, IV, NV, IV, IV, const int, const double);
RL set_rowseq_to_smat(IV, IV, NV, const int, const int, IV, IV, NV);
RL set_arbitrary_rows_to_smat(IV, IV, NV, IV, IV, IV, NV);

static RL g_result;
static SEXP g_inputs[3];
static IV g_p, g_j;
static NV g_x;

extern "C" {

/* status 0, or 1 with the exception's message in msg */
int asg_ref_call(const char *name, const int *p, int np, const int *j, const double *x, int nnz, int ncols, int row,
                 int col, int rst, int rend, int cst, int cend, const int *rows, int n_rows, const int *cols,
                 int n_cols, double val, const int *vp, int nvp, const int *vj, const double *vx, int vnnz, char *msg,
                 int msglen)
{
    try {
        g_p = IV(p, p + np);
        g_j = IV(j, j + nnz);
        g_x = NV(x, x + nnz);
        g_inputs[0] = g_p.get__(); g_inputs[1] = g_j.get__(); g_inputs[2] = g_x.get__();
        IV R(rows, rows + n_rows), C(cols, cols + n_cols), VP(vp, vp + nvp), VJ(vj, vj + vnnz);
        NV VX(vx, vx + vnnz);
        const std::string f(name);
        if (f == "set_single_row_to_zero") g_result = set_single_row_to_zero(g_p, g_j, g_x, row);
        else if (f == "set_single_col_to_zero") g_result = set_single_col_to_zero(g_p, g_j, g_x, col);
        else if (f == "set_single_row_to_const") g_result = set_single_row_to_const(g_p, g_j, g_x, ncols, row, val);
        else if (f == "set_single_col_to_const") g_result = set_single_col_to_const(g_p, g_j, g_x, ncols, col, val);
        else if (f == "set_single_val_to_zero") g_result = set_single_val_to_zero(g_p, g_j, g_x, row, col);
        else if (f == "set_single_val_to_const") g_result = set_single_val_to_const(g_p, g_j, g_x, ncols, row, col, val);
        else if (f == "set_rowseq_to_zero") g_result = set_rowseq_to_zero(g_p, g_j, g_x, rst, rend);
        else if (f == "set_rowseq_to_const") g_result = set_rowseq_to_const(g_p, g_j, g_x, rst, rend, ncols, val);
        else if (f == "set_colseq_to_zero") g_result = set_colseq_to_zero(g_p, g_j, g_x, cst, cend, ncols);
        else if (f == "set_colseq_to_const") g_result = set_colseq_to_const(g_p, g_j, g_x, cst, cend, ncols, val);
        else if (f == "set_arbitrary_rows_to_zero") g_result = set_arbitrary_rows_to_zero(g_p, g_j, g_x, R);
        else if (f == "set_arbitrary_rows_to_const") g_result = set_arbitrary_rows_to_const(g_p, g_j, g_x, R, ncols, val);
        else if (f == "set_arbitrary_cols_to_zero") g_result = set_arbitrary_cols_to_zero(g_p, g_j, g_x, C, ncols);
        else if (f == "set_arbitrary_cols_to_const") g_result = set_arbitrary_cols_to_const(g_p, g_j, g_x, C, ncols, val);
        else if (f == "set_arbitrary_rows_single_col_to_zero")
            g_result = set_arbitrary_rows_single_col_to_zero(g_p, g_j, g_x, R, col, ncols);
        else if (f == "set_arbitrary_rows_single_col_to_const")
            g_result = set_arbitrary_rows_single_col_to_const(g_p, g_j, g_x, R, col, val, ncols);
        else if (f == "set_single_row_arbitrary_cols_to_zero")
            g_result = set_single_row_arbitrary_cols_to_zero(g_p, g_j, g_x, row, C, ncols);
        else if (f == "set_single_row_arbitrary_cols_to_const")
            g_result = set_single_row_arbitrary_cols_to_const(g_p, g_j, g_x, row, C, ncols, val);
        else if (f == "set_arbitrary_rows_arbitrary_cols_to_zero")
            g_result = set_arbitrary_rows_arbitrary_cols_to_zero(g_p, g_j, g_x, R, C, ncols);
        else if (f == "set_arbitrary_rows_arbitrary_cols_to_const")
            g_result = set_arbitrary_rows_arbitrary_cols_to_const(g_p, g_j, g_x, R, C, ncols, val);
        else if (f == "set_rowseq_to_smat") g_result = set_rowseq_to_smat(g_p, g_j, g_x, rst, rend, VP, VJ, VX);
        else if (f == "set_arbitrary_rows_to_smat") g_result = set_arbitrary_rows_to_smat(g_p, g_j, g_x, R, VP, VJ, VX);
        else throw std::runtime_error("unknown routine " + f);
        return 0;
    } catch (const std::exception &e) {
        std::strncpy(msg, e.what(), (size_t)msglen - 1);
        msg[msglen - 1] = 0;
        return 1;
    }
}

static const char *const KEYS[3] = {"indptr", "indices", "values"};

int asg_ref_len(int k) { return (int)((SEXP)g_result[KEYS[k]])->length; }
int asg_ref_is_input(int k) { return (SEXP)g_result[KEYS[k]] == g_inputs[k]; }
void asg_ref_copy(int k, void *dst)
{
    SEXP s = g_result[KEYS[k]];
    std::memcpy(dst, s->data, (size_t)s->length * (k == 2 ? sizeof(double) : sizeof(int)));
}

}

// api_assign.hip — export level of `[<-` for a dgRMatrix (host pointers): the set_* routines of the reference's
// src/assignment.cpp as four entries over the kernels of assign.hip and assignvec.hip.  Arguments are checked before any device call;
// the alias cases (the reference returning its input vectors) are decided from the count pass, before any fill.
#include "mx_export.h"

#include <algorithm>
#include <vector>

using namespace mx;

namespace {

// One selector on the device: the axis the kernels read, the vectors a map lives in, and its length.
struct Selector {
    mx_coo_axis axis;
    Dev<int32_t> start, pos, sorted;
    int64_t n = 0;
};

// Host checks of a selector, before any device call: its kind, its bounds, and no index twice.
static int selector_check(const char *what, const char *name, int kind, int lo, int hi, const int32_t *set,
                          int64_t n_set, int n)
{
    switch (kind) {
        case MX_SEL_ALL: return 0;
        case MX_SEL_SINGLE:
            MX_REQUIRE(lo >= 0 && lo < n, "%s: %s index %d outside [0, %d)", what, name, lo, n);
            return 0;
        case MX_SEL_RANGE:
            MX_REQUIRE(lo <= hi, "%s: %s range has lo %d > hi %d", what, name, lo, hi);
            MX_REQUIRE(lo >= 0 && hi < n, "%s: %s range [%d, %d] outside [0, %d)", what, name, lo, hi, n);
            return 0;
        case MX_SEL_ARBITRARY: {
            MX_REQUIRE(n_set >= 0 && (n_set == 0 || set), "%s: null %s selector", what, name);
            MX_REQUIRE(n_set <= n, "%s: %s selector has duplicates", what, name);
            std::vector<char> seen((size_t)n, 0);
            for (int64_t t = 0; t < n_set; t++) {
                MX_REQUIRE(set[t] >= 0 && set[t] < n, "%s: %s index %d outside [0, %d)", what, name, set[t], n);
                MX_REQUIRE(!seen[set[t]], "%s: %s selector has duplicates", what, name);
                seen[set[t]] = 1;
            }
            return 0;
        }
        default: return set_error("%s: unknown %s selector kind %d", what, name, kind);
    }
}

// The axis of a checked selector.  An arbitrary one becomes mxd_colmap_build's layout of the 1-based selector, made
// here by a counting sort (as for the COO slice), and its ascending list when the const route wants it.
static int selector_setup(int kind, int lo, int hi, const int32_t *set, int64_t n_set, int n, bool want_sorted,
                          Selector &s)
{
    s.axis = mx_coo_axis{MX_AXIS_AFFINE, 0, n - 1, 0, 0, nullptr, nullptr};
    s.n = n;
    if (kind == MX_SEL_ALL) return 0;
    if (kind == MX_SEL_SINGLE) hi = lo;
    if (kind != MX_SEL_ARBITRARY) {
        s.axis.lo = lo;
        s.axis.hi = hi;
        s.n = (int64_t)hi - lo + 1;
        return 0;
    }
    s.n = n_set;
    int max_v = -1;
    for (int64_t t = 0; t < n_set; t++) max_v = std::max(max_v, set[t]);
    const int nmap = max_v + 2;                                   // keys are set[t] + 1 <= nmap - 1
    std::vector<int32_t> h_start((size_t)nmap + 1, 0), h_pos((size_t)n_set), h_sorted;
    for (int64_t t = 0; t < n_set; t++) h_start[set[t] + 2]++;    // key v counted at v + 1
    for (int v = 1; v <= nmap; v++) h_start[v] += h_start[v - 1]; // start[v] = entries with key < v
    for (int64_t t = 0; t < n_set; t++) h_pos[h_start[set[t] + 1]] = (int32_t)t;      // no duplicates: one slot each
    if (s.start.upload(h_start.data(), (int64_t)nmap + 1)) return 1;
    if (s.pos.upload(h_pos.data(), n_set)) return 1;
    if (want_sorted) {
        h_sorted.assign(set, set + n_set);
        std::sort(h_sorted.begin(), h_sorted.end());
        if (s.sorted.upload(h_sorted.data(), n_set)) return 1;
    }
    s.axis = mx_coo_axis{MX_AXIS_MAP, 0, 0, 0, nmap, s.start, s.pos};
    return 0;
}

static int csr_args_check(const char *what, const int32_t *indptr, int nrows, const int32_t *indices,
                          const double *values)
{
    MX_REQUIRE(nrows >= 0, "%s: negative number of rows %d", what, nrows);
    MX_REQUIRE(indptr, "%s: null index pointer", what);
    MX_REQUIRE(indptr[0] == 0 && indptr[nrows] >= 0, "%s: bad index pointer", what);
    MX_REQUIRE(indptr[nrows] == 0 || (indices && values), "%s: null indices or values", what);
    return 0;
}

}  // namespace

static int scalar_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values, int ncols,
                        int i_kind, int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set, int j_kind,
                        int j_lo, int j_hi, const int32_t *cols_set, int64_t n_cols_set, double value,
                        mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_assign_csr_scalar_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    if (csr_args_check(what, indptr, nrows, indices, values)) return 1;
    MX_REQUIRE(ncols >= 0, "%s: negative number of columns %d", what, ncols);
    if (selector_check(what, "row", i_kind, i_lo, i_hi, rows_set, n_rows_set, nrows)) return 1;
    if (selector_check(what, "column", j_kind, j_lo, j_hi, cols_set, n_cols_set, ncols)) return 1;
    *res_out = nullptr;
    const bool is_const = !(value == 0.0);                       // R/assignment.R:121: NA and NaN are not zero
    // the two exports that always build new vectors: set_rowseq_to_zero (:1135-1171), set_colseq_to_const (:1293-1364)
    const bool never_alias = is_const ? (i_kind == MX_SEL_ALL && j_kind == MX_SEL_RANGE)
                                      : (i_kind == MX_SEL_RANGE && j_kind == MX_SEL_ALL);
    const int64_t nnz = indptr[nrows];
    const double avg = nrows > 0 ? (double)nnz / (double)nrows : 0.0;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Selector si, sj;
        if (selector_setup(i_kind, i_lo, i_hi, rows_set, n_rows_set, nrows, false, si)) return 1;
        if (selector_setup(j_kind, j_lo, j_hi, cols_set, n_cols_set, ncols, is_const, sj)) return 1;
        Csr X;
        DevBuf ws;
        if (X.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        // the const route merges, which wants sorted rows: rows that are not are sorted in the device copy (the
        // reference sorts the selected rows of the caller's vectors in place instead, assignment.cpp:2184-2191, :2383)
        int sorted = 1;
        if (is_const && nnz > 1) {
            Dev<int32_t> flag;
            if (flag.alloc(4)) return 1;
            if (mxd_csr_rows_sorted(nrows, X.p, X.j, flag, &sorted, nullptr)) return 1;
            if (!sorted) {
                Dev<int32_t> tj;
                Dev<double> tx;
                if (tj.alloc(nnz) || tx.alloc(nnz)) return 1;
                if (mxd_csr_sort_rows(nrows, nnz, X.p, X.j, X.x, MX_F64, tj, tx, nullptr)) return 1;
                MX_HIP(hipStreamSynchronize(nullptr));             // tj / tx are freed on leaving this block
            }
        }
        if (ws.alloc_bytes(mxd_gather_workspace_bytes(nrows))) return 1;
        Dev<int32_t> new_p;                                       // the result's only once no alias case applies
        if (new_p.alloc((int64_t)nrows + 1)) return 1;
        int64_t total = 0, hits = 0;
        if (mxd_csr_assign_count(nrows, ncols, X.p, X.j, nnz, &si.axis, &sj.axis, si.n, sj.n, is_const, avg, new_p, ws,
                                 &total, &hits, nullptr)) return 1;
        if (!never_alias && !is_const && hits == 0) {             // nothing to remove: the input vectors themselves
            res.alias(MX_ALIAS_ALL, (int64_t)nrows + 1, nnz);
            return 0;
        }
        // the diff == 0 branches; rows sorted here are new vectors, not the caller's
        const bool same_structure = !never_alias && is_const && total == nnz && sorted;
        if (same_structure) {
            res.alias(1, (int64_t)nrows + 1, nnz);
            if (res.alloc_values(nnz, sizeof(double))) return 1;
        } else {
            if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
            if (res.indptr.copy_from(new_p, (int64_t)nrows + 1)) return 1;
            if (res.alloc_entries(total, sizeof(double))) return 1;
        }
        const int32_t *const rp = same_structure ? (const int32_t *)X.p : (const int32_t *)res.indptr;
        int32_t *const rj = same_structure ? nullptr : (int32_t *)res.indices;
        return mxd_csr_assign_fill(nrows, ncols, X.p, X.j, X.x, &si.axis, &sj.axis, sj.sorted, sj.n, is_const, value,
                                   avg, rp, rj, res.values, nullptr);
    });
}

static int rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values, int i_kind,
                      int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set, const int32_t *v_indptr,
                      int64_t v_nrows, const int32_t *v_indices, const double *v_values, mx_result **res_out,
                      mx_result_info *info)
{
    const char *what = "mx_assign_csr_rows_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    if (csr_args_check(what, indptr, nrows, indices, values)) return 1;
    MX_REQUIRE(v_nrows >= 0 && v_nrows <= nrows, "%s: the value has %lld rows, the matrix %d", what,
               (long long)v_nrows, nrows);
    if (csr_args_check(what, v_indptr, (int)v_nrows, v_indices, v_values)) return 1;
    if (selector_check(what, "row", i_kind, i_lo, i_hi, rows_set, n_rows_set, nrows)) return 1;
    const int64_t n_sel = i_kind == MX_SEL_ALL ? nrows : i_kind == MX_SEL_SINGLE ? 1
                        : i_kind == MX_SEL_RANGE ? (int64_t)i_hi - i_lo + 1 : n_rows_set;
    MX_REQUIRE(n_sel == v_nrows, "%s: the value has %lld rows, the row selector %lld entries", what,
               (long long)v_nrows, (long long)n_sel);
    *res_out = nullptr;
    const int64_t nnz = indptr[nrows], v_nnz = v_indptr[v_nrows];
    const double avg = nrows > 0 ? (double)(nnz + v_nnz) / (double)nrows : 0.0;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Selector si;
        if (selector_setup(i_kind, i_lo, i_hi, rows_set, n_rows_set, nrows, false, si)) return 1;
        Csr X, V;
        DevBuf ws;
        if (X.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        if (V.upload(v_indptr, v_indices, v_values, (int)v_nrows, sizeof(double))) return 1;
        if (ws.alloc_bytes(mxd_gather_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t total = 0;
        if (mxd_csr_replace_rows_count(nrows, X.p, &si.axis, (int)v_nrows, V.p, res.indptr, ws, &total, nullptr))
            return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        return mxd_csr_replace_rows_fill(nrows, X.p, X.j, X.x, &si.axis, (int)v_nrows, V.p, V.j, V.x, avg, res.indptr, res.indices,
                                         res.values, nullptr);
    });
}

// ---- vector values: one row or one column -------------------------------------------------------
// Host checks of a pattern (ii, xx, n_xx, length) recycled along an axis of n entries, before any device call.
static int pattern_check(const char *what, const char *axis, const int32_t *ii, const double *xx, int64_t n_xx,
                         int length, int n, bool ascending)
{
    MX_REQUIRE(length > 0, "%s: the value's length %d is not positive", what, length);
    MX_REQUIRE(length <= n && n % length == 0, "%s: the value's length %d does not divide the %d %s", what, length, n,
               axis);
    MX_REQUIRE(n_xx >= 0 && n_xx <= length, "%s: the value has %lld entries, its length is %d", what,
               (long long)n_xx, length);
    MX_REQUIRE(n_xx == 0 || xx, "%s: null values of the vector", what);
    if (!ii || n_xx == 0) {
        MX_REQUIRE(n_xx == 0 || n_xx == length, "%s: a dense vector of %lld values, its length is %d", what,
                   (long long)n_xx, length);
        return 0;
    }
    for (int64_t t = 0; t < n_xx; t++) {
        MX_REQUIRE(ii[t] >= 0 && ii[t] < length, "%s: vector index %d outside [0, %d)", what, ii[t], length);
        MX_REQUIRE(!ascending || t == 0 || ii[t] > ii[t - 1], "%s: the vector's indices are not strictly ascending",
                   what);
    }
    return 0;
}

// The pattern on the device.  A sparse pattern without entries keeps a non-null ii, which is what says "sparse" to
// the device level.
struct Pattern {
    Dev<int32_t> ii;
    Dev<double> xx;
    bool dense = false;
    int upload(const int32_t *h_ii, const double *h_xx, int64_t n_xx)
    {
        dense = !h_ii && n_xx > 0;
        if (!dense && ii.upload(h_ii, n_xx)) return 1;
        return xx.upload(h_xx, n_xx);
    }
    const int32_t *ii_ptr() const { return dense ? nullptr : (const int32_t *)ii; }
};

static int row_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values, int ncols,
                         int row, const int32_t *ii, const double *xx, int64_t n_xx, int length, mx_result **res_out,
                         mx_result_info *info)
{
    const char *what = "mx_assign_csr_row_vec_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    if (csr_args_check(what, indptr, nrows, indices, values)) return 1;
    MX_REQUIRE(ncols >= 0, "%s: negative number of columns %d", what, ncols);
    MX_REQUIRE(row >= 0 && row < nrows, "%s: row index %d outside [0, %d)", what, row, nrows);
    if (pattern_check(what, "columns", ii, xx, n_xx, length, ncols, false)) return 1;
    *res_out = nullptr;
    const bool dense = !ii && n_xx > 0;
    const int n_repeats = ncols / length;
    const int64_t nnz = indptr[nrows], v_nnz = n_xx * n_repeats;
    const int s = indptr[row], e = indptr[row + 1];
    // the caller's own vectors hold the row: does it already spell the recycled pattern, element for element?
    bool same = (int64_t)e - s == v_nnz && v_nnz > 0;
    for (int64_t t = 0; same && t < v_nnz; t++)
        same = indices[s + t] == (dense ? (int32_t)t : ii[t % n_xx] + length * (int32_t)(t / n_xx));
    const double avg = nrows > 0 ? (double)(nnz + v_nnz) / (double)nrows : 0.0;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Pattern pat;
        if (pat.upload(ii, xx, n_xx)) return 1;
        if (same) {                                              // values only, beside the caller's structure
            res.alias(1, (int64_t)nrows + 1, nnz);
            if (res.alloc_values(nnz, sizeof(double))) return 1;
            if (mx::xfer_h2d(res.values, values, (size_t)nnz * sizeof(double))) return 1;
            return mxd_csr_expand_pattern_row(pat.ii_ptr(), pat.xx, n_xx, length, n_repeats, nullptr, nullptr,
                                              (double *)res.values + s, nullptr);
        }
        Csr X;
        Dev<int32_t> vp, vj;
        Dev<double> vx;
        DevBuf ws;
        if (X.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        if (vp.alloc(2) || vj.alloc(v_nnz) || vx.alloc(v_nnz)) return 1;
        if (mxd_csr_expand_pattern_row(pat.ii_ptr(), pat.xx, n_xx, length, n_repeats, vp, vj, vx, nullptr)) return 1;
        const mx_coo_axis ai = {MX_AXIS_AFFINE, row, row, 0, 0, nullptr, nullptr};
        if (ws.alloc_bytes(mxd_gather_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t total = 0;
        if (mxd_csr_replace_rows_count(nrows, X.p, &ai, 1, vp, res.indptr, ws, &total, nullptr)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        return mxd_csr_replace_rows_fill(nrows, X.p, X.j, X.x, &ai, 1, vp, vj, vx, avg, res.indptr, res.indices,
                                         res.values, nullptr);
    });
}

static int col_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values, int ncols,
                         int col, const int32_t *ii, const double *xx, int64_t n_xx, int length, mx_result **res_out,
                         mx_result_info *info)
{
    const char *what = "mx_assign_csr_col_vec_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    if (csr_args_check(what, indptr, nrows, indices, values)) return 1;
    MX_REQUIRE(ncols >= 0, "%s: negative number of columns %d", what, ncols);
    MX_REQUIRE(col >= 0 && col < ncols, "%s: column index %d outside [0, %d)", what, col, ncols);
    if (pattern_check(what, "rows", ii, xx, n_xx, length, nrows, true)) return 1;
    *res_out = nullptr;
    const int64_t nnz = indptr[nrows];
    const double avg = nrows > 0 ? (double)nnz / (double)nrows : 0.0;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Pattern pat;
        if (pat.upload(ii, xx, n_xx)) return 1;
        Csr X;
        DevBuf ws;
        if (X.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        // an insert wants a sorted row: rows that are not are sorted in the device copy, all of them (the reference
        // sorts the rows it inserts into, src/assignment.cpp:67-112, and leaves the others as stored)
        int sorted = 1;
        if (nnz > 1) {
            Dev<int32_t> flag;
            if (flag.alloc(4)) return 1;
            if (mxd_csr_rows_sorted(nrows, X.p, X.j, flag, &sorted, nullptr)) return 1;
            if (!sorted) {
                Dev<int32_t> tj;
                Dev<double> tx;
                if (tj.alloc(nnz) || tx.alloc(nnz)) return 1;
                if (mxd_csr_sort_rows(nrows, nnz, X.p, X.j, X.x, MX_F64, tj, tx, nullptr)) return 1;
                MX_HIP(hipStreamSynchronize(nullptr));             // tj / tx are freed on leaving this block
            }
        }
        if (ws.alloc_bytes(mxd_gather_workspace_bytes(nrows))) return 1;
        Dev<int32_t> new_p;                                       // the result's only when the structure changes
        if (new_p.alloc((int64_t)nrows + 1)) return 1;
        int64_t total = 0, changed = 0;
        if (mxd_csr_assign_col_count(nrows, ncols, X.p, X.j, nnz, col, pat.ii_ptr(), n_xx, length, avg, new_p, ws,
                                     &total, &changed, nullptr)) return 1;
        // set_single_col_to_colvec's diff == 0 branch (:856-873); set_single_col_to_svec always builds new vectors
        const bool same_structure = pat.dense && changed == 0 && sorted;
        if (same_structure) {
            res.alias(1, (int64_t)nrows + 1, nnz);
            if (res.alloc_values(nnz, sizeof(double))) return 1;
        } else {
            if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
            if (res.indptr.copy_from(new_p, (int64_t)nrows + 1)) return 1;
            if (res.alloc_entries(total, sizeof(double))) return 1;
        }
        const int32_t *const rp = same_structure ? (const int32_t *)X.p : (const int32_t *)res.indptr;
        int32_t *const rj = same_structure ? nullptr : (int32_t *)res.indices;
        return mxd_csr_assign_col_fill(nrows, ncols, X.p, X.j, X.x, col, pat.ii_ptr(), pat.xx, n_xx, length, avg, rp,
                                       rj, res.values, nullptr);
    });
}

// the selector maps live in std::vector: an allocation failure becomes an error, not an exception through the C ABI
extern "C" {

int mx_assign_csr_scalar_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                               int ncols, int i_kind, int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set,
                               int j_kind, int j_lo, int j_hi, const int32_t *cols_set, int64_t n_cols_set,
                               double value, mx_result **res, mx_result_info *info)
{
    try {
        return scalar_begin(indptr, nrows, indices, values, ncols, i_kind, i_lo, i_hi, rows_set, n_rows_set, j_kind,
                            j_lo, j_hi, cols_set, n_cols_set, value, res, info);
    } catch (const std::bad_alloc &) {
        return set_error("out of host memory");
    }
}

int mx_assign_csr_rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                             int i_kind, int i_lo, int i_hi, const int32_t *rows_set, int64_t n_rows_set,
                             const int32_t *v_indptr, int64_t v_nrows, const int32_t *v_indices,
                             const double *v_values, mx_result **res, mx_result_info *info)
{
    try {
        return rows_begin(indptr, nrows, indices, values, i_kind, i_lo, i_hi, rows_set, n_rows_set, v_indptr, v_nrows,
                          v_indices, v_values, res, info);
    } catch (const std::bad_alloc &) {
        return set_error("out of host memory");
    }
}

int mx_assign_csr_row_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                int ncols, int row, const int32_t *ii, const double *xx, int64_t n_xx, int length,
                                mx_result **res, mx_result_info *info)
{
    try {
        return row_vec_begin(indptr, nrows, indices, values, ncols, row, ii, xx, n_xx, length, res, info);
    } catch (const std::bad_alloc &) {
        return set_error("out of host memory");
    }
}

int mx_assign_csr_col_vec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                int ncols, int col, const int32_t *ii, const double *xx, int64_t n_xx, int length,
                                mx_result **res, mx_result_info *info)
{
    try {
        return col_vec_begin(indptr, nrows, indices, values, ncols, col, ii, xx, n_xx, length, res, info);
    } catch (const std::bad_alloc &) {
        return set_error("out of host memory");
    }
}

}  // extern "C"

// assign.hip — X[i, j] <- scalar and X[i, ] <- CSR of a dgRMatrix for gfx950.
//
// Replaces the serial loops of src/assignment.cpp:
//   set_single_{row,col,val}_to_{zero,const}                        :384-769
//   set_{rowseq,colseq}_to_{zero,const}                             :1135-1364
//   set_arbitrary_{rows,cols}_to_{zero,const}                       :1366-1793
//   set_arbitrary_rows_single_col_to_*, set_single_row_arbitrary_cols_to_*,
//   set_arbitrary_rows_arbitrary_cols_to_*                          :1795-2476
//   set_rowseq_to_smat, set_arbitrary_rows_to_smat                  :2478-2598
//
// One skeleton, as the gathers of gather.hip and colslice.hip: per-row output lengths -> exclusive scan -> fill, one
// G-lane group per row.  Both selectors are mx_coo_axis values (cooslice.hip): AFFINE for all / single / seq /
// rev-seq, MAP for an arbitrary selector without duplicates.  From an axis the kernels take whether an index is
// selected and how many selected indices lie below it: arithmetic for AFFINE, start[] for MAP.
//
// Scalar value.  A row the row selector does not select is copied.  In a selected row
//   zero:  the entries whose column is selected are dropped, the rest keep their order (ballot compaction);
//   const: the row becomes the ascending merge of its kept entries and one (col, value) per selected column.  The
//          rows are sorted and free of duplicates here (the callers see to it), so the slot of every output follows
//          from counts alone: a kept entry, the i-th of its row, lands at i + (selected columns below its column)
//          - (hits before it); a selected column c lands at (row entries below c) + (selected columns below c that
//          the row does not store).  For an AFFINE column axis the selected columns are one run behind the entries
//          left of it and need no search; for a MAP they come from the ascending list of selected columns and a
//          binary search in the row.  Every slot is written once; a slot outside [new_indptr[r], new_indptr[r+1]),
//          which only a row that is not sorted can produce, is not written.
// Row replacement.  A selected row r becomes row k of `value`, k = r's position in the selector; a two-source gather.
#include "mx_assign.h"

namespace mx {

struct AsgAxis {
    int map, lo, hi, rev, nmap;
    const int32_t *start, *pos;
};

static AsgAxis asg_axis(const mx_coo_axis &a)
{
    return AsgAxis{a.kind == MX_AXIS_MAP, a.lo, a.hi, a.reversed, a.nmap, a.start, a.pos};
}

// is 0-based index r selected?  (the map is keyed by the 1-based selector)
__device__ __forceinline__ bool asg_selected(const AsgAxis &ax, int r)
{
    if (ax.map) return r >= 0 && r + 1 < ax.nmap && ax.start[r + 2] > ax.start[r + 1];
    return r >= ax.lo && r <= ax.hi;
}

// number of selected indices below c (the selector has no duplicates)
__device__ __forceinline__ int asg_below(const AsgAxis &ax, int c)
{
    if (ax.map) return c < 0 ? 0 : ax.start[c + 1 < ax.nmap ? c + 1 : ax.nmap];
    return c <= ax.lo ? 0 : c > ax.hi ? ax.hi - ax.lo + 1 : c - ax.lo;
}

// position of the selected index r in the selector
__device__ __forceinline__ int asg_position(const AsgAxis &ax, int r)
{
    if (ax.map) return ax.pos[ax.start[r + 1]];
    return ax.rev ? ax.hi - r : r - ax.lo;
}

// ---- scalar value: count -----------------------------------------------------------------------------------------
// lens[row] = len - hits + add for a selected row (add = selected columns on the const route, 0 on the zero route),
// len otherwise.  all_j: every column is selected, so hits = len and the indices are not read.
template <int G>
__global__ __launch_bounds__(AS_BLOCK)
void assign_count_kernel(int nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                         AsgAxis ai, AsgAxis aj, int add, int all_j, int32_t *__restrict__ lens)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (AS_BLOCK / G) + threadIdx.x / G;
    const bool valid = row < nrows;
    int s = 0, e = 0;
    bool sel = false;
    if (valid) { s = indptr[row]; e = indptr[row + 1]; sel = asg_selected(ai, (int)row); }
    int hits = 0;
    if (sel && all_j) hits = e - s;
    else if (sel) {
        for (int k0 = s; k0 < e; k0 += G) {            // e - s is uniform inside the group
            const int k = k0 + lg;
            const bool hit = k < e && asg_selected(aj, indices[k]);
            hits += __popcll(group_ballot<G>(hit));
        }
    }
    if (valid && lg == 0) lens[row] = e - s - hits + (sel ? add : 0);
}

// ---- scalar value: fill ------------------------------------------------------------------------------------------
// every store goes through asg_store (mx_assign.h): values as their 64 bits, never outside the row's own slots
template <int G, bool CONST>
__global__ __launch_bounds__(AS_BLOCK)
void assign_fill_kernel(int nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                        const uint64_t *__restrict__ values, AsgAxis ai, AsgAxis aj,
                        const int32_t *__restrict__ cols_sorted, int nsel_j, uint64_t vbits,
                        const int32_t *__restrict__ new_indptr, int32_t *__restrict__ new_indices,
                        uint64_t *__restrict__ new_values)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (AS_BLOCK / G) + threadIdx.x / G;
    const bool valid = row < nrows;
    int s = 0, e = 0, o = 0, oe = 0;
    bool sel = false;
    if (valid) {
        s = indptr[row]; e = indptr[row + 1];
        o = new_indptr[row]; oe = new_indptr[row + 1];
        sel = asg_selected(ai, (int)row);
    }
    const unsigned long long below = (1ULL << lg) - 1ULL;
    if (!sel) {                                        // uniform inside the group: a straight copy
        for (int k = s + lg; k < e; k += G) asg_store(new_indices, new_values, o, oe, o + (k - s), indices[k], values[k]);
        return;
    }
    int hits = 0, nleft = 0;                           // hits so far; entries left of an AFFINE column run
    for (int k0 = s; k0 < e; k0 += G) {
        const int k = k0 + lg;
        const bool in = k < e;
        const int c = in ? indices[k] : 0;
        const bool hit = in && asg_selected(aj, c);
        const unsigned long long hb = group_ballot<G>(hit);
        if (in && !hit) {
            const int before = hits + __popcll(hb & below);
            const int pos = o + (k - s) - before + (CONST ? asg_below(aj, c) : 0);
            asg_store(new_indices, new_values, o, oe, pos, c, values[k]);
        }
        hits += __popcll(hb);
        if constexpr (CONST) nleft += __popcll(group_ballot<G>(in && !aj.map && c < aj.lo));
    }
    if constexpr (CONST) {
        if (!aj.map) {                                 // one run lo..hi behind the entries left of it
            for (int t = lg; t < nsel_j; t += G) asg_store(new_indices, new_values, o, oe, o + nleft + t, aj.lo + t, vbits);
            return;
        }
        int absent = 0;                                // selected columns so far that the row does not store
        for (int t0 = 0; t0 < nsel_j; t0 += G) {       // nsel_j is uniform
            const int t = t0 + lg;
            const bool in = t < nsel_j;
            int c = 0, L = 0;
            bool present = false;
            if (in) {
                c = cols_sorted[t];
                L = lower_bound_dev(indices + s, e - s, c);
                present = L < e - s && indices[s + L] == c;
            }
            const unsigned long long ab = group_ballot<G>(in && !present);
            if (in) asg_store(new_indices, new_values, o, oe, o + L + absent + __popcll(ab & below), c, vbits);
            absent += __popcll(ab);
        }
    }
}

// ---- row replacement ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_BLOCK)
void replace_rows_count_kernel(int nrows, const int32_t *__restrict__ indptr, AsgAxis ai, int nvalue_rows,
                               const int32_t *__restrict__ v_indptr, int32_t *__restrict__ lens)
{
    const long long row = (long long)blockIdx.x * AS_BLOCK + threadIdx.x;
    if (row >= nrows) return;
    if (asg_selected(ai, (int)row)) {
        const int k = asg_position(ai, (int)row);                  // a position outside `value` takes nothing
        lens[row] = (unsigned)k < (unsigned)nvalue_rows ? v_indptr[k + 1] - v_indptr[k] : 0;
    } else lens[row] = indptr[row + 1] - indptr[row];
}

template <int G>
__global__ __launch_bounds__(AS_BLOCK)
void replace_rows_fill_kernel(int nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                              const uint64_t *__restrict__ values, AsgAxis ai, int nvalue_rows,
                              const int32_t *__restrict__ v_indptr, const int32_t *__restrict__ v_indices,
                              const uint64_t *__restrict__ v_values,
                              const int32_t *__restrict__ new_indptr, int32_t *__restrict__ new_indices,
                              uint64_t *__restrict__ new_values)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (AS_BLOCK / G) + threadIdx.x / G;
    if (row >= nrows) return;
    const int o = new_indptr[row], oe = new_indptr[row + 1];
    const int32_t *src_j = indices;
    const uint64_t *src_x = values;
    int s;
    if (asg_selected(ai, (int)row)) {
        const int k = asg_position(ai, (int)row);
        if ((unsigned)k >= (unsigned)nvalue_rows) return;         // the count pass gave such a row no slot
        s = v_indptr[k];
        src_j = v_indices; src_x = v_values;
    } else s = indptr[row];
    for (int t = lg; t < oe - o; t += G) {             // the length is the count pass's: never past the row's slots
        new_indices[o + t] = src_j[s + t];
        new_values[o + t] = src_x[s + t];
    }
}

static int asg_check_axis(const char *what, const mx_coo_axis *a, int n, const char *name)
{
    MX_REQUIRE(a, "%s: null %s axis", what, name);
    if (a->kind == MX_AXIS_MAP) {
        MX_REQUIRE(a->nmap >= 0 && a->nmap <= n + 1 && (a->nmap == 0 || (a->start && a->pos)), "%s: bad %s map", what,
                   name);
    } else {
        MX_REQUIRE(a->kind == MX_AXIS_AFFINE, "%s: unknown %s axis kind %d", what, name, a->kind);
        MX_REQUIRE(a->lo >= 0 && a->lo <= a->hi && a->hi < n, "%s: %s range [%d, %d] outside [0, %d)", what, name,
                   a->lo, a->hi, n);
    }
    return 0;
}

}  // namespace mx

extern "C" int mxd_csr_assign_count(int nrows, int ncols, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                                    const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, int64_t nsel_i,
                                    int64_t nsel_j, int is_const, double avg_row_len, int32_t *new_indptr,
                                    void *workspace, int64_t *nnz_out_host, int64_t *hits_out_host, void *stream)
{
    const char *what = "mxd_csr_assign_count";
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0 && nnz <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(indptr && new_indptr && workspace && nnz_out_host && hits_out_host, "%s: null pointer", what);
    if (mx::asg_check_axis(what, axis_i, nrows, "row") || mx::asg_check_axis(what, axis_j, ncols, "column")) return 1;
    MX_REQUIRE(nsel_i >= 0 && nsel_i <= nrows && nsel_j >= 0 && nsel_j <= ncols, "%s: bad selector length", what);
    hipStream_t st = mx::as_stream(stream);
    const int all_j = axis_j->kind == MX_AXIS_AFFINE && axis_j->lo == 0 && axis_j->hi == ncols - 1;
    MX_REQUIRE(all_j || nnz == 0 || indices, "%s: null indices", what);
    int32_t *lens = mx::CountLayout(workspace, nrows).counts;
    if (nrows > 0) {
        const mx::AsgAxis ai = mx::asg_axis(*axis_i), aj = mx::asg_axis(*axis_j);
        const int add = is_const ? (int)nsel_j : 0;
        const int rc = mx::launch_rows(mx::lane_groups{}, what, mx::pick_group(avg_row_len), nrows, mx::AS_BLOCK,
                                       [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::assign_count_kernel<g()>), grid, block, 0, st, nrows, indptr, indices, ai, aj, add,
                               all_j, lens);
        });
        if (rc) return rc;
    }
    if (mx::asg_finish_count(nrows, workspace, new_indptr, nnz_out_host, st)) return 1;
    // total = nnz - hits (+ one entry per selected cell on the const route)
    *hits_out_host = nnz + (is_const ? nsel_i * nsel_j : 0) - *nnz_out_host;
    return 0;
}

extern "C" int mxd_csr_assign_fill(int nrows, int ncols, const int32_t *indptr, const int32_t *indices,
                                   const double *values, const mx_coo_axis *axis_i, const mx_coo_axis *axis_j,
                                   const int32_t *cols_sorted, int64_t nsel_j, int is_const, double value,
                                   double avg_row_len, const int32_t *new_indptr, int32_t *new_indices,
                                   double *new_values, void *stream)
{
    const char *what = "mxd_csr_assign_fill";
    MX_REQUIRE(nrows >= 0 && ncols >= 0, "%s: bad size", what);
    if (mx::asg_check_axis(what, axis_i, nrows, "row") || mx::asg_check_axis(what, axis_j, ncols, "column")) return 1;
    MX_REQUIRE(nsel_j >= 0 && nsel_j <= ncols, "%s: bad selector length", what);
    if (nrows == 0) return 0;
    MX_REQUIRE(indptr && new_indptr && new_values, "%s: null pointer", what);
    MX_REQUIRE(!is_const || axis_j->kind != MX_AXIS_MAP || nsel_j == 0 || cols_sorted,
               "%s: an arbitrary column selector needs its ascending list", what);
    hipStream_t st = mx::as_stream(stream);
    const mx::AsgAxis ai = mx::asg_axis(*axis_i), aj = mx::asg_axis(*axis_j);
    uint64_t vbits;
    static_assert(sizeof(vbits) == sizeof(value), "f64 bits");
    __builtin_memcpy(&vbits, &value, sizeof(vbits));
    using routes = mx::int_list<0, 1>;
    return mx::dispatch_int(routes{}, what, "route", is_const ? 1 : 0, [&](auto route) {
        return mx::launch_rows(mx::lane_groups{}, what, mx::pick_group(avg_row_len), nrows, mx::AS_BLOCK,
                               [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::assign_fill_kernel<g(), route() == 1>), grid, block, 0, st, nrows, indptr, indices,
                               (const uint64_t *)values, ai, aj, cols_sorted, (int)nsel_j, vbits, new_indptr,
                               new_indices, (uint64_t *)new_values);
        });
    });
}

extern "C" int mxd_csr_replace_rows_count(int nrows, const int32_t *indptr, const mx_coo_axis *axis_i,
                                          int nvalue_rows, const int32_t *v_indptr, int32_t *new_indptr,
                                          void *workspace, int64_t *nnz_out_host, void *stream)
{
    const char *what = "mxd_csr_replace_rows_count";
    MX_REQUIRE(nrows >= 0, "%s: bad size", what);
    MX_REQUIRE(indptr && v_indptr && new_indptr && workspace && nnz_out_host, "%s: null pointer", what);
    if (mx::asg_check_axis(what, axis_i, nrows, "row")) return 1;
    MX_REQUIRE(nvalue_rows >= 0 && (axis_i->kind == MX_AXIS_MAP || axis_i->hi - axis_i->lo + 1 == nvalue_rows),
               "%s: the value has %d rows, the row selector another length", what, nvalue_rows);
    hipStream_t st = mx::as_stream(stream);
    int32_t *lens = mx::CountLayout(workspace, nrows).counts;
    if (nrows > 0) {
        hipLaunchKernelGGL(mx::replace_rows_count_kernel, dim3(mx::grid_for(nrows, mx::AS_BLOCK)), dim3(mx::AS_BLOCK), 0,
                           st, nrows, indptr, mx::asg_axis(*axis_i), nvalue_rows, v_indptr, lens);
        MX_LAUNCH_CHECK();
    }
    return mx::asg_finish_count(nrows, workspace, new_indptr, nnz_out_host, st);
}

extern "C" int mxd_csr_replace_rows_fill(int nrows, const int32_t *indptr, const int32_t *indices,
                                         const double *values, const mx_coo_axis *axis_i, int nvalue_rows,
                                         const int32_t *v_indptr, const int32_t *v_indices, const double *v_values,
                                         double avg_row_len,
                                         const int32_t *new_indptr, int32_t *new_indices, double *new_values,
                                         void *stream)
{
    const char *what = "mxd_csr_replace_rows_fill";
    MX_REQUIRE(nrows >= 0, "%s: bad size", what);
    if (mx::asg_check_axis(what, axis_i, nrows, "row")) return 1;
    if (nrows == 0) return 0;
    MX_REQUIRE(indptr && v_indptr && new_indptr && new_indices && new_values, "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    const mx::AsgAxis ai = mx::asg_axis(*axis_i);
    return mx::launch_rows(mx::lane_groups{}, what, mx::pick_group(avg_row_len), nrows, mx::AS_BLOCK,
                           [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((mx::replace_rows_fill_kernel<g()>), grid, block, 0, st, nrows, indptr, indices,
                           (const uint64_t *)values, ai, nvalue_rows, v_indptr, v_indices, (const uint64_t *)v_values,
                           new_indptr,
                           new_indices, (uint64_t *)new_values);
    });
}

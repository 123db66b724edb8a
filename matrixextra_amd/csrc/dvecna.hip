// dvecna.hip — RsparseMatrix (op) dense vector keeping what R's arithmetic makes NA / NaN / 1 / Inf, for gfx950.
//
// Replaces multiply_csr_by_dvec_with_NAs (src/operators.cpp:2258-2852), a serial push_back loop that the R caller
// takes when the vector holds an NA / NaN, a zero under / %% %/% ^, an Inf under * or a negative exponent under ^
// (R/operators.R:981-988).  X is m x ncol in CSR with f64 values and rows sorted by column (the caller sorts,
// R/operators.R:1113); the vector dvec has length L.  The reference has two regimes, both reproduced as written
// (DESIGN.md §4.12), the second one's fill values being the other way round from the first's:
//
// A. row-ruled, L <= m and m % L == 0 (:2314-2513).  Row r is ruled by val = dvec[r % L]: a plain row keeps its
//    entries with x op val, a filled row has all ncol columns.  The count needs indptr and val only (one lane per
//    row, no pass over the entries); count -> finish_count (scan, 64-bit total, one read-back) -> fill with one
//    G-lane group per plain row, and the filled rows written by the whole wave (mx_dense_row.h).
//      *         val NaN: NA_real_ under an NA val, else the default NaN, in every column;
//                val +-Inf: the default NaN, and x * val at the stored columns          (:2342-2352)
//      / %% %/%  val == 0: the default NaN, and x op val at the stored columns;
//                val NaN: val in every column                                            (:2364-2389 and siblings)
//      ^         val NaN: val; val == 0: 1; val < 0: +Inf; R_pow(x, val) at the stored columns (:2475-2493)
//
// B. flat, every other length (:2515-2841).  A stored (r, c) gets x op dvec[(r + c*m) % L]: mxd_csr_by_dvec.  A
//    position ix of the vector is special when dvec[ix] is NaN, 0 under / %% %/% ^, negative under ^ or +-Inf under
//    *; every flat cell ix + rep*L < m*ncol of a special position (row = flat % m, col = flat / m) outside the
//    pattern of X becomes a new entry: the default NaN for an NA or a zero divisor, 1 / +Inf for a zero / negative
//    exponent, NA_real_ for anything else (:2618-2636).  Here: flag and compact the special positions (scan), one
//    lane per (special, rep) pair binary-searches its row of X (count -> scan -> fill of COO triplets), then the
//    existing COO -> CSR sort and the union merge's fill join them with X's transformed values; the patterns are
//    disjoint, so the output row starts are the sums of the two index pointers and every value is copied.
//    The pairs are enumerated in closed form: with R = ceil(N / L) and cut = N - (R-1)*L, a special position below
//    cut has R cells and any other R - 1, so the work is the number of candidate cells, never N.
//
// Row bounds are clamped into [0, nnz], every write position comes from a scanned count, and the candidate count is
// refused at INT_MAX before anything is allocated for it.
#include "mx_dispatch.h"
#include "mx_workspace.h"
#include "mx_rarith.h"
#include "mx_dense_row.h"

namespace mx {

constexpr int DN_BLOCK = 256;

// R's ISNA (arithmetic.c R_IsNA): a NaN whose low word is 1954
__device__ __forceinline__ bool dn_is_na(double v)
{
    return isnan(v) && (unsigned)((unsigned long long)__double_as_longlong(v) & 0xFFFFFFFFULL) == 1954u;
}
__device__ __forceinline__ bool dn_is_div(int op) { return op == MX_DV_DIVIDE || op == MX_DV_DIVREST || op == MX_DV_INTDIV; }

// regime A: does val fill its rows?
__device__ __forceinline__ bool dn_row_filled(int op, double val)
{
    if (op == MX_DV_MULTIPLY) return isnan(val) || isinf(val);
    if (op == MX_DV_POWERTO) return isnan(val) || val <= 0;
    return val == 0 || isnan(val);
}

// regime A's filled rows (mx_dense_row.h); the operation is always applied with X on the left
struct DnRowRule {
    int op;
    __device__ __forceinline__ bool looks_up(double val) const
    {
        if (op == MX_DV_MULTIPLY) return isinf(val);
        if (op == MX_DV_POWERTO) return true;
        return val == 0;
    }
    __device__ __forceinline__ double fill(double val) const
    {
        if (op == MX_DV_MULTIPLY) return dn_is_na(val) ? na_real() : dv_nan();
        if (op == MX_DV_POWERTO) return isnan(val) ? val : (val == 0 ? 1.0 : __builtin_inf());
        return val == 0 ? dv_nan() : val;
    }
    __device__ __forceinline__ double at(double x, double val) const { return dv_apply(op, true, x, val); }
};

struct DnRow {
    int s, len;
    double val;
    bool filled;
};

__device__ __forceinline__ DnRow dn_row(long long r, int64_t nnz, const int32_t *__restrict__ indptr,
                                        const double *__restrict__ dvec, int L, int op)
{
    DnRow w;
    const RowBounds b = row_bounds(indptr[r], indptr[r + 1], nnz);
    w.s = (int)b.start;
    w.len = (int)b.len;
    w.val = dvec[r % L];
    w.filled = dn_row_filled(op, w.val);
    return w;
}

__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_count_kernel(int m, int ncol, int64_t nnz, const int32_t *__restrict__ indptr,
                          const double *__restrict__ dvec, int L, int op, int32_t *__restrict__ counts)
{
    const long long r = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (r >= m) return;
    const DnRow w = dn_row(r, nnz, indptr, dvec, L, op);
    counts[r] = w.filled ? ncol : w.len;
}

template <int G>
__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_fill_kernel(int m, int ncol, int64_t nnz, const int32_t *__restrict__ indptr,
                         const int32_t *__restrict__ indices, const double *__restrict__ values,
                         const double *__restrict__ dvec, int L, int op, const int32_t *__restrict__ out_indptr,
                         int32_t *__restrict__ out_indices, double *__restrict__ out_values)
{
    const int lg = threadIdx.x % G;
    const long long r = (long long)blockIdx.x * (DN_BLOCK / G) + threadIdx.x / G;
    DnRow w{0, 0, 1.0, false};
    int64_t dst = 0;
    if (r < m) { w = dn_row(r, nnz, indptr, dvec, L, op); dst = out_indptr[r]; }
    if (!w.filled) {                                        // a plain row: x op val, structure kept
        for (int k = lg; k < w.len; k += G) {
            out_indices[dst + k] = indices[w.s + k];
            out_values[dst + k] = dv_apply(op, true, values[w.s + k], w.val);
        }
    }
    // no lane has left: the wave writes the filled rows of its groups, 64 consecutive columns per store
    write_dense_rows(w.filled && lg == 0, dst, w.s, w.len, w.val, ncol, indices, values, out_indices, out_values,
                     DnRowRule{op});
}

// ---- regime B ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool dn_special(int op, double v)
{
    return isnan(v) || ((dn_is_div(op) || op == MX_DV_POWERTO) && v == 0) || (op == MX_DV_POWERTO && v < 0) ||
           (op == MX_DV_MULTIPLY && isinf(v));
}

// the value of a new cell, in the reference's order (:2618-2636)
__device__ __forceinline__ double dn_cell_value(int op, double v)
{
    if ((dn_is_div(op) && v == 0) || dn_is_na(v)) return dv_nan();
    if (op == MX_DV_POWERTO && v == 0) return 1.0;
    if (op == MX_DV_POWERTO && v < 0) return __builtin_inf();
    return na_real();
}

__global__ __launch_bounds__(DN_BLOCK)
void dn_special_flag_kernel(const double *__restrict__ dvec, int L, int op, int32_t *__restrict__ flags)
{
    const long long ix = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (ix < L) flags[ix] = dn_special(op, dvec[ix]) ? 1 : 0;
}

// offsets: the scanned flags; the special positions come out ascending
__global__ __launch_bounds__(DN_BLOCK)
void dn_special_scatter_kernel(int L, const int32_t *__restrict__ offsets, int32_t *__restrict__ special)
{
    const long long ix = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (ix >= L) return;
    const int o = offsets[ix];
    if (offsets[ix + 1] != o) special[o] = (int)ix;
}

// the candidate cells in closed form: the first nfull special positions have R cells each, the others R - 1
struct DnPairs {
    long long candidates, nfull, R, L, N;
    int m;
};

__device__ __forceinline__ bool dn_pair_cell(const DnPairs &pp, long long t, const int32_t *__restrict__ special,
                                             int &ix, int &row, int &col)
{
    const long long head = pp.nfull * pp.R;
    long long sp, rep;
    if (t < head) { sp = t / pp.R; rep = t - sp * pp.R; }
    else {
        const long long u = t - head, q = pp.R - 1;        // q >= 1 here: with R == 1 every special position is full
        sp = pp.nfull + u / q;
        rep = u % q;
    }
    ix = special[sp];
    const long long flat = (long long)ix + rep * pp.L;
    if (flat >= pp.N) return false;                         // cannot happen with the closed form; never used to index
    row = (int)(flat % pp.m);
    col = (int)(flat / pp.m);
    return true;
}

// is (row, col) outside the pattern of X?  (:2607-2615: the first / last column test, then lower_bound)
__device__ __forceinline__ bool dn_cell_is_new(int row, int col, int64_t nnz, const int32_t *__restrict__ indptr,
                                               const int32_t *__restrict__ indices)
{
    const RowBounds b = row_bounds(indptr[row], indptr[row + 1], nnz);
    const int64_t s = b.start;
    const int len = (int)b.len;
    if (len == 0) return true;
    const int lb = lower_bound_dev(indices + s, len, col);
    return lb >= len || indices[s + lb] != col;
}

__global__ __launch_bounds__(DN_BLOCK)
void dn_cells_count_kernel(DnPairs pp, int64_t nnz, const int32_t *__restrict__ indptr,
                           const int32_t *__restrict__ indices, const int32_t *__restrict__ special,
                           int32_t *__restrict__ flags)
{
    const long long t = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (t >= pp.candidates) return;
    int ix, row, col;
    flags[t] = dn_pair_cell(pp, t, special, ix, row, col) && dn_cell_is_new(row, col, nnz, indptr, indices) ? 1 : 0;
}

// offsets: the scanned flags of the count; the search is not repeated
__global__ __launch_bounds__(DN_BLOCK)
void dn_cells_fill_kernel(DnPairs pp, const double *__restrict__ dvec, int op, const int32_t *__restrict__ special,
                          const int32_t *__restrict__ offsets, int32_t *__restrict__ out_rows,
                          int32_t *__restrict__ out_cols, double *__restrict__ out_values)
{
    const long long t = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (t >= pp.candidates) return;
    const int o = offsets[t];
    if (offsets[t + 1] == o) return;
    int ix, row, col;
    if (!dn_pair_cell(pp, t, special, ix, row, col)) return;
    out_rows[o] = row;
    out_cols[o] = col;
    out_values[o] = dn_cell_value(op, dvec[ix]);
}

__global__ __launch_bounds__(DN_BLOCK)
void dn_indptr_sum_kernel(int m, const int32_t *__restrict__ p1, const int32_t *__restrict__ p2,
                          int32_t *__restrict__ out)
{
    const long long r = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (r <= m) out[r] = p1[r] + p2[r];
}

static inline bool dn_op_known(int op) { return op >= MX_DV_MULTIPLY && op <= MX_DV_INTDIV; }

// the special positions of the vector: a flag per position, the scanned flags, the positions compacted
struct DnSpecialLayout {
    WsCursor c;
    int64_t L;
    int32_t *counts = c.take_counts(L), *offsets = c.take_i32(L + 1), *list = c.take_i32(L);
    size_t bytes = c.bytes();
    DnSpecialLayout(const void *ws, int64_t L_) : c(ws), L(L_ > 0 ? L_ : 0) {}
};
using DnCellsLayout = CountOffsetsLayout;   // per candidate cell: is it new, then its position among the new ones

static const char *const DN_OVERFLOW =
    "Error: the resulting matrix would have too many entries for a sparse CSR representation (int overflow).";

static int dn_pairs(const char *what, int m, int ncols, int64_t dvec_len, int64_t nspecial, int64_t candidates,
                    DnPairs *pp)
{
    MX_REQUIRE(m > 0 && ncols > 0 && dvec_len >= 1 && dvec_len <= INT_MAX, "%s: bad arguments", what);
    const long long N = (long long)m * ncols, L = dvec_len;
    MX_REQUIRE(L <= N, "%s: the vector has more entries than the matrix", what);
    const long long R = (N + L - 1) / L;
    const long long nfull = candidates - nspecial * (R - 1);
    MX_REQUIRE(nspecial >= 0 && nspecial <= L && candidates >= 0 && candidates < INT_MAX && nfull >= 0 &&
               nfull <= nspecial, "%s: the counts are not those of mxd_dvec_na_special", what);
    *pp = DnPairs{candidates, nfull, R, L, N, m};
    return 0;
}

}  // namespace mx

extern "C" size_t mxd_csr_by_dvec_na_rows_workspace_bytes(int m) { return mx::CountLayout(nullptr, m).bytes; }

static int dn_rows_check(const char *what, int m, int ncols, int64_t nnz, int64_t dvec_len, int op)
{
    MX_REQUIRE(m >= 0 && ncols >= 0 && nnz >= 0 && nnz <= INT_MAX, "%s: bad arguments", what);
    MX_REQUIRE(mx::dn_op_known(op), "%s: unknown operation %d", what, op);
    MX_REQUIRE(m == 0 || (dvec_len >= 1 && dvec_len <= m && m % dvec_len == 0),
               "%s: the vector's length must divide the number of rows", what);
    return 0;
}

extern "C" int mxd_csr_by_dvec_na_rows_count(int m, int ncols, int64_t nnz, const int32_t *indptr, const double *dvec,
                                             int64_t dvec_len, int op, void *workspace, int32_t *out_indptr,
                                             int64_t *nnz_out_host, void *stream)
{
    if (dn_rows_check("mxd_csr_by_dvec_na_rows_count", m, ncols, nnz, dvec_len, op)) return 1;
    MX_REQUIRE(workspace && out_indptr && nnz_out_host && (m == 0 || (indptr && dvec)),
               "mxd_csr_by_dvec_na_rows_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    *nnz_out_host = 0;
    if (m > 0) {
        hipLaunchKernelGGL(mx::dn_rows_count_kernel, dim3(mx::grid_for(m, mx::DN_BLOCK)), dim3(mx::DN_BLOCK), 0, st, m,
                           ncols, nnz, indptr, dvec, (int)dvec_len, op, mx::CountLayout(workspace, m).counts);
        MX_LAUNCH_CHECK();
    }
    // the 64-bit total is read back (one synchronise) and refused above INT_MAX before any output exists
    return mx::finish_count(m, workspace, out_indptr, nnz_out_host, st);
}

extern "C" int mxd_csr_by_dvec_na_rows_fill(int m, int ncols, int64_t nnz, const int32_t *indptr,
                                            const int32_t *indices, const double *values, const double *dvec,
                                            int64_t dvec_len, int op, const int32_t *out_indptr, int32_t *out_indices,
                                            double *out_values, void *stream)
{
    if (dn_rows_check("mxd_csr_by_dvec_na_rows_fill", m, ncols, nnz, dvec_len, op)) return 1;
    if (m == 0) return 0;
    MX_REQUIRE(indptr && dvec && out_indptr && out_indices && out_values && (nnz == 0 || (indices && values)),
               "mxd_csr_by_dvec_na_rows_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const int G = mx::pick_group((double)nnz / (double)m);
    return mx::launch_rows(mx::lane_groups{}, "mxd_csr_by_dvec_na_rows_fill", G, m, mx::DN_BLOCK,
                           [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(mx::dn_rows_fill_kernel<g()>, grid, block, 0, st, m, ncols, nnz, indptr, indices, values,
                           dvec, (int)dvec_len, op, out_indptr, out_indices, out_values);
    });
}

extern "C" size_t mxd_dvec_na_special_workspace_bytes(int64_t L) { return mx::DnSpecialLayout(nullptr, L).bytes; }

extern "C" int mxd_dvec_na_special(int m, int ncols, const double *dvec, int64_t dvec_len, int op, void *special_ws,
                                   int64_t *nspecial_host, int64_t *candidates_host, void *stream)
{
    MX_REQUIRE(m > 0 && ncols > 0 && dvec && special_ws && nspecial_host && candidates_host,
               "mxd_dvec_na_special: bad arguments");
    MX_REQUIRE(mx::dn_op_known(op), "mxd_dvec_na_special: unknown operation %d", op);
    MX_REQUIRE(dvec_len >= 1 && dvec_len <= INT_MAX, "mxd_dvec_na_special: a vector of %lld entries is not supported",
               (long long)dvec_len);
    const long long N = (long long)m * ncols, L = dvec_len;
    MX_REQUIRE(L <= N, "mxd_dvec_na_special: the vector has more entries than the matrix");
    hipStream_t st = mx::as_stream(stream);
    *nspecial_host = *candidates_host = 0;
    const mx::DnSpecialLayout S(special_ws, L);
    int32_t *offsets = S.offsets;
    hipLaunchKernelGGL(mx::dn_special_flag_kernel, dim3(mx::grid_for(L, mx::DN_BLOCK)), dim3(mx::DN_BLOCK), 0, st, dvec,
                       (int)L, op, S.counts);
    MX_LAUNCH_CHECK();
    if (mx::finish_count(L, S.counts, offsets, nspecial_host, st)) return 1;
    if (*nspecial_host == 0) return 0;
    hipLaunchKernelGGL(mx::dn_special_scatter_kernel, dim3(mx::grid_for(L, mx::DN_BLOCK)), dim3(mx::DN_BLOCK), 0, st,
                       (int)L, offsets, S.list);
    MX_LAUNCH_CHECK();
    // sum over the special positions of ceil((N - ix) / L): R for those below cut, R - 1 for the others
    const long long R = (N + L - 1) / L, cut = N - (R - 1) * L;             // 0 < cut <= L
    int32_t nfull = 0;
    MX_HIP(hipMemcpyAsync(&nfull, offsets + cut, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    *candidates_host = (long long)nfull * R + (*nspecial_host - nfull) * (R - 1);
    // every candidate is a new entry or falls on one of X's, so new + nnz >= candidates (:2654-2660)
    MX_REQUIRE(*candidates_host < (int64_t)INT_MAX, "%s", mx::DN_OVERFLOW);
    return 0;
}

extern "C" size_t mxd_dvec_na_cells_workspace_bytes(int64_t n) { return mx::DnCellsLayout(nullptr, n).bytes; }

extern "C" int mxd_dvec_na_cells_count(int m, int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                       int64_t dvec_len, const void *special_ws, int64_t nspecial, int64_t candidates,
                                       void *cells_ws, int64_t *new_host, void *stream)
{
    mx::DnPairs pp;
    if (mx::dn_pairs("mxd_dvec_na_cells_count", m, ncols, dvec_len, nspecial, candidates, &pp)) return 1;
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX && indptr && (nnz == 0 || indices) && special_ws && cells_ws && new_host,
               "mxd_dvec_na_cells_count: bad arguments");
    hipStream_t st = mx::as_stream(stream);
    *new_host = 0;
    const mx::DnCellsLayout cells(cells_ws, candidates);
    if (candidates > 0) {
        hipLaunchKernelGGL(mx::dn_cells_count_kernel, dim3(mx::grid_for(candidates, mx::DN_BLOCK)), dim3(mx::DN_BLOCK),
                           0, st, pp, nnz, indptr, indices, mx::DnSpecialLayout(special_ws, dvec_len).list,
                           cells.counts);
        MX_LAUNCH_CHECK();
    }
    if (mx::finish_count(candidates, cells.counts, cells.offsets, new_host, st)) return 1;
    MX_REQUIRE(*new_host == 0 || *new_host + nnz < (int64_t)INT_MAX, "%s", mx::DN_OVERFLOW);   // :2654-2660
    return 0;
}

extern "C" int mxd_dvec_na_cells_fill(int m, int ncols, const double *dvec, int64_t dvec_len, int op,
                                      const void *special_ws, int64_t nspecial, int64_t candidates,
                                      const void *cells_ws, int32_t *out_rows, int32_t *out_cols, double *out_values,
                                      void *stream)
{
    mx::DnPairs pp;
    if (mx::dn_pairs("mxd_dvec_na_cells_fill", m, ncols, dvec_len, nspecial, candidates, &pp)) return 1;
    MX_REQUIRE(mx::dn_op_known(op), "mxd_dvec_na_cells_fill: unknown operation %d", op);
    if (candidates == 0) return 0;
    MX_REQUIRE(dvec && special_ws && cells_ws && out_rows && out_cols && out_values,
               "mxd_dvec_na_cells_fill: null pointer");
    hipLaunchKernelGGL(mx::dn_cells_fill_kernel, dim3(mx::grid_for(candidates, mx::DN_BLOCK)), dim3(mx::DN_BLOCK), 0,
                       mx::as_stream(stream), pp, dvec, op, mx::DnSpecialLayout(special_ws, dvec_len).list,
                       mx::DnCellsLayout(cells_ws, candidates).offsets, out_rows, out_cols, out_values);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" int mxd_csr_join_disjoint(int m, const int32_t *indptr1, const int32_t *indices1, const double *values1,
                                     int64_t nnz1, const int32_t *indptr2, const int32_t *indices2,
                                     const double *values2, int64_t nnz2, int32_t *out_indptr, int32_t *out_indices,
                                     double *out_values, void *stream)
{
    MX_REQUIRE(m >= 0 && nnz1 >= 0 && nnz2 >= 0 && nnz1 + nnz2 <= INT_MAX, "mxd_csr_join_disjoint: bad arguments");
    MX_REQUIRE(indptr1 && indptr2 && out_indptr, "mxd_csr_join_disjoint: null pointer");
    hipLaunchKernelGGL(mx::dn_indptr_sum_kernel, dim3(mx::grid_for((int64_t)m + 1, mx::DN_BLOCK)), dim3(mx::DN_BLOCK),
                       0, mx::as_stream(stream), m, indptr1, indptr2, out_indptr);
    MX_LAUNCH_CHECK();
    if (m == 0 || nnz1 + nnz2 == 0) return 0;
    MX_REQUIRE(out_indices && out_values, "mxd_csr_join_disjoint: null pointer");
    return mxd_csr_merge_fill(MX_OP_ADD, m, indptr1, indices1, values1, nnz1, indptr2, indices2, values2, nnz2,
                              out_indptr, out_indices, out_values, stream);
}

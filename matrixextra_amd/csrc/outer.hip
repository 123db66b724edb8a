// outer.hip — the outer products of `%*%` with a one-column CSR, and the float32 row vector x CSC product, for gfx950.
//
// Replaces:
//   matmul_colvec_by_scolvecascsr{,_f32}                               src/matmul.cpp:686-781
//   matmul_spcolvec_by_scolvecascsr_{numeric,integer,logical,binary}   src/matmul.cpp:783-938
//   matmul_rowvec_by_csc, matmul_rowvec_by_cscbin                      src/matmul.cpp:643-684
// (serial loops; the sparse one push_backs entry after entry).
//
// X is the CSR triple of a one-column matrix with m rows: a row is non-empty when indptr[r] < indptr[r+1], and its
// value is values[indptr[r]], the FIRST stored entry; `indices` is never read.
//
// dense outer   CSR out, m rows: a non-empty row r holds columns 0..dim-1 with a * colvec[c].
//               count: one lane per row marks dim or 0 -> finish_count (scan, 64-bit total, one read-back).
//               fill:  one G-lane group per row (G from dim) writes the iota and the scaled vector, G consecutive
//                      columns per store.
//               f64: 0.0 + a*v with the product rounded on its own (daxpy on a zeroed slot: -0 products come out as
//               +0), and a == 0 leaves the zeros (daxpy's quick return: no NaN from 0 * Inf).  f32: a narrowed to
//               float first (:53-57), 0.0f + a*v in float, widened for the output.
// sparse outer  CSC out, y_length columns: column y_i[k]-1 holds every non-empty row, ascending, with y_x[k] * a.
//               count: the non-empty rows are compacted once (row ids and first values, through compact.hip's
//                      mask rule), the per-column count is scattered to the stored positions and scanned.
//               fill:  one lane group per (stored y entry, chunk of OP_CHUNK compacted rows).
// Deviations from the reference (also in mxgpu.h and DESIGN.md §4.14):
//   * its output arrays have length(indices) * dim entries, a zero tail when a row stores more than one entry; here
//     they have out_indptr[m] entries;
//   * the entry count, (non-empty rows) * dim or * nnz(y), is checked against INT32_MAX, which it does not check;
//   * known defect, not copied: :808 reads y_values[col] where it means y_values[ix], an out-of-bounds read
//     whenever y stores fewer positions than its length.  y_values[k] is used here.
// Every write position comes from the scanned counts and is bounded by them again in the fill, positions of y
// outside [1, y_length] are skipped in both passes, and a row start outside [0, nnz) reads nothing.
#include "mx_dispatch.h"
#include "mx_workspace.h"

namespace mx {

constexpr int OP_BLOCK = 256;
constexpr int OP_CHUNK = 1024;       // compacted rows per lane group in the sparse fill

__global__ __launch_bounds__(OP_BLOCK)
void outer_mark_kernel(int m, int dim, const int32_t *__restrict__ indptr, int32_t *__restrict__ counts)
{
    const long long r = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (r < m) counts[r] = indptr[r] < indptr[r + 1] ? dim : 0;
}

template <typename T> __device__ __forceinline__ double outer_dense_value(double a, T v);
// daxpy into a zeroed slot; __dmul_rn / __fmul_rn keep the product from being fused into the add, which would
// turn an underflowing negative product into -0
template <> __device__ __forceinline__ double outer_dense_value<double>(double a, double v)
{
    return a == 0.0 ? 0.0 : __dadd_rn(0.0, __dmul_rn(a, v));
}
template <> __device__ __forceinline__ double outer_dense_value<float>(double a, float v)
{
    return (double)__fadd_rn(0.0f, __fmul_rn((float)a, v));
}

template <int G, typename T>
__global__ __launch_bounds__(OP_BLOCK)
void outer_dense_fill_kernel(int m, int dim, int64_t nnz, const int32_t *__restrict__ indptr,
                             const double *__restrict__ values, const T *__restrict__ colvec,
                             const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                             double *__restrict__ out_values)
{
    const int lg = threadIdx.x % G;
    const long long r = (long long)blockIdx.x * (OP_BLOCK / G) + threadIdx.x / G;
    if (r >= m) return;
    const int64_t dst = out_indptr[r];
    int cnt = out_indptr[r + 1] - (int32_t)dst;
    cnt = cnt < dim ? cnt : dim;
    if (cnt <= 0) return;                                   // an empty row reads nothing more
    const int64_t s = indptr[r];
    if (s < 0 || s >= nnz) return;
    const double a = values[s];
    for (int c = lg; c < cnt; c += G) {
        out_indices[dst + c] = c;
        out_values[dst + c] = outer_dense_value<T>(a, colvec[c]);
    }
}

// per row: non-empty flag, its own id and its first value, the three inputs of compact.hip's mask rule
__global__ __launch_bounds__(OP_BLOCK)
void outer_rows_kernel(int m, int64_t nnz, const int32_t *__restrict__ indptr, const double *__restrict__ values,
                       int32_t *__restrict__ flags, int32_t *__restrict__ ids, double *__restrict__ firsts)
{
    const long long r = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (r >= m) return;
    const int64_t s = indptr[r], e = indptr[r + 1];
    const bool full = s < e && s >= 0 && s < nnz;
    flags[r] = full;
    ids[r] = (int32_t)r;
    firsts[r] = full ? values[s] : 0.0;
}

__global__ __launch_bounds__(OP_BLOCK)
void outer_cols_kernel(int64_t ny, const int32_t *__restrict__ yi, int y_length, int per_col,
                       int32_t *__restrict__ counts)
{
    const long long k = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (k >= ny) return;
    const long long c = (long long)yi[k] - 1;
    if (c >= 0 && c < y_length) counts[c] = per_col;
}

// lane group `item` = (stored y entry k, chunk of the compacted rows)
template <int G, typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(OP_BLOCK)
void outer_svec_fill_kernel(int64_t items, int64_t chunks, const int32_t *__restrict__ yi,
                            const VT *__restrict__ yv, int y_length, const int32_t *__restrict__ rows,
                            const double *__restrict__ firsts, int nonempty, const int32_t *__restrict__ out_indptr,
                            int32_t *__restrict__ out_indices, double *__restrict__ out_values)
{
    const int lg = threadIdx.x % G;
    const long long item = (long long)blockIdx.x * (OP_BLOCK / G) + threadIdx.x / G;
    if (item >= items) return;
    const long long k = item / chunks;
    const long long col = (long long)yi[k] - 1;
    if (col < 0 || col >= y_length) return;
    const int64_t dst = out_indptr[col];
    int cnt = out_indptr[col + 1] - (int32_t)dst;
    cnt = cnt < nonempty ? cnt : nonempty;
    VT y{};
    if constexpr (HAS_VALUES) y = yv[k];
    const int t0 = (int)(item % chunks) * OP_CHUNK;
    const int t1 = t0 + OP_CHUNK < cnt ? t0 + OP_CHUNK : cnt;
    for (int t = t0 + lg; t < t1; t += G) {
        const double a = firsts[t];
        double o;
        if constexpr (!HAS_VALUES) o = a;                                    // :822-824
        else if constexpr (std::is_same<VT, double>::value) o = __dmul_rn(y, a);   // :826-828
        else o = y == MX_NA_INT ? na_real() : __dmul_rn((double)y, a);       // :815-820 (logicals arrive as ints)
        out_indices[dst + t] = rows[t];
        out_values[dst + t] = o;
    }
}

// workspace of the sparse outer product
struct OuterLayout {
    WsCursor c;
    int m, y_length;
    void *compact = c.take((mxd_compact_workspace_bytes(m) + 15) & ~(size_t)15);   // mxd_compact_* over the m rows
    int32_t *flags = c.take_i32(m), *ids = c.take_i32(m);              // per row: non-empty, its own id
    int32_t *rows = c.take_i32(m);                                      // the non-empty rows, compacted
    double *firsts = c.take<double>(2 * padded_i32_bytes(m));           // per row: its first value
    double *kept_firsts = c.take<double>(2 * padded_i32_bytes(m));      // the same, compacted
    int32_t *col_counts = c.take_counts(y_length);                      // per column of the result
    size_t bytes = c.bytes();
    OuterLayout(const void *ws, int m_, int y_length_) : c(ws), m(m_), y_length(y_length_) {}
};

static const char *const OUTER_OVERFLOW = "%s: the outer product has %lld entries: exceeds R's int32 index range";

}  // namespace mx

extern "C" size_t mxd_csr_outer_dense_workspace_bytes(int m) { return mx::CountLayout(nullptr, m).bytes; }

extern "C" int mxd_csr_outer_dense_count(int m, int dim, const int32_t *indptr, void *workspace, int32_t *out_indptr,
                                         int64_t *nnz_out_host, void *stream)
{
    MX_REQUIRE(m >= 0 && dim >= 0, "mxd_csr_outer_dense_count: bad arguments");
    MX_REQUIRE(workspace && out_indptr && nnz_out_host && (m == 0 || indptr), "mxd_csr_outer_dense_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    *nnz_out_host = 0;
    if (m > 0) {
        hipLaunchKernelGGL(mx::outer_mark_kernel, dim3((unsigned)mx::ceil_div(m, mx::OP_BLOCK)), dim3(mx::OP_BLOCK), 0,
                           st, m, dim, indptr, mx::CountLayout(workspace, m).counts);
        MX_LAUNCH_CHECK();
    }
    return mx::finish_count(m, workspace, out_indptr, nnz_out_host, st);
}

extern "C" int mxd_csr_outer_dense_fill(int m, int dim, int64_t nnz, const int32_t *indptr, const double *values,
                                        const void *colvec, int colvec_dtype, const int32_t *out_indptr,
                                        int32_t *out_indices, double *out_values, void *stream)
{
    MX_REQUIRE(m >= 0 && dim >= 0 && nnz >= 0, "mxd_csr_outer_dense_fill: bad arguments");
    if (m == 0 || dim == 0 || nnz == 0) return 0;
    MX_REQUIRE(indptr && values && colvec && out_indptr && out_indices && out_values,
               "mxd_csr_outer_dense_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    return mx::dispatch_dense("mxd_csr_outer_dense_fill", colvec_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return mx::launch_rows(mx::lane_groups{}, "mxd_csr_outer_dense_fill", mx::pick_group((double)dim), m,
                               mx::OP_BLOCK, [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::outer_dense_fill_kernel<g(), T>), grid, block, 0, st, m, dim, nnz, indptr, values,
                               (const T *)colvec, out_indptr, out_indices, out_values);
        });
    });
}

extern "C" size_t mxd_csr_outer_svec_workspace_bytes(int m, int y_length)
{
    return mx::OuterLayout(nullptr, m, y_length).bytes;
}

extern "C" int mxd_csr_outer_svec_count(int m, int64_t nnz, const int32_t *indptr, const double *values,
                                        const int32_t *y_indices_base1, int64_t ny, int y_length, void *workspace,
                                        int32_t *out_indptr, int64_t *nonempty_host, int64_t *nnz_out_host,
                                        void *stream)
{
    MX_REQUIRE(m >= 0 && nnz >= 0 && ny >= 0 && ny <= INT_MAX && y_length >= 0,
               "mxd_csr_outer_svec_count: bad arguments");
    MX_REQUIRE(workspace && out_indptr && nonempty_host && nnz_out_host && (m == 0 || indptr) &&
               (nnz == 0 || values) && (ny == 0 || y_indices_base1), "mxd_csr_outer_svec_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const mx::OuterLayout ws(workspace, m, y_length);
    *nonempty_host = 0;
    *nnz_out_host = 0;
    if (m > 0) {
        hipLaunchKernelGGL(mx::outer_rows_kernel, dim3((unsigned)mx::ceil_div(m, mx::OP_BLOCK)), dim3(mx::OP_BLOCK), 0,
                           st, m, nnz, indptr, values, ws.flags, ws.ids, ws.firsts);
        MX_LAUNCH_CHECK();
        if (mxd_compact_count(m, ws.firsts, MX_F64, MX_KEEP_MASK, ws.flags, ws.compact, nonempty_host, stream))
            return 1;
        if (mxd_compact_fill(m, ws.firsts, MX_F64, MX_KEEP_MASK, ws.flags, ws.ids, nullptr, 0, nullptr,
                             ws.compact, ws.rows, nullptr, ws.kept_firsts, nullptr, stream)) return 1;
    }
    MX_REQUIRE(*nonempty_host * ny <= (int64_t)INT_MAX, mx::OUTER_OVERFLOW, "mxd_csr_outer_svec_count",
               (long long)(*nonempty_host * ny));
    MX_HIP(hipMemsetAsync(ws.col_counts, 0, sizeof(int32_t) * (size_t)(y_length > 0 ? y_length : 1), st));
    if (ny > 0 && y_length > 0) {
        hipLaunchKernelGGL(mx::outer_cols_kernel, dim3((unsigned)mx::ceil_div(ny, mx::OP_BLOCK)), dim3(mx::OP_BLOCK), 0,
                           st, ny, y_indices_base1, y_length, (int)*nonempty_host, ws.col_counts);
        MX_LAUNCH_CHECK();
    }
    return mx::finish_count(y_length, ws.col_counts, out_indptr, nnz_out_host, st);
}

extern "C" int mxd_csr_outer_svec_fill(int m, const int32_t *y_indices_base1, int64_t ny, const void *y_values,
                                       int value_dtype, int y_length, int64_t nonempty, const void *workspace,
                                       const int32_t *out_indptr, int32_t *out_indices, double *out_values,
                                       void *stream)
{
    MX_REQUIRE(m >= 0 && ny >= 0 && ny <= INT_MAX && y_length >= 0 && nonempty >= 0 && nonempty <= m,
               "mxd_csr_outer_svec_fill: bad arguments");
    if (ny == 0 || nonempty == 0 || y_length == 0) return 0;
    MX_REQUIRE(workspace && y_indices_base1 && out_indptr && out_indices && out_values &&
               (value_dtype == MX_NONE || y_values), "mxd_csr_outer_svec_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const mx::OuterLayout ws(workspace, m, y_length);
    const int64_t chunks = mx::ceil_div(nonempty, mx::OP_CHUNK), items = ny * chunks;
    const int G = mx::pick_group((double)(nonempty < mx::OP_CHUNK ? nonempty : mx::OP_CHUNK));
    return mx::dispatch_values("mxd_csr_outer_svec_fill", value_dtype, [&](auto kind) {
        using K = decltype(kind);
        return mx::launch_rows(mx::lane_groups{}, "mxd_csr_outer_svec_fill", G, items, mx::OP_BLOCK,
                               [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::outer_svec_fill_kernel<g(), typename K::VT, K::has_values>), grid, block, 0, st,
                               items, chunks, y_indices_base1, (const typename K::VT *)y_values, y_length, ws.rows,
                               ws.kept_firsts, (int)nonempty, out_indptr, out_indices, out_values);
        });
    });
}

// out[col] = sum over the compressed column of values[ix] * rowvec[indices[ix]]: SpMV's float32 kind on the CSC
// arrays (double product, float accumulator, as :659), or its no-values kind (:680)
extern "C" int mxd_rowvec_by_csc(int ncols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                 const double *values, const float *rowvec, float *out, void *stream)
{
    MX_REQUIRE(ncols >= 0, "mxd_rowvec_by_csc: negative size");
    if (ncols == 0) return 0;
    MX_REQUIRE(indptr && out, "mxd_rowvec_by_csc: null pointer");
    return mx::spmv_launch(ncols, nnz, indptr, indices, values, rowvec, values ? MX_F32 : mx::SPMV_F32_PATTERN, out,
                           mx::as_stream(stream));
}

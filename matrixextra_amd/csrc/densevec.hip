// densevec.hip — dense matrix * sparseVector and COO * dense matrix, for gfx950.
//
// Replaces:
//   multiply_elemwise_dense_by_svec_template<>  src/operators.cpp:3699-4303  (numeric, integer, logical, float32)
//   multiply_coo_by_dense<>                     src/operators.cpp:721-770    (the four products and the logical and)
// (the first is a serial loop that push_backs cell after cell).
//
// X is nrows x ncols, column-major, of kind DK (0 double, 1 float32, 2 R integer, 3 R logical, as in cscdense.hip).
// The vector (1-based positions vi[0..nv), f64 values vx, length L) is scattered once into a position map
// pos[0..L): the entry index, or -1.  No kernel searches vi after that.
//   routes A, D (dense result)  one thread per cell f of the column-major output: p = pos[f mod L]; stored ->
//                               the product, else the fill under keep_na (:3725-3743), else 0.  One store per cell,
//                               X is read only where the result depends on it, and nothing races.
//   routes B, C (CSR result)    count: one thread per row, lanes along consecutive rows (the contiguous direction of
//                               X): ncols when pos[r mod L] is stored, else under keep_na the row's special cells.
//                               scan:  the shared finish_count (64-bit total, refused above INT32_MAX).
//                               fill:  tiles of DSV_T rows x DSV_T columns go through LDS: X is read along the rows
//                               of the tile (lanes = consecutive rows, coalesced), the products are written along the
//                               columns (lanes = consecutive entries of one output row, coalesced).  The tile's row
//                               stride is DSV_T + 1 doubles, so that the transposed 8-byte stores (16-lane groups, 32
//                               banks) and the row-wise ds_read_b64 (32-lane groups, 64 banks) are both conflict-free.
//                               Rows the vector does not store write their few special cells from a second kernel,
//                               one thread per row, in column order.
// Every write position comes from the scanned counts and every row / column / cell index is checked against its
// bound, so that nothing is read or written out of bounds whatever the input.
#include "mx_dispatch.h"
#include "mx_workspace.h"

namespace mx {

constexpr int DSV_BLOCK = 256;
constexpr int DSV_T = 64;                       // tile edge: one wave of rows, one wave of columns
constexpr int DSV_LD = DSV_T + 1;               // LDS row stride in doubles
constexpr int DSV_WAVES = DSV_BLOCK / MX_WAVE;
static_assert(DSV_T == MX_WAVE, "a wave reads one column of the tile and writes one row of it");

template <int DK> struct DsvDense { using T = int32_t; };
template <> struct DsvDense<0> { using T = double; };
template <> struct DsvDense<1> { using T = float; };

__device__ __forceinline__ double dsv_nan() { return __longlong_as_double(0x7FF8000000000000LL); }   // C's NAN

// a cell that the vector does not cover and that keep_NAs still writes (:3729-3742, :3831-3872)
template <int DK>
__device__ __forceinline__ bool dsv_special(typename DsvDense<DK>::T x)
{
    if constexpr (DK <= 1) return isnan(x) || isinf(x);
    else return x == MX_NA_INT;
}

// its value: an f64 NaN unchanged, an f64 +-Inf and every float32 special as C's NAN, NA_INTEGER as NA_real_
template <int DK>
__device__ __forceinline__ double dsv_fill(typename DsvDense<DK>::T x)
{
    if constexpr (DK == 0) return isnan(x) ? x : dsv_nan();
    else if constexpr (DK == 1) return dsv_nan();
    else return na_real();
}

// MODE of a stored cell's product
constexpr int DSV_PLAIN = 0;      // x * val; NA_INTEGER -> C's NAN                     (routes A, D, B / C with keep_NAs, C)
constexpr int DSV_NA_REAL = 1;    // integer / logical, route B without keep_NAs: NA_INTEGER -> NA_real_   (:3803)
constexpr int DSV_DAXPY = 2;      // f64, route C without keep_NAs: 0.0 + val * x, and +0.0 when val == 0  (:4012)

template <int DK, int MODE>
__device__ __forceinline__ double dsv_product(typename DsvDense<DK>::T x, double val)
{
    if constexpr (DK == 0) {
        if constexpr (MODE == DSV_DAXPY) return val == 0.0 ? 0.0 : 0.0 + val * x;
        else return x * val;
    } else if constexpr (DK == 1) {
        return (double)x * val;
    } else {
        if (x == MX_NA_INT) return MODE == DSV_NA_REAL ? na_real() : dsv_nan();
        return (double)x * val;
    }
}

// pos[vi[k] - 1] = k; a repeated position keeps its first entry (FIRST: the lower_bound skip of :3908-3912) or its
// last (the overwriting scatter of :3747-3751); pos starts as all ones.  Positions outside 1..length are skipped.
template <bool FIRST>
__global__ __launch_bounds__(DSV_BLOCK)
void dsv_map_kernel(const int32_t *__restrict__ vi, int64_t nv, int length, int32_t *__restrict__ pos)
{
    const int64_t k = (int64_t)blockIdx.x * DSV_BLOCK + threadIdx.x;
    if (k >= nv) return;
    const int64_t t = (int64_t)vi[k] - 1;
    if (t < 0 || t >= length) return;
    if constexpr (FIRST) atomicMin((unsigned int *)pos + t, (unsigned int)k);
    else atomicMax(pos + t, (int)k);
}

// routes A and D
template <int DK>
__global__ __launch_bounds__(DSV_BLOCK)
void dsv_dense_kernel(int64_t F, const void *__restrict__ dense, const int32_t *__restrict__ pos,
                      const double *__restrict__ vx, int length, int keep_na, double *__restrict__ out)
{
    using T = typename DsvDense<DK>::T;
    const int64_t f = (int64_t)blockIdx.x * DSV_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int p = pos[f % length];
    double v = 0.0;
    if (p >= 0) {
        v = dsv_product<DK, DSV_PLAIN>(((const T *)dense)[f], vx[p]);
    } else if (keep_na) {
        const T x = ((const T *)dense)[f];
        if (dsv_special<DK>(x)) v = dsv_fill<DK>(x);
    }
    out[f] = v;
}

// routes B and C: entries of each row
template <int DK>
__global__ __launch_bounds__(DSV_BLOCK)
void dsv_count_kernel(int nrows, int ncols, const void *__restrict__ dense, const int32_t *__restrict__ pos,
                      int length, int keep_na, int32_t *__restrict__ counts)
{
    using T = typename DsvDense<DK>::T;
    const int64_t r = (int64_t)blockIdx.x * DSV_BLOCK + threadIdx.x;
    if (r >= nrows) return;
    int cnt = 0;
    if (pos[r % length] >= 0) {
        cnt = ncols;
    } else if (keep_na) {
        const T *x = (const T *)dense + r;
        for (int c = 0; c < ncols; c++) cnt += dsv_special<DK>(x[(int64_t)c * nrows]);
    }
    counts[r] = cnt;
}

// routes B and C: the rows that the vector stores, one DSV_T x DSV_T tile a block
template <int DK, int MODE>
__global__ __launch_bounds__(DSV_BLOCK)
void dsv_fill_kernel(int nrows, int ncols, int col_tiles, const void *__restrict__ dense,
                     const int32_t *__restrict__ pos, const double *__restrict__ vx, int length,
                     const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                     double *__restrict__ out_values)
{
    using T = typename DsvDense<DK>::T;
    __shared__ double s_tile[DSV_T * DSV_LD];
    __shared__ int32_t s_dst[DSV_T];            // where the row's entries start, or -1: not a stored row
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const int64_t r0 = (int64_t)(blockIdx.x / (unsigned)col_tiles) * DSV_T;
    const int c0 = (int)(blockIdx.x % (unsigned)col_tiles) * DSV_T;

    // lane = row of the tile
    const int64_t r = r0 + lane;
    int p = -1;
    if (r < nrows) p = pos[r % length];
    if (wave == 0) s_dst[lane] = p >= 0 ? out_indptr[r] : -1;
    if (p >= 0) {
        const double val = vx[p];
        const T *x = (const T *)dense + r;
        T xv[DSV_T / DSV_WAVES];                 // all loads of the lane issued before the first use
#pragma unroll
        for (int k = 0; k < DSV_T / DSV_WAVES; k++) {
            const int c = c0 + wave + k * DSV_WAVES;
            xv[k] = c < ncols ? x[(int64_t)c * nrows] : T{};
        }
#pragma unroll
        for (int k = 0; k < DSV_T / DSV_WAVES; k++)
            s_tile[lane * DSV_LD + wave + k * DSV_WAVES] = dsv_product<DK, MODE>(xv[k], val);
    }
    __syncthreads();

    // lane = column of the tile
    const int c = c0 + lane;
    if (c >= ncols) return;
#pragma unroll 4
    for (int lr = wave; lr < DSV_T; lr += DSV_WAVES) {
        const int dst = s_dst[lr];
        if (dst < 0) continue;
        out_indices[(int64_t)dst + c] = c;
        out_values[(int64_t)dst + c] = s_tile[lr * DSV_LD + lane];
    }
}

// routes B and C under keep_na: the special cells of the rows that the vector does not store, in column order
template <int DK>
__global__ __launch_bounds__(DSV_BLOCK)
void dsv_fill_special_kernel(int nrows, int ncols, const void *__restrict__ dense, const int32_t *__restrict__ pos,
                             int length, const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                             double *__restrict__ out_values)
{
    using T = typename DsvDense<DK>::T;
    const int64_t r = (int64_t)blockIdx.x * DSV_BLOCK + threadIdx.x;
    if (r >= nrows) return;
    int64_t o = out_indptr[r];
    const int64_t end = out_indptr[r + 1];
    if (o >= end || pos[r % length] >= 0) return;
    const T *x = (const T *)dense + r;
    for (int c = 0; c < ncols && o < end; c++) {
        const T v = x[(int64_t)c * nrows];
        if (dsv_special<DK>(v)) {
            out_indices[o] = c;
            out_values[o] = dsv_fill<DK>(v);
            o++;
        }
    }
}

// kind 0-3: out f64 = xx * X[ii + jj * nrows] (:736-754), NA_INTEGER / NA_LOGICAL -> NA_real_, a logical X read as
// bool; kind 4: R's three-valued and of R logicals (:759-760).  An entry outside the matrix gives NA and reads nothing.
template <int KIND>
__global__ __launch_bounds__(DSV_BLOCK)
void coo_by_dense_kernel(int64_t nnz, const int32_t *__restrict__ ii, const int32_t *__restrict__ jj,
                         const void *__restrict__ xx, const void *__restrict__ dense, int nrows, int ncols,
                         void *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * DSV_BLOCK + threadIdx.x;
    if (k >= nnz) return;
    const int i = ii[k], j = jj[k];
    const bool inside = i >= 0 && i < nrows && j >= 0 && j < ncols;
    const int64_t f = (int64_t)i + (int64_t)j * nrows;
    if constexpr (KIND == 4) {
        ((int32_t *)out)[k] = inside ? r_logical_and(((const int32_t *)xx)[k], ((const int32_t *)dense)[f]) : MX_NA_INT;
    } else {
        double v = na_real();
        if (inside) {
            const double x = ((const double *)xx)[k];
            if constexpr (KIND == 0) v = x * ((const double *)dense)[f];
            else if constexpr (KIND == 1) v = x * ((const float *)dense)[f];
            else {
                const int32_t d = ((const int32_t *)dense)[f];
                if (d != MX_NA_INT) v = KIND == 2 ? x * d : x * (double)(d != 0);
            }
        }
        ((double *)out)[k] = v;
    }
}

using dsv_kinds = int_list<0, 1, 2, 3>;
using coo_dense_kinds = int_list<0, 1, 2, 3, 4>;

struct DsvLayout {
    WsCursor c;
    int32_t *pos, *counts;                  // position map: `length` entries; counts per row
    size_t bytes = c.bytes();
    DsvLayout(const void *ws, int nrows, int length) : c(ws), pos(c.take_i32(length)), counts(c.take_counts(nrows)) {}
};

static int dsv_check(const char *what, int nrows, int ncols, int64_t nv, int length, int kind)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nv >= 0 && nv <= INT_MAX && kind >= 0 && kind <= 3, "%s: bad arguments",
               what);
    MX_REQUIRE((int64_t)nrows * ncols == 0 || length > 0, "%s: the vector has no length", what);
    return 0;
}

static int dsv_build_map(const int32_t *vi, int64_t nv, int length, bool first, int32_t *pos, hipStream_t st)
{
    MX_HIP(hipMemsetAsync(pos, 0xFF, sizeof(int32_t) * (size_t)length, st));
    if (nv == 0) return 0;
    const dim3 grid((unsigned)ceil_div(nv, DSV_BLOCK)), block(DSV_BLOCK);
    if (first) hipLaunchKernelGGL(dsv_map_kernel<true>, grid, block, 0, st, vi, nv, length, pos);
    else hipLaunchKernelGGL(dsv_map_kernel<false>, grid, block, 0, st, vi, nv, length, pos);
    MX_LAUNCH_CHECK();
    return 0;
}

}  // namespace mx

extern "C" size_t mxd_dense_by_svec_workspace_bytes(int nrows, int length)
{
    return mx::DsvLayout(nullptr, nrows, length).bytes;
}

extern "C" int mxd_dense_by_svec_dense(int nrows, int ncols, const void *dense_colmajor, int dense_kind,
                                       const int32_t *vi_base1, int64_t nv, const double *vx, int length,
                                       int keep_na, void *workspace, double *out_colmajor, void *stream)
{
    if (mx::dsv_check("mxd_dense_by_svec_dense", nrows, ncols, nv, length, dense_kind)) return 1;
    const int64_t F = (int64_t)nrows * (int64_t)ncols;
    if (F == 0) return 0;
    MX_REQUIRE(workspace && dense_colmajor && out_colmajor && (nv == 0 || (vi_base1 && vx)),
               "mxd_dense_by_svec_dense: null pointer");
    MX_REQUIRE(mx::ceil_div(F, mx::DSV_BLOCK) <= (int64_t)UINT_MAX, "mxd_dense_by_svec_dense: dense operand too large");
    hipStream_t st = mx::as_stream(stream);
    int32_t *pos = mx::DsvLayout(workspace, nrows, length).pos;
    if (mx::dsv_build_map(vi_base1, nv, length, false, pos, st)) return 1;
    return mx::dispatch_int(mx::dsv_kinds{}, "mxd_dense_by_svec_dense", "dense kind", dense_kind, [&](auto dk) {
        hipLaunchKernelGGL(mx::dsv_dense_kernel<dk()>, dim3((unsigned)mx::ceil_div(F, mx::DSV_BLOCK)),
                           dim3(mx::DSV_BLOCK), 0, st, F, dense_colmajor, pos, vx, length, keep_na, out_colmajor);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int mxd_dense_by_svec_count(int nrows, int ncols, const void *dense_colmajor, int dense_kind,
                                       const int32_t *vi_base1, int64_t nv, int length, int keep_na, void *workspace,
                                       int32_t *out_indptr, int64_t *nnz_out_host, void *stream)
{
    if (mx::dsv_check("mxd_dense_by_svec_count", nrows, ncols, nv, length, dense_kind)) return 1;
    MX_REQUIRE(workspace && out_indptr && nnz_out_host, "mxd_dense_by_svec_count: null pointer");
    MX_REQUIRE(nrows == 0 || (length > 0 && length <= nrows && nrows % length == 0),
               "mxd_dense_by_svec_count: the vector's length must divide the number of rows");
    MX_REQUIRE(nrows == 0 || ((nv == 0 || vi_base1) && (!keep_na || ncols == 0 || dense_colmajor)),
               "mxd_dense_by_svec_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    *nnz_out_host = 0;
    const mx::DsvLayout L(workspace, nrows, length);
    if (nrows > 0) {
        int32_t *pos = L.pos;
        if (mx::dsv_build_map(vi_base1, nv, length, true, pos, st)) return 1;
        const int rc = mx::dispatch_int(mx::dsv_kinds{}, "mxd_dense_by_svec_count", "dense kind", dense_kind,
                                        [&](auto dk) {
            hipLaunchKernelGGL(mx::dsv_count_kernel<dk()>, dim3((unsigned)mx::ceil_div(nrows, mx::DSV_BLOCK)),
                               dim3(mx::DSV_BLOCK), 0, st, nrows, ncols, dense_colmajor, pos, length, keep_na,
                               L.counts);
            MX_LAUNCH_CHECK();
            return 0;
        });
        if (rc) return rc;
    }
    // the 64-bit total is read back (one synchronise) and refused above INT_MAX before any output exists
    return mx::finish_count(nrows, L.counts, out_indptr, nnz_out_host, st);
}

extern "C" int mxd_dense_by_svec_fill(int nrows, int ncols, const void *dense_colmajor, int dense_kind,
                                      const double *vx, int length, int keep_na, const void *workspace,
                                      const int32_t *out_indptr, int32_t *out_indices, double *out_values,
                                      void *stream)
{
    if (mx::dsv_check("mxd_dense_by_svec_fill", nrows, ncols, 0, length, dense_kind)) return 1;
    if (nrows == 0 || ncols == 0) return 0;
    MX_REQUIRE(length <= nrows && nrows % length == 0,
               "mxd_dense_by_svec_fill: the vector's length must divide the number of rows");
    MX_REQUIRE(workspace && dense_colmajor && out_indptr && out_indices && out_values,
               "mxd_dense_by_svec_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const int32_t *pos = mx::DsvLayout(workspace, nrows, length).pos;
    const int col_tiles = (int)mx::ceil_div(ncols, mx::DSV_T);
    const int64_t tiles = mx::ceil_div(nrows, mx::DSV_T) * col_tiles;
    MX_REQUIRE(tiles <= (int64_t)UINT_MAX, "mxd_dense_by_svec_fill: dense operand too large");
    // the product of a stored cell (densevec.hip, dsv_product): route B is length == nrows, route C a shorter vector
    const int mode = keep_na ? mx::DSV_PLAIN
                             : length == nrows ? (dense_kind >= 2 ? mx::DSV_NA_REAL : mx::DSV_PLAIN)
                                               : (dense_kind == 0 ? mx::DSV_DAXPY : mx::DSV_PLAIN);
    int rc = mx::dispatch_int(mx::dsv_kinds{}, "mxd_dense_by_svec_fill", "dense kind", dense_kind, [&](auto dk) {
        return mx::dispatch_int(mx::int_list<mx::DSV_PLAIN, mx::DSV_NA_REAL, mx::DSV_DAXPY>{},
                                "mxd_dense_by_svec_fill", "product mode", mode, [&](auto md) {
            hipLaunchKernelGGL((mx::dsv_fill_kernel<dk(), md()>), dim3((unsigned)tiles), dim3(mx::DSV_BLOCK), 0, st,
                               nrows, ncols, col_tiles, dense_colmajor, pos, vx, length, out_indptr, out_indices,
                               out_values);
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
    if (rc || !keep_na) return rc;
    return mx::dispatch_int(mx::dsv_kinds{}, "mxd_dense_by_svec_fill", "dense kind", dense_kind, [&](auto dk) {
        hipLaunchKernelGGL(mx::dsv_fill_special_kernel<dk()>, dim3((unsigned)mx::ceil_div(nrows, mx::DSV_BLOCK)),
                           dim3(mx::DSV_BLOCK), 0, st, nrows, ncols, dense_colmajor, pos, length, out_indptr,
                           out_indices, out_values);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int mxd_coo_by_dense(int64_t nnz, const int32_t *ii, const int32_t *jj, const void *xx,
                                const void *dense_colmajor, int nrows, int ncols, int kind, void *out, void *stream)
{
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX && nrows >= 0 && ncols >= 0 && kind >= 0 && kind <= 4,
               "mxd_coo_by_dense: bad arguments");
    if (nnz == 0) return 0;
    MX_REQUIRE(ii && jj && xx && out && ((int64_t)nrows * ncols == 0 || dense_colmajor),
               "mxd_coo_by_dense: null pointer");
    hipStream_t st = mx::as_stream(stream);
    return mx::dispatch_int(mx::coo_dense_kinds{}, "mxd_coo_by_dense", "kind", kind, [&](auto kd) {
        hipLaunchKernelGGL(mx::coo_by_dense_kernel<kd()>, dim3((unsigned)mx::ceil_div(nnz, mx::DSV_BLOCK)),
                           dim3(mx::DSV_BLOCK), 0, st, nnz, ii, jj, xx, dense_colmajor, nrows, ncols, out);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

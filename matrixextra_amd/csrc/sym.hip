// sym.hip — device level of the structured-matrix family (include/mxgpu_sym.h): the general CSR of a symmetric CSR
// that stores one triangle, of a unit-triangular CSR, and the triangle check.  Copies only.
//
// Symmetric expansion.  Row r of the result is the stored row r and the stored column r without its (r, r) entries.
// The column comes from the column order of the pattern (transpose.hip: perm + colptr, stable, rows ascending inside
// a column), so with a valid triangle the (r, r) entries of column r are its LAST d (uplo U: every other row of the
// column is < r) or its FIRST d (uplo L: every other row is > r), and the mirrored segment is the rest of the list in
// the order the specification asks for.  d is not kept: the fill has rowlen + collen - outlen from the three pointers.
// The row of a gathered entry is read from the expanded row ids (what mxd_csr_to_coo gives, 4 B per entry of
// workspace): one load at the position the value is gathered from, instead of a search of indptr per entry.  The count
// pass writes them, since it walks every row anyway: a coalesced store per entry and no search at all.
#include "mx_dispatch.h"
#include "mx_workspace.h"
#include "../../include/mxgpu_reduce.h"      // mxd_csr_column_order
#include "../../include/mxgpu_sym.h"

namespace mx {

constexpr int SYM_BLOCK = 256;

// outside the triangle: uplo U stores c >= r, uplo L c <= r; strict: the diagonal is outside as well
__device__ __forceinline__ bool sym_outside(int r, int c, int lower, int strict)
{
    return (lower ? c > r : c < r) || (strict && c == r);
}

// G lanes per row: entries outside the triangle, added to *outside (an integer counter)
template <int G>
__global__ __launch_bounds__(SYM_BLOCK)
void sym_check_kernel(int n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t nnz,
                      int lower, int strict, unsigned long long *__restrict__ outside)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int gl = lane_id() & (G - 1);
    int bad = 0;
    if (r < n) {
        const RowBounds rb = row_bounds(indptr[r], indptr[r + 1], nnz);
        for (int64_t e = gl; e < rb.len; e += G) bad += sym_outside((int)r, indices[rb.start + e], lower, strict);
    }
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) bad += __shfl_xor(bad, off, MX_WAVE);
    if (lane_id() == 0 && bad) atomicAdd(outside, (unsigned long long)bad);
}

// G lanes per row: len[r] = rowlen + collen - d[r], d[r] the stored (r, r); wrong-triangle entries added to *outside;
// rowid[e] = r for every entry e of the row
template <int G>
__global__ __launch_bounds__(SYM_BLOCK)
void sym_count_kernel(int n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t nnz,
                      int lower, const int32_t *__restrict__ colptr, int32_t *__restrict__ len,
                      int32_t *__restrict__ rowid, unsigned long long *__restrict__ outside)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int gl = lane_id() & (G - 1);
    const bool live = r < n;
    RowBounds rb = {0, 0};
    if (live) rb = row_bounds(indptr[r], indptr[r + 1], nnz);
    int d = 0, bad = 0;
    for (int64_t e = gl; e < rb.len; e += G) {
        const int c = indices[rb.start + e];
        rowid[rb.start + e] = (int)r;
        d += c == (int)r;
        bad += sym_outside((int)r, c, lower, 0);
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, G);
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) bad += __shfl_xor(bad, off, MX_WAVE);
    if (lane_id() == 0 && bad) atomicAdd(outside, (unsigned long long)bad);
    if (live && gl == 0) {
        const RowBounds cb = row_bounds(colptr[r], colptr[r + 1], nnz);
        len[r] = (int32_t)(rb.len + cb.len - d);          // <= 2 nnz; the scan's int64 total catches an overflow
    }
}

// G lanes per output row: the mirrored segment gathered through perm, the stored row copied
template <int G, typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(SYM_BLOCK)
void sym_fill_kernel(int n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                     const VT *__restrict__ values, int64_t nnz, int lower, const int32_t *__restrict__ colptr,
                     const int32_t *__restrict__ perm, const int32_t *__restrict__ rowid,
                     const int32_t *__restrict__ out_indptr, int64_t nnz_out, int32_t *__restrict__ out_indices,
                     VT *__restrict__ out_values)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int gl = lane_id() & (G - 1);
    if (r >= n) return;
    const RowBounds rb = row_bounds(indptr[r], indptr[r + 1], nnz);
    const RowBounds cb = row_bounds(colptr[r], colptr[r + 1], nnz);
    const RowBounds ob = row_bounds(out_indptr[r], out_indptr[r + 1], nnz_out);
    int64_t d = rb.len + cb.len - ob.len;                                 // the stored (r, r) entries of column r
    d = d < 0 ? 0 : d > cb.len ? cb.len : d;
    const int64_t mlen = cb.len - d, oend = ob.start + ob.len;
    const int64_t q0 = cb.start + (lower ? d : 0);                        // U: the diagonal is last; L: first
    const int64_t m_out = ob.start + (lower ? rb.len : 0), s_out = ob.start + (lower ? 0 : mlen);
    for (int64_t k = gl; k < mlen; k += G) {
        const int64_t o = m_out + k;
        int64_t p = perm[q0 + k];
        p = p < 0 ? 0 : p >= nnz ? nnz - 1 : p;
        if (o < oend) {
            out_indices[o] = rowid[p];
            if constexpr (HAS_VALUES) out_values[o] = values[p];
        }
    }
    for (int64_t k = gl; k < rb.len; k += G) {
        const int64_t o = s_out + k;
        if (o < oend) {
            out_indices[o] = indices[rb.start + k];
            if constexpr (HAS_VALUES) out_values[o] = values[rb.start + k];
        }
    }
}

template <typename VT> __device__ __forceinline__ VT sym_one();
template <> __device__ __forceinline__ double sym_one<double>() { return 1.0; }
template <> __device__ __forceinline__ int32_t sym_one<int32_t>() { return 1; }

// G lanes per row r <= n: out_indptr[r] = indptr[r] + r; rows r < n copy their entries and gain (r, r) = 1
template <int G, typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(SYM_BLOCK)
void unit_tri_kernel(int n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                     const VT *__restrict__ values, int64_t nnz, int lower, int32_t *__restrict__ out_indptr,
                     int32_t *__restrict__ out_indices, VT *__restrict__ out_values)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int gl = lane_id() & (G - 1);
    if (r > n) return;
    if (r == n) {
        if (gl == 0) out_indptr[n] = (int32_t)(nnz + n);
        return;
    }
    const RowBounds rb = row_bounds(indptr[r], indptr[r + 1], nnz);
    const int64_t o0 = rb.start + r;                                      // <= nnz + n - 1 - rb.len
    if (gl == 0) {
        out_indptr[r] = (int32_t)o0;
        const int64_t od = lower ? o0 + rb.len : o0;
        out_indices[od] = (int32_t)r;
        if constexpr (HAS_VALUES) out_values[od] = sym_one<VT>();
    }
    const int64_t s_out = o0 + (lower ? 0 : 1);
    for (int64_t k = gl; k < rb.len; k += G) {
        out_indices[s_out + k] = indices[rb.start + k];
        if constexpr (HAS_VALUES) out_values[s_out + k] = values[rb.start + k];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------
// counter (16 B) | colptr[n + 1] | perm[nnz] | rowid[nnz] | the column order's own workspace | len[n] + scan
struct SymLayout {
    WsCursor c;
    int64_t n, nnz;
    unsigned long long *outside = c.take<unsigned long long>(16);
    int32_t *colptr = c.take_i32(n + 1), *perm = c.take_i32(nnz), *rowid = c.take_i32(nnz);
    void *order_ws = c.take((mxd_csr_transpose_workspace_bytes(nnz) + 15) & ~(size_t)15);
    int32_t *len = c.take_counts(n);
    size_t bytes = c.bytes();
    SymLayout(const void *ws, int64_t n_, int64_t nnz_) : c(ws), n(n_ > 0 ? n_ : 0), nnz(nnz_ > 0 ? nnz_ : 0) {}
};

static int check_uplo(const char *what, int uplo)
{
    MX_REQUIRE(uplo == MX_UPLO_UPPER || uplo == MX_UPLO_LOWER, "%s: uplo must be MX_UPLO_UPPER or MX_UPLO_LOWER, got %d",
               what, uplo);
    return 0;
}

static int triangle_check(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int uplo, int strict,
                          void *workspace, int64_t *outside_host, hipStream_t st)
{
    MX_REQUIRE(n >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_triangle_check: bad size");
    if (check_uplo("mxd_csr_triangle_check", uplo)) return 1;
    MX_REQUIRE(outside_host, "mxd_csr_triangle_check: null result pointer");
    *outside_host = 0;
    if (n == 0 || nnz == 0) return 0;
    MX_REQUIRE(indptr && indices && workspace, "mxd_csr_triangle_check: null pointer");
    unsigned long long *counter = (unsigned long long *)workspace;
    MX_HIP(hipMemsetAsync(counter, 0, sizeof(*counter), st));
    const int G = pick_group((double)nnz / (double)n);
    const int rc = launch_rows(lane_groups{}, "sym_check", G, n, SYM_BLOCK, [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((sym_check_kernel<g()>), grid, block, 0, st, n, indptr, indices, nnz,
                           uplo == MX_UPLO_LOWER, strict ? 1 : 0, counter);
    });
    if (rc) return rc;
    unsigned long long outside = 0;
    MX_HIP(hipMemcpyAsync(&outside, counter, sizeof(outside), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    *outside_host = (int64_t)outside;
    return 0;
}

static int sym_count(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int uplo, int32_t *out_indptr,
                     void *workspace, int64_t *nnz_out_host, hipStream_t st)
{
    const char *what = "mxd_csr_symmetric_to_general_count";
    MX_REQUIRE(n >= 0 && nnz >= 0 && nnz <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(n > 0 || nnz == 0, "%s: entries without rows", what);
    if (check_uplo(what, uplo)) return 1;
    MX_REQUIRE(out_indptr && nnz_out_host, "%s: null pointer", what);
    *nnz_out_host = 0;
    if (n == 0 || nnz == 0) {
        MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)n + 1), st));
        return 0;
    }
    MX_REQUIRE(indptr && indices && workspace, "%s: null pointer", what);
    const SymLayout L(workspace, n, nnz);
    if (mxd_csr_column_order(n, n, indptr, indices, nnz, L.perm, L.colptr, L.order_ws, st)) return 1;
    MX_HIP(hipMemsetAsync(L.outside, 0, sizeof(*L.outside), st));
    const int G = pick_group((double)nnz / (double)n);
    const int rc = launch_rows(lane_groups{}, "sym_count", G, n, SYM_BLOCK, [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((sym_count_kernel<g()>), grid, block, 0, st, n, indptr, indices, nnz,
                           uplo == MX_UPLO_LOWER, L.colptr, L.len, L.rowid, L.outside);
    });
    if (rc) return rc;
    unsigned long long outside = 0;
    MX_HIP(hipMemcpyAsync(&outside, L.outside, sizeof(outside), hipMemcpyDeviceToHost, st));
    int64_t total = 0;
    const int scan_rc = finish_count(n, L.len, out_indptr, &total, st);   // synchronises: `outside` has arrived too
    if (scan_rc) (void)hipStreamSynchronize(st);                          // (a scan that failed to launch has not)
    MX_REQUIRE(!outside, "%s: %llu entr%s outside the stored triangle (uplo = \"%s\")", what, outside,
               outside == 1 ? "y lies" : "ies lie", uplo == MX_UPLO_LOWER ? "L" : "U");
    if (scan_rc) return scan_rc;
    *nnz_out_host = total;
    return 0;
}

static int sym_fill(int n, const int32_t *indptr, const int32_t *indices, const void *values, int value_dtype,
                    int64_t nnz, int uplo, const int32_t *out_indptr, int64_t nnz_out, int32_t *out_indices,
                    void *out_values, const void *workspace, hipStream_t st)
{
    const char *what = "mxd_csr_symmetric_to_general_fill";
    MX_REQUIRE(n >= 0 && nnz >= 0 && nnz <= INT_MAX && nnz_out >= 0 && nnz_out <= INT_MAX, "%s: bad size", what);
    if (check_uplo(what, uplo)) return 1;
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "%s: unsupported value dtype %d", what, value_dtype);
    if (n == 0 || nnz == 0 || nnz_out == 0) return 0;
    MX_REQUIRE(indptr && indices && out_indptr && out_indices && workspace, "%s: null pointer", what);
    MX_REQUIRE(value_dtype == MX_NONE || (values && out_values), "%s: null values pointer", what);
    const SymLayout L(workspace, n, nnz);
    const int G = pick_group((double)nnz_out / (double)n);
    return dispatch_values(what, value_dtype, [&](auto vk) {
        using VT = typename decltype(vk)::VT;
        return launch_rows(lane_groups{}, "sym_fill", G, n, SYM_BLOCK, [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((sym_fill_kernel<g(), VT, vk.has_values>), grid, block, 0, st, n, indptr, indices,
                               (const VT *)values, nnz, uplo == MX_UPLO_LOWER, L.colptr, L.perm, L.rowid, out_indptr,
                               nnz_out, out_indices, (VT *)out_values);
        });
    });
}

static int unit_triangular(int n, const int32_t *indptr, const int32_t *indices, const void *values, int value_dtype,
                           int64_t nnz, int uplo, int32_t *out_indptr, int32_t *out_indices, void *out_values,
                           hipStream_t st)
{
    const char *what = "mxd_csr_unit_triangular_to_general";
    MX_REQUIRE(n >= 0 && nnz >= 0 && nnz <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(n > 0 || nnz == 0, "%s: entries without rows", what);
    MX_REQUIRE(nnz + (int64_t)n <= INT_MAX, "%s: result has %lld entries: exceeds R's int32 index range", what,
               (long long)(nnz + n));
    if (check_uplo(what, uplo)) return 1;
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "%s: unsupported value dtype %d", what, value_dtype);
    MX_REQUIRE(out_indptr && (n == 0 || (indptr && out_indices)) && (nnz == 0 || indices), "%s: null pointer", what);
    MX_REQUIRE(value_dtype == MX_NONE || n == 0 || (out_values && (nnz == 0 || values)), "%s: null values pointer", what);
    const int G = pick_group((double)(nnz + n) / (double)(n > 0 ? n : 1));
    return dispatch_values(what, value_dtype, [&](auto vk) {
        using VT = typename decltype(vk)::VT;
        return launch_rows(lane_groups{}, "unit_tri", G, (int64_t)n + 1, SYM_BLOCK, [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((unit_tri_kernel<g(), VT, vk.has_values>), grid, block, 0, st, n, indptr, indices,
                               (const VT *)values, nnz, uplo == MX_UPLO_LOWER, out_indptr, out_indices,
                               (VT *)out_values);
        });
    });
}

}  // namespace mx

extern "C" size_t mxd_csr_sym_workspace_bytes(int n, int64_t nnz) { return mx::SymLayout(nullptr, n, nnz).bytes; }

extern "C" int mxd_csr_triangle_check(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz, int uplo,
                                      int strict, void *workspace, int64_t *outside_host, void *stream)
{
    return mx::triangle_check(n, indptr, indices, nnz, uplo, strict, workspace, outside_host, mx::as_stream(stream));
}

extern "C" int mxd_csr_symmetric_to_general_count(int n, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                                                  int uplo, int32_t *out_indptr, void *workspace,
                                                  int64_t *nnz_out_host, void *stream)
{
    return mx::sym_count(n, indptr, indices, nnz, uplo, out_indptr, workspace, nnz_out_host, mx::as_stream(stream));
}

extern "C" int mxd_csr_symmetric_to_general_fill(int n, const int32_t *indptr, const int32_t *indices,
                                                 const void *values, int value_dtype, int64_t nnz, int uplo,
                                                 const int32_t *out_indptr, int64_t nnz_out, int32_t *out_indices,
                                                 void *out_values, const void *workspace, void *stream)
{
    return mx::sym_fill(n, indptr, indices, values, value_dtype, nnz, uplo, out_indptr, nnz_out, out_indices,
                        out_values, workspace, mx::as_stream(stream));
}

extern "C" int mxd_csr_unit_triangular_to_general(int n, const int32_t *indptr, const int32_t *indices,
                                                  const void *values, int value_dtype, int64_t nnz, int uplo,
                                                  int32_t *out_indptr, int32_t *out_indices, void *out_values,
                                                  void *stream)
{
    return mx::unit_triangular(n, indptr, indices, values, value_dtype, nnz, uplo, out_indptr, out_indices, out_values,
                               mx::as_stream(stream));
}

// compact.hip — stable compaction of sparse entries by a keep rule, and the index validation reduction.
//
// Replaces:
//   remove_zero_valued_csr<>           src/misc.cpp:553-666   (CSR, and CSC run on (p, i))
//   remove_zero_valued_coo<>           src/misc.cpp:701-789
//   remove_zero_valued_svec<>          src/misc.cpp:824-924
//   rebuild_indptr_after_filter        src/misc.cpp:1099-1116 (and the x[mask] / j[mask] of filterSparse,
//                                      R/utils.R:582-681)
//   check_valid_{csr,coo}_matrix, check_valid_svec   src/misc.cpp:970-1097
//
// Compaction is a tiled two-pass stream compaction over the entry arrays:
//   count  one workgroup per tile of CP_TILE entries reads the values (or the mask) only, evaluates the keep rule and
//          stores the tile's kept count; the shared scan (finish_count) turns the counts into tile offsets and reads
//          the total back to the host (8 bytes).
//   fill   the same tiles again: a wave ballot per round of 256 entries gives every kept entry its rank inside the
//          tile (64 masks + 64 offsets in LDS), and kept entries are written in input order.  For a CSR / CSC, every
//          row whose old start p[r] lies inside the tile gets p'[r] = tile offset + in-tile rank of p[r]; the first
//          such row is found by one binary search of p per tile, and rows that start at nnz get the total.
// So each value is read twice, each index once and p once, and the work per tile does not depend on how the entries
// fall into rows: a 1 M-entry row is 256 tiles like any other 1 M entries.
// Loads of a tile are issued together ahead of their first use, in blocks hoisted out of any per-element condition
// (a wave-uniform condition per element still makes hipcc wait for each load in turn).
#include "mx_compact_tile.h"
#include "mx_workspace.h"

namespace mx {

template <int VB> struct CpValue { using T = int32_t; };     // 4: R logical / integer; 0: no values
template <> struct CpValue<8> { using T = double; };

// the keep rule (mx_keep_rule) on a loaded value / mask entry
template <int VB>
__device__ __forceinline__ bool cp_keep(int rule, typename CpValue<VB>::T v, int mk)
{
    if constexpr (VB == 8) {
        const bool nz = v != 0, nn = !isnan(v);          // NaN != 0: a NaN counts as non-zero
        return rule == MX_KEEP_MASK ? mk != 0 : rule == MX_KEEP_NONZERO ? nz
             : rule == MX_KEEP_NONZERO_NOT_NA ? nz && nn : nn;
    } else if constexpr (VB == 4) {
        const bool nz = v != 0, nn = v != MX_NA_INT;
        return rule == MX_KEEP_MASK ? mk != 0 : rule == MX_KEEP_NONZERO ? nz
             : rule == MX_KEEP_NONZERO_NOT_NA ? nz && nn : nn;
    } else {
        return mk != 0;                                   // no values: MX_KEEP_MASK only (NA keeps the entry)
    }
}

template <int VB>
__global__ __launch_bounds__(CP_BLOCK)
void compact_count_kernel(int64_t n, const void *__restrict__ values, int rule, const int32_t *__restrict__ mask,
                          int32_t *__restrict__ tile_counts)
{
    using T = typename CpValue<VB>::T;
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    T v[CP_ROUNDS];
    int mk[CP_ROUNDS];
    if (rule == MX_KEEP_MASK) {
        cp_load(mk, mask, base, n);
#pragma unroll
        for (int r = 0; r < CP_ROUNDS; r++) v[r] = T{};
    } else {
        if constexpr (VB != 0) cp_load(v, (const T *)values, base, n);
#pragma unroll
        for (int r = 0; r < CP_ROUNDS; r++) mk[r] = 0;
    }
    int cnt = 0;                                          // wave-uniform
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        const bool in = base + r * CP_BLOCK + threadIdx.x < n;
        cnt += __popcll(__ballot(in && cp_keep<VB>(rule, v[r], mk[r])));
    }
    cp_store_tile_count(cnt, tile_counts);
}

// tile_off[tile] = kept entries before the tile (exclusive scan of the counts).  Outputs may be null (not written).
template <int VB>
__global__ __launch_bounds__(CP_BLOCK)
void compact_fill_kernel(int64_t n, int64_t ntiles, const void *__restrict__ values, int rule,
                         const int32_t *__restrict__ mask, const int32_t *__restrict__ idx0,
                         const int32_t *__restrict__ idx1, int m, const int32_t *__restrict__ indptr,
                         const int32_t *__restrict__ tile_off, int32_t *__restrict__ out0,
                         int32_t *__restrict__ out1, void *__restrict__ out_values, int32_t *__restrict__ out_indptr)
{
    using T = typename CpValue<VB>::T;
    __shared__ CpTileRanks S;
    const int lane = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    const int64_t len = n - base < CP_TILE ? n - base : CP_TILE;

    T v[CP_ROUNDS];
    int mk[CP_ROUNDS], i0[CP_ROUNDS], i1[CP_ROUNDS];
    if constexpr (VB != 0) cp_load(v, (const T *)values, base, n);
    if (rule == MX_KEEP_MASK) cp_load(mk, mask, base, n);
    if (out0) cp_load(i0, idx0, base, n);
    if (out1) cp_load(i1, idx1, base, n);
    unsigned long long bal[CP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if constexpr (VB == 0) v[r] = T{};
        if (rule != MX_KEEP_MASK) mk[r] = 0;
        const bool in = base + r * CP_BLOCK + threadIdx.x < n;
        bal[r] = __ballot(in && cp_keep<VB>(rule, v[r], mk[r]));
    }
    cp_rank_tile(S, bal);
    const int64_t t0 = tile_off[blockIdx.x];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if (!((bal[r] >> lane) & 1)) continue;
        const int64_t q = t0 + cp_rank_of(S, r, bal[r]);
        if (out0) out0[q] = i0[r];
        if (out1) out1[q] = i1[r];
        if constexpr (VB != 0) {
            if (out_values) {
                T x = v[r];
                if (rule == MX_KEEP_MASK && mk[r] == MX_NA_INT) {
                    if constexpr (VB == 8) x = na_real(); // x[NA] is NA_real_ (R/utils.R:625)
                    else x = MX_NA_INT;
                }
                ((T *)out_values)[q] = x;
            }
        }
    }
    if (!out_indptr) return;
    // rows whose old start lies in [base, base + CP_TILE) — in the last tile, every row from base on, so that rows
    // starting at nnz get the total
    const bool last = (int64_t)blockIdx.x == ntiles - 1;
    const int64_t end = last ? INT64_MAX : base + CP_TILE;
    int r0 = 0;                                           // first r in [0, m] with indptr[r] >= base
    {
        int cnt = m + 1;
        while (cnt > 0) {
            const int step = cnt >> 1;
            if ((int64_t)indptr[r0 + step] < base) { r0 += step + 1; cnt -= step + 1; }
            else cnt = step;
        }
    }
    for (int64_t r = (int64_t)r0 + threadIdx.x; r <= m; r += CP_BLOCK) {
        const int64_t p = indptr[r];
        if (p >= end) break;                              // p is non-decreasing: later rows start later still
        if (p < base) continue;                           // only for a non-monotone p: never index LDS with it
        const int64_t qi = p - base;
        const int rank = qi >= len ? S.total : cp_rank_before(S, (int)qi);
        out_indptr[r] = (int32_t)(t0 + rank);
    }
}

// validation flags of idx[0..n) against [0, bound) and, when indptr is given, of indptr[0..nptr) (NA) and
// indptr[0..mono] (non-decreasing); one atomic OR per wave that found something
__global__ __launch_bounds__(CP_BLOCK)
void validate_kernel(const int32_t *__restrict__ idx, int64_t n, int bound, const int32_t *__restrict__ indptr,
                     int64_t nptr, int64_t mono, int32_t *__restrict__ flags)
{
    const int64_t total = n > nptr ? n : nptr;
    int f = 0;
    for (int64_t k = (int64_t)blockIdx.x * CP_BLOCK + threadIdx.x; k < total; k += (int64_t)gridDim.x * CP_BLOCK) {
        if (k < n) {
            const int x = idx[k];
            if (x < 0) f |= MX_BAD_NEGATIVE;
            if (x >= bound) f |= MX_BAD_BOUND;
            if (x == MX_NA_INT) f |= MX_BAD_NA;
        }
        if (k < nptr) {
            const int p = indptr[k];
            if (p == MX_NA_INT) f |= MX_BAD_PTR_NA;
            if (k < mono && p > indptr[k + 1]) f |= MX_BAD_PTR_ORDER;
        }
    }
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) f |= __shfl_xor(f, off, MX_WAVE);
    if (lane_id() == 0 && f) atomicOr(flags, f);
}

// A dense R vector as a dsparseVector: the second pass of the same compaction with the cell's 1-based position as
// its index and the value widened to f64 (NA_integer_ / NA -> NA_real_; LGL: TRUE -> 1).  The keep rule is
// MX_KEEP_NONZERO, under which NaN and NA count as non-zero, so the count pass is compact_count_kernel itself.
template <int VB, bool LGL>
__global__ __launch_bounds__(CP_BLOCK)
void dense_to_svec_fill_kernel(int64_t n, const void *__restrict__ dense, const int32_t *__restrict__ tile_off,
                               int32_t *__restrict__ out_idx, double *__restrict__ out_values)
{
    using T = typename CpValue<VB>::T;
    __shared__ CpTileRanks S;
    const int lane = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    T v[CP_ROUNDS];
    cp_load(v, (const T *)dense, base, n);
    unsigned long long bal[CP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        const bool in = base + r * CP_BLOCK + threadIdx.x < n;
        bal[r] = __ballot(in && cp_keep<VB>(MX_KEEP_NONZERO, v[r], 0));
    }
    cp_rank_tile(S, bal);
    const int64_t t0 = tile_off[blockIdx.x];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if (!((bal[r] >> lane) & 1)) continue;
        const int64_t q = t0 + cp_rank_of(S, r, bal[r]);
        out_idx[q] = (int32_t)(base + r * CP_BLOCK + threadIdx.x + 1);
        if constexpr (VB == 8) out_values[q] = v[r];
        else out_values[q] = v[r] == MX_NA_INT ? na_real() : LGL ? (double)(v[r] != 0) : (double)v[r];
    }
}

static int64_t compact_ntiles(int64_t n) { return ceil_div(n > 0 ? n : 0, CP_TILE); }
// per tile: its count, then its offset in the output
struct CompactLayout : CountOffsetsLayout {
    CompactLayout(const void *ws, int64_t n) : CountOffsetsLayout(ws, compact_ntiles(n)) {}
};

static bool rule_ok(int rule, int value_dtype, const void *values, const int32_t *mask)
{
    if (rule == MX_KEEP_MASK) return mask != nullptr && (value_dtype == MX_NONE || values != nullptr);
    if (rule < MX_KEEP_NONZERO || rule > MX_KEEP_NOT_NA) return false;
    return value_dtype != MX_NONE && values != nullptr;
}

static int value_bytes(int value_dtype)
{
    switch (value_dtype) { case MX_F64: return 8; case MX_LGL: case MX_I32: return 4; case MX_NONE: return 0; }
    return -1;
}

}  // namespace mx

extern "C" size_t mxd_compact_workspace_bytes(int64_t n) { return mx::CompactLayout(nullptr, n).bytes; }

extern "C" int mxd_compact_count(int64_t n, const void *values, int value_dtype, int rule, const int32_t *mask,
                                 void *workspace, int64_t *kept_host, void *stream)
{
    MX_REQUIRE(n >= 0 && n <= INT_MAX, "mxd_compact_count: bad size");
    MX_REQUIRE(kept_host, "mxd_compact_count: null pointer");
    const int vb = mx::value_bytes(value_dtype);
    MX_REQUIRE(vb >= 0, "mxd_compact_count: unsupported value dtype %d", value_dtype);
    if (n == 0) { *kept_host = 0; return 0; }
    MX_REQUIRE(workspace && mx::rule_ok(rule, value_dtype, values, mask), "mxd_compact_count: bad rule or null pointer");
    hipStream_t st = mx::as_stream(stream);
    const int64_t t = mx::compact_ntiles(n);
    const mx::CompactLayout L(workspace, n);
    int32_t *counts = L.counts;
    if (vb == 8)
        hipLaunchKernelGGL(mx::compact_count_kernel<8>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, values, rule,
                           mask, counts);
    else if (vb == 4)
        hipLaunchKernelGGL(mx::compact_count_kernel<4>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, values, rule,
                           mask, counts);
    else
        hipLaunchKernelGGL(mx::compact_count_kernel<0>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, values, rule,
                           mask, counts);
    MX_LAUNCH_CHECK();
    return mx::finish_count(t, L.counts, L.offsets, kept_host, st);
}

extern "C" int mxd_compact_fill(int64_t n, const void *values, int value_dtype, int rule, const int32_t *mask,
                                const int32_t *idx0, const int32_t *idx1, int m, const int32_t *indptr,
                                const void *workspace, int32_t *out_idx0, int32_t *out_idx1, void *out_values,
                                int32_t *out_indptr, void *stream)
{
    MX_REQUIRE(n >= 0 && n <= INT_MAX && m >= 0 && m < INT_MAX, "mxd_compact_fill: bad size");
    const int vb = mx::value_bytes(value_dtype);
    MX_REQUIRE(vb >= 0, "mxd_compact_fill: unsupported value dtype %d", value_dtype);
    MX_REQUIRE((!out_idx0 || idx0) && (!out_idx1 || idx1) && (!out_indptr || indptr),
               "mxd_compact_fill: output without its input");
    hipStream_t st = mx::as_stream(stream);
    if (n == 0) {                                          // nothing kept: every row pointer is 0
        if (out_indptr) MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)m + 1), st));
        return 0;
    }
    MX_REQUIRE(workspace && mx::rule_ok(rule, value_dtype, values, mask), "mxd_compact_fill: bad rule or null pointer");
    const int64_t t = mx::compact_ntiles(n);
    const int32_t *off = mx::CompactLayout(workspace, n).offsets;
    void *ov = vb ? out_values : nullptr;
    if (vb == 8)
        hipLaunchKernelGGL(mx::compact_fill_kernel<8>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, t, values, rule,
                           mask, idx0, idx1, m, indptr, off, out_idx0, out_idx1, ov, out_indptr);
    else if (vb == 4)
        hipLaunchKernelGGL(mx::compact_fill_kernel<4>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, t, values, rule,
                           mask, idx0, idx1, m, indptr, off, out_idx0, out_idx1, ov, out_indptr);
    else
        hipLaunchKernelGGL(mx::compact_fill_kernel<0>, dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n, t, values, rule,
                           mask, idx0, idx1, m, indptr, off, out_idx0, out_idx1, ov, out_indptr);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" int mxd_dense_to_svec_count(int64_t n, const void *dense, int dtype, void *workspace, int64_t *kept_host,
                                       void *stream)
{
    MX_REQUIRE(dtype == MX_F64 || dtype == MX_I32 || dtype == MX_LGL, "mxd_dense_to_svec_count: unsupported dtype %d",
               dtype);
    MX_REQUIRE(n >= 0 && n < INT_MAX, "mxd_dense_to_svec_count: bad size");
    return mxd_compact_count(n, dense, dtype, MX_KEEP_NONZERO, nullptr, workspace, kept_host, stream);
}

extern "C" int mxd_dense_to_svec_fill(int64_t n, const void *dense, int dtype, const void *workspace,
                                      int32_t *out_indices_base1, double *out_values, void *stream)
{
    const char *what = "mxd_dense_to_svec_fill";
    MX_REQUIRE(dtype == MX_F64 || dtype == MX_I32 || dtype == MX_LGL, "%s: unsupported dtype %d", what, dtype);
    MX_REQUIRE(n >= 0 && n < INT_MAX, "%s: bad size", what);
    if (n == 0) return 0;
    MX_REQUIRE(dense && workspace && out_indices_base1 && out_values, "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    const int64_t t = mx::compact_ntiles(n);
    const int32_t *off = mx::CompactLayout(workspace, n).offsets;
    if (dtype == MX_F64)
        hipLaunchKernelGGL((mx::dense_to_svec_fill_kernel<8, false>), dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n,
                           dense, off, out_indices_base1, out_values);
    else if (dtype == MX_LGL)
        hipLaunchKernelGGL((mx::dense_to_svec_fill_kernel<4, true>), dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n,
                           dense, off, out_indices_base1, out_values);
    else
        hipLaunchKernelGGL((mx::dense_to_svec_fill_kernel<4, false>), dim3((unsigned)t), dim3(mx::CP_BLOCK), 0, st, n,
                           dense, off, out_indices_base1, out_values);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" int mxd_validate_indices(const int32_t *indices, int64_t n, int bound, const int32_t *indptr,
                                    int64_t n_ptr, int64_t n_mono, int32_t *workspace4, int *flags_host, void *stream)
{
    MX_REQUIRE(n >= 0 && n_ptr >= 0 && n_mono >= 0 && (n_mono == 0 || n_mono < n_ptr),
               "mxd_validate_indices: bad size");
    MX_REQUIRE(flags_host && workspace4 && (n == 0 || indices) && (n_ptr == 0 || indptr),
               "mxd_validate_indices: null pointer");
    *flags_host = 0;
    const int64_t total = n > n_ptr ? n : n_ptr;
    if (total == 0) return 0;
    hipStream_t st = mx::as_stream(stream);
    MX_HIP(hipMemsetAsync(workspace4, 0, sizeof(int32_t), st));
    const int64_t blocks = mx::ceil_div(total, mx::CP_BLOCK);
    const unsigned g = (unsigned)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(mx::validate_kernel, dim3(g), dim3(mx::CP_BLOCK), 0, st, indices, n, bound, indptr, n_ptr,
                       n_mono, workspace4);
    MX_LAUNCH_CHECK();
    MX_HIP(hipMemcpyAsync(flags_host, workspace4, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    return 0;
}

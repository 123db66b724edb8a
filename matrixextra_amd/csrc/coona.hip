// coona.hip — what finishes `[`: NA rows / columns injected into a COO, the CSR scalar lookup, the recycled indices
// of a sparseVector selector, and the drop of a one-row / one-column result to a dense vector.
//
// Replaces:
//   inject_NAs_inplace_coo_template<>, add_rows_cols_NA   src/slice_coo.cpp:708-946
//   extract_single_val_csr<> (is_sorted = false)          src/slice.cpp:661-785
//   repeat_indices_n_times                                src/slice.cpp:636-659
// and serves drop_slice's as.vector() (R/slice.R:210-236).
//
// NA injection.  rows_na / cols_na are 0-based, ascending and distinct.  The output is
//   1. the kept triplets in storage order: a triplet is dropped when its row is an NA row (rows only), its column an
//      NA column (columns only), or BOTH (both lists given: the reference's rule, :789-809, so a triplet of an NA
//      row outside the NA columns stays and the NA block stores its cell again);
//   2. the NA block.  The axis with more NA lines is the major one (ties: columns).  First every major NA line in
//      full, (line, 0 .. L-1); then, per minor NA line, its cells on the major lines rem[0 .. n_major - n_major_na),
//      where rem is what the reference's swap loop (:729-739) leaves of iota(n_major).
// Membership goes through one dense int32 map per axis holding rank + 1 of the index in its list, built from the list
// by one store per list entry while the list is checked (in range, strictly ascending).  The ranks also give rem in
// closed form: the loop swaps positions move_to(ix) = n - cnt + ix and list[ix], ix descending, and list[ix] is
// untouched when its turn comes, so position p < n - cnt ends with p when p is no NA line, else with the value that
// sat at move_to(rank(p)) — itself move_to's own index unless that position is an NA line too, in which case the chain
// goes on from its rank.  Ranks grow along a chain, so it ends within cnt steps; chains share no position.
// The kept pass is compact.hip's tiled count -> scan -> fill (mx_compact_tile.h) with the keep rule above; the NA
// block is one store per output entry.  No atomics.
#include "mx_compact_tile.h"
#include "mx_dispatch.h"
#include "mx_workspace.h"

#include <cstring>

namespace mx {

constexpr int NA_BLOCK = 256;

// map[list[t]] = t + 1 for a valid entry; *flag = 1 when one is out of [0, n) or not above its predecessor
__global__ __launch_bounds__(NA_BLOCK)
void na_mark_kernel(const int32_t *__restrict__ list, int64_t cnt, int n, int32_t *__restrict__ map,
                    int32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (t < cnt) {
        const int v = list[t];
        bad = (unsigned)v >= (unsigned)n || (t > 0 && list[t - 1] >= v);
        if ((unsigned)v < (unsigned)n) map[v] = (int32_t)(t + 1);
    }
    if (__ballot(bad) != 0ULL && lane_id() == 0) *flag = 1;
}

// rem[p] for p < n - cnt (see the header); map holds rank + 1
__global__ __launch_bounds__(NA_BLOCK)
void na_remainder_kernel(int n, int cnt, const int32_t *__restrict__ map, int32_t *__restrict__ rem)
{
    const int left = n - cnt;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= left) return;
    int v = p, rank = map[p];
    for (int step = 0; rank > 0 && step < cnt; step++) {
        v = left + rank - 1;                              // move_to(rank - 1) < n
        rank = map[v];
    }
    rem[p] = v;
}

// MODE: bit 0 = NA rows given, bit 1 = NA columns given.  Whether entry (r, c) stays.
template <int MODE>
__device__ __forceinline__ bool na_keep(int r, int c, int nrow, int ncol, const int32_t *__restrict__ rowmap,
                                        const int32_t *__restrict__ colmap)
{
    bool drop = MODE != 0;
    if constexpr ((MODE & 1) != 0) drop = (unsigned)r < (unsigned)nrow && rowmap[r] != 0;
    if constexpr ((MODE & 2) != 0) drop = drop && (unsigned)c < (unsigned)ncol && colmap[c] != 0;
    return !drop;
}

template <int MODE>
__device__ __forceinline__ void na_tile_ballots(unsigned long long (&bal)[CP_ROUNDS], const int (&ri)[CP_ROUNDS],
                                                const int (&ci)[CP_ROUNDS], int64_t base, int64_t nnz, int nrow,
                                                int ncol, const int32_t *__restrict__ rowmap,
                                                const int32_t *__restrict__ colmap)
{
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        const bool in = base + r * CP_BLOCK + threadIdx.x < nnz;
        bal[r] = __ballot(in && na_keep<MODE>(ri[r], ci[r], nrow, ncol, rowmap, colmap));
    }
}

template <int MODE>
__global__ __launch_bounds__(CP_BLOCK)
void na_count_kernel(int nrow, int ncol, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                     int64_t nnz, const int32_t *__restrict__ rowmap, const int32_t *__restrict__ colmap,
                     int32_t *__restrict__ tile_counts)
{
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    int ri[CP_ROUNDS], ci[CP_ROUNDS];
    if constexpr ((MODE & 1) != 0) cp_load(ri, rows, base, nnz);
    if constexpr ((MODE & 2) != 0) cp_load(ci, cols, base, nnz);
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if constexpr ((MODE & 1) == 0) ri[r] = 0;
        if constexpr ((MODE & 2) == 0) ci[r] = 0;
    }
    unsigned long long bal[CP_ROUNDS];
    na_tile_ballots<MODE>(bal, ri, ci, base, nnz, nrow, ncol, rowmap, colmap);
    int cnt = 0;                                          // wave-uniform
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) cnt += __popcll(bal[r]);
    cp_store_tile_count(cnt, tile_counts);
}

template <int MODE, int VK>
__global__ __launch_bounds__(CP_BLOCK)
void na_keep_fill_kernel(int nrow, int ncol, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                         const void *__restrict__ vals, int64_t nnz, const int32_t *__restrict__ rowmap,
                         const int32_t *__restrict__ colmap, const int32_t *__restrict__ tile_off,
                         int32_t *__restrict__ out_rows, int32_t *__restrict__ out_cols, void *__restrict__ out_vals)
{
    using T = std::conditional_t<VK == MX_F64, uint64_t, uint32_t>;      // values move as bits
    __shared__ CpTileRanks S;
    const int lane = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    int ri[CP_ROUNDS], ci[CP_ROUNDS];
    T v[CP_ROUNDS];
    cp_load(ri, rows, base, nnz);
    cp_load(ci, cols, base, nnz);
    cp_load(v, (const T *)vals, base, nnz);
    unsigned long long bal[CP_ROUNDS];
    na_tile_ballots<MODE>(bal, ri, ci, base, nnz, nrow, ncol, rowmap, colmap);
    cp_rank_tile(S, bal);
    const int64_t t0 = tile_off[blockIdx.x];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if (!((bal[r] >> lane) & 1)) continue;
        const int64_t q = t0 + cp_rank_of(S, r, bal[r]);
        out_rows[q] = ri[r];
        out_cols[q] = ci[r];
        ((T *)out_vals)[q] = v[r];
    }
}

// The NA block, entry e of na_size behind the *kept_dev kept triplets.  major / minor: the NA lists of the axis with
// more NA lines and of the other; n_major / n_minor: the axis lengths; out_major / out_minor: the index vectors of
// those axes.
template <int VK>
__global__ __launch_bounds__(NA_BLOCK)
void na_block_kernel(const int32_t *__restrict__ major, int n_major_na, int n_major, int n_minor,
                     const int32_t *__restrict__ minor, const int32_t *__restrict__ rem, int64_t na_size,
                     const int32_t *__restrict__ kept_dev, int32_t *__restrict__ out_major,
                     int32_t *__restrict__ out_minor, void *__restrict__ out_vals)
{
    const int64_t kept = *kept_dev;
    const unsigned full = (unsigned)n_major_na * (unsigned)n_minor;       // <= na_size <= INT32_MAX
    const unsigned left = (unsigned)(n_major - n_major_na);
    for (int64_t e64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e64 < na_size;
         e64 += (int64_t)gridDim.x * blockDim.x) {
        const unsigned e = (unsigned)e64;
        int a, b;
        if (e < full) {
            const unsigned k = e / (unsigned)n_minor;
            a = major[k];
            b = (int)(e - k * (unsigned)n_minor);
        } else {
            const unsigned f = e - full, k = f / left;
            a = rem[f - k * left];
            b = minor[k];
        }
        const int64_t q = kept + e64;
        out_major[q] = a;
        out_minor[q] = b;
        if constexpr (VK == MX_F64) ((uint64_t *)out_vals)[q] = MX_NA_REAL_BITS;
        else ((int32_t *)out_vals)[q] = MX_NA_INT;
    }
}

// The two caller-allocated regions.  `workspace` is compact.hip's own (mxd_compact_workspace_bytes(nnz)): the kept
// pass is its tiled compaction, one count and one offset per tile, and offsets[ntiles] is the kept total.  `maps` is
// int32[4 + nrow + ncol + max(nrow, ncol)]: the two list flags (and two spare words), the row map, the column map, rem.
struct NaLayout {
    CountOffsetsLayout tiles;
    int64_t ntiles = tiles.n;
    int32_t *counts = tiles.counts, *offsets = tiles.offsets;
    int32_t *flags, *rowmap, *colmap, *rem;
    NaLayout(const void *ws, const int32_t *maps, int64_t nnz, int nrow, int ncol)
        : tiles(ws, ceil_div(nnz > 0 ? nnz : 0, CP_TILE)), flags(const_cast<int32_t *>(maps)), rowmap(flags + 4),
          colmap(rowmap + nrow), rem(colmap + ncol) {}
};

static int na_check_sizes(const char *what, int nrow, int ncol, int64_t nnz, int64_t n_rna, int64_t n_cna)
{
    MX_REQUIRE(nrow >= 0 && ncol >= 0 && nnz >= 0 && nnz <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(n_rna >= 0 && n_rna <= nrow, "%s: %lld NA rows, the matrix has %d (the list must be ascending and "
               "distinct)", what, (long long)n_rna, nrow);
    MX_REQUIRE(n_cna >= 0 && n_cna <= ncol, "%s: %lld NA columns, the matrix has %d (the list must be ascending and "
               "distinct)", what, (long long)n_cna, ncol);
    return 0;
}

static int64_t na_block_size(int nrow, int ncol, int64_t n_rna, int64_t n_cna)
{
    return n_rna * (int64_t)ncol + n_cna * ((int64_t)nrow - n_rna);
}

using na_modes = int_list<0, 1, 2, 3>;

// ---- X[i, j] with scalar i, j of a CSR: the first k of row r, in storage order, with indices[k] == c ---------------
// one wavefront; out[0] = k or -1, out[1] = the bits of values[k]
__global__ __launch_bounds__(MX_WAVE)
void csr_single_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                       const void *__restrict__ vals, int value_dtype, int64_t nnz, int r, int c,
                       long long *__restrict__ out)
{
    const RowBounds rb = row_bounds(indptr[r], indptr[r + 1], nnz);
    const int lane = lane_id();
    long long hit = -1;
    for (int64_t at = 0; at < rb.len; at += MX_WAVE) {                   // wave-uniform trip count
        const int64_t k = rb.start + at + lane;
        const unsigned long long b = __ballot(at + lane < rb.len && indices[k] == c);
        if (b) { hit = rb.start + at + __builtin_ctzll(b); break; }
    }
    if (lane == 0) {
        long long bits = 0;
        if (hit >= 0 && vals) {
            if (value_dtype == MX_F64) bits = ((const long long *)vals)[hit];
            else if (value_dtype == MX_LGL) bits = ((const int32_t *)vals)[hit];
        }
        out[0] = hit;
        out[1] = bits;
    }
}

// out[t + n * rep] = indices[t] + ix_length * rep for rep < full, then the remainder block
__global__ __launch_bounds__(NA_BLOCK)
void repeat_indices_kernel(const int32_t *__restrict__ indices, int n, const int32_t *__restrict__ remainder,
                           int n_rem, int ix_length, int full, int32_t *__restrict__ out)
{
    const int64_t body = (int64_t)n * full, total = body + n_rem;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (e < body) {
            const int rep = (int)(e / n);
            out[e] = indices[e - (int64_t)rep * n] + ix_length * rep;
        } else {
            out[e] = remainder[e - body] + ix_length * full;
        }
    }
}

// out[pos[k]] = values[k] (1 without values) for the positions inside [0, len)
template <typename T, bool HAS>
__global__ __launch_bounds__(NA_BLOCK)
void scatter_entries_kernel(const int32_t *__restrict__ pos, const T *__restrict__ values, int64_t n,
                            T *__restrict__ out, int64_t len)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = pos[k];
        if (p < 0 || p >= len) continue;
        if constexpr (HAS) out[p] = values[k];
        else out[p] = T(1);
    }
}

}  // namespace mx

extern "C" int mxd_coo_inject_na_count(int nrow, int ncol, const int32_t *rows, const int32_t *cols, int64_t nnz,
                                       const int32_t *rows_na, int64_t n_rna, const int32_t *cols_na, int64_t n_cna,
                                       void *workspace, int32_t *maps, int64_t *nnz_out_host, void *stream)
{
    const char *what = "mxd_coo_inject_na_count";
    if (mx::na_check_sizes(what, nrow, ncol, nnz, n_rna, n_cna)) return 1;
    MX_REQUIRE(nnz_out_host && workspace && maps && (nnz == 0 || (rows && cols)) && (n_rna == 0 || rows_na) &&
               (n_cna == 0 || cols_na), "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    const mx::NaLayout L(workspace, maps, nnz, nrow, ncol);
    MX_HIP(hipMemsetAsync(L.flags, 0, 16, st));
    MX_HIP(hipMemsetAsync(L.offsets, 0, sizeof(int32_t), st));             // nnz = 0: no kept triplets
    if (n_rna) {
        MX_HIP(hipMemsetAsync(L.rowmap, 0, sizeof(int32_t) * (size_t)nrow, st));
        hipLaunchKernelGGL(mx::na_mark_kernel, dim3(mx::grid_for(n_rna, mx::NA_BLOCK)), dim3(mx::NA_BLOCK), 0, st,
                           rows_na, n_rna, nrow, L.rowmap, L.flags);
        MX_LAUNCH_CHECK();
    }
    if (n_cna) {
        MX_HIP(hipMemsetAsync(L.colmap, 0, sizeof(int32_t) * (size_t)ncol, st));
        hipLaunchKernelGGL(mx::na_mark_kernel, dim3(mx::grid_for(n_cna, mx::NA_BLOCK)), dim3(mx::NA_BLOCK), 0, st,
                           cols_na, n_cna, ncol, L.colmap, L.flags + 1);
        MX_LAUNCH_CHECK();
    }
    if (n_rna && n_cna) {                                                  // the minor lines run over rem
        const bool rows_major = n_rna > n_cna;
        const int n = rows_major ? nrow : ncol, cnt = (int)(rows_major ? n_rna : n_cna);
        if (n > cnt) {
            hipLaunchKernelGGL(mx::na_remainder_kernel, dim3(mx::grid_for(n - cnt, mx::NA_BLOCK)),
                               dim3(mx::NA_BLOCK), 0, st, n, cnt, rows_major ? L.rowmap : L.colmap, L.rem);
            MX_LAUNCH_CHECK();
        }
    }
    if (nnz > 0) {
        const int mode = (n_rna ? 1 : 0) | (n_cna ? 2 : 0);
        const int rc = mx::dispatch_int(mx::na_modes{}, what, "mode", mode, [&](auto m) {
            hipLaunchKernelGGL((mx::na_count_kernel<m()>), dim3((unsigned)L.ntiles), dim3(mx::CP_BLOCK), 0, st, nrow,
                               ncol, rows, cols, nnz, L.rowmap, L.colmap, L.counts);
            MX_LAUNCH_CHECK();
            return 0;
        });
        if (rc) return rc;
        if (mx::finish_count(L.ntiles, L.counts, L.offsets, nullptr, st)) return 1;
    }
    int32_t kept = 0, hf[2] = {0, 0};                                      // the one read-back
    MX_HIP(hipMemcpyAsync(&kept, L.offsets + L.ntiles, sizeof(kept), hipMemcpyDeviceToHost, st));
    MX_HIP(hipMemcpyAsync(hf, L.flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!hf[0], "%s: the NA rows are not ascending, distinct and inside [0, %d)", what, nrow);
    MX_REQUIRE(!hf[1], "%s: the NA columns are not ascending, distinct and inside [0, %d)", what, ncol);
    const int64_t total = (int64_t)kept + mx::na_block_size(nrow, ncol, n_rna, n_cna);
    MX_REQUIRE(total <= (int64_t)INT_MAX, "NA injection into a COO: the result has %lld entries (exceeds R's int32 "
               "index range)", (long long)total);
    *nnz_out_host = total;
    return 0;
}

extern "C" int mxd_coo_inject_na_fill(int nrow, int ncol, const int32_t *rows, const int32_t *cols,
                                      const void *values, int value_dtype, int64_t nnz, const int32_t *rows_na,
                                      int64_t n_rna, const int32_t *cols_na, int64_t n_cna, const void *workspace,
                                      const int32_t *maps, int32_t *out_rows, int32_t *out_cols, void *out_values, void *stream)
{
    const char *what = "mxd_coo_inject_na_fill";
    if (mx::na_check_sizes(what, nrow, ncol, nnz, n_rna, n_cna)) return 1;
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL, "%s: unsupported value dtype %d", what, value_dtype);
    const int64_t na_size = mx::na_block_size(nrow, ncol, n_rna, n_cna);
    MX_REQUIRE(nnz + na_size <= (int64_t)INT_MAX, "%s: the result exceeds R's int32 index range", what);
    if (nnz == 0 && na_size == 0) return 0;
    MX_REQUIRE(workspace && maps && out_rows && out_cols && out_values && (nnz == 0 || (rows && cols && values)) &&
               (n_rna == 0 || rows_na) && (n_cna == 0 || cols_na), "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    const mx::NaLayout L(workspace, maps, nnz, nrow, ncol);
    using kinds = mx::int_list<MX_F64, MX_LGL>;
    return mx::dispatch_int(kinds{}, what, "value dtype", value_dtype, [&](auto vk) {
        if (nnz > 0) {
            const int mode = (n_rna ? 1 : 0) | (n_cna ? 2 : 0);
            const int rc = mx::dispatch_int(mx::na_modes{}, what, "mode", mode, [&](auto m) {
                hipLaunchKernelGGL((mx::na_keep_fill_kernel<m(), vk()>), dim3((unsigned)L.ntiles), dim3(mx::CP_BLOCK),
                                   0, st, nrow, ncol, rows, cols, values, nnz, L.rowmap, L.colmap, L.offsets,
                                   out_rows, out_cols, out_values);
                MX_LAUNCH_CHECK();
                return 0;
            });
            if (rc) return rc;
        }
        if (na_size > 0) {
            const bool rows_major = n_rna > n_cna;
            const unsigned g = mx::grid_for(na_size, mx::NA_BLOCK, 8192);
            if (rows_major)
                hipLaunchKernelGGL((mx::na_block_kernel<vk()>), dim3(g), dim3(mx::NA_BLOCK), 0, st, rows_na, (int)n_rna,
                                   nrow, ncol, cols_na, L.rem, na_size, L.offsets + L.ntiles, out_rows, out_cols,
                                   out_values);
            else
                hipLaunchKernelGGL((mx::na_block_kernel<vk()>), dim3(g), dim3(mx::NA_BLOCK), 0, st, cols_na, (int)n_cna,
                                   ncol, nrow, rows_na, L.rem, na_size, L.offsets + L.ntiles, out_cols, out_rows,
                                   out_values);
            MX_LAUNCH_CHECK();
        }
        return 0;
    });
}

extern "C" int mxd_csr_single(int nrows, const int32_t *indptr, const int32_t *indices, const void *values,
                              int value_dtype, int64_t nnz, int r, int c, void *workspace, int64_t *k_host,
                              void *value_host, void *stream)
{
    MX_REQUIRE(nrows >= 0 && nnz >= 0 && k_host && workspace && indptr, "mxd_csr_single: bad arguments");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_csr_single: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(r >= 0 && r < nrows, "mxd_csr_single: row %d outside [0, %d)", r, nrows);
    MX_REQUIRE(nnz == 0 || (indices && (value_dtype == MX_NONE || values)), "mxd_csr_single: null pointer");
    *k_host = -1;
    if (nnz == 0) return 0;
    hipStream_t st = mx::as_stream(stream);
    long long *out = (long long *)workspace;
    hipLaunchKernelGGL(mx::csr_single_kernel, dim3(1), dim3(MX_WAVE), 0, st, indptr, indices,
                       value_dtype == MX_NONE ? nullptr : values, value_dtype, nnz, r, c, out);
    MX_LAUNCH_CHECK();
    long long h[2] = {-1, 0};
    MX_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    *k_host = h[0];
    if (h[0] >= 0 && value_host) {
        if (value_dtype == MX_F64) memcpy(value_host, &h[1], sizeof(double));
        else if (value_dtype == MX_LGL) { const int32_t l = (int32_t)h[1]; memcpy(value_host, &l, sizeof(l)); }
    }
    return 0;
}

extern "C" int mxd_repeat_indices(const int32_t *indices, int64_t n_indices, const int32_t *remainder,
                                  int64_t n_remainder, int ix_length, int desired_length, int32_t *out, void *stream)
{
    MX_REQUIRE(n_indices >= 0 && n_remainder >= 0 && ix_length > 0 && desired_length >= 0,
               "mxd_repeat_indices: bad size");
    const int full = desired_length / ix_length;
    const int64_t total = n_indices * full + n_remainder;
    MX_REQUIRE(n_indices <= INT_MAX && n_remainder <= INT_MAX && total <= (int64_t)INT_MAX,
               "mxd_repeat_indices: %lld indices exceed R's int32 index range", (long long)total);
    if (total == 0) return 0;
    MX_REQUIRE(out && (n_indices == 0 || indices) && (n_remainder == 0 || remainder),
               "mxd_repeat_indices: null pointer");
    hipLaunchKernelGGL(mx::repeat_indices_kernel, dim3(mx::grid_for(total, mx::NA_BLOCK, 8192)), dim3(mx::NA_BLOCK), 0,
                       mx::as_stream(stream), indices, (int)n_indices, remainder, (int)n_remainder, ix_length, full,
                       out);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" int mxd_entries_to_dense_vector(const int32_t *pos, const void *values, int value_dtype, int64_t n,
                                           void *out, int out_dtype, int64_t len, void *stream)
{
    const char *what = "mxd_entries_to_dense_vector";
    MX_REQUIRE(n >= 0 && len >= 0, "%s: bad size", what);
    MX_REQUIRE(out_dtype == MX_F64 || out_dtype == MX_LGL, "%s: unsupported output dtype %d", what, out_dtype);
    MX_REQUIRE(value_dtype == MX_NONE || value_dtype == out_dtype, "%s: values of dtype %d into a vector of dtype %d",
               what, value_dtype, out_dtype);
    if (len == 0) return 0;
    MX_REQUIRE(out && (n == 0 || (pos && (value_dtype == MX_NONE || values))), "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    MX_HIP(hipMemsetAsync(out, 0, (size_t)len * (out_dtype == MX_F64 ? sizeof(double) : sizeof(int32_t)), st));
    if (n == 0) return 0;
    const dim3 g(mx::grid_for(n, mx::NA_BLOCK, 8192)), b(mx::NA_BLOCK);
    const bool has = value_dtype != MX_NONE;
    if (out_dtype == MX_F64) {
        if (has) hipLaunchKernelGGL((mx::scatter_entries_kernel<double, true>), g, b, 0, st, pos, (const double *)values,
                                    n, (double *)out, len);
        else hipLaunchKernelGGL((mx::scatter_entries_kernel<double, false>), g, b, 0, st, pos, (const double *)nullptr,
                                n, (double *)out, len);
    } else {
        if (has) hipLaunchKernelGGL((mx::scatter_entries_kernel<int32_t, true>), g, b, 0, st, pos,
                                    (const int32_t *)values, n, (int32_t *)out, len);
        else hipLaunchKernelGGL((mx::scatter_entries_kernel<int32_t, false>), g, b, 0, st, pos,
                                (const int32_t *)nullptr, n, (int32_t *)out, len);
    }
    MX_LAUNCH_CHECK();
    return 0;
}

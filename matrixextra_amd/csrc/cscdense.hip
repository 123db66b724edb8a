// cscdense.hip — CSC (.) dense that keeps R's NA cells, for gfx950.
//
// Replaces:
//   multiply_csc_by_dense_keep_NAs_template<>  src/operators.cpp:1207-1460  (numeric, integer, logical, float32)
// (the values-only twin, multiply_csc_by_dense_ignore_NAs<>, is svec.hip's csr_by_dense_kernel with CSC addressing)
//
// Output column c = the stored rows of X's column c (values x (op) d) merged with every row r whose dense cell
// (r, c) is NA and that is not stored (value NA_real_), rows ascending.  For a column-sorted CSC the stored entries
// are ascending in the flat column-major cell index f = c*m + r, so the result is the sorted union of two ascending
// streams over f.  The flat index is cut into tiles of CD_TILE cells, whatever the shape:
//   count  per tile: the dense cells are read once (coalesced), NA cells are balloted into a 1-bit-per-cell mask
//          that goes to global memory (m*n/8 bytes), the tile's stored entries [ks, ke) (two wave-wide searches) are
//          marked in an LDS bitmap, and the tile writes popcount(NA | stored); a tile with an NA cell outside the
//          pattern also sets one flag, so that the host can skip the fill when there is none.
//   scan   the shared finish_count (tile offsets, 8-byte total read back and checked against INT_MAX).
//   fill   per tile: the NA mask and the stored bitmap again (the tile's entry range is the count's, so no search
//          chain delays the tile), ranks by popcount over the 64 words of the union; every union cell writes its row,
//          NA-only cells write NA_real_, the first entry of each stored row gathers its one dense value, and columns
//          whose first cell c*m falls in the tile get p'[c] (as compact_fill_kernel does).
// A repeated row inside a column marks one cell: the first entry writes its value, later ones are skipped, as the
// reference's lower_bound skip does (:1329-1331).  Every write position comes from the same bitmaps in both passes,
// and an entry whose cell falls outside its tile (an index outside [0, m)) is ignored in both, so that nothing is
// written or read out of bounds whatever the input.
#include "mx_dispatch.h"
#include "mx_workspace.h"

namespace mx {

constexpr int CD_BLOCK = 256;
constexpr int CD_WAVES = CD_BLOCK / MX_WAVE;
constexpr int CD_ROUNDS = 16;
constexpr int CD_TILE = CD_BLOCK * CD_ROUNDS;    // 4096 cells per tile
constexpr int CD_WORDS = CD_TILE / MX_WAVE;      // 64 mask words per tile: word w covers cells [64 w, 64 w + 64)
static_assert(CD_WORDS == CD_ROUNDS * CD_WAVES, "round r of wave v covers mask word r * CD_WAVES + v");

// DK: dense kind 0 double, 1 float32, 2 R integer, 3 R logical (the value kinds 0-3 of csr_by_dense_kernel)
template <int DK> struct CdDense { using T = int32_t; };
template <> struct CdDense<0> { using T = double; };
template <> struct CdDense<1> { using T = float; };

template <int DK>
__device__ __forceinline__ bool cd_is_na(typename CdDense<DK>::T d)
{
    if constexpr (DK <= 1) return isnan(d);              // ISNAN: any NaN payload (:1239, :1284, :1338)
    else return d == MX_NA_INT;
}

// stored entry value (:1317-1323): f64 / float32 x * d (NaN propagates); integer / logical NA -> NA_real_
template <int DK>
__device__ __forceinline__ double cd_value(double x, typename CdDense<DK>::T d)
{
    if constexpr (DK == 0) return x * d;
    else if constexpr (DK == 1) return x * (double)d;
    else if constexpr (DK == 2) return d == MX_NA_INT ? na_real() : x * (double)d;
    else return d == MX_NA_INT ? na_real() : x * (double)(d != 0);
}

// first entry k whose flat index c*m + indices[k] is >= f (a column-sorted CSC), in [0, nnz] whatever the input;
// called by a whole wave with the same f: 64-way splits of the column's range, so that a search of 4096 entries is
// two dependent loads instead of twelve
__device__ __forceinline__ int64_t cd_first_at(int64_t f, int64_t m, int n, const int32_t *__restrict__ indptr,
                                               const int32_t *__restrict__ indices, int64_t nnz)
{
    const int64_t c = f / m;
    if (c >= n) return nnz;
    const RowBounds b = row_bounds(indptr[c], indptr[c + 1], nnz);
    int64_t s = b.start, e = b.start + b.len;
    const int key = (int)(f - c * m);
    while (e > s) {                                       // the answer lies in [s, e]
        const int64_t step = (e - s + MX_WAVE - 1) / MX_WAVE;
        const int64_t pos = s + (int64_t)lane_id() * step;
        const int below = __popcll(__ballot(pos < e && indices[pos] < key));   // chunks starting below the key
        if (below == 0) return s;
        const int64_t ns = s + (int64_t)(below - 1) * step + 1, ne = s + (int64_t)below * step;
        s = ns;
        e = ne < e ? ne : e;
    }
    return s;
}

// column of entry k among the tile's columns [c0, c1]: the last c there with indptr[c] <= k
__device__ __forceinline__ int cd_col_of(int k, int c0, int c1, const int32_t *__restrict__ indptr)
{
    const int32_t *q = indptr + c0 + 1;
    int lo = 0, cnt = c1 - c0;
    while (cnt > 0) {
        const int step = cnt >> 1;
        if (q[lo + step] <= k) { lo += step + 1; cnt -= step + 1; }
        else cnt = step;
    }
    return c0 + lo;
}

struct CdTile {
    int64_t base, len;        // cells [base, base + len)
    int c0, c1;               // columns the tile touches (c1 clamped to n - 1)
};

__device__ __forceinline__ CdTile cd_tile(int64_t m, int n, int64_t F)
{
    CdTile t;
    t.base = (int64_t)blockIdx.x * CD_TILE;
    t.len = F - t.base < CD_TILE ? F - t.base : CD_TILE;
    t.c0 = (int)(t.base / m);
    const int64_t c1 = (t.base + t.len - 1) / m;
    t.c1 = c1 < n - 1 ? (int)c1 : n - 1;
    return t;
}

// s_st: one bit per stored cell of the tile (LDS, zeroed by the caller); s_k = {ks, ke}
__device__ __forceinline__ void cd_mark_stored(const CdTile &t, int64_t m, const int32_t *__restrict__ indptr,
                                               const int32_t *__restrict__ indices, const int64_t *s_k,
                                               unsigned long long *s_st)
{
    for (int64_t k = s_k[0] + threadIdx.x; k < s_k[1]; k += CD_BLOCK) {
        const int c = cd_col_of((int)k, t.c0, t.c1, indptr);
        const int64_t q = (int64_t)c * m + indices[k] - t.base;
        if (q >= 0 && q < t.len) atomicOr(&s_st[q >> 6], 1ull << (q & 63));
    }
}

template <int DK>
__global__ __launch_bounds__(CD_BLOCK)
void cd_count_kernel(int64_t m, int n, int64_t F, const int32_t *__restrict__ indptr,
                     const int32_t *__restrict__ indices, int64_t nnz, const void *__restrict__ dense,
                     unsigned long long *__restrict__ na_mask, int32_t *__restrict__ tile_counts,
                     int32_t *__restrict__ tile_first, volatile unsigned long long *__restrict__ na_outside)
{
    using T = typename CdDense<DK>::T;
    __shared__ unsigned long long s_st[CD_WORDS];
    __shared__ int64_t s_k[2];
    __shared__ int s_cnt[CD_WAVES], s_out[CD_WAVES];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const CdTile t = cd_tile(m, n, F);

    // the tile's dense cells, all loads issued before the first use
    T d[CD_ROUNDS];
    const T *src = (const T *)dense + t.base + threadIdx.x;
    if (t.len == CD_TILE) {
#pragma unroll
        for (int r = 0; r < CD_ROUNDS; r++) d[r] = src[r * CD_BLOCK];
    } else {
#pragma unroll
        for (int r = 0; r < CD_ROUNDS; r++) d[r] = r * CD_BLOCK + (int)threadIdx.x < t.len ? src[r * CD_BLOCK] : T{};
    }
    if (threadIdx.x < CD_WORDS) s_st[threadIdx.x] = 0;
    if (wave < 2) {                                       // wave 0: ks, wave 1: ke
        const int64_t k = cd_first_at(t.base + (wave ? t.len : 0), m, n, indptr, indices, nnz);
        if (lane == 0) s_k[wave] = k;
    }
    __syncthreads();
    cd_mark_stored(t, m, indptr, indices, s_k, s_st);
    __syncthreads();
    int cnt = 0, out = 0;                                 // wave-uniform
#pragma unroll
    for (int r = 0; r < CD_ROUNDS; r++) {
        const bool in = r * CD_BLOCK + (int)threadIdx.x < t.len;
        const unsigned long long na = __ballot(in && cd_is_na<DK>(d[r]));
        const int w = r * CD_WAVES + wave;
        const unsigned long long st = s_st[w];
        if (lane == 0) na_mask[(int64_t)blockIdx.x * CD_WORDS + w] = na;
        cnt += __popcll(na | st);
        out += __popcll(na & ~st);
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_out[wave] = out; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0, o = 0;
#pragma unroll
        for (int w = 0; w < CD_WAVES; w++) { c += s_cnt[w]; o += s_out[w]; }
        tile_counts[blockIdx.x] = c;
        tile_first[blockIdx.x] = (int32_t)s_k[0];
        if (o && *na_outside == 0) *na_outside = 1;     // a flag: one counter for every tile would serialise them
    }
}

template <int DK>
__global__ __launch_bounds__(CD_BLOCK)
void cd_fill_kernel(int64_t m, int n, int64_t F, int64_t ntiles, const int32_t *__restrict__ indptr,
                    const int32_t *__restrict__ indices, int64_t nnz, const double *__restrict__ values,
                    const void *__restrict__ dense, const unsigned long long *__restrict__ na_mask,
                    const int32_t *__restrict__ tile_off, const int32_t *__restrict__ tile_first,
                    int32_t *__restrict__ out_indptr,
                    int32_t *__restrict__ out_indices, double *__restrict__ out_values)
{
    using T = typename CdDense<DK>::T;
    __shared__ unsigned long long s_st[CD_WORDS], s_u[CD_WORDS];
    __shared__ int s_off[CD_WORDS];
    __shared__ int s_total;
    __shared__ int64_t s_k[2];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const unsigned long long below = (1ull << lane) - 1;
    const CdTile t = cd_tile(m, n, F);

    const bool last = (int64_t)blockIdx.x == ntiles - 1;
    const unsigned long long na = wave == 0 ? na_mask[(int64_t)blockIdx.x * CD_WORDS + lane] : 0;
    const int64_t t0 = tile_off[blockIdx.x];
    if (threadIdx.x < CD_WORDS) s_st[threadIdx.x] = 0;
    if (threadIdx.x < 2)                                  // the count pass's searches: ke of a tile = ks of the next
        s_k[threadIdx.x] = threadIdx.x == 0 ? tile_first[blockIdx.x] : last ? nnz : tile_first[blockIdx.x + 1];
    __syncthreads();
    cd_mark_stored(t, m, indptr, indices, s_k, s_st);
    __syncthreads();
    if (wave == 0) {                                      // lane = mask word: union, popcount, exclusive scan
        const unsigned long long u = s_st[lane] | na;
        s_u[lane] = u;
        const int c = __popcll(u);
        int incl = c;
#pragma unroll
        for (int off = 1; off < MX_WAVE; off <<= 1) {
            const int o = __shfl_up(incl, off, MX_WAVE);
            if (lane >= off) incl += o;
        }
        s_off[lane] = incl - c;
        if (lane == MX_WAVE - 1) s_total = incl;
    }
    __syncthreads();

    // every union cell: its row; a cell that is NA and not stored: NA_real_ (:1239-1243, :1283-1287, :1337-1341)
    const uint32_t r0 = (uint32_t)(t.base % m), um = (uint32_t)m;
#pragma unroll
    for (int r = 0; r < CD_ROUNDS; r++) {
        const int w = r * CD_WAVES + wave;
        const unsigned long long u = s_u[w];
        if (!((u >> lane) & 1)) continue;
        const int64_t q = t0 + s_off[w] + __popcll(u & below);
        out_indices[q] = (int32_t)((r0 + (uint32_t)(w * MX_WAVE + lane)) % um);
        if (!((s_st[w] >> lane) & 1)) out_values[q] = na_real();
    }

    // stored rows: x (op) d of the first entry of the row (:1315-1331)
    for (int64_t k = s_k[0] + threadIdx.x; k < s_k[1]; k += CD_BLOCK) {
        const int c = cd_col_of((int)k, t.c0, t.c1, indptr);
        const int64_t ql = (int64_t)c * m + indices[k] - t.base;
        if (ql < 0 || ql >= t.len) continue;
        if (k > 0 && k > indptr[c] && indices[k - 1] == indices[k]) continue;     // repeated row: the first stays
        const int w = (int)(ql >> 6);
        const int64_t q = t0 + s_off[w] + __popcll(s_u[w] & ((1ull << (ql & 63)) - 1));
        out_values[q] = cd_value<DK>(values[k], ((const T *)dense)[t.base + ql]);
    }

    // p'[c] for the columns whose first cell c*m lies in the tile; the last tile also writes every later column
    // (those that start at F, c = n included)
    const int64_t cfirst = (t.base + m - 1) / m;
    for (int64_t c = cfirst + threadIdx.x; c <= n; c += CD_BLOCK) {
        const int64_t ql = c * m - t.base;
        if (!last && ql >= CD_TILE) break;               // c*m grows with c
        int rank;
        if (ql >= t.len) rank = s_total;
        else {
            const int w = (int)(ql >> 6);
            rank = s_off[w] + __popcll(s_u[w] & ((1ull << (ql & 63)) - 1));
        }
        out_indptr[c] = (int32_t)(t0 + rank);
    }
}

static int64_t cd_ntiles(int m, int n) { return ceil_div((int64_t)m * (int64_t)n, CD_TILE); }

struct CdLayout {
    WsCursor c;
    int64_t ntiles;
    int32_t *counts = c.take_counts(ntiles), *offsets = c.take_i32(ntiles + 1);       // per tile; offsets one more
    unsigned long long *na_outside = c.take<unsigned long long>(16);    // one word in 16 B: an NA outside the pattern
    unsigned long long *na_mask = c.take<unsigned long long>(sizeof(unsigned long long) * (size_t)ntiles * CD_WORDS);
    int32_t *first = c.take_i32(ntiles);                                // first entry of each tile
    size_t bytes = c.bytes();
    CdLayout(const void *ws, int m, int n) : c(ws), ntiles(m > 0 && n > 0 ? cd_ntiles(m, n) : 0) {}
};

using cd_kinds = int_list<0, 1, 2, 3>;

}  // namespace mx

extern "C" size_t mxd_csc_dense_na_workspace_bytes(int m, int n) { return mx::CdLayout(nullptr, m, n).bytes; }

extern "C" int mxd_csc_dense_na_count(int m, int n, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                      const void *dense_colmajor, int dense_kind, void *workspace,
                                      int64_t *nnz_out_host, int64_t *na_outside_host, void *stream)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && nnz <= INT_MAX && dense_kind >= 0 && dense_kind <= 3,
               "mxd_csc_dense_na_count: bad arguments");
    MX_REQUIRE(nnz_out_host && na_outside_host, "mxd_csc_dense_na_count: null pointer");
    *nnz_out_host = 0;
    *na_outside_host = 0;
    if (m == 0 || n == 0) return 0;
    MX_REQUIRE(workspace && indptr && dense_colmajor && (nnz == 0 || indices), "mxd_csc_dense_na_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const mx::CdLayout L(workspace, m, n);
    const int64_t t = L.ntiles;
    MX_REQUIRE(t <= (int64_t)UINT_MAX, "mxd_csc_dense_na_count: dense operand too large");
    unsigned long long *outside = L.na_outside;
    MX_HIP(hipMemsetAsync(outside, 0, sizeof(unsigned long long), st));
    const int64_t F = (int64_t)m * (int64_t)n;
    const int rc = mx::dispatch_int(mx::cd_kinds{}, "mxd_csc_dense_na_count", "dense kind", dense_kind, [&](auto dk) {
        hipLaunchKernelGGL(mx::cd_count_kernel<dk()>, dim3((unsigned)t), dim3(mx::CD_BLOCK), 0, st, (int64_t)m, n, F,
                           indptr, indices, nnz, dense_colmajor, L.na_mask, L.counts, L.first, outside);
        MX_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    MX_HIP(hipMemcpyAsync(na_outside_host, outside, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    // the 64-bit total is read back (one synchronise) and refused above INT_MAX before any output exists
    return mx::finish_count(t, L.counts, L.offsets, nnz_out_host, st);
}

extern "C" int mxd_csc_dense_na_fill(int m, int n, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                     const double *values, const void *dense_colmajor, int dense_kind,
                                     const void *workspace, int32_t *out_indptr, int32_t *out_indices,
                                     double *out_values, void *stream)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && nnz <= INT_MAX && dense_kind >= 0 && dense_kind <= 3,
               "mxd_csc_dense_na_fill: bad arguments");
    MX_REQUIRE(out_indptr, "mxd_csc_dense_na_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    if (m == 0 || n == 0) {                               // no cells: every column is empty
        MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)n + 1), st));
        return 0;
    }
    MX_REQUIRE(workspace && indptr && dense_colmajor && (nnz == 0 || (indices && values)) && out_indices && out_values,
               "mxd_csc_dense_na_fill: null pointer");
    const mx::CdLayout L(workspace, m, n);
    const int64_t t = L.ntiles;
    const int64_t F = (int64_t)m * (int64_t)n;
    return mx::dispatch_int(mx::cd_kinds{}, "mxd_csc_dense_na_fill", "dense kind", dense_kind, [&](auto dk) {
        hipLaunchKernelGGL(mx::cd_fill_kernel<dk()>, dim3((unsigned)t), dim3(mx::CD_BLOCK), 0, st, (int64_t)m, n, F, t,
                           indptr, indices, nnz, values, dense_colmajor, L.na_mask, L.offsets, L.first, out_indptr,
                           out_indices, out_values);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

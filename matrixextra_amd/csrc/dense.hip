// dense.hip — dense <-> compressed sparse conversions, for gfx950 (include/mxgpu_dense.h).
//
// Replaces what the reference leaves to Matrix: as(m, "RsparseMatrix") / as(m, "CsparseMatrix") behind as.csr.matrix and
// as.csc.matrix of a dense matrix (R/conversions.R:180-295), and as.matrix() of a sparse one.
//
// The dense side is m x n, column-major, leading dimension ld >= m in elements; every cell offset is 64-bit.  The
// compressed side is CSC arrays with by_col = 1 (a segment is a column: contiguous in the dense matrix) and CSR arrays
// with by_col = 0 (a segment is a row: strided by ld).
//
//   dense -> compressed, by_col = 1   a stable compaction over the flat cell index q = c * m + r on the tiles of
//       mx_compact_tile.h.  count: a tile's kept count, and for every column that starts inside the tile the in-tile
//       rank of its first cell; the shared finish_count scans the tile counts, and one small kernel adds each column's
//       tile offset: indptr.  fill: the same tiles again, index = r.  The padding rows r >= m are never addressed.
//   dense -> compressed, by_col = 0   panels of DN_T rows; a workgroup sweeps a range of DN_T-column chunks of its
//       panel.  count: lanes along consecutive rows (a wave reads one column of the chunk, coalesced), one count per
//       (row, split), scanned in (row, split) order by finish_count.  fill: the chunk goes through an LDS tile (read
//       with lanes along rows, compacted with lanes along columns: one ballot per tile row, written as a contiguous run
//       at the row's running offset, which stays in a register across the sweep), so rows come out sorted.
//   compressed -> dense, by_col = 1   a wave takes DN_RANGE rows of one column, 64 rows per store instruction, with a
//       cursor into the sorted segment whose entries it holds 64 at a time in registers.
//   compressed -> dense, by_col = 0   the LDS tile the other way round: four threads per tile row scatter the row's
//       entries of the current column chunk (a shared cursor per row), and the tile is stored column by column.
// compressed -> dense stores every cell of the m x n output exactly once: no memset pass, no atomics.  Every entry is
// checked against its predecessor (strictly ascending), the index bound and the range of the workgroup that owns it; an
// offending entry is never used to write and sets *flag.  The position ranges of the workgroups of one segment come
// from binary searches of the range edges and are checked to be ordered, so that they cover the segment: without a
// flag, every entry has been checked.
// The LDS tile's row stride is DN_T + 1 elements: the stores with lanes along rows (bank = row + col mod 32) and the
// reads with lanes along columns (consecutive) are both conflict-free for 4- and 8-byte elements, as are the 8-byte
// reads with lanes along rows (32-lane groups over 64 banks).
#include "mx_compact_tile.h"
#include "mx_dispatch.h"
#include "mx_workspace.h"
#include "../../include/mxgpu_dense.h"

namespace mx {

constexpr int DN_BLOCK = 256;
constexpr int DN_T = 64;                         // tile edge: one wave of rows, one wave of columns
constexpr int DN_LD = DN_T + 1;                  // LDS row stride in elements
constexpr int DN_WAVES = DN_BLOCK / MX_WAVE;
constexpr int DN_PER = DN_T / DN_WAVES;          // tile columns (or rows) per wave
constexpr int DN_RANGE = 4096;                   // rows of one column per wave, compressed -> dense by_col = 1
constexpr int DN_MAX_SPLITS = 4096;
constexpr int DN_TARGET_GROUPS = 2048;           // workgroups the chosen col_splits aims at
static_assert(DN_T == MX_WAVE && CP_BLOCK == DN_BLOCK, "a wave reads one column of the tile and writes one row of it");

// element type of a dense kind (MX_F64, MX_F32, MX_I32, MX_LGL)
template <int DK> struct DnDense { using T = int32_t; };
template <> struct DnDense<MX_F64> { using T = double; };
template <> struct DnDense<MX_F32> { using T = float; };
// element type of a compressed / dense output kind (MX_F64; MX_LGL; MX_NONE: unused)
template <int K> struct DnOut { using T = int32_t; };
template <> struct DnOut<MX_F64> { using T = double; };

using dn_dense_kinds = int_list<MX_F64, MX_F32, MX_I32, MX_LGL>;
using dn_value_kinds = int_list<MX_F64, MX_LGL, MX_NONE>;
using dn_out_kinds = int_list<MX_F64, MX_LGL>;

// the keep rule: not zero; NaN and NA count as not zero, -0.0 as zero
template <int DK>
__device__ __forceinline__ bool dn_keep(typename DnDense<DK>::T x) { return x != 0; }

// the value of a kept cell in the output kind OK
template <int DK, int OK>
__device__ __forceinline__ typename DnOut<OK>::T dn_value(typename DnDense<DK>::T x)
{
    if constexpr (OK == MX_F64) {
        if constexpr (DK == MX_F64) return x;                        // the bits, a NaN's payload included
        else if constexpr (DK == MX_F32) return (double)x;
        else return x == MX_NA_INT ? na_real() : (double)x;
    } else {
        if constexpr (DK == MX_F64 || DK == MX_F32) return isnan(x) ? MX_NA_INT : 1;
        else if constexpr (DK == MX_I32) return x == MX_NA_INT ? MX_NA_INT : 1;
        else return x;                                               // a logical is copied
    }
}

// a stored value of kind VK as a dense cell of kind OK
template <int VK, int OK>
__device__ __forceinline__ typename DnOut<OK>::T dn_cell(const void *__restrict__ values, int64_t k)
{
    if constexpr (VK == MX_NONE) {
        return 1;
    } else if constexpr (VK == MX_F64) {
        const double x = ((const double *)values)[k];
        if constexpr (OK == MX_F64) return x;
        else return isnan(x) ? MX_NA_INT : (int32_t)(x != 0);
    } else {
        const int32_t x = ((const int32_t *)values)[k];
        if constexpr (OK == MX_F64) return x == MX_NA_INT ? na_real() : (double)x;
        else return x;
    }
}

// ---- dense -> compressed, by_col = 1 ---------------------------------------------------------------------------------
// The cells of a tile in flat order: lane t holds cells base + r * CP_BLOCK + t; (col, row) of the first comes from one
// 64-bit division, the others follow by the quotient and remainder of CP_BLOCK by m.
struct DnFlat {
    int64_t col;
    int row, step_c, step_r;
    __device__ __forceinline__ DnFlat(int64_t q, int m) : col(q / m), row((int)(q - col * m)), step_c(CP_BLOCK / m),
                                                          step_r(CP_BLOCK % m) {}
    __device__ __forceinline__ void next(int m)
    {
        col += step_c;
        row += step_r;
        if (row >= m) { row -= m; col++; }
    }
};

template <typename T>
__device__ __forceinline__ void dn_load_flat(T (&a)[CP_ROUNDS], int (&row)[CP_ROUNDS], const T *__restrict__ dense,
                                             int64_t ld, int m, int64_t base, int64_t cells)
{
    DnFlat at(base + threadIdx.x, m);
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        row[r] = at.row;
        a[r] = base + r * CP_BLOCK + threadIdx.x < cells ? dense[at.col * ld + at.row] : T{};
        at.next(m);
    }
}

// tile_counts[tile] = its kept cells; out_indptr[c] = the kept cells of the tile in front of cell (0, c), for every
// column c that starts inside the tile
template <int DK>
__global__ __launch_bounds__(CP_BLOCK)
void dn_flat_count_kernel(int m, int n, const void *__restrict__ dense, int64_t ld, int32_t *__restrict__ tile_counts,
                          int32_t *__restrict__ out_indptr)
{
    using T = typename DnDense<DK>::T;
    __shared__ CpTileRanks S;
    const int64_t cells = (int64_t)m * n, base = (int64_t)blockIdx.x * CP_TILE;
    const int64_t len = cells - base < CP_TILE ? cells - base : CP_TILE;
    T v[CP_ROUNDS];
    int row[CP_ROUNDS];
    dn_load_flat(v, row, (const T *)dense, ld, m, base, cells);
    unsigned long long bal[CP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++)
        bal[r] = __ballot(base + r * CP_BLOCK + threadIdx.x < cells && dn_keep<DK>(v[r]));
    cp_rank_tile(S, bal);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = S.total;
    for (int64_t c = (base + m - 1) / m + threadIdx.x; c < n; c += CP_BLOCK) {
        const int64_t q = c * m - base;
        if (q >= len) break;
        out_indptr[c] = cp_rank_before(S, (int)q);
    }
}

// out_indptr[c] += the offset of the tile that cell (0, c) lies in; out_indptr[n] = the total
__global__ __launch_bounds__(DN_BLOCK)
void dn_flat_indptr_kernel(int m, int n, int64_t ntiles, const int32_t *__restrict__ tile_off,
                           int32_t *__restrict__ out_indptr)
{
    const int64_t c = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (c > n) return;
    if (c == n) { out_indptr[c] = tile_off[ntiles]; return; }
    const int64_t tile = c * m / CP_TILE;
    if (tile < ntiles) out_indptr[c] += tile_off[tile];
}

template <int DK, int OK>
__global__ __launch_bounds__(CP_BLOCK)
void dn_flat_fill_kernel(int m, int n, const void *__restrict__ dense, int64_t ld, const int32_t *__restrict__ tile_off,
                         const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                         void *__restrict__ out_values)
{
    using T = typename DnDense<DK>::T;
    __shared__ CpTileRanks S;
    const int lane = lane_id();
    const int64_t nnz = out_indptr[n];
    const int64_t cells = (int64_t)m * n, base = (int64_t)blockIdx.x * CP_TILE;
    T v[CP_ROUNDS];
    int row[CP_ROUNDS];
    dn_load_flat(v, row, (const T *)dense, ld, m, base, cells);
    unsigned long long bal[CP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++)
        bal[r] = __ballot(base + r * CP_BLOCK + threadIdx.x < cells && dn_keep<DK>(v[r]));
    cp_rank_tile(S, bal);
    const int64_t t0 = tile_off[blockIdx.x];
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; r++) {
        if (!((bal[r] >> lane) & 1)) continue;
        const int64_t q = t0 + cp_rank_of(S, r, bal[r]);
        if (q < 0 || q >= nnz) continue;                   // the offsets are the count pass's: bounded all the same
        out_indices[q] = row[r];
        if constexpr (OK != MX_NONE) ((typename DnOut<OK>::T *)out_values)[q] = dn_value<DK, OK>(v[r]);
    }
}

// ---- dense -> compressed, by_col = 0 ---------------------------------------------------------------------------------
// the column chunks [first, last) that split `split` of `splits` sweeps, of `chunks` in all
struct DnSweep { int first, last; };
__host__ __device__ __forceinline__ DnSweep dn_sweep(int chunks, int splits, int split)
{
    const int per = (chunks + splits - 1) / splits;
    const int64_t a = (int64_t)split * per, b = a + per;
    return {(int)(a < chunks ? a : chunks), (int)(b < chunks ? b : chunks)};
}

// counts[row * splits + split] = the kept cells of the row in the split's columns
template <int DK>
__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_count_kernel(int m, int n, const void *__restrict__ dense, int64_t ld, int splits,
                          int32_t *__restrict__ counts)
{
    using T = typename DnDense<DK>::T;
    __shared__ int s_cnt[DN_WAVES][DN_T];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const int64_t r = (int64_t)(blockIdx.x / (unsigned)splits) * DN_T + lane;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const DnSweep sw = dn_sweep((n + DN_T - 1) / DN_T, splits, split);
    int cnt = 0;
    if (r < m) {
        const T *x = (const T *)dense + r;
        for (int ch = sw.first; ch < sw.last; ch++) {
            T xv[DN_PER];                                  // all loads of the lane issued before the first use
#pragma unroll
            for (int k = 0; k < DN_PER; k++) {
                const int c = ch * DN_T + wave + k * DN_WAVES;
                xv[k] = c < n ? x[(int64_t)c * ld] : T{};
            }
#pragma unroll
            for (int k = 0; k < DN_PER; k++) cnt += dn_keep<DK>(xv[k]);
        }
    }
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && r < m) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < DN_WAVES; w++) t += s_cnt[w][lane];
        counts[r * splits + split] = t;
    }
}

// out_indptr[r] = offsets[r * splits] for r in [0, m]
__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_indptr_kernel(int m, int splits, const int32_t *__restrict__ offsets, int32_t *__restrict__ out_indptr)
{
    const int64_t r = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (r <= m) out_indptr[r] = offsets[r * splits];
}

template <int DK, int OK>
__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_fill_kernel(int m, int n, const void *__restrict__ dense, int64_t ld, int splits,
                         const int32_t *__restrict__ offsets, const int32_t *__restrict__ out_indptr,
                         int32_t *__restrict__ out_indices, void *__restrict__ out_values)
{
    using T = typename DnDense<DK>::T;
    __shared__ T s_tile[DN_T * DN_LD];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const int64_t nnz = out_indptr[m];
    const int64_t r0 = (int64_t)(blockIdx.x / (unsigned)splits) * DN_T;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const DnSweep sw = dn_sweep((n + DN_T - 1) / DN_T, splits, split);
    // the running offsets of the rows this wave compacts (tile rows wave, wave + DN_WAVES, ...): wave-uniform
    int64_t run[DN_PER];
#pragma unroll
    for (int k = 0; k < DN_PER; k++) {
        const int64_t row = r0 + wave + k * DN_WAVES;
        run[k] = row < m ? offsets[row * splits + split] : 0;
    }
    const int64_t r = r0 + lane;
    const T *x = (const T *)dense + r;
    for (int ch = sw.first; ch < sw.last; ch++) {
        const int c0 = ch * DN_T;
        // lane = row of the tile
        T xv[DN_PER];
#pragma unroll
        for (int k = 0; k < DN_PER; k++) {
            const int c = c0 + wave + k * DN_WAVES;
            xv[k] = r < m && c < n ? x[(int64_t)c * ld] : T{};
        }
#pragma unroll
        for (int k = 0; k < DN_PER; k++) s_tile[lane * DN_LD + wave + k * DN_WAVES] = xv[k];
        __syncthreads();
        // lane = column of the tile
        const int c = c0 + lane;
#pragma unroll
        for (int k = 0; k < DN_PER; k++) {
            const T v = s_tile[(wave + k * DN_WAVES) * DN_LD + lane];
            const unsigned long long bal = __ballot(c < n && dn_keep<DK>(v));      // rows past m hold zeros
            const int64_t q = run[k] + __popcll(bal & ((1ull << lane) - 1));
            if (((bal >> lane) & 1) && q >= 0 && q < nnz) {
                out_indices[q] = c;
                if constexpr (OK != MX_NONE) ((typename DnOut<OK>::T *)out_values)[q] = dn_value<DK, OK>(v);
            }
            run[k] += __popcll(bal);
        }
        __syncthreads();
    }
}

// ---- compressed -> dense, by_col = 1 ---------------------------------------------------------------------------------
// first position in [0, count) whose index is >= key (any content: the probes stay inside the segment)
__device__ __forceinline__ int64_t dn_edge(const int32_t *__restrict__ idx, int64_t start, int64_t len, int64_t key)
{
    return start + lower_bound_dev(idx + start, (int)len, (int)(key < INT_MAX ? key : INT_MAX));
}

template <int VK, int OK>
__global__ __launch_bounds__(DN_BLOCK)
void dn_cols_to_dense_kernel(int nseg, int nother, int blocks_per_seg, const int32_t *__restrict__ indptr,
                             const int32_t *__restrict__ indices, const void *__restrict__ values,
                             void *__restrict__ out, int64_t ld, int32_t *__restrict__ flag)
{
    using O = typename DnOut<OK>::T;
    __shared__ O s_row[DN_WAVES][MX_WAVE];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const int64_t item = (int64_t)blockIdx.x * DN_WAVES + wave;
    if (item >= (int64_t)nseg * blocks_per_seg) return;          // no barrier below: waves are on their own
    const int seg = (int)(item / blocks_per_seg), blk = (int)(item % blocks_per_seg);
    const int64_t nnz = indptr[nseg];
    const RowBounds rb = row_bounds(indptr[seg], indptr[seg + 1], nnz);
    const int lo = blk * DN_RANGE;
    const int hi = blk == blocks_per_seg - 1 ? nother : lo + DN_RANGE;
    // the positions this wave owns: [pa, pb), from the range edges; in order, or the segment is not sorted
    const int64_t pa = blk == 0 ? rb.start : dn_edge(indices, rb.start, rb.len, lo);
    const int64_t pb = blk == blocks_per_seg - 1 ? rb.start + rb.len : dn_edge(indices, rb.start, rb.len, hi);
    bool bad = pa > pb;
    O *o = (O *)out + (int64_t)seg * ld;
    // a batch: the entries at positions [bcur, bcur + 64), one a lane; cur: the first one not consumed yet
    int64_t bcur = pa, cur = pa;
    int idx = 0;
    bool have = false, ok = false;
    O val = O{};
    auto load_batch = [&]() {
        const int64_t k = bcur + lane;
        have = k < pb;
        idx = have ? indices[k] : 0;
        int pred = __shfl_up(idx, 1, MX_WAVE);
        if (lane == 0) pred = have && k > rb.start ? indices[k - 1] : -1;
        ok = have && idx >= lo && idx < hi && idx > pred;
        bad |= have && !ok;
        val = ok ? dn_cell<VK, OK>(values, k) : O{};
    };
    load_batch();
    for (int i0 = lo; i0 < hi; i0 += MX_WAVE) {
        s_row[wave][lane] = O{};
        while (true) {
            // consumed here: from cur on, every entry up to the first valid one of a later chunk
            const int off = (int)(cur - bcur);
            const bool through = lane < off || (have && (!ok || idx < i0 + MX_WAVE));
            const unsigned long long stop = ~__ballot(through);
            const int upto = stop ? __ffsll((long long)stop) - 1 : MX_WAVE;
            if (ok && lane >= off && lane < upto && idx >= i0) s_row[wave][idx - i0] = val;
            cur = bcur + upto;
            if (upto < MX_WAVE || cur >= pb) break;
            bcur = cur;
            load_batch();
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (i0 + lane < hi) o[i0 + lane] = s_row[wave][lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (bad || cur < pb) *flag = 1;                         // an entry the walk never reached has no row to go to
}

// ---- compressed -> dense, by_col = 0 ---------------------------------------------------------------------------------
template <int VK, int OK>
__global__ __launch_bounds__(DN_BLOCK)
void dn_rows_to_dense_kernel(int nseg, int nother, int splits, const int32_t *__restrict__ indptr,
                             const int32_t *__restrict__ indices, const void *__restrict__ values,
                             void *__restrict__ out, int64_t ld, int32_t *__restrict__ flag)
{
    using O = typename DnOut<OK>::T;
    __shared__ O s_tile[DN_T * DN_LD];
    __shared__ int64_t s_stop[DN_WAVES][DN_T];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    const int64_t r0 = (int64_t)(blockIdx.x / (unsigned)splits) * DN_T;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const DnSweep sw = dn_sweep((nother + DN_T - 1) / DN_T, splits, split);
    // the split's columns are [lo, edge); its positions in a row run from the edge lo to the edge `edge`, so that the
    // splits of a row meet, and an index in [nother, edge) is checked by the split that owns its position
    const int lo = sw.first * DN_T;
    const int64_t edge = (int64_t)sw.last * DN_T;
    const int hi = edge < nother ? (int)edge : nother;
    // lane = row of the tile; the four waves share the row's cursor and take every fourth entry from it
    const int64_t r = r0 + lane;
    const int64_t nnz = indptr[nseg];
    RowBounds rb = {0, 0};
    if (r < nseg) rb = row_bounds(indptr[r], indptr[r + 1], nnz);
    const int64_t pa = split == 0 ? rb.start : dn_edge(indices, rb.start, rb.len, lo);
    const int64_t pb = split == splits - 1 ? rb.start + rb.len : dn_edge(indices, rb.start, rb.len, edge);
    bool bad = pa > pb;
    int64_t cur = pa;
#pragma unroll
    for (int k = 0; k < DN_PER; k++) s_tile[lane * DN_LD + wave + k * DN_WAVES] = O{};
    __syncthreads();
    O *o = (O *)out + r;
    for (int ch = sw.first; ch < sw.last; ch++) {
        const int c0 = ch * DN_T;
        const int c1 = c0 + DN_T < hi ? c0 + DN_T : hi;
        int64_t k = cur + wave;
        while (k < pb) {
            const int idx = indices[k];
            const int pred = k > rb.start ? indices[k - 1] : -1;
            const bool ok = idx >= lo && idx < hi && idx > pred;
            if (ok && idx >= c1) break;
            bad |= !ok;
            if (ok && idx >= c0) s_tile[lane * DN_LD + idx - c0] = dn_cell<VK, OK>(values, k);
            k += DN_WAVES;
        }
        s_stop[wave][lane] = k < pb ? k : pb;
        __syncthreads();
        cur = s_stop[0][lane];
#pragma unroll
        for (int w = 1; w < DN_WAVES; w++) cur = s_stop[w][lane] < cur ? s_stop[w][lane] : cur;
        // the tile goes out column by column, 64 consecutive rows a store, and is zero again behind it
#pragma unroll
        for (int q = 0; q < DN_PER; q++) {
            const int col = wave + q * DN_WAVES;
            const O v = s_tile[lane * DN_LD + col];
            s_tile[lane * DN_LD + col] = O{};
            if (r < nseg && c0 + col < c1) o[(int64_t)(c0 + col) * ld] = v;
        }
        __syncthreads();
    }
    // a split without a column (more splits than chunks) walks nothing: an entry in its positions has no cell to go to
    if (bad || cur < pb) *flag = 1;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int64_t dn_tiles(int64_t cells) { return ceil_div(cells > 0 ? cells : 0, CP_TILE); }
static int64_t dn_panels(int m) { return ceil_div(m > 0 ? m : 0, DN_T); }

// col_splits as the kernels use it: a positive value as given, else enough splits for DN_TARGET_GROUPS workgroups
static int dn_splits(int rows, int cols, int col_splits)
{
    if (col_splits > 0) return col_splits;
    const int64_t panels = dn_panels(rows), chunks = ceil_div(cols > 0 ? cols : 0, DN_T);
    if (panels == 0 || chunks == 0) return 1;
    int64_t s = ceil_div(DN_TARGET_GROUPS, panels);
    s = s < chunks ? s : chunks;
    return (int)(s < 1 ? 1 : s > DN_MAX_SPLITS ? DN_MAX_SPLITS : s);
}

// by_col = 1: a count and an offset per tile; by_col = 0: a count and an offset per (row, split)
struct DenseLayout : CountOffsetsLayout {
    DenseLayout(const void *ws, int m, int n, int by_col, int col_splits)
        : CountOffsetsLayout(ws, by_col ? dn_tiles((int64_t)m * n) : (int64_t)m * dn_splits(m, n, col_splits)) {}
};

static int dn_check(const char *what, int m, int n, int64_t ld, int dense_dtype, int by_col, int col_splits)
{
    MX_REQUIRE(m >= 0 && n >= 0, "%s: negative dimension", what);
    MX_REQUIRE(m < INT_MAX && n < INT_MAX, "%s: dimension too large", what);
    MX_REQUIRE(ld >= m, "%s: ld %lld is smaller than the %d rows", what, (long long)ld, m);
    MX_REQUIRE(dense_dtype == MX_F64 || dense_dtype == MX_F32 || dense_dtype == MX_I32 || dense_dtype == MX_LGL,
               "%s: unsupported dense dtype %d", what, dense_dtype);
    MX_REQUIRE(col_splits >= 0 && col_splits <= DN_MAX_SPLITS, "%s: col_splits must be in [0, %d]", what, DN_MAX_SPLITS);
    if (by_col) MX_REQUIRE(dn_tiles((int64_t)m * n) < INT_MAX, "%s: dense operand too large", what);
    else MX_REQUIRE((int64_t)m * dn_splits(m, n, col_splits) < INT_MAX && dn_panels(m) * dn_splits(m, n, col_splits) < INT_MAX,
                    "%s: dense operand too large", what);
    return 0;
}

}  // namespace mx

extern "C" size_t mxd_dense_to_csr_workspace_bytes(int m, int n, int by_col, int col_splits)
{
    if (m < 0 || n < 0 || col_splits < 0 || col_splits > mx::DN_MAX_SPLITS) return 0;
    return mx::DenseLayout(nullptr, m, n, by_col, col_splits).bytes;
}

extern "C" int mxd_dense_to_csr_count(int m, int n, const void *dense, int64_t ld, int dense_dtype, int by_col,
                                      int col_splits, int32_t *out_indptr, void *workspace, int64_t *nnz_host,
                                      void *stream)
{
    const char *what = "mxd_dense_to_csr_count";
    if (mx::dn_check(what, m, n, ld, dense_dtype, by_col, col_splits)) return 1;
    const int64_t cells = (int64_t)m * n;
    MX_REQUIRE(out_indptr && nnz_host && (cells == 0 || (dense && workspace)), "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    *nnz_host = 0;
    const int nseg = by_col ? n : m;
    if (cells == 0) {
        MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)nseg + 1), st));
        MX_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const mx::DenseLayout L(workspace, m, n, by_col, col_splits);
    if (by_col) {
        const int64_t tiles = mx::dn_tiles(cells);
        int rc = mx::dispatch_int(mx::dn_dense_kinds{}, what, "dense dtype", dense_dtype, [&](auto dk) {
            hipLaunchKernelGGL(mx::dn_flat_count_kernel<dk()>, dim3((unsigned)tiles), dim3(mx::CP_BLOCK), 0, st, m, n,
                               dense, ld, L.counts, out_indptr);
            MX_LAUNCH_CHECK();
            return 0;
        });
        if (rc) return rc;
        if (mx::finish_count(tiles, L.counts, L.offsets, nnz_host, st)) return 1;
        hipLaunchKernelGGL(mx::dn_flat_indptr_kernel, dim3(mx::grid_for((int64_t)n + 1, mx::DN_BLOCK)),
                           dim3(mx::DN_BLOCK), 0, st, m, n, tiles, L.offsets, out_indptr);
        MX_LAUNCH_CHECK();
        return 0;
    }
    const int splits = mx::dn_splits(m, n, col_splits);
    const int64_t groups = mx::dn_panels(m) * splits;
    int rc = mx::dispatch_int(mx::dn_dense_kinds{}, what, "dense dtype", dense_dtype, [&](auto dk) {
        hipLaunchKernelGGL(mx::dn_rows_count_kernel<dk()>, dim3((unsigned)groups), dim3(mx::DN_BLOCK), 0, st, m, n, dense,
                           ld, splits, L.counts);
        MX_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    if (mx::finish_count((int64_t)m * splits, L.counts, L.offsets, nnz_host, st)) return 1;
    hipLaunchKernelGGL(mx::dn_rows_indptr_kernel, dim3(mx::grid_for((int64_t)m + 1, mx::DN_BLOCK)), dim3(mx::DN_BLOCK), 0,
                       st, m, splits, L.offsets, out_indptr);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" int mxd_dense_to_csr_fill(int m, int n, const void *dense, int64_t ld, int dense_dtype, int by_col,
                                     int col_splits, const int32_t *out_indptr, const void *workspace,
                                     int32_t *out_indices, void *out_values, int out_dtype, void *stream)
{
    const char *what = "mxd_dense_to_csr_fill";
    if (mx::dn_check(what, m, n, ld, dense_dtype, by_col, col_splits)) return 1;
    MX_REQUIRE(out_dtype == MX_F64 || out_dtype == MX_LGL || out_dtype == MX_NONE, "%s: unsupported output dtype %d", what,
               out_dtype);
    const int64_t cells = (int64_t)m * n;
    if (cells == 0) return 0;
    MX_REQUIRE(dense && out_indptr && workspace && out_indices && (out_dtype == MX_NONE || out_values), "%s: null pointer",
               what);
    hipStream_t st = mx::as_stream(stream);
    const mx::DenseLayout L(workspace, m, n, by_col, col_splits);
    const int splits = mx::dn_splits(m, n, col_splits);
    return mx::dispatch_int(mx::dn_dense_kinds{}, what, "dense dtype", dense_dtype, [&](auto dk) {
        return mx::dispatch_int(mx::dn_value_kinds{}, what, "output dtype", out_dtype, [&](auto ok) {
            if (by_col)
                hipLaunchKernelGGL((mx::dn_flat_fill_kernel<dk(), ok()>), dim3((unsigned)mx::dn_tiles(cells)),
                                   dim3(mx::CP_BLOCK), 0, st, m, n, dense, ld, L.offsets, out_indptr, out_indices, out_values);
            else
                hipLaunchKernelGGL((mx::dn_rows_fill_kernel<dk(), ok()>), dim3((unsigned)(mx::dn_panels(m) * splits)),
                                   dim3(mx::DN_BLOCK), 0, st, m, n, dense, ld, splits, L.offsets, out_indptr, out_indices,
                                   out_values);
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
}

extern "C" int mxd_csr_to_dense(int nseg, int nother, const int32_t *indptr, const int32_t *indices, const void *values,
                                int value_dtype, int by_col, int col_splits, void *out, int64_t ld, int out_dtype,
                                int32_t *flag_dev, void *stream)
{
    const char *what = "mxd_csr_to_dense";
    MX_REQUIRE(nseg >= 0 && nother >= 0, "%s: negative dimension", what);
    MX_REQUIRE(nseg < INT_MAX && nother < INT_MAX, "%s: dimension too large", what);
    const int m = by_col ? nother : nseg;
    MX_REQUIRE(ld >= m, "%s: ld %lld is smaller than the %d rows", what, (long long)ld, m);
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE, "%s: unsupported value dtype %d",
               what, value_dtype);
    MX_REQUIRE(out_dtype == MX_F64 || out_dtype == MX_LGL, "%s: unsupported output dtype %d", what, out_dtype);
    MX_REQUIRE(col_splits >= 0 && col_splits <= mx::DN_MAX_SPLITS, "%s: col_splits must be in [0, %d]", what,
               mx::DN_MAX_SPLITS);
    if (nseg == 0 || nother == 0) return 0;
    MX_REQUIRE(indptr && out && flag_dev, "%s: null pointer", what);
    // indices and values may be null for a matrix without entries only, which the kernels never read
    hipStream_t st = mx::as_stream(stream);
    const int blocks_per_seg = (int)mx::ceil_div(nother, mx::DN_RANGE);
    const int splits = mx::dn_splits(nseg, nother, col_splits);
    const int64_t groups = by_col ? mx::ceil_div((int64_t)nseg * blocks_per_seg, mx::DN_WAVES) : mx::dn_panels(nseg) * splits;
    MX_REQUIRE(groups < INT_MAX, "%s: matrix too large", what);
    return mx::dispatch_int(mx::dn_value_kinds{}, what, "value dtype", value_dtype, [&](auto vk) {
        return mx::dispatch_int(mx::dn_out_kinds{}, what, "output dtype", out_dtype, [&](auto ok) {
            if (by_col)
                hipLaunchKernelGGL((mx::dn_cols_to_dense_kernel<vk(), ok()>), dim3((unsigned)groups), dim3(mx::DN_BLOCK), 0,
                                   st, nseg, nother, blocks_per_seg, indptr, indices, values, out, ld, flag_dev);
            else
                hipLaunchKernelGGL((mx::dn_rows_to_dense_kernel<vk(), ok()>), dim3((unsigned)groups), dim3(mx::DN_BLOCK), 0,
                                   st, nseg, nother, splits, indptr, indices, values, out, ld, flag_dev);
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
}

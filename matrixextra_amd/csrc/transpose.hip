// transpose.hip — stable device transpose of a CSR structure (t_deep, CSR <-> CSC).
//
// The CSC arrays of a matrix are the CSR arrays of its transpose, so one routine serves CSR -> CSR of X^T
// (t_deep_internal, R/trans.R:46-56), CSR -> CSC (as.csc.matrix) and CSC -> CSR (as.csr.matrix of a dgCMatrix).
//
// Output row c of the transpose holds the source rows of every input entry in column c, in strictly ascending
// source-row order whatever the order inside the input rows.  The transpose is a stable sort of the row-major
// entries by column, done as an LSD radix sort with 8-bit digits (one pass when n <= 256, else
// ceil(bits(n-1) / 8)), carrying the entry index k and the source row as payloads:
//
//   per pass    count:   per-tile digit counts -> table[digit][tile]          (no global atomics: a hot column,
//               scan:    exclusive scan of the table (exclusive_scan_i32)      such as cbind(1, X)'s intercept,
//               scatter: stable in-tile rank from wave64 ballots + a            costs what any column costs)
//                        per-wave count table in LDS, tile staged in LDS in digit order, then plain stores of
//                        each digit's contiguous run; pass 0 finds source rows by a binary search of indptr
//                        over the rows its tile spans
//   gather      out_indices[q] = carried row, out_values[q] = values[perm[q]] (bit copies), duplicate flag
//   indptr      out_indptr[c] = first q with sorted key >= c (binary search, one thread per column)
//
// Column indices are checked where they are first read (pass 0's count and scatter): an index outside [0, n)
// raises the error flag and is replaced by 0 before it is used, so bad input is reported, never written out of
// bounds.  Later passes read only the clamped keys.
//
// Duplicates, (row, col) pairs that occur more than once in one input row, end up adjacent after the sort.  The
// gather pass flags them for the cost of one compare per entry; only when the flag is set does a compaction
// run: heads -> scan -> merge each run in source order -> remap indptr.  The merge rule is what Matrix's
// TsparseMatrix coercion (which t_deep_internal goes through) does to repeated triplets: f64 values are summed
// in source order, R logicals are combined with R's `|`, pattern entries collapse to one.  The logical rule is
// Matrix's documented behaviour for l-sparse triplets; it was not re-checked against a running R (none was
// available when this was written).
// Each run is merged by one thread, sequentially, because an f64 sum in source order is sequential.
//
// COO -> CSR (mxd_coo_to_csr, at the end of this file) runs the same passes twice: pass 0 can take the source
// rows from the caller instead of an indptr search (TP_SRC_ROWS).  The sort of a sparse vector
// (mxd_sort_vector_indices, after it) runs them once, on one key.  The sort of COO triplets (mxd_coo_sort, last)
// runs them on both keys, the second run taking up the first run's permutation, and gathers the values once.
// The column order of a CSR pattern (mxd_csr_column_order, after the transpose) is the transpose's passes and its
// indptr step without the gather: the permutation itself is the result.
#include "mx_dispatch.h"
#include "mx_reduce.h"
#include "mx_workspace.h"

namespace mx {

constexpr int TP_BLOCK = 256;
constexpr int TP_ITEMS = 16;
constexpr int TP_WAVES = TP_BLOCK / MX_WAVE;
constexpr int TP_TILE = TP_BLOCK * TP_ITEMS;            // 4096 entries per tile
constexpr int TP_WAVE_SPAN = MX_WAVE * TP_ITEMS;        // each wave owns 1024 consecutive entries of its tile
constexpr int TP_RADIX = 256;
static_assert(TP_BLOCK == TP_RADIX, "the per-digit prefix step uses one thread per digit");

// flags in the workspace: [0] a column index outside [0, n), [1] duplicates present
constexpr size_t TP_FLAG_BYTES = 256;
// the sparse-vector sort keeps its words in the same block, clear of the transpose's [0..1] and of COO stage 1's [4..7]
constexpr int TP_SV_PASS_FLAGS = 8;      // [8..11] the radix passes' flags (bad key, duplicates, bad row)
constexpr int TP_SV_WORDS = 16;          // [16..18] the sortedness reduction: descents, largest index, negative index
static_assert((TP_SV_WORDS + 3) * sizeof(int32_t) <= TP_FLAG_BYTES, "the sort's words lie inside the flag block");
// the COO sort's words: [24..26] its passes' flags, [32..35] descents, largest row, negative index, largest column
constexpr int TP_COO_PASS_FLAGS = 24;
constexpr int TP_COO_WORDS = 32;
static_assert((TP_COO_WORDS + 4) * sizeof(int32_t) <= TP_FLAG_BYTES, "the COO sort's words lie inside the flag block");

// last row r in [lo, m) with indptr[r] <= k (indptr[lo] <= k holds for every caller)
__device__ __forceinline__ int tp_row_of(const int32_t *__restrict__ indptr, int lo, int m, int64_t k)
{
    int hi = m;
    while (hi - lo > 1) {
        const int mid = (int)(((int64_t)lo + hi) >> 1);
        if (indptr[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

// lanes of the wave holding the same digit (nbits significant low bits) as this lane, among the valid lanes
__device__ __forceinline__ uint64_t tp_peers(int d, bool valid, int nbits)
{
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < nbits; b++) {
        const bool bit = (d >> b) & 1;
        const uint64_t bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// pass 0 reads the caller's indices: check before the key is used anywhere
template <bool FIRST>
__device__ __forceinline__ int tp_load_key(const int32_t *__restrict__ keys, int64_t k, int n, bool &bad)
{
    int key = keys[k];
    if (FIRST && (unsigned)key >= (unsigned)n) { bad = true; key = 0; }
    return key;
}

// per-tile digit counts -> table[d * ntiles + tile]
template <bool FIRST>
__global__ __launch_bounds__(TP_BLOCK)
void tp_count_kernel(const int32_t *__restrict__ keys, int64_t nnz, int n, int shift, int nbits, int ntiles,
                     int32_t *__restrict__ table, int32_t *__restrict__ flags)
{
    __shared__ int32_t hist[TP_WAVES][TP_RADIX];
    for (int i = threadIdx.x; i < TP_WAVES * TP_RADIX; i += TP_BLOCK) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int wave = threadIdx.x / MX_WAVE, lane = lane_id();
    const int64_t base = (int64_t)blockIdx.x * TP_TILE + wave * TP_WAVE_SPAN;
    bool bad = false;
    for (int it = 0; it < TP_ITEMS; it++) {
        const int64_t k = base + it * MX_WAVE + lane;
        const bool valid = k < nnz;
        const int key = valid ? tp_load_key<FIRST>(keys, k, n, bad) : 0;
        const int d = (key >> shift) & (TP_RADIX - 1);
        const uint64_t peers = tp_peers(d, valid, nbits);
        // one add per (wave, digit) group, by the group's lowest lane; the table is private to the wave
        if (valid && lane == __builtin_ctzll(peers)) hist[wave][d] += __popcll(peers);
    }
    if (FIRST && bad) flags[0] = 1;
    __syncthreads();
    const int d = threadIdx.x;
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TP_WAVES; w++) sum += hist[w][d];
    table[(int64_t)d * ntiles + blockIdx.x] = sum;
}

// Stable scatter of one tile.  Each entry's slot in the tile's digit-sorted order is the tile-local start of its
// digit + the counts of earlier waves + its rank inside the wave; the tile is staged in LDS in that order and
// written out slot by slot, so consecutive lanes store consecutive positions of one digit's run (global position =
// offset of (digit, tile) + slot - tile-local start of the digit).
// Payloads: the entry index k (for the values, gathered once at the end) and the source row.  Pass 0 finds the
// rows of its tile's consecutive entries by a binary search of indptr over the rows the tile spans, staged in LDS
// when there are at most TP_SPAN_CAP of them.
constexpr int TP_SPAN_CAP = 1024;

// SRC: where the pass reads its source rows.  TP_SRC_SORTED: a later pass (rows_in / perm_in of the previous
// pass); TP_SRC_INDPTR: pass 0 of a CSR (binary search of indptr); TP_SRC_ROWS: pass 0 of a COO (the caller's
// row ids in rows_in, checked against [0, m) where they are read: a bad one sets flags[2] and is replaced by 0).
enum { TP_SRC_SORTED = 0, TP_SRC_INDPTR = 1, TP_SRC_ROWS = 2 };

template <int SRC>
__global__ __launch_bounds__(TP_BLOCK)
void tp_scatter_kernel(const int32_t *__restrict__ keys_in, const int32_t *__restrict__ perm_in,
                       const int32_t *__restrict__ rows_in, const int32_t *__restrict__ indptr, int m, int64_t nnz,
                       int n, int shift, int nbits, int ntiles, const int32_t *__restrict__ offsets,
                       int32_t *__restrict__ keys_out, int32_t *__restrict__ perm_out, int32_t *__restrict__ rows_out,
                       int32_t *__restrict__ flags)
{
    constexpr bool FIRST = SRC != TP_SRC_SORTED;
    constexpr bool SEARCH = SRC == TP_SRC_INDPTR;
    __shared__ int32_t cnt[TP_WAVES][TP_RADIX];
    __shared__ int32_t delta[TP_RADIX];
    __shared__ int32_t stage[3][TP_TILE];              // keys, entry index, row in slot order (48 KiB)
    __shared__ int32_t span_ptr[SEARCH ? TP_SPAN_CAP : 1];
    __shared__ int32_t row_span[2];
    __shared__ int32_t wave_tot[TP_WAVES];
    const int64_t t0 = (int64_t)blockIdx.x * TP_TILE;
    for (int i = threadIdx.x; i < TP_WAVES * TP_RADIX; i += TP_BLOCK) (&cnt[0][0])[i] = 0;
    if (SEARCH && threadIdx.x < 2) {
        const int64_t k = threadIdx.x == 0 ? t0 : (t0 + TP_TILE - 1 < nnz ? t0 + TP_TILE - 1 : nnz - 1);
        row_span[threadIdx.x] = tp_row_of(indptr, 0, m, k);
    }
    __syncthreads();
    int r0 = 0, nspan = 0;
    if (SEARCH) {
        r0 = row_span[0];
        nspan = row_span[1] - r0 + 1;
        if (nspan <= TP_SPAN_CAP)
            for (int i = threadIdx.x; i < nspan; i += TP_BLOCK) span_ptr[i] = indptr[r0 + i];
        __syncthreads();
    }
    const int wave = threadIdx.x / MX_WAVE, lane = lane_id();
    const uint64_t lt_mask = (1ULL << lane) - 1;
    const int64_t base = t0 + wave * TP_WAVE_SPAN;
    int key[TP_ITEMS], rank[TP_ITEMS], pay[TP_ITEMS], row[TP_ITEMS];
    bool bad = false, bad_row = false;
#pragma unroll
    for (int it = 0; it < TP_ITEMS; it++) {
        const int64_t k = base + it * MX_WAVE + lane;
        const bool valid = k < nnz;
        key[it] = valid ? tp_load_key<FIRST>(keys_in, k, n, bad) : 0;
        pay[it] = valid ? (FIRST ? (int)k : perm_in[k]) : 0;
        if (!SEARCH) {
            row[it] = valid ? rows_in[k] : 0;
            if (SRC == TP_SRC_ROWS && (unsigned)row[it] >= (unsigned)m) { bad_row = true; row[it] = 0; }
        } else if (!valid) {
            row[it] = 0;
        } else if (nspan <= TP_SPAN_CAP) {          // last r in the span with indptr[r] <= k
            int lo = 0, hi = nspan;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (span_ptr[mid] <= k) lo = mid; else hi = mid;
            }
            row[it] = r0 + lo;
        } else {
            row[it] = tp_row_of(indptr, r0, row_span[1] + 1, k);
        }
        const int d = (key[it] >> shift) & (TP_RADIX - 1);
        const uint64_t peers = tp_peers(d, valid, nbits);
        const int before = valid ? cnt[wave][d] : 0;
        rank[it] = before + __popcll(peers & lt_mask);
        if (valid && lane == __builtin_ctzll(peers)) cnt[wave][d] = before + __popcll(peers);
    }
    if (SRC == TP_SRC_ROWS && bad_row) flags[2] = 1;
    __syncthreads();
    {   // one thread per digit: tile-local start of the digit (block exclusive scan of the digit totals), then
        // cnt[w][d] -> first slot of wave w's digit-d entries, delta[d] -> global position of slot 0
        const int d = threadIdx.x;
        int total = 0;
#pragma unroll
        for (int w = 0; w < TP_WAVES; w++) total += cnt[w][d];
        int incl = total;
#pragma unroll
        for (int off = 1; off < MX_WAVE; off <<= 1) {
            const int o = __shfl_up(incl, off, MX_WAVE);
            if (lane >= off) incl += o;
        }
        if (lane == MX_WAVE - 1) wave_tot[wave] = incl;
        __syncthreads();
        int start = incl - total;
        for (int w = 0; w < wave; w++) start += wave_tot[w];
        delta[d] = offsets[(int64_t)d * ntiles + blockIdx.x] - start;
        int run = start;
#pragma unroll
        for (int w = 0; w < TP_WAVES; w++) { const int c = cnt[w][d]; cnt[w][d] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < TP_ITEMS; it++) {
        if (base + it * MX_WAVE + lane >= nnz) break;
        const int slot = cnt[wave][(key[it] >> shift) & (TP_RADIX - 1)] + rank[it];
        stage[0][slot] = key[it];
        stage[1][slot] = pay[it];
        stage[2][slot] = row[it];
    }
    __syncthreads();
    const int tile_n = nnz - t0 < TP_TILE ? (int)(nnz - t0) : TP_TILE;
    for (int i = threadIdx.x; i < tile_n; i += TP_BLOCK) {
        const int kk = stage[0][i];
        const int pos = delta[(kk >> shift) & (TP_RADIX - 1)] + i;
        keys_out[pos] = kk;
        perm_out[pos] = stage[1][i];
        rows_out[pos] = stage[2][i];
    }
}

// out_rows[q] / out_values[q] from the sorted permutation; flags[1] = 1 when two neighbours are the same (col, row)
template <typename VT, bool HAS_VALUES>
__global__ __launch_bounds__(256)
void tp_gather_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ perm, int64_t nnz,
                      const int32_t *__restrict__ rows, const VT *__restrict__ values, int32_t *__restrict__ out_rows,
                      VT *__restrict__ out_values, int32_t *__restrict__ flags)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const bool valid = q < nnz;
    int key = -1, row = -1;
    if (valid) {
        row = rows[q];
        key = keys[q];
        out_rows[q] = row;
        if (HAS_VALUES) out_values[q] = values[perm[q]];
    }
    int pkey = __shfl_up(key, 1, MX_WAVE), prow = __shfl_up(row, 1, MX_WAVE);
    if (lane == 0 && valid && q > 0) { pkey = keys[q - 1]; prow = rows[q - 1]; }
    const bool dup = valid && q > 0 && pkey == key && prow == row;
    if (__ballot(dup) != 0ULL && lane == 0) flags[1] = 1;
}

// out_indptr[c] = number of sorted keys < c, for c in [0, n]
__global__ __launch_bounds__(256)
void tp_indptr_kernel(const int32_t *__restrict__ keys, int64_t nnz, int64_t n, int32_t *__restrict__ out_indptr)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, count = nnz;
        while (count > 0) {
            const int64_t step = count >> 1;
            if (keys[lo + step] < c) { lo += step + 1; count -= step + 1; }
            else count = step;
        }
        out_indptr[c] = (int32_t)lo;
    }
}

// ---- duplicate compaction (runs only when the gather pass saw duplicates) --------------------------------
__device__ __forceinline__ bool tp_is_head(const int32_t *__restrict__ keys, const int32_t *__restrict__ rows,
                                           int64_t q)
{
    return q == 0 || keys[q] != keys[q - 1] || rows[q] != rows[q - 1];
}

__global__ __launch_bounds__(256)
void tp_heads_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ rows, int64_t nnz,
                     int32_t *__restrict__ heads)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nnz) heads[q] = tp_is_head(keys, rows, q) ? 1 : 0;
}

// VK: 0 f64 (sum in source order), 1 R logical (R's `|`), 2 pattern (one entry)
template <int VK>
__global__ __launch_bounds__(256)
void tp_merge_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ rows, const void *__restrict__ vals,
                     int64_t nnz, const int32_t *__restrict__ newpos, int32_t *__restrict__ merged_rows,
                     void *__restrict__ merged_vals)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz || !tp_is_head(keys, rows, q)) return;
    const int64_t dest = newpos[q];
    merged_rows[dest] = rows[q];
    int64_t e = q + 1;
    if (VK == 0) {
        const double *v = (const double *)vals;
        double acc = v[q];
        for (; e < nnz && !tp_is_head(keys, rows, e); e++) acc += v[e];
        ((double *)merged_vals)[dest] = acc;
    } else if (VK == 1) {
        const int32_t *v = (const int32_t *)vals;
        int acc = v[q];
        for (; e < nnz && !tp_is_head(keys, rows, e); e++) acc = r_logical_or(acc, v[e]);
        ((int32_t *)merged_vals)[dest] = acc;
    }
}

__global__ __launch_bounds__(256)
void tp_remap_indptr_kernel(int64_t n, const int32_t *__restrict__ newpos, int32_t *__restrict__ indptr)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n; c += (int64_t)gridDim.x * blockDim.x)
        indptr[c] = newpos[indptr[c]];
}

// ---- host side ----------------------------------------------------------------------------------------------
static int64_t tp_ntiles(int64_t nnz) { return ceil_div(nnz > 0 ? nnz : 1, TP_TILE); }

static size_t tp_scan_ws_bytes(int64_t nnz)
{
    const size_t a = scan_workspace_bytes(TP_RADIX * tp_ntiles(nnz)), b = scan_workspace_bytes(nnz);
    return ((a > b ? a : b) + 15) & ~(size_t)15;
}

// nnz values of 8 bytes, padded to 16 B
static size_t tp_f64_bytes(int64_t nnz) { return ((size_t)8 * (size_t)(nnz > 0 ? nnz : 1) + 15) & ~(size_t)15; }

// The radix passes' workspace.  Each keys/perm pair is contiguous, so a free pair also holds nnz doubles during
// compaction.
struct TpLayout {
    WsCursor c;
    int64_t nnz;
    int32_t *flags = c.take<int32_t>(TP_FLAG_BYTES);
    int32_t *keys[2], *perm[2], *rows[2];   // double-buffered: keys and rows nnz + 1, perm nnz
    int32_t *table, *offsets;               // digit counts per tile (T = TP_RADIX * tiles), scanned into T + 1
    void *scan_ws;
    size_t bytes;
    TpLayout(const void *ws, int64_t nnz_) : c(ws), nnz(nnz_ > 0 ? nnz_ : 0)
    {
        const int64_t T = TP_RADIX * tp_ntiles(nnz);
        for (int b = 0; b < 2; b++) {
            keys[b] = c.take_i32(nnz + 1);
            perm[b] = c.take_i32(nnz);
        }
        for (int b = 0; b < 2; b++) rows[b] = c.take_i32(nnz + 1);
        table = c.take_i32(T);
        offsets = c.take_i32(T + 1);
        scan_ws = c.take(tp_scan_ws_bytes(nnz));
        bytes = c.bytes();
    }
};

// COO -> CSR: the passes' workspace (used by both stages), then stage 1's CSC
struct CooLayout {
    TpLayout tp;
    int64_t n;
    WsCursor c = tp.c;
    int32_t *csc_indptr = c.take_i32(n + 1), *csc_rows = c.take_i32(tp.nnz);
    void *csc_values = c.take(tp_f64_bytes(tp.nnz));                    // 8 bytes an entry
    size_t bytes = c.bytes();
    CooLayout(const void *ws, int64_t nnz, int n_) : tp(ws, nnz), n(n_ > 0 ? n_ : 0) {}
};

// the sorts of a sparse vector and of COO triplets: the passes' workspace, then the gathered values on their way back
struct SortLayout {
    TpLayout tp;
    WsCursor c = tp.c;
    void *tmp_values = c.take(tp_f64_bytes(tp.nnz));                    // 8 bytes an entry
    size_t bytes = c.bytes();
    SortLayout(const void *ws, int64_t n) : tp(ws, n) {}
};

static int bits_of(int64_t v)   // bits needed to hold v >= 0
{
    int b = 0;
    while (v > 0) { b++; v >>= 1; }
    return b;
}

constexpr int64_t TP_GRID_CAP = (int64_t)1 << 20;      // the per-column kernels stride over what is left

// out_rows[q] = rows[q] and out_values[q] = values[perm[q]] over the sorted entries, by value kind
static int tp_gather(const char *what, int value_dtype, const int32_t *keys, const int32_t *perm, int64_t nnz,
                     const int32_t *rows, const void *values, int32_t *out_rows, void *out_values, int32_t *flags,
                     hipStream_t st)
{
    return dispatch_values(what, value_dtype, [&](auto kind) {
        using K = decltype(kind);
        using VT = typename K::VT;
        hipLaunchKernelGGL((tp_gather_kernel<VT, K::has_values>), dim3((unsigned)ceil_div(nnz, 256)), dim3(256), 0, st,
                           keys, perm, nnz, rows, K::has_values ? (const VT *)values : nullptr, out_rows,
                           K::has_values ? (VT *)out_values : nullptr, flags);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

// The LSD radix passes shared by the CSR transpose and the COO sort: a stable sort of nnz entries by key
// (keys in [0, n), checked in pass 0), carrying the entry index and the source row (src0 says where pass 0 finds
// it).  *fin receives the buffer index of the sorted keys / perm / rows in L.
// A run that continues an earlier one (src0 == TP_SRC_SORTED) takes that run's permutation in perm0 instead of
// starting from the identity, so the entry index it carries is still the caller's.  Its keys0 / perm0 / rows0 may be
// the earlier run's buffers L.*[b]: with buf0 = b ^ 1 pass 0 writes the other set.  Its keys are not checked: they
// are what an earlier pass wrote.
static int tp_sort_passes(int src0, const int32_t *keys0, const int32_t *rows0, const int32_t *indptr, int m, int n,
                          int64_t nnz, const TpLayout &L, int32_t *flags, int *fin, hipStream_t st,
                          const int32_t *perm0 = nullptr, int buf0 = 0)
{
    const int key_bits = bits_of(n > 0 ? n - 1 : 0);
    const int npasses = n <= TP_RADIX ? 1 : (key_bits + 7) / 8;
    const int ntiles = (int)tp_ntiles(nnz);
    const int64_t T = (int64_t)TP_RADIX * ntiles;
    for (int pass = 0; pass < npasses; pass++) {
        const int shift = 8 * pass;
        const int nbits = key_bits - shift < 8 ? (key_bits - shift > 0 ? key_bits - shift : 0) : 8;
        const int in = (pass - 1 + buf0) & 1, out = (pass + buf0) & 1;
        const int32_t *kin = pass == 0 ? keys0 : L.keys[in];
        const int32_t *pin = pass == 0 ? perm0 : L.perm[in];
        const int32_t *rin = pass == 0 ? rows0 : L.rows[in];
        int32_t *kout = L.keys[out], *pout = L.perm[out], *rout = L.rows[out];
        const bool first = pass == 0 && src0 != TP_SRC_SORTED;
        if (first)
            hipLaunchKernelGGL(tp_count_kernel<true>, dim3(ntiles), dim3(TP_BLOCK), 0, st, kin, nnz, n, shift, nbits,
                               ntiles, L.table, flags);
        else
            hipLaunchKernelGGL(tp_count_kernel<false>, dim3(ntiles), dim3(TP_BLOCK), 0, st, kin, nnz, n, shift, nbits,
                               ntiles, L.table, flags);
        MX_LAUNCH_CHECK();
        if (exclusive_scan_i32(L.table, T, L.offsets, nullptr, L.scan_ws, st)) return 1;
        if (!first)
            hipLaunchKernelGGL(tp_scatter_kernel<TP_SRC_SORTED>, dim3(ntiles), dim3(TP_BLOCK), 0, st, kin, pin, rin,
                               indptr, m, nnz, n, shift, nbits, ntiles, L.offsets, kout, pout, rout, flags);
        else if (src0 == TP_SRC_INDPTR)
            hipLaunchKernelGGL(tp_scatter_kernel<TP_SRC_INDPTR>, dim3(ntiles), dim3(TP_BLOCK), 0, st, kin, pin, rin,
                               indptr, m, nnz, n, shift, nbits, ntiles, L.offsets, kout, pout, rout, flags);
        else
            hipLaunchKernelGGL(tp_scatter_kernel<TP_SRC_ROWS>, dim3(ntiles), dim3(TP_BLOCK), 0, st, kin, pin, rin,
                               indptr, m, nnz, n, shift, nbits, ntiles, L.offsets, kout, pout, rout, flags);
        MX_LAUNCH_CHECK();
    }
    *fin = (npasses - 1 + buf0) & 1;
    return 0;
}

static int csr_transpose(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values,
                         int value_dtype, int64_t nnz, int32_t *out_indptr, int32_t *out_indices, void *out_values,
                         void *workspace, int64_t *nnz_out_host, hipStream_t st)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_transpose: bad size");
    MX_REQUIRE(m > 0 || nnz == 0, "mxd_csr_transpose: entries without rows");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_csr_transpose: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(nnz_out_host && out_indptr && (nnz == 0 || (indptr && indices && out_indices && workspace)),
               "mxd_csr_transpose: null pointer");
    const bool has_values = value_dtype != MX_NONE;
    MX_REQUIRE(!has_values || nnz == 0 || (values && out_values), "mxd_csr_transpose: null values pointer");
    if (nnz == 0) {
        MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)n + 1), st));
        *nnz_out_host = 0;
        return 0;
    }
    TpLayout L(workspace, nnz);
    MX_HIP(hipMemsetAsync(L.flags, 0, 2 * sizeof(int32_t), st));

    int fin = 0;
    if (tp_sort_passes(TP_SRC_INDPTR, indices, nullptr, indptr, m, n, nnz, L, L.flags, &fin, st)) return 1;
    const int32_t *skeys = L.keys[fin], *sperm = L.perm[fin], *srows = L.rows[fin];
    if (tp_gather("mxd_csr_transpose", value_dtype, skeys, sperm, nnz, srows, values, out_indices, out_values,
                  L.flags, st))
        return 1;
    hipLaunchKernelGGL(tp_indptr_kernel, dim3(grid_for((int64_t)n + 1, 256, TP_GRID_CAP)), dim3(256), 0, st, skeys, nnz,
                       (int64_t)n, out_indptr);
    MX_LAUNCH_CHECK();

    int32_t flags[2] = {0, 0};
    MX_HIP(hipMemcpyAsync(flags, L.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!flags[0], "mxd_csr_transpose: column index outside [0, %d)", n);
    if (!flags[1]) { *nnz_out_host = nnz; return 0; }

    // duplicates: the other keys/perm pair and the other rows buffer are free now; perm[fin] takes the head flags
    int32_t *heads = L.perm[fin], *newpos = L.rows[fin ^ 1];
    int32_t *merged_rows = L.perm[fin];                          // heads are consumed by the scan before the merge
    void *merged_vals = L.keys[fin ^ 1];                         // keys + perm of the free pair: >= 8 * nnz bytes
    const unsigned gq = (unsigned)ceil_div(nnz, 256);
    hipLaunchKernelGGL(tp_heads_kernel, dim3(gq), dim3(256), 0, st, skeys, out_indices, nnz, heads);
    MX_LAUNCH_CHECK();
    int64_t *total_dev = (int64_t *)L.scan_ws;
    if (exclusive_scan_i32(heads, nnz, newpos, total_dev, L.scan_ws, st)) return 1;
    if (value_dtype == MX_F64)
        hipLaunchKernelGGL(tp_merge_kernel<0>, dim3(gq), dim3(256), 0, st, skeys, out_indices, out_values, nnz, newpos,
                           merged_rows, merged_vals);
    else if (value_dtype == MX_LGL)
        hipLaunchKernelGGL(tp_merge_kernel<1>, dim3(gq), dim3(256), 0, st, skeys, out_indices, out_values, nnz, newpos,
                           merged_rows, merged_vals);
    else
        hipLaunchKernelGGL(tp_merge_kernel<2>, dim3(gq), dim3(256), 0, st, skeys, out_indices, out_values, nnz, newpos,
                           merged_rows, merged_vals);
    MX_LAUNCH_CHECK();
    hipLaunchKernelGGL(tp_remap_indptr_kernel, dim3(grid_for((int64_t)n + 1, 256, TP_GRID_CAP)), dim3(256), 0, st,
                       (int64_t)n, newpos, out_indptr);
    MX_LAUNCH_CHECK();
    int64_t total = 0;
    MX_HIP(hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_HIP(hipMemcpyAsync(out_indices, merged_rows, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToDevice, st));
    if (has_values)
        MX_HIP(hipMemcpyAsync(out_values, merged_vals, (value_dtype == MX_F64 ? 8 : 4) * (size_t)total,
                              hipMemcpyDeviceToDevice, st));
    *nnz_out_host = total;
    return 0;
}

// ---- column order of a CSR pattern: the transpose's sort, its permutation handed out -------------------------
// perm_out[q] = row-major position of the q-th entry in column-major order (stable: rows ascend inside a column),
// colptr_out = the column pointer.  The reductions over columns (reduce.hip) read the values through it, for every
// matrix that shares the pattern.
static int csr_column_order(int m, int n, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                            int32_t *perm_out, int32_t *colptr_out, void *workspace, hipStream_t st)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_column_order: bad size");
    MX_REQUIRE(m > 0 || nnz == 0, "mxd_csr_column_order: entries without rows");
    MX_REQUIRE(colptr_out && (nnz == 0 || (indptr && indices && perm_out && workspace)),
               "mxd_csr_column_order: null pointer");
    if (nnz == 0) {
        MX_HIP(hipMemsetAsync(colptr_out, 0, sizeof(int32_t) * ((size_t)n + 1), st));
        return 0;
    }
    TpLayout L(workspace, nnz);
    MX_HIP(hipMemsetAsync(L.flags, 0, 2 * sizeof(int32_t), st));
    int fin = 0;
    if (tp_sort_passes(TP_SRC_INDPTR, indices, nullptr, indptr, m, n, nnz, L, L.flags, &fin, st)) return 1;
    MX_HIP(hipMemcpyAsync(perm_out, L.perm[fin], sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(tp_indptr_kernel, dim3(grid_for((int64_t)n + 1, 256, TP_GRID_CAP)), dim3(256), 0, st,
                       L.keys[fin], nnz, (int64_t)n, colptr_out);
    MX_LAUNCH_CHECK();
    int32_t bad = 0;
    MX_HIP(hipMemcpyAsync(&bad, L.flags, sizeof(bad), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!bad, "mxd_csr_column_order: column index outside [0, %d)", n);
    return 0;
}

// ---- COO -> CSR: the transpose's passes run twice -----------------------------------------------------------
// Stage 1 stably sorts the triplets by column, carrying the row id and the entry index: pass 0 reads the rows
// from the caller (TP_SRC_ROWS) instead of searching an indptr.  The result is a CSC whose columns list their
// rows in input order.  Stage 2 is csr_transpose of that CSC: its stable sort by row gives each CSR row its
// columns in ascending order with repeated (row, col) pairs adjacent and in input order, and its compaction
// merges them by Matrix's triplet rules.
// Stage 2 re-uses the passes' part of the workspace (CooLayout).  Stage 1's flags sit at L.flags[4..7] ([4] column
// out of range, [5] the gather's duplicate flag, unused, [6] row out of range), out of the way of stage 2's
// flags[0..1].
static int coo_to_csr(int m, int n, const int32_t *rows, const int32_t *cols, const void *values, int value_dtype,
                      int64_t nnz, int32_t *out_indptr, int32_t *out_indices, void *out_values, void *workspace,
                      int64_t *nnz_out_host, hipStream_t st)
{
    MX_REQUIRE(m >= 0 && n >= 0 && nnz >= 0, "mxd_coo_to_csr: negative size");
    MX_REQUIRE(nnz <= INT_MAX, "mxd_coo_to_csr: %lld entries exceed R's int32 index range", (long long)nnz);
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_coo_to_csr: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(nnz_out_host && out_indptr && (nnz == 0 || (rows && cols && out_indices && workspace)),
               "mxd_coo_to_csr: null pointer");
    const bool has_values = value_dtype != MX_NONE;
    MX_REQUIRE(!has_values || nnz == 0 || (values && out_values), "mxd_coo_to_csr: null values pointer");
    if (nnz == 0) {
        MX_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int32_t) * ((size_t)m + 1), st));
        *nnz_out_host = 0;
        return 0;
    }
    MX_REQUIRE(m > 0 && n > 0, "mxd_coo_to_csr: %lld entries in a %d x %d matrix: index outside the matrix",
               (long long)nnz, m, n);
    const CooLayout C(workspace, nnz, n);
    const TpLayout &L = C.tp;
    int32_t *F = L.flags + 4;
    MX_HIP(hipMemsetAsync(F, 0, 4 * sizeof(int32_t), st));

    int fin = 0;
    if (tp_sort_passes(TP_SRC_ROWS, cols, rows, nullptr, m, n, nnz, L, F, &fin, st)) return 1;
    const int32_t *skeys = L.keys[fin], *sperm = L.perm[fin], *srows = L.rows[fin];
    if (tp_gather("mxd_coo_to_csr", value_dtype, skeys, sperm, nnz, srows, values, C.csc_rows, C.csc_values, F, st))
        return 1;
    hipLaunchKernelGGL(tp_indptr_kernel, dim3(grid_for((int64_t)n + 1, 256, TP_GRID_CAP)), dim3(256), 0, st, skeys, nnz,
                       (int64_t)n, C.csc_indptr);
    MX_LAUNCH_CHECK();

    // stage 2 ends with the stream synchronised; bad indices were clamped to 0, so it runs safely either way
    if (csr_transpose(n, m, C.csc_indptr, C.csc_rows, has_values ? C.csc_values : nullptr, value_dtype, nnz, out_indptr,
                      out_indices, out_values, workspace, nnz_out_host, st))
        return 1;
    int32_t flags[4] = {0, 0, 0, 0};
    MX_HIP(hipMemcpyAsync(flags, F, sizeof(flags), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!flags[0], "mxd_coo_to_csr: column index outside [0, %d)", n);
    MX_REQUIRE(!flags[2], "mxd_coo_to_csr: row index outside [0, %d)", m);
    return 0;
}

// ---- CSR -> COO: row id of every entry, storage order kept -------------------------------------------------
__global__ __launch_bounds__(256)
void csr_rows_of_entries_kernel(const int32_t *__restrict__ indptr, int m, int64_t nnz, int32_t *__restrict__ rows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz) rows[k] = tp_row_of(indptr, 0, m, k);
}

// ---- sparse vector: one segment sorted by its index, values carried ----------------------------------------
// sort_vector_indices_* (src/misc.cpp:460-527) sorts a permutation with std::sort and applies it.  Here one
// reduction finds out whether anything is out of order and how many key bits there are (words[0] descents,
// words[1] largest index, words[2] a negative index); only an unsorted vector goes through the radix passes
// above (one key, the entry index carried for the values; the pass-0 "row" payload is the key itself).
__global__ __launch_bounds__(256)
void sv_sorted_kernel(const int32_t *__restrict__ ii, int64_t n, int32_t *__restrict__ words)
{
    bool desc = false, neg = false;
    int mx_key = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int key = ii[k];
        desc |= k > 0 && key < ii[k - 1];
        neg |= key < 0;
        mx_key = key > mx_key ? key : mx_key;
    }
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) {
        const int o = __shfl_down(mx_key, off, MX_WAVE);
        mx_key = o > mx_key ? o : mx_key;
    }
    const bool any_desc = __ballot(desc) != 0ULL, any_neg = __ballot(neg) != 0ULL;
    if (lane_id() == 0) {
        if (any_desc) words[0] = 1;
        if (any_neg) words[2] = 1;
        atomicMax(&words[1], mx_key);
    }
}

static int sort_vector(int32_t *ii, void *xx, int64_t n, int value_dtype, void *workspace, int *was_sorted_host,
                       hipStream_t st)
{
    MX_REQUIRE(n >= 0 && n <= INT_MAX, "mxd_sort_vector_indices: bad size");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_I32 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_sort_vector_indices: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(was_sorted_host, "mxd_sort_vector_indices: null pointer");
    *was_sorted_host = 1;
    if (n < 2) return 0;
    const bool has_values = value_dtype != MX_NONE;
    MX_REQUIRE(ii && workspace && (!has_values || xx), "mxd_sort_vector_indices: null pointer");
    const SortLayout S(workspace, n);
    const TpLayout &L = S.tp;
    void *tmp_values = S.tmp_values;
    // the passes' own flags (F[0] bad key, F[2] bad row) cannot fire once the reduction below has passed (no
    // negative index, keys < nkeys), and the gather's duplicate flag F[1] means nothing here: none is read back
    int32_t *F = L.flags + TP_SV_PASS_FLAGS, *words = L.flags + TP_SV_WORDS;
    MX_HIP(hipMemsetAsync(L.flags, 0, TP_FLAG_BYTES, st));
    hipLaunchKernelGGL(sv_sorted_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st, ii, n, words);
    MX_LAUNCH_CHECK();
    int32_t w[3] = {0, 0, 0};
    MX_HIP(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    if (!w[0]) return 0;                                    // already sorted: nothing is touched
    *was_sorted_host = 0;
    MX_REQUIRE(!w[2] && w[1] < INT_MAX, "mxd_sort_vector_indices: index outside [0, %d)", INT_MAX);
    const int nkeys = w[1] + 1;

    int fin = 0;
    if (tp_sort_passes(TP_SRC_ROWS, ii, ii, nullptr, nkeys, nkeys, n, L, F, &fin, st)) return 1;
    const int32_t *skeys = L.keys[fin], *sperm = L.perm[fin], *srows = L.rows[fin];
    if (tp_gather("mxd_sort_vector_indices", value_dtype, skeys, sperm, n, srows, xx, ii, tmp_values, F, st)) return 1;
    if (has_values)
        MX_HIP(hipMemcpyAsync(xx, tmp_values, (value_dtype == MX_F64 ? 8 : 4) * (size_t)n, hipMemcpyDeviceToDevice,
                              st));
    return 0;
}

// ---- COO triplets sorted by (row, column) in place, values carried -----------------------------------------
// sort_coo_indices<T> (src/misc.cpp:387-457) argsorts the triplets by (indices1, indices2) with std::sort and
// permutes all three arrays.  Here one reduction over both index arrays finds out whether anything is out of order,
// whether an index is negative, and the two largest indices, which size the radix passes (words[0] descents,
// words[1] largest ii, words[2] a negative index, words[3] largest jj).  The maxima go through one slot per block and
// a one-block second step: no global atomics.  Only unsorted triplets go further: a stable sort by jj (the run of
// mxd_coo_to_csr's stage 1, carrying ii as its "row"), then a stable sort by ii that takes up that permutation
// (carrying jj), so the entry index that arrives is the caller's and the values are gathered once, by the composed
// permutation.  Equal cells stay in input order, one of the orders std::sort may give.
constexpr int COO_SORTED_BLOCKS = 2048;

__global__ __launch_bounds__(256)
void coo_sorted_kernel(const int32_t *__restrict__ ii, const int32_t *__restrict__ jj, int64_t n,
                       int32_t *__restrict__ words, int32_t *__restrict__ part_i, int32_t *__restrict__ part_j)
{
    __shared__ int32_t wave_max[2][256 / MX_WAVE];
    bool desc = false, neg = false;
    int mx_i = 0, mx_j = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int i = ii[k], j = jj[k];
        if (k > 0) {
            const int pi = ii[k - 1];
            desc |= i < pi || (i == pi && j < jj[k - 1]);
        }
        neg |= (i | j) < 0;
        mx_i = i > mx_i ? i : mx_i;
        mx_j = j > mx_j ? j : mx_j;
    }
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) {
        const int oi = __shfl_down(mx_i, off, MX_WAVE), oj = __shfl_down(mx_j, off, MX_WAVE);
        mx_i = oi > mx_i ? oi : mx_i;
        mx_j = oj > mx_j ? oj : mx_j;
    }
    const bool any_desc = __ballot(desc) != 0ULL, any_neg = __ballot(neg) != 0ULL;
    const int wave = threadIdx.x / MX_WAVE;
    if (lane_id() == 0) {
        if (any_desc) words[0] = 1;
        if (any_neg) words[2] = 1;
        wave_max[0][wave] = mx_i;
        wave_max[1][wave] = mx_j;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / MX_WAVE; w++) {
            mx_i = wave_max[0][w] > mx_i ? wave_max[0][w] : mx_i;
            mx_j = wave_max[1][w] > mx_j ? wave_max[1][w] : mx_j;
        }
        part_i[blockIdx.x] = mx_i;
        part_j[blockIdx.x] = mx_j;
    }
}

// one wave: words[1] / words[3] = the largest of the per-block maxima
__global__ __launch_bounds__(MX_WAVE)
void coo_max_kernel(const int32_t *__restrict__ part_i, const int32_t *__restrict__ part_j, int nparts,
                    int32_t *__restrict__ words)
{
    int mx_i = 0, mx_j = 0;
    for (int b = threadIdx.x; b < nparts; b += MX_WAVE) {
        mx_i = part_i[b] > mx_i ? part_i[b] : mx_i;
        mx_j = part_j[b] > mx_j ? part_j[b] : mx_j;
    }
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) {
        const int oi = __shfl_down(mx_i, off, MX_WAVE), oj = __shfl_down(mx_j, off, MX_WAVE);
        mx_i = oi > mx_i ? oi : mx_i;
        mx_j = oj > mx_j ? oj : mx_j;
    }
    if (threadIdx.x == 0) { words[1] = mx_i; words[3] = mx_j; }
}

static int coo_sort(int32_t *ii, int32_t *jj, void *xx, int64_t nnz, int value_dtype, void *workspace,
                    int *was_sorted_host, hipStream_t st)
{
    MX_REQUIRE(nnz >= 0, "mxd_coo_sort: negative size");
    MX_REQUIRE(nnz <= INT_MAX, "mxd_coo_sort: %lld entries exceed R's int32 index range", (long long)nnz);
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_coo_sort: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(was_sorted_host, "mxd_coo_sort: null pointer");
    *was_sorted_host = 1;
    if (nnz == 0) return 0;
    const bool has_values = value_dtype != MX_NONE;
    MX_REQUIRE(ii && jj && workspace && (!has_values || xx), "mxd_coo_sort: null pointer");
    const SortLayout S(workspace, nnz);
    const TpLayout &L = S.tp;
    void *tmp_values = S.tmp_values;
    // the passes' own flags (F[0] bad key, F[2] bad row) cannot fire once the reduction below has passed, and the
    // gather's duplicate flag F[1] means nothing here: none is read back
    int32_t *F = L.flags + TP_COO_PASS_FLAGS, *words = L.flags + TP_COO_WORDS;
    MX_HIP(hipMemsetAsync(L.flags, 0, TP_FLAG_BYTES, st));
    // the per-block maxima lie where the first pass will write, at most nnz of them
    const unsigned nparts = grid_for(nnz, 256, COO_SORTED_BLOCKS);
    hipLaunchKernelGGL(coo_sorted_kernel, dim3(nparts), dim3(256), 0, st, ii, jj, nnz, words, L.keys[0], L.perm[0]);
    MX_LAUNCH_CHECK();
    hipLaunchKernelGGL(coo_max_kernel, dim3(1), dim3(MX_WAVE), 0, st, L.keys[0], L.perm[0], (int)nparts, words);
    MX_LAUNCH_CHECK();
    int32_t w[4] = {0, 0, 0, 0};
    MX_HIP(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!w[2], "mxd_coo_sort: negative index");
    if (!w[0]) return 0;                                    // already sorted: nothing is touched
    *was_sorted_host = 0;
    MX_REQUIRE(w[1] < INT_MAX && w[3] < INT_MAX, "mxd_coo_sort: index outside [0, %d)", INT_MAX);
    const int nrow_keys = w[1] + 1, ncol_keys = w[3] + 1;

    // by column, carrying the row; then by row, carrying the column and the first run's permutation
    int fin = 0;
    if (tp_sort_passes(TP_SRC_ROWS, jj, ii, nullptr, nrow_keys, ncol_keys, nnz, L, F, &fin, st)) return 1;
    if (tp_sort_passes(TP_SRC_SORTED, L.rows[fin], L.keys[fin], nullptr, ncol_keys, nrow_keys, nnz, L, F, &fin, st,
                       L.perm[fin], fin ^ 1))
        return 1;
    // the sorted rows, columns and permutation are all in the workspace: nothing below reads what it overwrites,
    // except the values, which go through tmp_values
    const int32_t *srows = L.keys[fin], *sperm = L.perm[fin], *scols = L.rows[fin];
    if (tp_gather("mxd_coo_sort", value_dtype, srows, sperm, nnz, scols, xx, jj, tmp_values, F, st)) return 1;
    MX_HIP(hipMemcpyAsync(ii, srows, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, st));
    if (has_values)
        MX_HIP(hipMemcpyAsync(xx, tmp_values, (value_dtype == MX_F64 ? 8 : 4) * (size_t)nnz, hipMemcpyDeviceToDevice,
                              st));
    return 0;
}

}  // namespace mx

extern "C" size_t mxd_coo_sort_workspace_bytes(int64_t nnz) { return mx::SortLayout(nullptr, nnz).bytes; }

extern "C" int mxd_coo_sort(int32_t *ii, int32_t *jj, void *xx, int64_t nnz, int value_dtype, void *workspace,
                            int *was_sorted, void *stream)
{
    return mx::coo_sort(ii, jj, xx, nnz, value_dtype, workspace, was_sorted, mx::as_stream(stream));
}

extern "C" size_t mxd_sort_vector_indices_workspace_bytes(int64_t n) { return mx::SortLayout(nullptr, n).bytes; }

extern "C" int mxd_sort_vector_indices(int32_t *ii, void *xx, int64_t n, int value_dtype, void *workspace,
                                       int *was_sorted_host, void *stream)
{
    return mx::sort_vector(ii, xx, n, value_dtype, workspace, was_sorted_host, mx::as_stream(stream));
}

extern "C" size_t mxd_coo_to_csr_workspace_bytes(int64_t nnz, int n) { return mx::CooLayout(nullptr, nnz, n).bytes; }

extern "C" int mxd_coo_to_csr(int m, int n, const int32_t *rows, const int32_t *cols, const void *values,
                              int value_dtype, int64_t nnz, int32_t *out_indptr, int32_t *out_indices,
                              void *out_values, void *workspace, int64_t *nnz_out_host, void *stream)
{
    return mx::coo_to_csr(m, n, rows, cols, values, value_dtype, nnz, out_indptr, out_indices, out_values, workspace,
                          nnz_out_host, mx::as_stream(stream));
}

extern "C" int mxd_csr_to_coo(int m, int64_t nnz, const int32_t *indptr, int32_t *out_rows, void *stream)
{
    MX_REQUIRE(m >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_csr_to_coo: bad size");
    MX_REQUIRE(m > 0 || nnz == 0, "mxd_csr_to_coo: entries without rows");
    if (nnz == 0) return 0;
    MX_REQUIRE(indptr && out_rows, "mxd_csr_to_coo: null pointer");
    hipLaunchKernelGGL(mx::csr_rows_of_entries_kernel, dim3((unsigned)mx::ceil_div(nnz, 256)), dim3(256), 0,
                       mx::as_stream(stream), indptr, m, nnz, out_rows);
    MX_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mxd_csr_transpose_workspace_bytes(int64_t nnz) { return mx::TpLayout(nullptr, nnz).bytes; }

extern "C" int mxd_csr_column_order(int m, int n, const int32_t *indptr, const int32_t *indices, int64_t nnz,
                                    int32_t *perm_out, int32_t *colptr_out, void *workspace, void *stream)
{
    return mx::csr_column_order(m, n, indptr, indices, nnz, perm_out, colptr_out, workspace, mx::as_stream(stream));
}

extern "C" int mxd_csr_transpose(int m, int n, const int32_t *indptr, const int32_t *indices, const void *values,
                                 int value_dtype, int64_t nnz, int32_t *out_indptr, int32_t *out_indices,
                                 void *out_values, void *workspace, int64_t *nnz_out_host, void *stream)
{
    return mx::csr_transpose(m, n, indptr, indices, values, value_dtype, nnz, out_indptr, out_indices, out_values,
                             workspace, nnz_out_host, mx::as_stream(stream));
}

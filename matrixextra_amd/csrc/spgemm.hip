// spgemm.hip — the sparse x sparse product's device level (include/mxgpu_spgemm.h): C = A B for two
// CSR matrices by rows (Gustavson), as count -> scan -> fill.
//
// Stands for: X %*% Y, crossprod(X, Y), tcrossprod(X, Y) with both operands sparse, which the reference leaves to Matrix.
//
//   bounds   per row i: f_i = sum over its entries (i, k) of len(B row k) (64-bit) and ub_i = min(f_i, n), an upper
//            bound on the row's entries.  The row goes into the list of its bin (wave-aggregated integer atomics on the
//            list lengths; the order of a list does not reach the result, every row is computed on its own):
//              ub_i = 0             nothing to do, its count is 0
//              ub_i <= SG_GROUP_UB  a lane group of 8, 16 or 32 lanes, by the row's own mean B-row length f_i / len_i
//              ub_i <= SG_LDS_UB    a workgroup
//              else                 a workgroup with a dense accumulator
//   group    an open-addressing table of SG_GROUP_SLOTS (key, value) slots per lane group in LDS.  A's entries are
//            taken one after another; for each the lanes take the entries of B row k in parallel.  B's columns are
//            unique, so every lane owns a distinct slot: the key goes in with an integer compare-and-swap, the value
//            with a plain read-modify-write.  A wavefront-scope fence between two A entries orders the LDS accesses;
//            that alone gives the defined order of the sums.  The pairs are then ranked inside the table and stored.
//   block    the same with 256 threads and one table of 64 .. SG_LDS_SLOTS slots (the power of two >= 2 ub_i),
//            __syncthreads() between A entries, a bitonic sort of the table.
//   dense    n f64 cells and a ceil(n / 32)-word bitmap per workgroup in the workspace: the first touch of a column
//            sets its bit (atomicOr) and stores the product, later touches add to it.  The output is a walk over the
//            bitmap with popcount prefixes, which also clears it for the workgroup's next row.
// The count pass runs the same kernels on keys and bitmaps only.  Every product is rounded on its own (__dmul_rn under
// a contract-off pragma, as tprod.hip does) and added in a statement of its own.  No atomic touches a value.
//
// One triangle (include/mxgpu_gram.h): every kernel takes a compile-time mask TRI.  SG_TRI_NONE is the
// product above, instruction for instruction.  Under SG_TRI_UPPER / SG_TRI_LOWER a product for cell (i, j) is kept when
// j >= i / j <= i, the bound is ub_i = min(f_i, w_i) with w_i the columns the mask leaves row i, and, when the caller
// promises ascending rows of B (b_sorted), each row of B is trimmed to the window by a binary search where it is staged:
// a step with nothing in the window is skipped, and f_i counts the trimmed lengths.
#include "mx_dispatch.h"
#include "mx_workspace.h"
#include "../../include/mxgpu_gram.h"

#include <initializer_list>

namespace mx {

constexpr int SG_BLOCK = 256;
constexpr int SG_GROUP_UB = 32, SG_GROUP_SLOTS = 64;        // 64 slots x 12 B x 32 groups of 8 lanes = 24 KiB a block
constexpr int SG_LDS_UB = 1024, SG_LDS_SLOTS = 2048;        // 2048 slots x 12 B = 24 KiB
constexpr int SG_EMPTY = INT_MAX;                           // no column: a column is below n <= INT_MAX
constexpr int SG_MAX_BLOCKS = 2048;                         // fixed grids that stride over a list
constexpr int SG_MAX_DENSE_GROUPS = 1024;
constexpr size_t SG_DENSE_CAP = (size_t)256 << 20;          // bytes of all dense accumulators together
enum { SG_BIN_G8, SG_BIN_G16, SG_BIN_G32, SG_BIN_BLOCK, SG_BIN_DENSE, SG_BINS };

using spgemm_groups = int_list<8, 16, 32>;

struct SgHeader {
    long long nnz_out, products;        // read back together by the count pass
    long long nnzA, nnzB;               // kept for the fill pass, whose prototype carries no entry counts
    int32_t len[SG_BINS];               // list lengths
    int32_t pad[3];
};
static_assert(sizeof(SgHeader) == 64, "SgHeader is 64 bytes");

static inline size_t sg_dense_bytes(int64_t n)              // of one accumulator: cells, then the bitmap
{
    return (size_t)n * 8 + (((size_t)ceil_div(n > 0 ? n : 1, 32) * 4 + 7) & ~(size_t)7);
}

static inline int sg_dense_groups(int64_t m, int64_t n)
{
    int64_t g = (int64_t)(SG_DENSE_CAP / sg_dense_bytes(n));
    g = g < SG_MAX_DENSE_GROUPS ? g : SG_MAX_DENSE_GROUPS;
    g = g < (m + 3) / 4 ? g : (m + 3) / 4;                  // four rows a workgroup before more memory is taken
    return (int)(g < 1 ? 1 : g);
}

struct SpgemmLayout {
    WsCursor c;
    int64_t m, n;
    int groups = sg_dense_groups(m, n);
    int32_t *counts = c.take_counts(m);
    SgHeader *head = c.take<SgHeader>(sizeof(SgHeader));
    int32_t *ub = c.take_i32(m);
    int32_t *lists = c.take<int32_t>(SG_BINS * padded_i32_bytes(m));
    // ub_i <= n: with n <= SG_LDS_UB no row reaches the dense bin, and nothing is reserved for it
    char *dense = c.take<char>(n > SG_LDS_UB ? (size_t)groups * sg_dense_bytes(n) : 0);
    size_t bytes = c.bytes();
    SpgemmLayout(const void *ws, int64_t m_, int64_t n_) : c(ws), m(m_ > 0 ? m_ : 0), n(n_ > 0 ? n_ : 0) {}
    int32_t *list(int bin) const { return (int32_t *)((char *)lists + bin * padded_i32_bytes(m)); }
    void *scan_ws() const { return (char *)counts + padded_i32_bytes(m); }
};

// an entry's value as the product reads it
__device__ __forceinline__ double sg_value(const void *__restrict__ x, int dtype, int64_t q)
{
    if (dtype == MX_F64) return ((const double *)x)[q];
    if (dtype == MX_LGL) {
        const int v = ((const int32_t *)x)[q];
        return v == MX_NA_INT ? na_real() : (double)(v != 0);
    }
    return 1.0;
}

__device__ __forceinline__ double sg_product(double a, double b)
{
#pragma clang fp contract(off)
    return __dmul_rn(a, b);                                             // rounded here: never part of an fma
}

// the LDS accesses of one step before those of the next, for lanes of one wavefront
__device__ __forceinline__ void sg_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (key, value) into an open-addressing table of `slots` (a power of two) slots, of which at least one stays empty
template <bool FILL>
__device__ __forceinline__ void sg_insert(int32_t *keys, double *vals, int slots, int j, double t)
{
    int s = j & (slots - 1);
    for (int probe = 0; probe < slots; probe++) {
        const int old = atomicCAS(&keys[s], SG_EMPTY, j);
        if (old == SG_EMPTY) {                                          // the first term as it is
            if (FILL) vals[s] = t;
            return;
        }
        if (old == j) {
            if (FILL) { const double c = vals[s]; vals[s] = c + t; }
            return;
        }
        s = (s + 1) & (slots - 1);
    }
}

// ---- the triangle mask (include/mxgpu_gram.h): a compile-time choice, SG_TRI_NONE is the whole product
enum { SG_TRI_NONE, SG_TRI_UPPER, SG_TRI_LOWER };

// whether the mask keeps a product for cell (row, j); it stands in front of every insert and every bitmap atomicOr,
// because the tables are sized from the window and sg_insert gives up silently when a table is full
template <int TRI>
__device__ __forceinline__ bool sg_keep(int row, int j)
{
    return TRI == SG_TRI_NONE || (TRI == SG_TRI_UPPER ? j >= row : j <= row);
}

// how many of the n columns the mask leaves row `row`
template <int TRI>
__device__ __forceinline__ long long sg_window(long long row, int n)
{
    if (TRI == SG_TRI_UPPER) return row < n ? n - row : 0;
    if (TRI == SG_TRI_LOWER) return row + 1 < n ? row + 1 : n;
    return n;
}

// an ascending row of B, [bs, bs + bl), trimmed to the window of `row`: upper from the first column >= row, lower up to
// the last column <= row.  On a row that is not ascending the search still ends inside [0, bl].
template <int TRI>
__device__ __forceinline__ void sg_trim(const int32_t *__restrict__ Bj, int row, long long &bs, int &bl)
{
    if (TRI == SG_TRI_UPPER) {
        const int at = lower_bound_dev(Bj + bs, bl, row);
        bs += at;
        bl -= at;
    } else if (TRI == SG_TRI_LOWER) {
        bl = lower_bound_dev(Bj + bs, bl, row + 1);                     // row < m <= INT_MAX
    }
}

// ---- bounds and bins: eight lanes a row ----------------------------------------------------------------------------
template <int TRI>
__global__ __launch_bounds__(SG_BLOCK)
void sg_bounds_kernel(int m, int K, int n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Aj, int64_t nnzA,
                      const int32_t *__restrict__ Bp, const int32_t *__restrict__ Bj, int64_t nnzB, int b_sorted,
                      int32_t *__restrict__ ub, int32_t *__restrict__ counts, int32_t *__restrict__ lists,
                      size_t list_stride, SgHeader *__restrict__ head)
{
    const int l8 = threadIdx.x & 7, lane = lane_id();
    const long long row = (long long)blockIdx.x * (SG_BLOCK / 8) + threadIdx.x / 8;
    const bool valid = row < m;
    long long f = 0, used = 0;
    if (valid) {
        const RowBounds ra = row_bounds(Ap[row], Ap[row + 1], nnzA);
        for (int64_t q = l8; q < ra.len; q += 8) {
            const int k = Aj[ra.start + q];
            if ((unsigned)k < (unsigned)K) {
                const RowBounds rb = row_bounds(Bp[k], Bp[k + 1], nnzB);
                if (TRI != SG_TRI_NONE && b_sorted) {                   // the trimmed length: what the steps will read
                    long long bs = rb.start;
                    int bl = (int)rb.len;
                    sg_trim<TRI>(Bj, (int)row, bs, bl);
                    f += bl;
                } else f += rb.len;
                used++;
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) { f += __shfl_xor(f, off); used += __shfl_xor(used, off); }
    const bool owner = valid && l8 == 0;
    int bin = -1;
    if (owner) {
        const long long w = sg_window<TRI>(row, n);
        const long long u = f < w ? f : w;
        ub[row] = (int32_t)u;
        if (u == 0) counts[row] = 0;
        else if (u <= SG_GROUP_UB) {
            const long long mean = (f + used - 1) / used;              // used >= 1 here
            bin = mean <= 8 ? SG_BIN_G8 : mean <= 16 ? SG_BIN_G16 : SG_BIN_G32;
        } else bin = u <= SG_LDS_UB ? SG_BIN_BLOCK : SG_BIN_DENSE;
    }
#pragma unroll
    for (int b = 0; b < SG_BINS; b++) {                                 // one atomic per wavefront and bin
        const unsigned long long mask = __ballot(bin == b);
        if (mask == 0ULL) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&head->len[b], __popcll(mask));
        base = __shfl(base, leader);
        if (bin == b) ((int32_t *)((char *)lists + b * list_stride))[base + __popcll(mask & ((1ULL << lane) - 1ULL))] = (int32_t)row;
    }
    long long pf = owner ? f : 0;
#pragma unroll
    for (int off = 8; off < MX_WAVE; off <<= 1) pf += __shfl_xor(pf, off);
    if (lane == 0 && pf) atomicAdd((unsigned long long *)&head->products, (unsigned long long)pf);
    if (blockIdx.x == 0 && threadIdx.x == 0) { head->nnzA = nnzA; head->nnzB = nnzB; }
}

// ---- a lane group a row ----------------------------------------------------------------------------------------------
template <int G, bool FILL, int TRI>
__global__ __launch_bounds__(SG_BLOCK)
void sg_group_kernel(int K, int n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Aj,
                     const void *__restrict__ Ax, int a_dtype, const int32_t *__restrict__ Bp,
                     const int32_t *__restrict__ Bj, const void *__restrict__ Bx, int b_dtype, int b_sorted,
                     const SgHeader *__restrict__ head, int bin, const int32_t *__restrict__ list,
                     int32_t *__restrict__ counts, const int32_t *__restrict__ out_indptr,
                     int32_t *__restrict__ out_indices, double *__restrict__ out_values)
{
    constexpr int NG = SG_BLOCK / G;
    __shared__ int32_t keys_all[NG * SG_GROUP_SLOTS];
    __shared__ double vals_all[FILL ? NG * SG_GROUP_SLOTS : 1];
    const int lg = threadIdx.x % G, grp = threadIdx.x / G;
    int32_t *keys = keys_all + grp * SG_GROUP_SLOTS;
    double *vals = vals_all + (FILL ? grp * SG_GROUP_SLOTS : 0);
    const int len = head->len[bin];
    const int64_t nnzA = head->nnzA, nnzB = head->nnzB;

    for (int64_t r = blockIdx.x * NG + grp; r < len; r += gridDim.x * NG) {      // the same for all lanes of a group
        const int row = list[r];
        for (int s = lg; s < SG_GROUP_SLOTS; s += G) keys[s] = SG_EMPTY;
        sg_wave_sync();
        const RowBounds ra = row_bounds(Ap[row], Ap[row + 1], nnzA);
        for (int64_t q0 = 0; q0 < ra.len; q0 += G) {
            // G entries of A at once, one a lane: its value and the bounds of its row of B
            int bl = 0;
            long long bs = 0;
            double a = 1.0;
            if (q0 + lg < ra.len) {
                const int64_t q = ra.start + q0 + lg;
                const int k = Aj[q];
                if ((unsigned)k < (unsigned)K) {
                    const RowBounds rb = row_bounds(Bp[k], Bp[k + 1], nnzB);
                    bs = rb.start;
                    bl = (int)rb.len;
                    if (TRI != SG_TRI_NONE && b_sorted) sg_trim<TRI>(Bj, row, bs, bl);
                    if (FILL) a = sg_value(Ax, a_dtype, q);
                }
            }
            const int cnt = ra.len - q0 < G ? (int)(ra.len - q0) : G;
            for (int t = 0; t < cnt; t++) {                             // then one after another
                const int blen = __shfl(bl, t, G);
                const int64_t bstart = __shfl(bs, t, G);
                const double at = FILL ? __shfl(a, t, G) : 1.0;
                if (blen == 0) continue;
                for (int u = lg; u < blen; u += G) {
                    const int j = Bj[bstart + u];
                    if ((unsigned)j >= (unsigned)n || !sg_keep<TRI>(row, j)) continue;
                    sg_insert<FILL>(keys, vals, SG_GROUP_SLOTS, j, FILL ? sg_product(at, sg_value(Bx, b_dtype, bstart + u)) : 0.0);
                }
                sg_wave_sync();
            }
        }
        if (!FILL) {
            int c = 0;
            for (int s = lg; s < SG_GROUP_SLOTS; s += G) c += keys[s] != SG_EMPTY;
#pragma unroll
            for (int off = 1; off < G; off <<= 1) c += __shfl_xor(c, off, G);
            if (lg == 0) counts[row] = c;
        } else {
            const int o = out_indptr[row], room = out_indptr[row + 1] - o;
            for (int s = lg; s < SG_GROUP_SLOTS; s += G) {
                const int key = keys[s];
                if (key == SG_EMPTY) continue;
                int rank = 0;
                for (int t = 0; t < SG_GROUP_SLOTS; t++) rank += keys[t] < key;     // an empty slot is INT_MAX
                if (rank < room) { out_indices[o + rank] = key; out_values[o + rank] = vals[s]; }
            }
        }
        sg_wave_sync();                                                 // the table is read before it is cleared
    }
}

// what the two workgroup kernels share: 256 entries of A staged in LDS, one a thread
struct SgStage {
    int32_t bl[SG_BLOCK];
    long long bs[SG_BLOCK];
    double a[SG_BLOCK];
};

template <bool FILL, int TRI>
__device__ __forceinline__ void sg_stage(SgStage &st, int row, const RowBounds ra, int64_t q0, int K, const int32_t *Aj,
                                         const void *Ax, int a_dtype, const int32_t *Bp, const int32_t *Bj, int64_t nnzB,
                                         int b_sorted)
{
    const int tid = threadIdx.x;
    int bl = 0;
    long long bs = 0;
    double a = 1.0;
    if (q0 + tid < ra.len) {
        const int64_t q = ra.start + q0 + tid;
        const int k = Aj[q];
        if ((unsigned)k < (unsigned)K) {
            const RowBounds rb = row_bounds(Bp[k], Bp[k + 1], nnzB);
            bs = rb.start;
            bl = (int)rb.len;
            if (TRI != SG_TRI_NONE && b_sorted) sg_trim<TRI>(Bj, row, bs, bl);
            if (FILL) a = sg_value(Ax, a_dtype, q);
        }
    }
    st.bl[tid] = bl;
    st.bs[tid] = bs;
    if (FILL) st.a[tid] = a;
}

// exclusive prefix of one int a thread over the 256 threads; *total their sum
__device__ __forceinline__ int sg_block_scan(int v, int *total)
{
    __shared__ int wave_sums[SG_BLOCK / MX_WAVE];
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    int incl = v;
#pragma unroll
    for (int off = 1; off < MX_WAVE; off <<= 1) {
        const int o = __shfl_up(incl, off, MX_WAVE);
        if (lane >= off) incl += o;
    }
    if (lane == MX_WAVE - 1) wave_sums[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SG_BLOCK / MX_WAVE; w++) {
        const int s = wave_sums[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// ---- a workgroup a row, one table in LDS -----------------------------------------------------------------------------
template <bool FILL, int TRI>
__global__ __launch_bounds__(SG_BLOCK)
void sg_block_kernel(int K, int n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Aj,
                     const void *__restrict__ Ax, int a_dtype, const int32_t *__restrict__ Bp,
                     const int32_t *__restrict__ Bj, const void *__restrict__ Bx, int b_dtype, int b_sorted,
                     const SgHeader *__restrict__ head, const int32_t *__restrict__ list,
                     const int32_t *__restrict__ ub, int32_t *__restrict__ counts,
                     const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                     double *__restrict__ out_values)
{
    __shared__ int32_t keys[SG_LDS_SLOTS];
    __shared__ double vals[FILL ? SG_LDS_SLOTS : 1];
    __shared__ SgStage st;
    const int tid = threadIdx.x;
    const int len = head->len[SG_BIN_BLOCK];
    const int64_t nnzA = head->nnzA, nnzB = head->nnzB;

    for (int64_t r = blockIdx.x; r < len; r += gridDim.x) {
        const int row = list[r];
        int bound = ub[row];
        bound = bound < SG_LDS_UB ? bound : SG_LDS_UB;                  // what the bin promises, whatever ub holds
        int slots = 64;
        while (slots < 2 * bound) slots <<= 1;
        for (int s = tid; s < slots; s += SG_BLOCK) keys[s] = SG_EMPTY;
        const RowBounds ra = row_bounds(Ap[row], Ap[row + 1], nnzA);
        for (int64_t q0 = 0; q0 < ra.len; q0 += SG_BLOCK) {
            __syncthreads();                                            // the stage is free, the table is clear
            sg_stage<FILL, TRI>(st, row, ra, q0, K, Aj, Ax, a_dtype, Bp, Bj, nnzB, b_sorted);
            __syncthreads();
            const int cnt = ra.len - q0 < SG_BLOCK ? (int)(ra.len - q0) : SG_BLOCK;
            for (int t = 0; t < cnt; t++) {
                const int blen = st.bl[t];
                if (blen == 0) continue;
                const int64_t bstart = st.bs[t];
                const double at = FILL ? st.a[t] : 1.0;
                for (int u = tid; u < blen; u += SG_BLOCK) {
                    const int j = Bj[bstart + u];
                    if ((unsigned)j >= (unsigned)n || !sg_keep<TRI>(row, j)) continue;
                    sg_insert<FILL>(keys, vals, slots, j, FILL ? sg_product(at, sg_value(Bx, b_dtype, bstart + u)) : 0.0);
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if (!FILL) {
            int c = 0, total;
            for (int s = tid; s < slots; s += SG_BLOCK) c += keys[s] != SG_EMPTY;
            sg_block_scan(c, &total);
            if (tid == 0) counts[row] = total;
        } else {
            for (int k = 2; k <= slots; k <<= 1)                        // bitonic: the empty slots, INT_MAX, go last
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < slots; i += SG_BLOCK) {
                        const int x = i ^ j;
                        if (x > i) {
                            const int ki = keys[i], kx = keys[x];
                            if ((ki > kx) == ((i & k) == 0)) {
                                keys[i] = kx;
                                keys[x] = ki;
                                const double vi = vals[i];
                                vals[i] = vals[x];
                                vals[x] = vi;
                            }
                        }
                    }
                    __syncthreads();
                }
            const int o = out_indptr[row], room = out_indptr[row + 1] - o;
            for (int i = tid; i < slots && i < room; i += SG_BLOCK)
                if (keys[i] != SG_EMPTY) { out_indices[o + i] = keys[i]; out_values[o + i] = vals[i]; }
        }
        __syncthreads();
    }
}

// ---- a workgroup a row, a dense accumulator in the workspace --------------------------------------------------------
template <bool FILL, int TRI>
__global__ __launch_bounds__(SG_BLOCK)
void sg_dense_kernel(int K, int n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Aj,
                     const void *__restrict__ Ax, int a_dtype, const int32_t *__restrict__ Bp,
                     const int32_t *__restrict__ Bj, const void *__restrict__ Bx, int b_dtype, int b_sorted,
                     const SgHeader *__restrict__ head, const int32_t *__restrict__ list, char *dense,
                     size_t dense_bytes, int32_t *__restrict__ counts, const int32_t *__restrict__ out_indptr,
                     int32_t *__restrict__ out_indices, double *__restrict__ out_values)
{
    __shared__ SgStage st;
    const int tid = threadIdx.x;
    const int len = head->len[SG_BIN_DENSE];
    const int64_t nnzA = head->nnzA, nnzB = head->nnzB;
    if ((int)blockIdx.x >= len) return;
    double *cell = (double *)(dense + (size_t)blockIdx.x * dense_bytes);
    unsigned *bits = (unsigned *)(cell + n);
    const int words = (n + 31) / 32;
    // the bitmap is touched by atomics alone, which meet in L2; each walk below leaves it clear again
    for (int w = tid; w < words; w += SG_BLOCK) atomicExch(&bits[w], 0u);

    for (int64_t r = blockIdx.x; r < len; r += gridDim.x) {
        const int row = list[r];
        const RowBounds ra = row_bounds(Ap[row], Ap[row + 1], nnzA);
        for (int64_t q0 = 0; q0 < ra.len; q0 += SG_BLOCK) {
            __syncthreads();
            sg_stage<FILL, TRI>(st, row, ra, q0, K, Aj, Ax, a_dtype, Bp, Bj, nnzB, b_sorted);
            __syncthreads();
            const int cnt = ra.len - q0 < SG_BLOCK ? (int)(ra.len - q0) : SG_BLOCK;
            for (int t = 0; t < cnt; t++) {
                const int blen = st.bl[t];
                if (blen == 0) continue;
                const int64_t bstart = st.bs[t];
                const double at = FILL ? st.a[t] : 1.0;
                for (int u = tid; u < blen; u += SG_BLOCK) {
                    const int j = Bj[bstart + u];
                    if ((unsigned)j >= (unsigned)n || !sg_keep<TRI>(row, j)) continue;
                    const unsigned bit = 1u << (j & 31);
                    const unsigned old = atomicOr(&bits[j >> 5], bit);
                    if (FILL) {
                        const double p = sg_product(at, sg_value(Bx, b_dtype, bstart + u));
                        if (old & bit) { const double c = cell[j]; cell[j] = c + p; }
                        else cell[j] = p;                               // the first term as it is
                    }
                }
                if (FILL) __syncthreads();                              // a set has no order: the count needs none
            }
        }
        __syncthreads();
        const int o = FILL ? out_indptr[row] : 0, room = FILL ? out_indptr[row + 1] - o : 0;
        // no bit outside the row's window is ever set: the walk covers the words of the window alone
        int w_first = 0, w_end = words;
        if (TRI == SG_TRI_UPPER) w_first = (row >> 5) < words ? row >> 5 : words;
        if (TRI == SG_TRI_LOWER) w_end = (row >> 5) + 1 < words ? (row >> 5) + 1 : words;
        int done = 0;
        for (int w0 = w_first; w0 < w_end; w0 += SG_BLOCK) {
            const int w = w0 + tid;
            unsigned word = 0u;
            if (w < w_end) word = atomicExch(&bits[w], 0u);
            int total;
            int at = done + sg_block_scan(__popc(word), &total);
            if (FILL)
                while (word) {
                    const int j = w * 32 + __ffs((int)word) - 1;
                    word &= word - 1;
                    if (at < room) { out_indices[o + at] = j; out_values[o + at] = cell[j]; }
                    at++;
                }
            done += total;
        }
        if (!FILL && tid == 0) counts[row] = done;
        __syncthreads();
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct SgOperands {
    int m, K, n;
    const int32_t *Ap, *Aj;
    const void *Ax;
    int a_dtype;
    const int32_t *Bp, *Bj;
    const void *Bx;
    int b_dtype;
};

using spgemm_masks = int_list<SG_TRI_NONE, SG_TRI_UPPER, SG_TRI_LOWER>;

// what the two passes of a masked product share beside the operands: the mask and the caller's promise about B
struct SgMask {
    int tri = SG_TRI_NONE;
    int b_sorted = 0;
};

template <bool FILL, int TRI>
static int sg_launch_bins(const char *what, const SgOperands &o, int b_sorted, const SpgemmLayout &L,
                          const int32_t *out_indptr, int32_t *out_indices, double *out_values, hipStream_t st)
{
    for (int G : {8, 16, 32}) {
        const int bin = G == 8 ? SG_BIN_G8 : G == 16 ? SG_BIN_G16 : SG_BIN_G32;
        const int64_t per_block = SG_BLOCK / G;
        const int64_t rows = o.m < SG_MAX_BLOCKS * per_block ? o.m : SG_MAX_BLOCKS * per_block;
        const int rc = launch_rows(spgemm_groups{}, what, G, rows, SG_BLOCK, [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((sg_group_kernel<g(), FILL, TRI>), grid, block, 0, st, o.K, o.n, o.Ap, o.Aj, o.Ax, o.a_dtype,
                               o.Bp, o.Bj, o.Bx, o.b_dtype, b_sorted, L.head, bin, L.list(bin), L.counts, out_indptr,
                               out_indices, out_values);
        });
        if (rc) return rc;
    }
    if (o.n > SG_GROUP_UB) {                                            // ub_i <= n: the bin is empty otherwise
        hipLaunchKernelGGL((sg_block_kernel<FILL, TRI>), dim3(grid_for(o.m, 1, SG_MAX_BLOCKS)), dim3(SG_BLOCK), 0, st, o.K,
                           o.n, o.Ap, o.Aj, o.Ax, o.a_dtype, o.Bp, o.Bj, o.Bx, o.b_dtype, b_sorted, L.head,
                           L.list(SG_BIN_BLOCK), L.ub, L.counts, out_indptr, out_indices, out_values);
        MX_LAUNCH_CHECK();
    }
    if (o.n > SG_LDS_UB) {
        hipLaunchKernelGGL((sg_dense_kernel<FILL, TRI>), dim3((unsigned)L.groups), dim3(SG_BLOCK), 0, st, o.K, o.n, o.Ap,
                           o.Aj, o.Ax, o.a_dtype, o.Bp, o.Bj, o.Bx, o.b_dtype, b_sorted, L.head, L.list(SG_BIN_DENSE),
                           L.dense, sg_dense_bytes(o.n), L.counts, out_indptr, out_indices, out_values);
        MX_LAUNCH_CHECK();
    }
    return 0;
}

static int sg_check_sizes(const char *what, int m, int K, int n)
{
    MX_REQUIRE(m >= 0 && K >= 0 && n >= 0, "%s: negative dimension", what);
    return 0;
}

// the mask of a one-triangle entry point: uplo must be an mx_uplo
static int sg_mask_of(const char *what, int uplo, int b_sorted, SgMask *mask)
{
    MX_REQUIRE(uplo == MX_UPLO_UPPER || uplo == MX_UPLO_LOWER, "%s: uplo must be MX_UPLO_UPPER or MX_UPLO_LOWER, got %d",
               what, uplo);
    mask->tri = uplo == MX_UPLO_UPPER ? SG_TRI_UPPER : SG_TRI_LOWER;
    mask->b_sorted = b_sorted != 0;
    return 0;
}

static int spgemm_count(const char *what, SgMask mask, int m, int K, int n, const int32_t *Ap, const int32_t *Aj,
                        int64_t nnzA, const int32_t *Bp, const int32_t *Bj, int64_t nnzB, int32_t *out_indptr,
                        void *workspace, int64_t *products_host, int64_t *nnz_out_host, hipStream_t st)
{
    if (sg_check_sizes(what, m, K, n)) return 1;
    MX_REQUIRE(nnzA >= 0 && nnzA <= INT_MAX && nnzB >= 0 && nnzB <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(out_indptr && workspace, "%s: null pointer", what);
    MX_REQUIRE(m == 0 || (Ap && (nnzA == 0 || Aj) && (K == 0 || Bp) && (nnzB == 0 || Bj)), "%s: null pointer", what);
    const SpgemmLayout L(workspace, m, n);
    MX_HIP(hipMemsetAsync(L.head, 0, sizeof(SgHeader), st));
    if (m > 0) {
        const SgOperands o{m, K, n, Ap, Aj, nullptr, MX_NONE, Bp, Bj, nullptr, MX_NONE};
        const int rc = dispatch_int(spgemm_masks{}, what, "triangle", mask.tri, [&](auto tri) {
            hipLaunchKernelGGL(sg_bounds_kernel<tri()>, dim3(grid_for(m, SG_BLOCK / 8)), dim3(SG_BLOCK), 0, st, m, K, n, Ap,
                               Aj, nnzA, Bp, Bj, nnzB, mask.b_sorted, L.ub, L.counts, L.lists, padded_i32_bytes(m), L.head);
            MX_LAUNCH_CHECK();
            return sg_launch_bins<false, tri()>(what, o, mask.b_sorted, L, nullptr, nullptr, nullptr, st);
        });
        if (rc) return rc;
    }
    if (exclusive_scan_i32(L.counts, m, out_indptr, (int64_t *)&L.head->nnz_out, L.scan_ws(), st)) return 1;
    if (!products_host && !nnz_out_host) return 0;
    long long totals[2];                                                // nnz_out, products: one read-back
    MX_HIP(hipMemcpyAsync(totals, L.head, sizeof(totals), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    if (nnz_out_host) *nnz_out_host = totals[0];
    if (products_host) *products_host = totals[1];
    MX_REQUIRE(totals[0] <= (long long)INT32_MAX, "%s: the product has %lld entries (of %lld products): more than INT32_MAX",
               what, totals[0], totals[1]);
    return 0;
}

static int spgemm_fill(const char *what, SgMask mask, int m, int K, int n, const int32_t *Ap, const int32_t *Aj,
                       const void *Ax, int a_dtype, const int32_t *Bp, const int32_t *Bj, const void *Bx, int b_dtype,
                       const int32_t *out_indptr, int32_t *out_indices, double *out_values, void *workspace, hipStream_t st)
{
    if (sg_check_sizes(what, m, K, n)) return 1;
    for (int dt : {a_dtype, b_dtype})
        MX_REQUIRE(dt == MX_F64 || dt == MX_LGL || dt == MX_NONE, "%s: unsupported value dtype %d", what, dt);
    if (m == 0) return 0;
    MX_REQUIRE(Ap && (K == 0 || Bp) && out_indptr && out_indices && out_values && workspace, "%s: null pointer", what);
    const SpgemmLayout L(workspace, m, n);
    const SgOperands o{m, K, n, Ap, Aj, Ax, a_dtype, Bp, Bj, Bx, b_dtype};
    return dispatch_int(spgemm_masks{}, what, "triangle", mask.tri, [&](auto tri) {
        return sg_launch_bins<true, tri()>(what, o, mask.b_sorted, L, out_indptr, out_indices, out_values, st);
    });
}

}  // namespace mx

extern "C" size_t mxd_csr_spgemm_workspace_bytes(int m, int n) { return mx::SpgemmLayout(nullptr, m, n).bytes; }

extern "C" int mxd_csr_spgemm_limits(int m, int n, int *group_ub, int *lds_ub, int *dense_groups)
{
    if (mx::sg_check_sizes("mxd_csr_spgemm_limits", m, 0, n)) return 1;
    if (group_ub) *group_ub = mx::SG_GROUP_UB;
    if (lds_ub) *lds_ub = mx::SG_LDS_UB;
    if (dense_groups) *dense_groups = mx::sg_dense_groups(m, n);
    return 0;
}

extern "C" int mxd_csr_spgemm_count(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, int64_t nnzA,
                                    const int32_t *Bp, const int32_t *Bj, int64_t nnzB, int32_t *out_indptr,
                                    void *workspace, int64_t *products_host, int64_t *nnz_out_host, void *stream)
{
    return mx::spgemm_count("mxd_csr_spgemm_count", mx::SgMask{}, m, K, n, Ap, Aj, nnzA, Bp, Bj, nnzB, out_indptr, workspace,
                            products_host, nnz_out_host, mx::as_stream(stream));
}

extern "C" int mxd_csr_spgemm_fill(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, const void *Ax, int a_dtype,
                                   const int32_t *Bp, const int32_t *Bj, const void *Bx, int b_dtype,
                                   const int32_t *out_indptr, int32_t *out_indices, double *out_values, void *workspace,
                                   void *stream)
{
    return mx::spgemm_fill("mxd_csr_spgemm_fill", mx::SgMask{}, m, K, n, Ap, Aj, Ax, a_dtype, Bp, Bj, Bx, b_dtype,
                           out_indptr, out_indices, out_values, workspace, mx::as_stream(stream));
}

// ---- one triangle (include/mxgpu_gram.h): the same two passes behind a mask; uplo and the sizes are checked before
// anything is launched
extern "C" int mxd_csr_spgemm_tri_count(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, int64_t nnzA,
                                        const int32_t *Bp, const int32_t *Bj, int64_t nnzB, int uplo, int b_sorted,
                                        int32_t *out_indptr, void *workspace, int64_t *products_host,
                                        int64_t *nnz_out_host, void *stream)
{
    const char *what = "mxd_csr_spgemm_tri_count";
    mx::SgMask mask;
    if (mx::sg_mask_of(what, uplo, b_sorted, &mask)) return 1;
    return mx::spgemm_count(what, mask, m, K, n, Ap, Aj, nnzA, Bp, Bj, nnzB, out_indptr, workspace, products_host,
                            nnz_out_host, mx::as_stream(stream));
}

extern "C" int mxd_csr_spgemm_tri_fill(int m, int K, int n, const int32_t *Ap, const int32_t *Aj, const void *Ax,
                                       int a_dtype, const int32_t *Bp, const int32_t *Bj, const void *Bx, int b_dtype,
                                       int uplo, int b_sorted, const int32_t *out_indptr, int32_t *out_indices,
                                       double *out_values, void *workspace, void *stream)
{
    const char *what = "mxd_csr_spgemm_tri_fill";
    mx::SgMask mask;
    if (mx::sg_mask_of(what, uplo, b_sorted, &mask)) return 1;
    return mx::spgemm_fill(what, mask, m, K, n, Ap, Aj, Ax, a_dtype, Bp, Bj, Bx, b_dtype, out_indptr, out_indices,
                           out_values, workspace, mx::as_stream(stream));
}

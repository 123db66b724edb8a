// cooslice.hip — X[i, j] of a COO (TsparseMatrix): arbitrary slices and the single-element lookup.
//
// Replaces:
//   slice_coo_arbitrary_template<>            src/slice_coo.cpp:123-706   (f64 / R logical / pattern)
//   slice_coo_single_template<>               src/slice_coo.cpp:3-71
// The reference walks the triplets once, keeping a hash map per arbitrary selector and replicating a triplet once
// per repeat of its row or column in the selector.  Its output is fixed by one rule, which the kernels follow: walk
// the triplets in storage order; triplet k = (r, c, x) gives one output (a, b, x) for every position a of r + 1 in
// the row selector (ascending, outer loop) and every position b of c + 1 in the column selector (ascending, inner
// loop).  The seq / rev-seq / no-duplicate branches of the reference (:160-700) are the special cases where a row
// or column has at most one position.
//
// Axis kinds (mx_coo_axis): AFFINE (all / seq / rev-seq: the position is r - lo or hi - r inside [lo, hi]) or MAP
// (the dense map of colslice.hip's mxd_colmap_build over the 1-based selector: pos[start[r+1] .. start[r+2]) are
// r's positions).  The kernels are templated on the two kinds, so a seq x seq slice reads no map.
//
// count: one lane per triplet, mult_k = cnt_i(r) * cnt_j(c) in 64 bits, stored saturated to int32 with a flag when
//        it does not fit; a row outside [0, nrow) or a column outside [0, ncol) counts 0 and sets a flag, so it is
//        never used to read a map.  Then the shared exclusive scan and read-back (scan.hip finish_count), whose
//        int64 total is refused above INT32_MAX before anything is written.
// fill:  outputs of triplet k go to offset[k] + a_rank * cnt_j(c) + b_rank.  A triplet with mult <= FILL_LANE_MAX
//        is written by its own lane (mult <= 1, the common case, is one coalesced store stream).  Heavier triplets
//        are taken by the whole wave, one after another (ballot), 64 outputs per step: a triplet of 100 000
//        outputs costs its wave ~1 600 steps of 64 coalesced stores instead of 100 000 serial stores by one lane
//        while 63 lanes idle (a divergent loop holds the whole wave64).  No global atomics.
// single: smallest k with (rows[k], cols[k]) == (r, c) by a per-block minimum and one final block; the final block
//        also reads the value, so the host reads back 16 bytes.
#include "mx_dispatch.h"
#include "mx_workspace.h"

#include <cstring>

namespace mx {

constexpr int CSL_BLOCK = 256;
constexpr int FILL_LANE_MAX = 8;             // per-lane fill up to this many outputs, wave-cooperative above

struct CslAxis {
    int lo, hi, rev, nmap;
    const int32_t *start, *pos;
};

static CslAxis csl_axis(const mx_coo_axis &a)
{
    return CslAxis{a.lo, a.hi, a.reversed, a.nmap, a.start, a.pos};
}

// number of positions of 0-based index r in the selector; *first = the first position (AFFINE) or the offset of
// r's list in pos (MAP).  r is in range here.
template <bool MAP>
__device__ __forceinline__ int csl_count(const CslAxis &ax, int r, int &first)
{
    if constexpr (MAP) {
        const int key = r + 1;                                    // the map is keyed by the 1-based selector
        if (key >= ax.nmap) { first = 0; return 0; }
        first = ax.start[key];
        return ax.start[key + 1] - first;
    } else {
        if (r < ax.lo || r > ax.hi) { first = 0; return 0; }
        first = ax.rev ? ax.hi - r : r - ax.lo;
        return 1;
    }
}

template <bool MAP>
__device__ __forceinline__ int csl_position(const CslAxis &ax, int first, int rank)
{
    if constexpr (MAP) return ax.pos[first + rank];
    else return first;
}

// flags: [0] row out of range, [1] column out of range, [2] one triplet's multiplicity exceeds INT32_MAX
template <bool MAP_I, bool MAP_J>
__global__ __launch_bounds__(CSL_BLOCK)
void coo_slice_count_kernel(int nrow, int ncol, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                            int64_t nnz, CslAxis ai, CslAxis aj, int32_t *__restrict__ counts,
                            int32_t *__restrict__ flags)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad_r = false, bad_c = false, over = false;
    if (k < nnz) {
        const int r = rows[k], c = cols[k];
        bad_r = (unsigned)r >= (unsigned)nrow;
        bad_c = (unsigned)c >= (unsigned)ncol;
        int32_t out = 0;
        if (!bad_r && !bad_c) {
            int fi, fj;
            const int ci = csl_count<MAP_I>(ai, r, fi);
            const int cj = ci ? csl_count<MAP_J>(aj, c, fj) : 0;
            const int64_t mult = (int64_t)ci * (int64_t)cj;
            over = mult > (int64_t)INT_MAX;
            out = over ? INT_MAX : (int32_t)mult;
        }
        counts[k] = out;
    }
    if (__ballot(bad_r) != 0ULL && lane_id() == 0) flags[0] = 1;
    if (__ballot(bad_c) != 0ULL && lane_id() == 0) flags[1] = 1;
    if (__ballot(over) != 0ULL && lane_id() == 0) flags[2] = 1;
}

template <int VK>
__device__ __forceinline__ void csl_store_value(void *__restrict__ out_vals, int64_t q, uint64_t v)
{
    if constexpr (VK == MX_F64) ((uint64_t *)out_vals)[q] = v;
    else if constexpr (VK == MX_LGL) ((uint32_t *)out_vals)[q] = (uint32_t)v;
}

template <bool MAP_I, bool MAP_J, int VK>
__global__ __launch_bounds__(CSL_BLOCK)
void coo_slice_fill_kernel(int nrow, int ncol, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                           const void *__restrict__ vals, int64_t nnz, CslAxis ai, CslAxis aj,
                           const int32_t *__restrict__ offsets, int32_t *__restrict__ out_rows,
                           int32_t *__restrict__ out_cols, void *__restrict__ out_vals)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t q = 0;
    int mult = 0, ci = 0, cj = 0, fi = 0, fj = 0;
    uint64_t v = 0;
    if (k < nnz) {
        q = offsets[k];
        mult = (int)(offsets[k + 1] - q);
        if (mult > 0) {
            const int r = rows[k], c = cols[k];
            if ((unsigned)r < (unsigned)nrow && (unsigned)c < (unsigned)ncol) {   // the count pass refused these
                ci = csl_count<MAP_I>(ai, r, fi);
                cj = csl_count<MAP_J>(aj, c, fj);
            }
            if ((int64_t)ci * cj != mult) mult = 0;                   // never write past what the count reserved
            if constexpr (VK == MX_F64) v = ((const uint64_t *)vals)[k];
            else if constexpr (VK == MX_LGL) v = ((const uint32_t *)vals)[k];
        }
    }
    if (mult > 0 && mult <= FILL_LANE_MAX) {
        int64_t o = q;
        for (int a = 0; a < ci; a++) {
            const int pr = csl_position<MAP_I>(ai, fi, a);
            for (int b = 0; b < cj; b++, o++) {
                out_rows[o] = pr;
                out_cols[o] = csl_position<MAP_J>(aj, fj, b);
                csl_store_value<VK>(out_vals, o, v);
            }
        }
    }
    // heavy triplets: the wave takes them one at a time, each lane striding over the outputs
    unsigned long long heavy = __ballot(mult > FILL_LANE_MAX);
    const int lane = lane_id();
    while (heavy) {
        const int src = __builtin_ctzll(heavy);
        heavy &= heavy - 1;
        const int hm = __builtin_amdgcn_readlane(mult, src);
        const int hcj = __builtin_amdgcn_readlane(cj, src);
        const int hfi = __builtin_amdgcn_readlane(fi, src);
        const int hfj = __builtin_amdgcn_readlane(fj, src);
        const int q_lo = __builtin_amdgcn_readlane((int)(uint32_t)q, src);   // q < INT32_MAX (count refused more)
        const uint32_t v_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
        const uint32_t v_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
        const uint64_t hv = ((uint64_t)v_hi << 32) | v_lo;
        for (int t = lane; t < hm; t += MX_WAVE) {
            const int a = t / hcj, b = t - a * hcj;
            const int64_t o = (int64_t)q_lo + t;
            out_rows[o] = csl_position<MAP_I>(ai, hfi, a);
            out_cols[o] = csl_position<MAP_J>(aj, hfj, b);
            csl_store_value<VK>(out_vals, o, hv);
        }
    }
}

// ---- single element: smallest k with (rows[k], cols[k]) == (r, c) ----------------------------------------------
constexpr int CSS_MAX_BLOCKS = 1024;

__device__ __forceinline__ long long block_min_i64(long long v)
{
    __shared__ long long wave_min[CSL_BLOCK / MX_WAVE];
#pragma unroll
    for (int off = MX_WAVE / 2; off > 0; off >>= 1) {
        const long long o = __shfl_xor(v, off, MX_WAVE);
        v = o < v ? o : v;
    }
    const int wave = threadIdx.x / MX_WAVE;
    if (lane_id() == 0) wave_min[wave] = v;
    __syncthreads();
    long long m = wave_min[0];
#pragma unroll
    for (int w = 1; w < CSL_BLOCK / MX_WAVE; w++) m = wave_min[w] < m ? wave_min[w] : m;
    return m;
}

__global__ __launch_bounds__(CSL_BLOCK)
void coo_single_partial_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ cols, int64_t nnz,
                               int r, int c, long long *__restrict__ partial)
{
    long long best = LLONG_MAX;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * blockDim.x)
        if (rows[k] == r && cols[k] == c) { best = k; break; }    // a lane's k ascend: its first hit is its minimum
    const long long m = block_min_i64(best);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// out[0] = the first matching k or -1, out[1] = the bits of its value (f64, or the int32 R logical); one block
__global__ __launch_bounds__(CSL_BLOCK)
void coo_single_final_kernel(const long long *__restrict__ partial, int nblocks, const void *__restrict__ vals,
                             int value_dtype, long long *__restrict__ out)
{
    long long best = LLONG_MAX;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) best = partial[b] < best ? partial[b] : best;
    const long long m = block_min_i64(best);
    if (threadIdx.x == 0) {
        long long bits = 0;
        if (m != LLONG_MAX && vals) {
            if (value_dtype == MX_F64) bits = ((const long long *)vals)[m];
            else if (value_dtype == MX_LGL) bits = ((const int32_t *)vals)[m];
        }
        out[0] = m == LLONG_MAX ? -1 : m;
        out[1] = bits;
    }
}

struct CslLayout {
    WsCursor c;
    int64_t nnz;
    int32_t *counts = c.take_counts(nnz), *offsets = c.take_i32(nnz + 1), *flags = c.take<int32_t>(16);
    size_t bytes = c.bytes();
    CslLayout(const void *ws, int64_t nnz_) : c(ws), nnz(nnz_ > 0 ? nnz_ : 0) {}
};

// the single-cell lookup: {entry index, value bits}, then one partial per block
struct CssLayout {
    WsCursor c;
    long long *out = c.take<long long>(2 * sizeof(long long));
    long long *partial = c.take<long long>(CSS_MAX_BLOCKS * sizeof(long long));
    size_t bytes = c.bytes();
    explicit CssLayout(const void *ws) : c(ws) {}
};

static int csl_check_axis(const mx_coo_axis *a, int n, const char *what)
{
    MX_REQUIRE(a, "mxd_coo_slice: null %s axis", what);
    if (a->kind == MX_AXIS_MAP) {
        MX_REQUIRE(a->nmap >= 0 && (a->nmap == 0 || (a->start && a->pos)), "mxd_coo_slice: bad %s map", what);
    } else {
        MX_REQUIRE(a->kind == MX_AXIS_AFFINE, "mxd_coo_slice: unknown %s axis kind %d", what, a->kind);
        MX_REQUIRE(a->lo >= 0 && a->lo <= a->hi && a->hi < n, "mxd_coo_slice: %s range [%d, %d] outside [0, %d)",
                   what, a->lo, a->hi, n);
    }
    return 0;
}

// f(map_i, map_j): the two axis kinds (checked by csl_check_axis) as compile-time bools
template <typename F>
static int csl_dispatch_axes(const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, F &&f)
{
    using kinds = int_list<MX_AXIS_MAP, MX_AXIS_AFFINE>;
    return dispatch_int(kinds{}, "mxd_coo_slice", "row axis kind", axis_i->kind, [&](auto ki) {
        return dispatch_int(kinds{}, "mxd_coo_slice", "column axis kind", axis_j->kind, [&](auto kj) {
            f(std::bool_constant<ki() == MX_AXIS_MAP>{}, std::bool_constant<kj() == MX_AXIS_MAP>{});
            MX_LAUNCH_CHECK();
            return 0;
        });
    });
}

}  // namespace mx

extern "C" size_t mxd_coo_slice_workspace_bytes(int64_t nnz) { return mx::CslLayout(nullptr, nnz).bytes; }

extern "C" int mxd_coo_slice_count(int nrow, int ncol, const int32_t *rows, const int32_t *cols, int64_t nnz,
                                   const mx_coo_axis *axis_i, const mx_coo_axis *axis_j, void *workspace,
                                   int64_t *nnz_out_host, void *stream)
{
    MX_REQUIRE(nrow >= 0 && ncol >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_coo_slice_count: bad size");
    MX_REQUIRE(nnz_out_host && (nnz == 0 || (rows && cols && workspace)), "mxd_coo_slice_count: null pointer");
    if (mx::csl_check_axis(axis_i, nrow, "row") || mx::csl_check_axis(axis_j, ncol, "column")) return 1;
    if (nnz == 0) { *nnz_out_host = 0; return 0; }
    hipStream_t st = mx::as_stream(stream);
    const mx::CslLayout L(workspace, nnz);
    int32_t *flags = L.flags;
    MX_HIP(hipMemsetAsync(flags, 0, 16, st));
    const mx::CslAxis ai = mx::csl_axis(*axis_i), aj = mx::csl_axis(*axis_j);
    const unsigned g = (unsigned)mx::ceil_div(nnz, mx::CSL_BLOCK);
    const int lrc = mx::csl_dispatch_axes(axis_i, axis_j, [&](auto mi, auto mj) {
        hipLaunchKernelGGL((mx::coo_slice_count_kernel<mi(), mj()>), dim3(g), dim3(mx::CSL_BLOCK), 0, st, nrow, ncol,
                           rows, cols, nnz, ai, aj, L.counts, flags);
    });
    if (lrc) return lrc;
    const int rc = mx::finish_count(nnz, L.counts, L.offsets, nnz_out_host, st);
    int32_t hf[4] = {0, 0, 0, 0};
    MX_HIP(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    MX_REQUIRE(!hf[0], "mxd_coo_slice_count: row index outside [0, %d)", nrow);
    MX_REQUIRE(!hf[1], "mxd_coo_slice_count: column index outside [0, %d)", ncol);
    MX_REQUIRE(!hf[2], "slice of a COO: one entry is selected more than %d times (exceeds R's int32 index range)",
               INT_MAX);
    return rc;
}

extern "C" int mxd_coo_slice_fill(int nrow, int ncol, const int32_t *rows, const int32_t *cols, const void *values,
                                  int value_dtype, int64_t nnz, const mx_coo_axis *axis_i, const mx_coo_axis *axis_j,
                                  const void *workspace, int32_t *out_rows, int32_t *out_cols, void *out_values,
                                  void *stream)
{
    MX_REQUIRE(nrow >= 0 && ncol >= 0 && nnz >= 0 && nnz <= INT_MAX, "mxd_coo_slice_fill: bad size");
    if (mx::csl_check_axis(axis_i, nrow, "row") || mx::csl_check_axis(axis_j, ncol, "column")) return 1;
    if (nnz == 0) return 0;
    MX_REQUIRE(rows && cols && workspace && out_rows && out_cols, "mxd_coo_slice_fill: null pointer");
    MX_REQUIRE(value_dtype == MX_NONE || (values && out_values), "mxd_coo_slice_fill: null values");
    hipStream_t st = mx::as_stream(stream);
    const int32_t *off = mx::CslLayout(workspace, nnz).offsets;
    const mx::CslAxis ai = mx::csl_axis(*axis_i), aj = mx::csl_axis(*axis_j);
    const unsigned g = (unsigned)mx::ceil_div(nnz, mx::CSL_BLOCK);
    using kinds = mx::int_list<MX_F64, MX_LGL, MX_NONE>;
    return mx::dispatch_int(kinds{}, "mxd_coo_slice_fill", "value dtype", value_dtype, [&](auto vk) {
        return mx::csl_dispatch_axes(axis_i, axis_j, [&](auto mi, auto mj) {
            hipLaunchKernelGGL((mx::coo_slice_fill_kernel<mi(), mj(), vk()>), dim3(g), dim3(mx::CSL_BLOCK), 0, st, nrow,
                               ncol, rows, cols, values, nnz, ai, aj, off, out_rows, out_cols, out_values);
        });
    });
}

extern "C" size_t mxd_coo_single_workspace_bytes(void) { return mx::CssLayout(nullptr).bytes; }

extern "C" int mxd_coo_single(const int32_t *rows, const int32_t *cols, const void *values, int value_dtype,
                              int64_t nnz, int r, int c, void *workspace, int64_t *k_host, void *value_host,
                              void *stream)
{
    MX_REQUIRE(nnz >= 0 && k_host && workspace, "mxd_coo_single: bad arguments");
    MX_REQUIRE(value_dtype == MX_F64 || value_dtype == MX_LGL || value_dtype == MX_NONE,
               "mxd_coo_single: unsupported value dtype %d", value_dtype);
    MX_REQUIRE(nnz == 0 || (rows && cols && (value_dtype == MX_NONE || values)), "mxd_coo_single: null pointer");
    *k_host = -1;
    if (nnz == 0) return 0;
    hipStream_t st = mx::as_stream(stream);
    const mx::CssLayout L(workspace);
    long long *out = L.out, *partial = L.partial;
    const int64_t want = mx::ceil_div(nnz, mx::CSL_BLOCK);
    const int nb = (int)(want < mx::CSS_MAX_BLOCKS ? want : mx::CSS_MAX_BLOCKS);
    hipLaunchKernelGGL(mx::coo_single_partial_kernel, dim3(nb), dim3(mx::CSL_BLOCK), 0, st, rows, cols, nnz, r, c,
                       partial);
    MX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mx::coo_single_final_kernel, dim3(1), dim3(mx::CSL_BLOCK), 0, st, partial, nb,
                       value_dtype == MX_NONE ? nullptr : values, value_dtype, out);
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

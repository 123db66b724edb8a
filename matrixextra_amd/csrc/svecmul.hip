// svecmul.hip — RsparseMatrix * sparseVector, the masked row scaling, for gfx950.
//
// Replaces:
//   multiply_csr_by_svec_no_NAs    src/operators.cpp:3426-3498
//   multiply_csr_by_svec_keep_NAs  src/operators.cpp:3500-3697
// (both serial loops that push_back row after row).
//
// The vector v (sorted 1-based positions vi[0..nv), f64 values vx or none, length L) is recycled down the rows:
// output row r looks up t = r mod L in vi (vi is small and stays in L2) once, in the count pass, by a G-ary search
// of its lane group; the position found goes to the workspace for the fill.  One G-lane group per row, G from the
// mean row length; count -> finish_count (scan, 64-bit total, one read-back) -> fill:
//   t not stored, ignore NAs                 nothing
//   t not stored, keep NAs                   the row's NaN / +-Inf entries in place order: a NaN keeps its payload,
//                                            +-Inf becomes the default quiet NaN (:3557-3565, :3623-3631)
//   t stored, val finite (or ignore NAs, or  the whole row, x * val; values copied when v has none
//     v without values)                      (:3463-3480, :3590-3607)
//   t stored, val NaN / +-Inf, keep NAs      all ncol columns: NaN val -> val everywhere; +-Inf val -> the default
//                                            NaN, and val * x at the stored columns (:3575-3586)
// The reference's "X has some NaN / Inf" switch (:3514) only chooses between two loops that give the same rows
// when X is clean, so no pass over all of X is made for it: the count pass reads the values of the rows that v
// does not store (it has to, to count them) and raises one flag word when it meets a NaN / Inf there.
//
// A dense-filled row is written by the whole wave, 64 consecutive columns per store instruction, whatever G is
// (mx_dense_row.h, shared with dvecna.hip).  Under an Inf val the value of column c comes from a binary search of
// the (sorted) row for its last entry with that column: with a repeated column the last one wins, as in the
// reference's scatter, without two stores racing.
// Row bounds are clamped into [0, nnz] in both passes and every write position comes from the scanned counts, so
// nothing is read or written out of bounds whatever the input.
#include "mx_dispatch.h"
#include "mx_workspace.h"
#include "mx_dense_row.h"

namespace mx {

constexpr int SV_BLOCK = 256;

__device__ __forceinline__ bool sv_nonfinite(double x) { return isnan(x) || isinf(x); }
__device__ __forceinline__ double sv_nan() { return __longlong_as_double(0x7FF8000000000000LL); }   // C's NAN

struct SvRow {
    int s, len;          // entries [s, s + len) of X
    bool stored, dense;  // t is in v; the row becomes ncol entries
    double val;          // v's value there (1.0 without values)
};

// position of `key` in the sorted vi[0..nv), or -1: a G-ary search by the row's lane group (each step every lane
// probes its own split point, as cd_first_at does wave-wide): about log2(nv) / log2(G) dependent loads instead of
// log2(nv), that is 4 for a million positions at G = 32 or 64 and 10 at G = 4, against 20.  Called by all G lanes
// of a group with the same key.
template <int G>
__device__ __forceinline__ int sv_find(const int32_t *__restrict__ vi, int nv, int key, int lg)
{
    static_assert(G >= 2, "with one lane the search would step through the vector entry by entry");
    int s = 0, e = nv;                                      // the first position with vi[.] >= key lies in [s, e]
    while (e > s) {
        const int step = (e - s + G - 1) / G;
        const int64_t q = (int64_t)s + (int64_t)lg * step;
        const int below = __popcll(group_ballot<G>(q < e && vi[q] < key));   // splits that start below the key
        if (below == 0) { e = s; break; }
        const int64_t ne = (int64_t)s + (int64_t)below * step;
        s += (below - 1) * step + 1;
        e = ne < e ? (int)ne : e;
    }
    return s < nv && vi[s] == key ? s : -1;
}

__device__ __forceinline__ SvRow sv_row(long long r, int64_t nnz, const int32_t *__restrict__ indptr, int pos,
                                        const double *__restrict__ vx, bool keep_na)
{
    SvRow w{0, 0, pos >= 0, false, 1.0};
    const RowBounds b = row_bounds(indptr[r], indptr[r + 1], nnz);
    w.s = (int)b.start;
    w.len = (int)b.len;
    if (w.stored && vx) {
        w.val = vx[pos];
        w.dense = keep_na && sv_nonfinite(w.val);
    }
    return w;
}

template <int G>
__global__ __launch_bounds__(SV_BLOCK)
void sv_count_kernel(int m, int ncol, int64_t nnz, const int32_t *__restrict__ indptr,
                     const double *__restrict__ values, const int32_t *__restrict__ vi, int nv,
                     const double *__restrict__ vx, int length, int keep_na, int32_t *__restrict__ counts,
                     int32_t *__restrict__ vpos, volatile unsigned long long *__restrict__ x_na_flag)
{
    const int lg = threadIdx.x % G;
    const long long r = (long long)blockIdx.x * (SV_BLOCK / G) + threadIdx.x / G;
    if (r >= m) return;                                     // whole groups leave: the ballots below stay group-wide
    const int pos = sv_find<G>(vi, nv, (int)(r % length) + 1, lg);
    const SvRow w = sv_row(r, nnz, indptr, pos, vx, keep_na != 0);
    int cnt = w.dense ? ncol : w.len;
    if (!w.stored) {
        cnt = 0;
        if (keep_na) {
            for (int k0 = 0; k0 < w.len; k0 += G) {
                const int k = k0 + lg;
                cnt += __popcll(group_ballot<G>(k < w.len && sv_nonfinite(values[w.s + k])));
            }
            if (cnt && lg == 0 && *x_na_flag == 0) *x_na_flag = 1;   // a flag: a counter would serialise the rows
        }
    }
    if (lg == 0) { counts[r] = cnt; vpos[r] = pos; }       // the fill reads the position back: one search a row
}

// a dense-filled row (mx_dense_row.h): NaN val -> val everywhere; +-Inf val -> the default NaN, val * x where stored
struct SvDenseRule {
    __device__ __forceinline__ bool looks_up(double val) const { return isinf(val); }
    __device__ __forceinline__ double fill(double val) const { return isinf(val) ? sv_nan() : val; }
    __device__ __forceinline__ double at(double x, double val) const { return val * x; }
};

template <int G>
__global__ __launch_bounds__(SV_BLOCK)
void sv_fill_kernel(int m, int ncol, int64_t nnz, const int32_t *__restrict__ indptr,
                    const int32_t *__restrict__ indices, const double *__restrict__ values,
                    const double *__restrict__ vx, int keep_na, const int32_t *__restrict__ vpos,
                    const int32_t *__restrict__ out_indptr, int32_t *__restrict__ out_indices,
                    double *__restrict__ out_values)
{
    const int lg = threadIdx.x % G;
    const long long r = (long long)blockIdx.x * (SV_BLOCK / G) + threadIdx.x / G;
    int64_t dst = 0;
    int cnt = 0;
    if (r < m) { dst = out_indptr[r]; cnt = out_indptr[r + 1] - (int32_t)dst; }
    SvRow w{0, 0, false, false, 1.0};
    if (cnt > 0) w = sv_row(r, nnz, indptr, vpos[r], vx, keep_na != 0);              // empty output rows read nothing

    if (w.stored && !w.dense) {                             // the whole row, scaled (or copied)
        for (int k = lg; k < w.len; k += G) {
            out_indices[dst + k] = indices[w.s + k];
            out_values[dst + k] = vx ? values[w.s + k] * w.val : values[w.s + k];
        }
    } else if (!w.stored && cnt > 0) {                      // the row's NaN / Inf entries, in place order
        const unsigned long long below = (1ULL << lg) - 1ULL;
        int64_t o = dst;
        for (int k0 = 0; k0 < w.len; k0 += G) {
            const int k = k0 + lg;
            double x = 0.0;
            bool keep = false;
            if (k < w.len) { x = values[w.s + k]; keep = sv_nonfinite(x); }
            const unsigned long long kb = group_ballot<G>(keep);
            if (keep) {
                const int64_t q = o + __popcll(kb & below);
                out_indices[q] = indices[w.s + k];
                out_values[q] = isinf(x) ? sv_nan() : x;
            }
            o += __popcll(kb);
        }
    }

    // dense-filled rows: the wave takes them one after another, 64 consecutive columns per store (mx_dense_row.h)
    write_dense_rows(w.dense && lg == 0, dst, w.s, w.len, w.val, ncol, indices, values, out_indices, out_values,
                     SvDenseRule{});
}

struct SvLayout {
    WsCursor c;
    int m;
    int32_t *counts = c.take_counts(m);
    unsigned long long *na_flag = c.take<unsigned long long>(16);      // one word in 16 B
    int32_t *pos = c.take_i32(m);                                       // position in v of each row, or -1
    size_t bytes = c.bytes();
    SvLayout(const void *ws, int m_) : c(ws), m(m_ > 0 ? m_ : 0) {}
};

static int sv_check(const char *what, int m, int ncol, int64_t nnz, int64_t nv, int length)
{
    MX_REQUIRE(m >= 0 && ncol >= 0 && nnz >= 0 && nnz <= INT_MAX && nv >= 0 && nv <= INT_MAX,
               "%s: bad arguments", what);
    MX_REQUIRE(m == 0 || length > 0, "%s: the vector has no length", what);
    return 0;
}

}  // namespace mx

extern "C" size_t mxd_csr_by_svec_workspace_bytes(int m) { return mx::SvLayout(nullptr, m).bytes; }

extern "C" int mxd_csr_by_svec_count(int m, int ncol, int64_t nnz, const int32_t *indptr, const double *values,
                                     const int32_t *vi_base1, int64_t nv, const double *vx, int length, int keep_na,
                                     void *workspace, int32_t *out_indptr, int64_t *nnz_out_host,
                                     int64_t *x_na_host, void *stream)
{
    if (mx::sv_check("mxd_csr_by_svec_count", m, ncol, nnz, nv, length)) return 1;
    MX_REQUIRE(workspace && out_indptr && nnz_out_host && x_na_host, "mxd_csr_by_svec_count: null pointer");
    MX_REQUIRE(m == 0 || (indptr && (nv == 0 || vi_base1) && (nnz == 0 || !keep_na || values)),
               "mxd_csr_by_svec_count: null pointer");
    hipStream_t st = mx::as_stream(stream);
    *nnz_out_host = 0;
    *x_na_host = 0;
    const mx::SvLayout L(workspace, m);
    unsigned long long *flag = L.na_flag;
    MX_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned long long), st));
    if (m > 0) {
        const int G = mx::pick_group((double)nnz / (double)m);
        const int rc = mx::launch_rows(mx::lane_groups{}, "mxd_csr_by_svec_count", G, m, mx::SV_BLOCK,
                                       [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(mx::sv_count_kernel<g()>, grid, block, 0, st, m, ncol, nnz, indptr, values, vi_base1,
                               (int)nv, vx, length, keep_na, L.counts, L.pos, flag);
        });
        if (rc) return rc;
    }
    MX_HIP(hipMemcpyAsync(x_na_host, flag, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    // the 64-bit total is read back (one synchronise) and refused above INT_MAX before any output exists
    return mx::finish_count(m, L.counts, out_indptr, nnz_out_host, st);
}

extern "C" int mxd_csr_by_svec_fill(int m, int ncol, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                    const double *values, const int32_t *vi_base1, int64_t nv, const double *vx,
                                    int length, int keep_na, const void *workspace, const int32_t *out_indptr,
                                    int32_t *out_indices, double *out_values, void *stream)
{
    if (mx::sv_check("mxd_csr_by_svec_fill", m, ncol, nnz, nv, length)) return 1;
    if (m == 0) return 0;
    MX_REQUIRE(workspace && indptr && out_indptr && out_indices && out_values && (nv == 0 || vi_base1) &&
               (nnz == 0 || (indices && values)), "mxd_csr_by_svec_fill: null pointer");
    hipStream_t st = mx::as_stream(stream);
    const int G = mx::pick_group((double)nnz / (double)m);
    return mx::launch_rows(mx::lane_groups{}, "mxd_csr_by_svec_fill", G, m, mx::SV_BLOCK,
                           [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(mx::sv_fill_kernel<g()>, grid, block, 0, st, m, ncol, nnz, indptr, indices, values, vx,
                           keep_na, mx::SvLayout(workspace, m).pos, out_indptr, out_indices, out_values);
    });
}

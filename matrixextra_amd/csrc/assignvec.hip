// assignvec.hip — X[, c] <- vector and the pattern of X[r, ] <- vector of a dgRMatrix for gfx950.
//
// Replaces the serial loops of src/assignment.cpp:
//   set_single_col_to_colvec  :839-913      set_single_col_to_svec  :1009-1133
//     (one insert_col_into_row :8-117 or remove_col_from_row :119-180 per row)
//   the recycling loops of set_single_row_to_rowvec :771-837 and set_single_row_to_svec :915-1007
//
// A pattern is (ii, xx, length): 0-based positions ii[0..nnz) inside [0, length) with their values; ii == nullptr is
// the dense pattern 0..length-1.  It is recycled along an axis of n = length * repeats entries.
//
// Column route.  Row r asks for position q = r % length: when the pattern stores q (always, when dense; a search
// of the ascending ii by the whole group otherwise) the row ends up holding (col, xx[.]), else it ends up without col.  The
// skeleton is assign.hip's: per-row lengths -> exclusive scan -> fill, one G-lane group per row.  What a row does
// follows from its two lengths alone (new - old = +1 insert, -1 remove, 0 replace or copy), so the fill needs no
// second search for the column before it starts writing.  Only the first entry of a row that holds col counts, as
// in the reference.  Rows must be sorted for an insert to land at its ascending place; every store goes through
// asg_store and stays inside the row's own slots whatever the row holds.
//
// Row route.  The pattern is expanded into a one-row CSR, which mxd_csr_replace_rows_* (assign.hip) puts in place.
#include "mx_assign.h"

namespace mx {

// q stored by the pattern?  *t = where its value is.  The whole group asks for the same q, so its G lanes search
// together: each step probes the last element of G equal chunks and a ballot names the chunk that holds the lower
// bound, log_G(nnz) dependent loads where a lane searching alone needs log_2(nnz).  Group-uniform; every lane of the
// group must call it.
template <int G>
__device__ __forceinline__ bool avc_stores(const int32_t *__restrict__ ii, int nnz_pat, int q, int lg, int *t)
{
    if (!ii) { *t = q; return true; }
    int lo = 0, len = nnz_pat;                         // the lower bound of q lies in [lo, lo + len]
    while (len > 0) {
        const int end = lo + len, chunk = (len + G - 1) / G;
        const long long at = (long long)lo + (long long)(lg + 1) * chunk - 1;      // last element of this lane's chunk
        const int below = __popcll(group_ballot<G>(at < end && ii[at] < q));         // chunks that lie wholly below q
        const long long next = (long long)lo + (long long)below * chunk;
        lo = next < end ? (int)next : end;
        len = chunk - 1 < end - lo ? chunk - 1 : end - lo;
    }
    *t = lo;
    return lo < nnz_pat && ii[lo] == q;
}

// ---- column route: count -----------------------------------------------------------------------------------------
// lens[row] = len - has_col + stores.  *removed (sparse patterns only) counts the rows that lose the column: with
// the total it gives the number of rows whose structure changes (see mxd_csr_assign_col_count).
template <int G>
__global__ __launch_bounds__(AS_BLOCK)
void assign_col_count_kernel(int nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                             int col, const int32_t *__restrict__ ii, int nnz_pat, int length,
                             int32_t *__restrict__ lens, int32_t *__restrict__ removed)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (AS_BLOCK / G) + threadIdx.x / G;
    const bool valid = row < nrows;
    int s = 0, e = 0;
    if (valid) { s = indptr[row]; e = indptr[row + 1]; }
    bool has = false;
    for (int k0 = s; k0 < e; k0 += G) {                // e - s is uniform inside the group
        const int k = k0 + lg;
        has |= group_ballot<G>(k < e && indices[k] == col) != 0ULL;
    }
    int t = 0;
    const bool stores = valid && avc_stores<G>(ii, nnz_pat, (int)(row % length), lg, &t);     // valid is group-uniform
    if (valid && lg == 0) lens[row] = e - s - (int)has + (int)stores;
    if (removed) {                                     // uniform over the grid
        const int n = __popcll(__ballot(valid && lg == 0 && has && !stores));
        if (n && lane_id() == 0) atomicAdd(removed, n);
    }
}

// ---- column route: fill ------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(AS_BLOCK)
void assign_col_fill_kernel(int nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                            const uint64_t *__restrict__ values, int col, const int32_t *__restrict__ ii,
                            const uint64_t *__restrict__ xx, int nnz_pat, int length,
                            const int32_t *__restrict__ new_indptr, int32_t *__restrict__ new_indices,
                            uint64_t *__restrict__ new_values)
{
    const int lg = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (AS_BLOCK / G) + threadIdx.x / G;
    const bool valid = row < nrows;
    int s = 0, e = 0, o = 0, oe = 0;
    if (valid) {
        s = indptr[row]; e = indptr[row + 1];
        o = new_indptr[row]; oe = new_indptr[row + 1];
    }
    int t = 0;
    const bool stores = valid && avc_stores<G>(ii, nnz_pat, (int)(row % length), lg, &t);     // valid is group-uniform
    const uint64_t v = stores ? xx[t] : 0ULL;
    const int grow = (oe - o) - (e - s);               // +1 insert, -1 remove, 0 replace or copy; uniform in the group
    if (grow > 0) {                                    // entries below col keep their offset, the others move up one
        const int L = lower_bound_dev(indices + s, e - s, col);
        for (int k = s + lg; k < e; k += G)
            asg_store(new_indices, new_values, o, oe, o + (k - s) + (k - s >= L ? 1 : 0), indices[k], values[k]);
        if (lg == 0 && stores) asg_store(new_indices, new_values, o, oe, o + L, col, v);
        return;
    }
    bool found = false;                                // the first entry that holds col is the one replaced or dropped
    for (int k0 = s; k0 < e; k0 += G) {
        const int k = k0 + lg;
        const bool in = k < e;
        const int c = in ? indices[k] : 0;
        const unsigned long long hb = group_ballot<G>(in && c == col);
        const int first = (!found && hb) ? __ffsll((long long)hb) - 1 : -1;
        if (in) {
            if (grow < 0) {                            // order-preserving compaction
                const int shift = (found || (first >= 0 && lg > first)) ? 1 : 0;
                if (lg != first) asg_store(new_indices, new_values, o, oe, o + (k - s) - shift, c, values[k]);
            } else {
                asg_store(new_indices, new_values, o, oe, o + (k - s), c, (lg == first && stores) ? v : values[k]);
            }
        }
        found = found || hb != 0ULL;
    }
}

// ---- the recycled pattern as one CSR row -------------------------------------------------------------------------
__global__ __launch_bounds__(AS_BLOCK)
void expand_pattern_row_kernel(const int32_t *__restrict__ ii, const uint64_t *__restrict__ xx, int nnz_pat,
                               int length, long long total, int32_t *__restrict__ row_indptr,
                               int32_t *__restrict__ row_indices, uint64_t *__restrict__ row_values)
{
    const long long t = (long long)blockIdx.x * AS_BLOCK + threadIdx.x;
    if (t == 0 && row_indptr) { row_indptr[0] = 0; row_indptr[1] = (int32_t)total; }
    if (t >= total) return;
    const int k = (int)(t % nnz_pat);
    if (row_indices) row_indices[t] = ii ? ii[k] + length * (int)(t / nnz_pat) : (int32_t)t;
    row_values[t] = xx[k];
}

static int avc_check(const char *what, int nrows, int col, int ncols, const int32_t *ii, int64_t n_xx, int length)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0, "%s: bad size", what);
    MX_REQUIRE(col >= 0 && col < ncols, "%s: column %d outside [0, %d)", what, col, ncols);
    MX_REQUIRE(length > 0 && n_xx >= 0 && n_xx <= length, "%s: bad pattern (%lld entries, length %d)", what,
               (long long)n_xx, length);
    MX_REQUIRE(ii || n_xx == length, "%s: a dense pattern has length entries", what);
    return 0;
}

}  // namespace mx

extern "C" int mxd_csr_assign_col_count(int nrows, int ncols, const int32_t *indptr, const int32_t *indices,
                                        int64_t nnz, int col, const int32_t *ii, int64_t n_xx, int length,
                                        double avg_row_len, int32_t *new_indptr, void *workspace,
                                        int64_t *nnz_out_host, int64_t *changed_out_host, void *stream)
{
    const char *what = "mxd_csr_assign_col_count";
    if (mx::avc_check(what, nrows, col, ncols, ii, n_xx, length)) return 1;
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX, "%s: bad size", what);
    MX_REQUIRE(indptr && new_indptr && workspace && nnz_out_host && changed_out_host, "%s: null pointer", what);
    MX_REQUIRE(nnz == 0 || indices, "%s: null indices", what);
    hipStream_t st = mx::as_stream(stream);
    int32_t *lens = mx::CountLayout(workspace, nrows).counts;
    // the rows that lose the column are counted in new_indptr[0], which the scan only writes afterwards; the count
    // travels to the host ahead of the scan and arrives with the total, behind the one synchronisation
    int32_t *removed = ii && nrows > 0 ? new_indptr : nullptr;
    int32_t removed_host = 0;
    if (nrows > 0) {
        if (removed) MX_HIP(hipMemsetAsync(removed, 0, sizeof(int32_t), st));
        const int rc = mx::launch_rows(mx::lane_groups{}, what, mx::pick_group(avg_row_len), nrows, mx::AS_BLOCK,
                                       [&](auto g, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((mx::assign_col_count_kernel<g()>), grid, block, 0, st, nrows, indptr, indices, col, ii,
                               (int)n_xx, length, lens, removed);
        });
        if (rc) return rc;
        if (removed) MX_HIP(hipMemcpyAsync(&removed_host, removed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    *changed_out_host = 0;
    if (mx::asg_finish_count(nrows, workspace, new_indptr, nnz_out_host, st)) {
        (void)hipStreamSynchronize(st);                // removed_host leaves scope: nothing may still be writing it
        return 1;
    }
    // inserted - removed = total - nnz, and a dense pattern removes nothing
    *changed_out_host = *nnz_out_host - nnz + 2 * (int64_t)removed_host;
    return 0;
}

extern "C" int mxd_csr_assign_col_fill(int nrows, int ncols, const int32_t *indptr, const int32_t *indices,
                                       const double *values, int col, const int32_t *ii, const double *xx,
                                       int64_t n_xx, int length, double avg_row_len, const int32_t *new_indptr,
                                       int32_t *new_indices, double *new_values, void *stream)
{
    const char *what = "mxd_csr_assign_col_fill";
    if (mx::avc_check(what, nrows, col, ncols, ii, n_xx, length)) return 1;
    if (nrows == 0) return 0;
    MX_REQUIRE(indptr && new_indptr && new_values && (xx || n_xx == 0), "%s: null pointer", what);
    hipStream_t st = mx::as_stream(stream);
    return mx::launch_rows(mx::lane_groups{}, what, mx::pick_group(avg_row_len), nrows, mx::AS_BLOCK,
                           [&](auto g, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((mx::assign_col_fill_kernel<g()>), grid, block, 0, st, nrows, indptr, indices,
                           (const uint64_t *)values, col, ii, (const uint64_t *)xx, (int)n_xx, length, new_indptr,
                           new_indices, (uint64_t *)new_values);
    });
}

extern "C" int mxd_csr_expand_pattern_row(const int32_t *ii, const double *xx, int64_t n_xx, int length,
                                          int n_repeats, int32_t *row_indptr, int32_t *row_indices,
                                          double *row_values, void *stream)
{
    const char *what = "mxd_csr_expand_pattern_row";
    MX_REQUIRE(length > 0 && n_repeats > 0 && n_xx >= 0 && n_xx <= length, "%s: bad pattern (%lld entries, length %d, "
               "%d repetitions)", what, (long long)n_xx, length, n_repeats);
    MX_REQUIRE(ii || n_xx == length, "%s: a dense pattern has length entries", what);
    MX_REQUIRE((int64_t)length * n_repeats <= INT_MAX, "%s: the recycled pattern is longer than INT_MAX", what);
    const int64_t total = n_xx * n_repeats;
    MX_REQUIRE(row_values || total == 0, "%s: null pointer", what);
    MX_REQUIRE(xx || n_xx == 0, "%s: null pointer", what);
    hipLaunchKernelGGL(mx::expand_pattern_row_kernel, dim3(mx::grid_for(total, mx::AS_BLOCK)), dim3(mx::AS_BLOCK), 0,
                       mx::as_stream(stream), ii, (const uint64_t *)xx, (int)n_xx, length, (long long)total,
                       row_indptr, row_indices, (uint64_t *)row_values);
    MX_LAUNCH_CHECK();
    return 0;
}

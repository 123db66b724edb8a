// mx_dense_row.h — the dense-filled rows of `CSR (op) vector` when R's NAs are kept: a row whose vector value makes
// every cell NA / NaN / 1 / Inf comes out with all ncol columns (svecmul.hip: multiply_csr_by_svec_keep_NAs,
// src/operators.cpp:3575-3586; dvecna.hip: multiply_csr_by_dvec_with_NAs, :2344-2351 and its siblings).
//
// Such a row is written by the whole wave, 64 consecutive columns per store instruction, whatever lane-group width
// the kernel around it runs at.  Where the stored columns keep a value of their own, column c's value comes from a
// binary search of the (sorted) row for its last entry with that column: with a repeated column the last one wins,
// as in the reference's scatter, without two stores racing.
#pragma once
#include "mx_common.h"

namespace mx {

#ifdef __HIPCC__
// Called by every lane of the wave (no lane may have left).  `leader` marks the lanes that hold a dense row: its
// output offset dst, its entries [s, s + len) of the source and the vector value val that rules it.  The wave takes
// the marked rows one after another.  Rule:
//   double fill(double val)            the value of a column the row does not store
//   bool   looks_up(double val)        whether the stored columns get a value of their own
//   double at(double x, double val)    that value, from the entry's x
template <typename Rule>
__device__ __forceinline__ void write_dense_rows(bool leader, int64_t dst, int s, int len, double val, int ncol,
                                                 const int32_t *__restrict__ indices,
                                                 const double *__restrict__ values,
                                                 int32_t *__restrict__ out_indices, double *__restrict__ out_values,
                                                 const Rule &rule)
{
    const int lane = lane_id();
    unsigned long long todo = __ballot(leader);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t d0 = __shfl(dst, src, MX_WAVE);
        const int rs = __shfl(s, src, MX_WAVE), rlen = __shfl(len, src, MX_WAVE);
        const double rval = __shfl(val, src, MX_WAVE);
        const bool looks_up = rule.looks_up(rval);
        const double fill = rule.fill(rval);
        for (int c = lane; c < ncol; c += MX_WAVE) {
            double v = fill;
            if (looks_up) {                                 // last entry of the row with column c, if any
                const int32_t *__restrict__ row = indices + rs;
                int lo = 0, n = rlen;
                while (n > 0) {                             // first position with row[.] > c
                    const int step = n >> 1;
                    if (row[lo + step] <= c) { lo += step + 1; n -= step + 1; }
                    else n = step;
                }
                if (lo > 0 && row[lo - 1] == c) v = rule.at(values[rs + lo - 1], rval);
            }
            out_indices[d0 + c] = c;
            out_values[d0 + c] = v;
        }
    }
}
#endif  // __HIPCC__

}  // namespace mx

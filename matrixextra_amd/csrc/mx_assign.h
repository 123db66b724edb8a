// mx_assign.h — what the two kernel units of `[<-` (assign.hip, assignvec.hip) share: the block size, the one store
// every fill goes through, and the end of every count pass.
#pragma once
#include "mx_dispatch.h"
#include "mx_workspace.h"

namespace mx {
#pragma GCC visibility push(hidden)

constexpr int AS_BLOCK = 256;

#ifdef __HIPCC__
// values travel as their 64 bits: a NaN's payload (R's NA_real_) is written as given.  new_indices may be null (the
// structure stays the caller's and only values are made).
__device__ __forceinline__ void asg_store(int32_t *__restrict__ new_indices, uint64_t *__restrict__ new_values,
                                          int lo, int hi, int pos, int c, uint64_t v)
{
    if (pos < lo || pos >= hi) return;                 // never outside the row's own slots
    if (new_indices) new_indices[pos] = c;
    new_values[pos] = v;
}
#endif

// scan the counts; a total beyond R's int32 index range fails with the reference's text (check_max_size,
// src/assignment.cpp:380-382) before the caller allocates anything
static inline int asg_finish_count(int nrows, void *workspace, int32_t *new_indptr, int64_t *nnz_out_host,
                                   hipStream_t st)
{
    *nnz_out_host = 0;
    if (finish_count(nrows, workspace, new_indptr, nnz_out_host, st)) {
        if (*nnz_out_host > (int64_t)INT_MAX)
            return set_error("Error: resulting matrix would be larger than INT_MAX limit.");
        return 1;
    }
    return 0;
}

#pragma GCC visibility pop
}  // namespace mx

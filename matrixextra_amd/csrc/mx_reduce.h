// mx_reduce.h — the reduction family inside libmxgpu: its C-ABI (include/mxgpu_reduce.h) and what the export level
// (api_reduce.hip) takes from reduce.hip besides it.
#pragma once
#include "mx_common.h"
#include "../../include/mxgpu_reduce.h"

namespace mx {
#pragma GCC visibility push(hidden)
// out[s] /= cells - skipped[s] for s < n (skipped may be null): the divisor of rowMeans / colMeans
int reduce_mean_divide(double *out, const int32_t *skipped, int64_t n, double cells, hipStream_t st);
#pragma GCC visibility pop
}  // namespace mx

// mx_workspace.h — host side only: how a caller-allocated workspace is cut into segments.
//
// Every workspace has ONE description: a struct whose constructor takes (workspace, sizes...), walks a WsCursor over
// it once, and leaves named, typed pointers plus `bytes`.  The members ARE the walk: the cursor and the sizes come
// first, each pointer member then takes its segment in its initialiser, and members are initialised in the order they
// are declared, so the declaration order is the order in memory (`bytes` is declared last).  The exported
// mxd_*_workspace_bytes function is Layout(nullptr, sizes...).bytes, and every user of the workspace constructs the
// same struct on the real pointer, so the size and the offsets cannot drift apart.  The cursor adds no alignment of
// its own: a segment starts where the previous one ended, and a layout that wants a rounded size says so in the bytes
// it takes.
#pragma once
#include "mx_common.h"

namespace mx {
#pragma GCC visibility push(hidden)

class WsCursor {
    uintptr_t base_, at_;

public:
    explicit WsCursor(const void *base) : base_((uintptr_t)base), at_(base_) {}
    // the current position (an offset from null when the base is null), then `bytes` further
    template <typename T = void> T *take(size_t bytes)
    {
        T *p = (T *)at_;
        at_ += bytes;
        return p;
    }
    // int32[max(n, 1)], padded to 16 B
    int32_t *take_i32(int64_t n) { return take<int32_t>(padded_i32_bytes(n)); }
    // the block finish_count(n, block, ...) works on: int32 counts[n], then the scan workspace; returns the counts
    int32_t *take_counts(int64_t n) { return take<int32_t>(count_workspace_bytes(n)); }
    size_t bytes() const { return (size_t)(at_ - base_); }
};

// a workspace that is one count block and nothing else (merge, gather, the row-ruled dvec-NA route, the dense outer
// product): counts[n], scanned by finish_count
struct CountLayout {
    WsCursor c;
    int32_t *counts;
    size_t bytes = c.bytes();
    CountLayout(const void *ws, int64_t n) : c(ws), counts(c.take_counts(n)) {}
};

// a count block and the offsets finish_count scans it into: counts[n], offsets[n + 1]
struct CountOffsetsLayout {
    WsCursor c;
    int64_t n;
    int32_t *counts = c.take_counts(n), *offsets = c.take_i32(n + 1);
    size_t bytes = c.bytes();
    CountOffsetsLayout(const void *ws, int64_t n_) : c(ws), n(n_ > 0 ? n_ : 0) {}
};

#pragma GCC visibility pop
}  // namespace mx

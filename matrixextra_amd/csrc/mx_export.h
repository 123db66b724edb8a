// mx_export.h — what the export level (the export-level units: api.hip, api_assign.hip) keeps its arrays and results
// in: owning device arrays that know their element size, the caller's values as one description, and the result under
// construction.  Host-only: no kernel unit includes it.  Byte counts and pointer casts live here and nowhere in those
// units.
#pragma once
#include "mx_common.h"
#include <cstring>
#include <memory>
#include <new>
#include <vector>
#pragma GCC visibility push(hidden)     // helpers of the unit that includes it: none of this joins the dynamic symbols
namespace mx {

static inline size_t dtype_bytes(int dt)
{
    switch (dt) { case MX_F64: return 8; case MX_F32: case MX_I32: case MX_LGL: return 4; default: return 0; }
}

// Owning device buffer of a run-time element size: value arrays, whose type an mx_dtype chooses, dense operands
// and workspaces.  It converts to whatever pointer the device routine declares; the dtype travels beside it.
// A buffer never allocated is a null pointer; an empty one still gets a non-null, 16-byte aligned pointer.
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> operator T *() const { return static_cast<T *>(p); }
    // the one place a count becomes bytes: a negative count (or one beyond size_t) fails before anything is allocated
    static int bytes_of(int64_t count, size_t elem_bytes, size_t *bytes)
    {
        MX_REQUIRE(count >= 0 && (uint64_t)count <= SIZE_MAX / (elem_bytes ? elem_bytes : 1),
                   "device array: bad element count %lld (of %zu bytes each)", (long long)count, elem_bytes);
        *bytes = (size_t)count * elem_bytes;
        return 0;
    }
    int alloc_bytes(size_t n)                // workspaces: the mxd_*_workspace_bytes functions give bytes
    {
        if (n == 0) n = 16;                  // keep pointers non-null and 16-B aligned
        MX_HIP(hipMalloc(&p, n));
        return 0;
    }
    int alloc(int64_t count, size_t elem_bytes) { size_t n; return bytes_of(count, elem_bytes, &n) || alloc_bytes(n); }
    int upload(const void *h, int64_t count, size_t elem_bytes)
    {
        size_t n;
        if (bytes_of(count, elem_bytes, &n) || alloc_bytes(n)) return 1;
        return n && mx::xfer_h2d(p, h, n);   // pipelined through pinned slots when large (xfer.hip)
    }
    int download(void *h, int64_t count, size_t elem_bytes) const
    {
        size_t n;
        return bytes_of(count, elem_bytes, &n) || mx::xfer_d2h(h, p, n);
    }
    int zero(int64_t count, size_t elem_bytes)                       // synchronous, on the null stream
    {
        size_t n;
        if (bytes_of(count, elem_bytes, &n)) return 1;
        MX_HIP(hipMemset(p, 0, n));
        return 0;
    }
    int copy_from(const DevBuf &src, int64_t count, size_t elem_bytes)     // device to device, on the null stream
    {
        size_t n;
        if (bytes_of(count, elem_bytes, &n)) return 1;
        MX_HIP(hipMemcpyAsync(p, src.p, n, hipMemcpyDeviceToDevice, nullptr));
        return 0;
    }
};

// Owning device array of T: what was uploaded as T is handed on as T *, and counts are elements.
template <typename T>
class Dev {
    DevBuf b;
public:
    operator T *() const { return static_cast<T *>(b.p); }
    int alloc(int64_t count) { return b.alloc(count, sizeof(T)); }
    int upload(const T *h, int64_t count) { return b.upload(h, count, sizeof(T)); }
    int download(T *h, int64_t count) const { return b.download(h, count, sizeof(T)); }
    int zero(int64_t count) { return b.zero(count, sizeof(T)); }
    int copy_from(const Dev &src, int64_t count) { return b.copy_from(src.b, count, sizeof(T)); }
};

// The caller's values, from an export's (value_dtype, n_values): an empty values vector means a pattern matrix,
// as the reference's `if (values.size())` does.
struct Values {
    int dtype;                               // what to pass on: MX_NONE when there are no values
    size_t bytes;                            // of one value, 0 when there are none
    explicit Values(int value_dtype, int64_t n_values = 1)
        : dtype(value_dtype != MX_NONE && n_values > 0 ? value_dtype : MX_NONE), bytes(dtype_bytes(dtype)) {}
    explicit operator bool() const { return dtype != MX_NONE; }
};

// Admission of a value dtype; `admitted` has bit 1 << dtype set for each kind the export takes.
constexpr unsigned kNumeric = 1u << MX_F64, kInteger = 1u << MX_I32, kLogical = 1u << MX_LGL, kPattern = 1u << MX_NONE;
static inline int admit_values(const char *what, int value_dtype, unsigned admitted = kNumeric | kLogical | kPattern)
{
    MX_REQUIRE(value_dtype >= 0 && value_dtype <= MX_NONE && (admitted >> value_dtype & 1u),
               "%s: unsupported value dtype %d", what, value_dtype);
    return 0;
}

// The reference's if/else chain over its five operator flags, in its precedence (operators.cpp:1620-1632,
// :2275-2289, :2872-2883); none set is its throw_internal_err().
static inline int dvec_op_of(int multiply, int powerto, int divide, int divrest, int intdiv, int *op)
{
    if (multiply) *op = MX_DV_MULTIPLY;
    else if (powerto) *op = MX_DV_POWERTO;
    else if (divide) *op = MX_DV_DIVIDE;
    else if (divrest) *op = MX_DV_DIVREST;
    else if (intdiv) *op = MX_DV_INTDIV;
    else return set_error("Internal error. Please file an issue in GitHub.");
    return 0;
}

struct Csr {
    Dev<int32_t> p, j;
    DevBuf x;
    int64_t nnz = 0;
    // uploads indptr[0..m], indices/values[0..indptr[m]); value_bytes 0 => no values
    int upload(const int32_t *indptr, const int32_t *indices, const void *values, int m, size_t value_bytes)
    {
        MX_REQUIRE(m >= 0 && indptr, "CSR upload: bad arguments");
        nnz = indptr[m];
        MX_REQUIRE(nnz >= 0 && indptr[0] >= 0, "CSR upload: negative index pointer");
        if (p.upload(indptr, (int64_t)m + 1)) return 1;
        if (j.upload(indices, nnz)) return 1;
        if (value_bytes && x.upload(values, nnz, value_bytes)) return 1;
        return 0;
    }
};

// Many host arrays in ONE device buffer (the operands of an rbind).  add() gives an array its 16-byte aligned place
// and remembers where its device pointer is to be written; upload() allocates, fills those pointers in and sends
// everything up as one stream (xfer_h2d_parts): no transfer per array and no host copy of the whole.
class BindStaging {
    std::vector<XferPart> parts;
    std::vector<const void **> devs;
    size_t total = 0;
    DevBuf buf;

public:
    // an absent array (host null or no bytes of it) keeps a null device pointer
    void add(const void *host, size_t bytes, const void **dev)
    {
        *dev = nullptr;
        if (!host || bytes == 0) return;
        parts.push_back(XferPart{host, bytes, total});
        devs.push_back(dev);
        total += (bytes + 15) & ~(size_t)15;
    }
    int upload()
    {
        if (buf.alloc_bytes(total)) return 1;
        for (size_t k = 0; k < parts.size(); k++) *devs[k] = (char *)buf.p + parts[k].at;
        return mx::xfer_h2d_parts(buf.p, total, parts.data(), parts.size());
    }
};

}  // namespace mx

// Variable-size result waiting on the device for the caller's vectors.  Its sizes and its three allocations are
// written here and nowhere else; a result starts with three empty vectors that are its own.
struct mx_result {
    mx::Dev<int32_t> indptr, indices;
    mx::DevBuf values;
    mx_result_info info = {};
    // the indptr vector, which the count pass writes (a COO carries its row ids there)
    int alloc_indptr(int64_t n) { info.indptr_len = n; return indptr.alloc(n); }
    // the values alone, beside a structure that stays the caller's; value_bytes 0 => no values
    int alloc_values(int64_t n, size_t value_bytes)
    { info.values_len = value_bytes ? n : 0; return value_bytes ? values.alloc(n, value_bytes) : 0; }
    // the entries: nnz indices and nnz values
    int alloc_entries(int64_t nnz, size_t value_bytes)
    { info.nnz = nnz; return indices.alloc(nnz) || alloc_values(nnz, value_bytes); }
    // sizes alone: no vectors at all, or vectors allocated for the input's entries of which the fill reports fewer
    void set_sizes(int64_t indptr_len, int64_t nnz, int64_t values_len)
    { info.indptr_len = indptr_len; info.nnz = nnz; info.values_len = values_len; }
    // how = 1: the structure stays the caller's and only values come back; MX_ALIAS_ALL: all three vectors do
    void alias(int how, int64_t indptr_len, int64_t nnz) { info.alias_structure = how; set_sizes(indptr_len, nnz, nnz); }
};

// The one owner of an mx_result under construction: `body` fills it and returns 0, or fails and the result is
// freed.  Every success ends with the null stream synchronised, which mx_result_finish's transfers rely on
// (device buffers the body frees on its way out are safe: hipFree synchronises the device).
template <typename Body>
static int begin_result(mx_result **res_out, mx_result_info *info, int values_dtype, Body &&body)
{
    std::unique_ptr<mx_result> res(new (std::nothrow) mx_result());
    MX_REQUIRE(res, "out of host memory");
    res->info.values_dtype = values_dtype;
    res->info.alias_structure = 0;
    if (const int rc = body(*res)) return rc;
    MX_HIP(hipStreamSynchronize(nullptr));
    *info = res->info;
    *res_out = res.release();
    return 0;
}
#pragma GCC visibility pop

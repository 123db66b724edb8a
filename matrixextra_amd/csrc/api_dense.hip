// api_dense.hip — export level of the dense <-> compressed conversions (host pointers, include/mxgpu_dense.h): upload,
// the count and fill passes or the one scatter launch of dense.hip, the result as an mx_result or in the caller's
// matrix.  Synchronous; everything runs on the null stream.
#include "mx_export.h"
#include "../../include/mxgpu_dense.h"

using namespace mx;

static int admit_sizes(const char *what, int a, int b)
{
    MX_REQUIRE(a >= 0 && b >= 0, "%s: negative dimension", what);
    return 0;
}

extern "C" int mx_dense_to_csr_begin(const void *dense, int m, int n, int dense_dtype, int by_col, int out_dtype,
                                     mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_dense_to_csr_begin";
    MX_REQUIRE(res_out && info, "%s: null pointer", what);
    if (admit_sizes(what, m, n)) return 1;
    MX_REQUIRE(dense_dtype == MX_F64 || dense_dtype == MX_F32 || dense_dtype == MX_I32 || dense_dtype == MX_LGL,
               "%s: unsupported dense dtype %d", what, dense_dtype);
    MX_REQUIRE(out_dtype == MX_F64 || out_dtype == MX_LGL || out_dtype == MX_NONE, "%s: unsupported output dtype %d", what,
               out_dtype);
    const int64_t cells = (int64_t)m * n;
    MX_REQUIRE(cells == 0 || dense, "%s: null pointer", what);
    *res_out = nullptr;
    return begin_result(res_out, info, out_dtype, [&](mx_result &res) {
        DevBuf d, ws;
        if (d.upload(dense, cells, dtype_bytes(dense_dtype))) return 1;
        if (ws.alloc_bytes(mxd_dense_to_csr_workspace_bytes(m, n, by_col, 0))) return 1;
        if (res.alloc_indptr((int64_t)(by_col ? n : m) + 1)) return 1;
        int64_t nnz = 0;
        if (mxd_dense_to_csr_count(m, n, d, m, dense_dtype, by_col, 0, res.indptr, ws, &nnz, nullptr)) return 1;
        if (res.alloc_entries(nnz, dtype_bytes(out_dtype))) return 1;
        if (mxd_dense_to_csr_fill(m, n, d, m, dense_dtype, by_col, 0, res.indptr, ws, res.indices, res.values, out_dtype,
                                  nullptr))
            return 1;
        MX_HIP(hipStreamSynchronize(nullptr));                          // the operand and the workspace go out of scope here
        return 0;
    });
}

extern "C" int mx_csr_to_dense(const int32_t *indptr, int nseg, int nother, const int32_t *indices, const void *values,
                               int value_dtype, int by_col, void *out, int out_dtype)
{
    const char *what = "mx_csr_to_dense";
    if (admit_sizes(what, nseg, nother)) return 1;
    if (admit_values(what, value_dtype)) return 1;
    MX_REQUIRE(out_dtype == MX_F64 || out_dtype == MX_LGL, "%s: unsupported output dtype %d", what, out_dtype);
    MX_REQUIRE(indptr, "%s: null pointer", what);
    MX_REQUIRE(indptr[0] == 0 && indptr[nseg] >= 0, "%s: bad index pointer", what);
    const int64_t nnz = indptr[nseg], cells = (int64_t)nseg * nother;
    MX_REQUIRE((nnz == 0 || (indices && (value_dtype == MX_NONE || values))) && (cells == 0 || out), "%s: null pointer",
               what);
    MX_REQUIRE(nnz == 0 || nother > 0, "%s: index out of bounds", what);
    if (cells == 0) return 0;
    const Values V(value_dtype, nnz);                  // an operand without values at all is a pattern
    const int m = by_col ? nother : nseg;
    Csr X;
    if (X.upload(indptr, indices, values, nseg, V.bytes)) return 1;
    DevBuf o;
    Dev<int32_t> flag;
    if (o.alloc(cells, dtype_bytes(out_dtype)) || flag.alloc(1) || flag.zero(1)) return 1;
    const void *x = V ? (const void *)X.x : nullptr;
    if (mxd_csr_to_dense(nseg, nother, X.p, X.j, x, V.dtype, by_col, 0, o, m, out_dtype, flag, nullptr)) return 1;
    int32_t flagged = 0;
    MX_HIP(hipStreamSynchronize(nullptr));             // the transfers below do not wait for the null stream
    if (flag.download(&flagged, 1)) return 1;
    if (flagged) {
        // not sorted, or a cell twice: the canonical arrays through the COO sort, which merges repeated cells and
        // refuses an index out of bounds; then the scatter again
        Dev<int32_t> rows, p2, j2;
        DevBuf x2, ws;
        if (rows.alloc(nnz) || p2.alloc((int64_t)nseg + 1) || j2.alloc(nnz)) return 1;
        if (V && x2.alloc(nnz, V.bytes)) return 1;
        if (ws.alloc_bytes(mxd_coo_to_csr_workspace_bytes(nnz, nother))) return 1;
        if (mxd_csr_to_coo(nseg, nnz, X.p, rows, nullptr)) return 1;
        int64_t merged = 0;
        if (mxd_coo_to_csr(nseg, nother, rows, X.j, x, V.dtype, nnz, p2, j2, V ? (void *)x2 : nullptr, ws, &merged, nullptr))
            return 1;
        if (flag.zero(1)) return 1;
        if (mxd_csr_to_dense(nseg, nother, p2, j2, V ? (const void *)x2 : nullptr, V.dtype, by_col, 0, o, m, out_dtype, flag,
                             nullptr))
            return 1;
        MX_HIP(hipStreamSynchronize(nullptr));
        if (flag.download(&flagged, 1)) return 1;
        MX_REQUIRE(!flagged, "%s: the arrays do not form a matrix", what);
    }
    return o.download(out, cells, dtype_bytes(out_dtype));
}

// api_sym.hip — export level of the structured-matrix family (host pointers, include/mxgpu_sym.h): the general CSR of
// a symmetric or unit-triangular operand as an mx_result, and the triangle check.  Synchronous; everything is computed
// by the routines of sym.hip on the null stream.
#include "mx_export.h"
#include "../../include/mxgpu_sym.h"

using namespace mx;

namespace {

// what the two expansions check before anything is uploaded
static int admit(const char *what, const int32_t *indptr, int n, const int32_t *indices, const void *values,
                 int value_dtype, int64_t n_values, int uplo, mx_result **res, mx_result_info *info)
{
    MX_REQUIRE(res && info && indptr, "%s: null pointer", what);
    MX_REQUIRE(n >= 0, "%s: negative dimension", what);
    if (admit_values(what, value_dtype)) return 1;
    MX_REQUIRE(uplo == MX_UPLO_UPPER || uplo == MX_UPLO_LOWER, "%s: uplo must be MX_UPLO_UPPER or MX_UPLO_LOWER, got %d",
               what, uplo);
    MX_REQUIRE(indptr[0] == 0 && indptr[n] >= 0, "%s: bad index pointer", what);
    const Values vals(value_dtype, n_values);
    MX_REQUIRE(!vals || n_values == indptr[n], "%s: lengths of indices and values differ", what);
    MX_REQUIRE(indptr[n] == 0 || (indices && (!vals || values)), "%s: null pointer", what);
    *res = nullptr;
    return 0;
}

}  // namespace

extern "C" int mx_csr_symmetric_to_general_begin(const int32_t *indptr, int n, const int32_t *indices,
                                                 const void *values, int value_dtype, int64_t n_values, int uplo,
                                                 mx_result **res_out, mx_result_info *info)
{
    if (admit("mx_csr_symmetric_to_general_begin", indptr, n, indices, values, value_dtype, n_values, uplo, res_out,
              info))
        return 1;
    const Values vals(value_dtype, n_values);
    return begin_result(res_out, info, vals.dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, n, vals.bytes)) return 1;
        DevBuf ws;
        if (ws.alloc_bytes(mxd_csr_sym_workspace_bytes(n, A.nnz))) return 1;
        if (res.alloc_indptr((int64_t)n + 1)) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_symmetric_to_general_count(n, A.p, A.j, A.nnz, uplo, res.indptr, ws, &nnz_out, nullptr)) return 1;
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        return mxd_csr_symmetric_to_general_fill(n, A.p, A.j, A.x, vals.dtype, A.nnz, uplo, res.indptr, nnz_out,
                                                 res.indices, res.values, ws, nullptr);
    });
}

extern "C" int mx_csr_unit_triangular_to_general_begin(const int32_t *indptr, int n, const int32_t *indices,
                                                       const void *values, int value_dtype, int64_t n_values, int uplo,
                                                       mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_csr_unit_triangular_to_general_begin";
    if (admit(what, indptr, n, indices, values, value_dtype, n_values, uplo, res_out, info)) return 1;
    const Values vals(value_dtype, n_values);
    return begin_result(res_out, info, vals.dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, n, vals.bytes)) return 1;
        DevBuf ws;
        int64_t outside = 0;
        if (ws.alloc_bytes(16)) return 1;
        if (mxd_csr_triangle_check(n, A.p, A.j, A.nnz, uplo, 1, ws, &outside, nullptr)) return 1;
        MX_REQUIRE(!outside, "%s: %lld entr%s on the diagonal or outside the stored triangle (uplo = \"%s\", diag = \"U\")",
                   what, (long long)outside, outside == 1 ? "y lies" : "ies lie", uplo == MX_UPLO_LOWER ? "L" : "U");
        if (res.alloc_indptr((int64_t)n + 1)) return 1;
        if (res.alloc_entries(A.nnz + n, vals.bytes)) return 1;
        return mxd_csr_unit_triangular_to_general(n, A.p, A.j, A.x, vals.dtype, A.nnz, uplo, res.indptr, res.indices,
                                                  res.values, nullptr);
    });
}

extern "C" int mx_csr_triangle_check(const int32_t *indptr, int n, const int32_t *indices, int uplo, int strict,
                                     int64_t *outside)
{
    MX_REQUIRE(indptr && outside && n >= 0, "mx_csr_triangle_check: bad arguments");
    MX_REQUIRE(indptr[0] == 0 && indptr[n] >= 0, "mx_csr_triangle_check: bad index pointer");
    MX_REQUIRE(indptr[n] == 0 || indices, "mx_csr_triangle_check: null pointer");
    Csr A;
    if (A.upload(indptr, indices, nullptr, n, 0)) return 1;
    DevBuf ws;
    if (ws.alloc_bytes(16)) return 1;
    return mxd_csr_triangle_check(n, A.p, A.j, A.nnz, uplo, strict, ws, outside, nullptr);
}

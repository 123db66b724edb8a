// api_spgemm.hip — export level of the sparse x sparse product (host pointers, include/mxgpu_spgemm.h): one upload, the
// transposes the signature asks for on the device (the column order of transpose.hip and the gather of tprod.hip: rows
// sorted, no second sort), the count and fill passes of spgemm.hip, the result as an mx_result.  Synchronous; everything
// runs on the null stream.
#include "mx_export.h"
#include "../../include/mxgpu_spgemm.h"

using namespace mx;

namespace {

// an operand as the product reads it: the uploaded CSR, or the CSR of its transpose put together on the device
struct Operand {
    Csr up;
    Dev<int32_t> perm, colptr, rows;
    DevBuf tx;
    int nrow = 0, ncol = 0;                  // of op(X)
    const int32_t *p = nullptr, *j = nullptr;
    const void *x = nullptr;
    int64_t nnz = 0;

    int build(const int32_t *indptr, const int32_t *indices, const void *values, const Values &V, int m, int K, int trans)
    {
        if (up.upload(indptr, indices, values, m, V.bytes)) return 1;
        nnz = up.nnz;
        if (!trans) {
            nrow = m, ncol = K, p = up.p, j = up.j, x = V ? (const void *)up.x : nullptr;
            return 0;
        }
        DevBuf tws;
        if (perm.alloc(nnz) || colptr.alloc((int64_t)K + 1) || rows.alloc(nnz)) return 1;
        if (V && tx.alloc(nnz, V.bytes)) return 1;
        if (tws.alloc_bytes(mxd_csr_transpose_workspace_bytes(nnz))) return 1;
        if (mxd_csr_column_order(m, K, up.p, up.j, nnz, perm, colptr, tws, nullptr)) return 1;
        if (mxd_csr_transpose_by_order(m, nnz, up.p, V ? (const void *)up.x : nullptr, V.dtype, perm, rows,
                                       V ? (void *)tx : nullptr, nullptr))
            return 1;
        MX_HIP(hipStreamSynchronize(nullptr));                          // tws goes out of scope here
        nrow = K, ncol = m, p = colptr, j = rows, x = V ? (const void *)tx : nullptr;
        return 0;
    }
};

static int admit(const char *what, const char *which, const int32_t *indptr, int nrow, int ncol, const int32_t *indices,
                 const void *values, int value_dtype)
{
    MX_REQUIRE(indptr, "%s: null pointer", what);
    MX_REQUIRE(nrow >= 0 && ncol >= 0, "%s: negative dimension", what);
    if (admit_values(what, value_dtype)) return 1;
    MX_REQUIRE(indptr[0] == 0 && indptr[nrow] >= 0, "%s: bad index pointer of %s", what, which);
    MX_REQUIRE(indptr[nrow] == 0 || (indices && (value_dtype == MX_NONE || values)), "%s: null pointer", what);
    return 0;
}

}  // namespace

extern "C" int mx_csr_spgemm_begin(const int32_t *Ap, int m, int K, const int32_t *Aj, const void *Ax, int a_dtype,
                                   int trans_a, const int32_t *Bp, int K2, int n, const int32_t *Bj, const void *Bx,
                                   int b_dtype, int trans_b, mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_csr_spgemm_begin";
    MX_REQUIRE(res_out && info, "%s: null pointer", what);
    if (admit(what, "A", Ap, m, K, Aj, Ax, a_dtype) || admit(what, "B", Bp, K2, n, Bj, Bx, b_dtype)) return 1;
    *res_out = nullptr;
    const int inner_a = trans_a ? m : K, inner_b = trans_b ? n : K2;
    MX_REQUIRE(inner_a == inner_b, "%s: the inner dimensions differ: op(A) has %d columns, op(B) %d rows", what, inner_a,
               inner_b);
    // an operand without values at all is a pattern, as everywhere in the export level
    const Values VA(a_dtype, Ap[m]), VB(b_dtype, Bp[K2]);
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Operand A, B;
        if (A.build(Ap, Aj, Ax, VA, m, K, trans_a) || B.build(Bp, Bj, Bx, VB, K2, n, trans_b)) return 1;
        DevBuf ws;
        if (ws.alloc_bytes(mxd_csr_spgemm_workspace_bytes(A.nrow, B.ncol))) return 1;
        if (res.alloc_indptr((int64_t)A.nrow + 1)) return 1;
        int64_t products = 0, nnz_out = 0;
        if (mxd_csr_spgemm_count(A.nrow, A.ncol, B.ncol, A.p, A.j, A.nnz, B.p, B.j, B.nnz, res.indptr, ws, &products,
                                 &nnz_out, nullptr))
            return 1;
        if (res.alloc_entries(nnz_out, sizeof(double))) return 1;
        return mxd_csr_spgemm_fill(A.nrow, A.ncol, B.ncol, A.p, A.j, A.x, VA.dtype, B.p, B.j, B.x, VB.dtype, res.indptr,
                                   res.indices, (double *)res.values, ws, nullptr);
    });
}

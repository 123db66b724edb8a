// api_gram.hip — export level of the one-triangle Gram product (host pointers, include/mxgpu_gram.h): one upload, one
// transpose on the device (the column order of transpose.hip and the gather of tprod.hip: rows sorted, no second sort),
// the masked count and fill passes of spgemm.hip, the result as an mx_result.  Synchronous; everything runs on the null
// stream.
#include "mx_export.h"
#include "../../include/mxgpu_gram.h"

using namespace mx;

extern "C" int mx_csr_gram_begin(const int32_t *indptr, int nrow, int ncol, const int32_t *indices, const void *values,
                                 int value_dtype, int trans, int uplo, mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_csr_gram_begin";
    MX_REQUIRE(res_out && info && indptr, "%s: null pointer", what);
    MX_REQUIRE(nrow >= 0 && ncol >= 0, "%s: negative dimension", what);
    if (admit_values(what, value_dtype)) return 1;
    MX_REQUIRE(uplo == MX_UPLO_UPPER || uplo == MX_UPLO_LOWER, "%s: uplo must be MX_UPLO_UPPER or MX_UPLO_LOWER, got %d",
               what, uplo);
    MX_REQUIRE(indptr[0] == 0 && indptr[nrow] >= 0, "%s: bad index pointer", what);
    MX_REQUIRE(indptr[nrow] == 0 || (indices && (value_dtype == MX_NONE || values)), "%s: null pointer", what);
    *res_out = nullptr;
    const Values V(value_dtype, indptr[nrow]);      // an operand without values at all is a pattern
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Csr X;
        if (X.upload(indptr, indices, values, nrow, V.bytes)) return 1;
        const int64_t nnz = X.nnz;
        const void *x = V ? (const void *)X.x : nullptr;
        // X^T (ncol x nrow) through the column order: its rows are sorted, the order is stable
        Dev<int32_t> perm, colptr, rows, flag_ws;
        DevBuf tx, tws, ws;
        if (perm.alloc(nnz) || colptr.alloc((int64_t)ncol + 1) || rows.alloc(nnz)) return 1;
        if (V && tx.alloc(nnz, V.bytes)) return 1;
        if (tws.alloc_bytes(mxd_csr_transpose_workspace_bytes(nnz))) return 1;
        if (mxd_csr_column_order(nrow, ncol, X.p, X.j, nnz, perm, colptr, tws, nullptr)) return 1;
        if (mxd_csr_transpose_by_order(nrow, nnz, X.p, x, V.dtype, perm, rows, V ? (void *)tx : nullptr, nullptr))
            return 1;
        const void *t = V ? (const void *)tx : nullptr;
        // trans = 0: X X^T, the transposed side on the right; else X^T X, whose right-hand rows are X's own
        int b_sorted = 1;
        if (trans) {
            if (flag_ws.alloc(4)) return 1;
            if (mxd_csr_rows_sorted(nrow, X.p, X.j, flag_ws, &b_sorted, nullptr)) return 1;
        }
        const int m = trans ? ncol : nrow, K = trans ? nrow : ncol;
        const int32_t *Ap = trans ? (const int32_t *)colptr : (const int32_t *)X.p;
        const int32_t *Aj = trans ? (const int32_t *)rows : (const int32_t *)X.j;
        const int32_t *Bp = trans ? (const int32_t *)X.p : (const int32_t *)colptr;
        const int32_t *Bj = trans ? (const int32_t *)X.j : (const int32_t *)rows;
        const void *Ax = trans ? t : x, *Bx = trans ? x : t;
        if (ws.alloc_bytes(mxd_csr_spgemm_workspace_bytes(m, m))) return 1;
        if (res.alloc_indptr((int64_t)m + 1)) return 1;
        int64_t products = 0, nnz_out = 0;
        if (mxd_csr_spgemm_tri_count(m, K, m, Ap, Aj, nnz, Bp, Bj, nnz, uplo, b_sorted, res.indptr, ws, &products, &nnz_out,
                                     nullptr))
            return 1;
        if (res.alloc_entries(nnz_out, sizeof(double))) return 1;
        if (mxd_csr_spgemm_tri_fill(m, K, m, Ap, Aj, Ax, V.dtype, Bp, Bj, Bx, V.dtype, uplo, b_sorted, res.indptr,
                                    res.indices, (double *)res.values, ws, nullptr))
            return 1;
        MX_HIP(hipStreamSynchronize(nullptr));                          // the operands and workspaces go out of scope here
        return 0;
    });
}

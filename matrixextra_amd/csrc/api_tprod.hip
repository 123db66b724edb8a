// api_tprod.hip — export level of the transposed products (host pointers, include/mxgpu_tprod.h): X^T v through the
// segmented dot of tprod.hip, X^T B through the SpMM launch path on the CSR of X^T, which is put together on the device
// from the column order of transpose.hip and never crosses PCIe.  Synchronous; results go into the caller's buffers.
#include "mx_export.h"
#include "mx_reduce.h"
#include "../../include/mxgpu_tprod.h"

#include <algorithm>

using namespace mx;

namespace {

// the column order of the uploaded A and the entry rows in that order: the pattern of A^T
struct Transposed {
    Dev<int32_t> perm, colptr, rows;
    int build(const Csr &A, int nrow, int ncol)
    {
        DevBuf tws;
        if (perm.alloc(A.nnz) || colptr.alloc((int64_t)ncol + 1) || rows.alloc(A.nnz)) return 1;
        if (tws.alloc_bytes(mxd_csr_transpose_workspace_bytes(A.nnz))) return 1;
        if (mxd_csr_column_order(nrow, ncol, A.p, A.j, A.nnz, perm, colptr, tws, nullptr)) return 1;
        return mxd_csr_transpose_by_order(nrow, A.nnz, A.p, nullptr, MX_NONE, perm, rows, nullptr, nullptr);
    }
};

static int check_csr(const char *what, int nrow, int ncol, const int32_t *indptr, const int32_t *indices,
                     const void *values, const Values &V)
{
    MX_REQUIRE(nrow >= 0 && ncol >= 0 && indptr, "%s: bad dimensions or null indptr", what);
    const int64_t nnz = indptr[nrow];
    MX_REQUIRE(nnz >= 0 && (nnz == 0 || (indices && (!V || values))), "%s: null pointer", what);
    return 0;
}

template <typename real_t>
static int tmatmul(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const double *values,
                   const real_t *B_host, int ldb, int n, real_t *C_host, int ldc, bool colmajor)
{
    const int64_t c_rows = colmajor ? n : ncol, c_cols = colmajor ? ncol : n;
    // reference early-out of the SpMM exports (matmul.cpp:128-129,160-161): the result is the zero matrix
    if (indptr[0] == indptr[nrow]) {
        for (int64_t r = 0; r < c_rows; r++) std::fill_n(C_host + r * ldc, c_cols, real_t(0));
        return 0;
    }
    Csr A;
    if (A.upload(indptr, indices, values, nrow, sizeof(double))) return 1;
    Dev<real_t> B, C;
    if (B.upload(B_host, (int64_t)(nrow - 1) * ldb + n)) return 1;
    if (C.alloc(c_rows * ldc)) return 1;
    Transposed T;
    Dev<double> tx;
    if (T.build(A, nrow, ncol) || tx.alloc(A.nnz)) return 1;
    if (mxd_csr_transpose_by_order(nrow, A.nnz, A.p, A.x, MX_F64, T.perm, nullptr, tx, nullptr)) return 1;
    // rows of X^T list their source rows in ascending order: the order is stable
    if (mxd_spmm_csr_dense_ex(ncol, n, nrow, T.colptr, T.rows, tx, B, ldb, C, ldc, sizeof(real_t) == 8 ? MX_F64 : MX_F32,
                              colmajor ? 1 : 0, MX_SPMM_AUTO, 1, 0, 0, nullptr))
        return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    if (ldc == c_cols) return C.download(C_host, c_rows * c_cols);
    for (int64_t r = 0; r < c_rows; r++)                                    // a padded C: the padding stays the caller's
        if (xfer_d2h(C_host + r * ldc, (const real_t *)C + r * ldc, (size_t)c_cols * sizeof(real_t))) return 1;
    return 0;
}

}  // namespace

extern "C" int mx_csr_tmatvec(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                              int value_dtype, const double *v, double *out)
{
    if (admit_values("mx_csr_tmatvec", value_dtype, kNumeric | kPattern)) return 1;
    const Values V(value_dtype);
    if (check_csr("mx_csr_tmatvec", nrow, ncol, indptr, indices, values, V)) return 1;
    if (ncol == 0) return 0;
    MX_REQUIRE(out, "mx_csr_tmatvec: null output");
    if (indptr[0] == indptr[nrow]) { std::fill_n(out, ncol, 0.0); return 0; }
    MX_REQUIRE(v, "mx_csr_tmatvec: null vector");
    Csr A;
    if (A.upload(indptr, indices, values, nrow, V.bytes)) return 1;
    Dev<double> dv, dout;
    if (dv.upload(v, nrow) || dout.alloc(ncol)) return 1;
    Transposed T;
    DevBuf ws;
    if (T.build(A, nrow, ncol) || ws.alloc_bytes(4 * mxd_compact_workspace_bytes(A.nnz))) return 1;
    if (mxd_segment_dot(A.x, V.dtype, T.perm, T.rows, dv, nrow, A.nnz, T.colptr, ncol, dout, ws, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    return dout.download(out, ncol);
}

extern "C" int mx_csr_tmatmul_dense(int nrow, int ncol, const int32_t *indptr, const int32_t *indices,
                                    const double *values, const void *B, int ldb, int n, int dense_dtype, void *C,
                                    int ldc, int c_colmajor)
{
    if (check_csr("mx_csr_tmatmul_dense", nrow, ncol, indptr, indices, values, Values(MX_F64))) return 1;
    MX_REQUIRE(n >= 0, "mx_csr_tmatmul_dense: negative dimension");
    MX_REQUIRE(dense_dtype == MX_F64 || dense_dtype == MX_F32, "mx_csr_tmatmul_dense: unsupported dense dtype %d",
               dense_dtype);
    if (ncol == 0 || n == 0) return 0;
    MX_REQUIRE(C && ldc >= (c_colmajor ? ncol : n), "mx_csr_tmatmul_dense: null output or ldc below the row length");
    MX_REQUIRE(indptr[0] == indptr[nrow] || (B && ldb >= n), "mx_csr_tmatmul_dense: null B or ldb below n");
    if (dense_dtype == MX_F64)
        return tmatmul<double>(nrow, ncol, indptr, indices, values, (const double *)B, ldb, n, (double *)C, ldc,
                               c_colmajor != 0);
    return tmatmul<float>(nrow, ncol, indptr, indices, values, (const float *)B, ldb, n, (float *)C, ldc, c_colmajor != 0);
}

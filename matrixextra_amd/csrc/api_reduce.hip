// api_reduce.hip — export level of the reduction family (host pointers, include/mxgpu_reduce.h): margin sums and
// means, norm and diag over the kernels of reduce.hip and the column order of transpose.hip.  Synchronous; results go
// into the caller's buffers.  The last step of norm "O" / "I" is the same segmented reduction over the margin sums,
// run as one MX_RED_ABS_MAX segment: nothing here loops over a result on the host.
#include "mx_export.h"
#include "mx_reduce.h"

#include <cmath>

using namespace mx;

namespace {

// the operand on the device and the scratch of one segmented reduction over n entries
static int reduce_ws(DevBuf &ws, int64_t n) { return ws.alloc_bytes(4 * mxd_compact_workspace_bytes(n)); }

// OP over the rows (axis 0) or the columns (axis 1) of the uploaded A into out[nrow or ncol]
static int margin(const Csr &A, const Values &V, int nrow, int ncol, int axis, int op, int na_rm, double *out,
                  int32_t *skipped)
{
    DevBuf ws;
    if (reduce_ws(ws, A.nnz)) return 1;
    if (axis == 0)
        return mxd_segment_reduce(op, A.x, V.dtype, nullptr, A.nnz, A.p, nrow, na_rm, out, skipped, ws, nullptr);
    Dev<int32_t> perm, colptr;
    DevBuf tws;
    if (perm.alloc(A.nnz) || colptr.alloc((int64_t)ncol + 1)) return 1;
    if (tws.alloc_bytes(mxd_csr_transpose_workspace_bytes(A.nnz))) return 1;
    if (mxd_csr_column_order(nrow, ncol, A.p, A.j, A.nnz, perm, colptr, tws, nullptr)) return 1;
    if (mxd_segment_reduce(op, A.x, V.dtype, perm, A.nnz, colptr, ncol, na_rm, out, skipped, ws, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));          // perm, colptr and the workspaces are freed on the way out
    return 0;
}

// OP over all n f64 / value_dtype entries of `values` as one segment, read back into *res
static int whole(int op, const void *values, int value_dtype, int64_t n, double *res)
{
    const int32_t bounds[2] = {0, (int32_t)n};
    Dev<int32_t> segptr;
    Dev<double> dres;
    DevBuf ws;
    if (segptr.upload(bounds, 2) || dres.alloc(1) || reduce_ws(ws, n)) return 1;
    if (mxd_segment_reduce(op, values, value_dtype, nullptr, n, segptr, 1, 0, dres, nullptr, ws, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    return dres.download(res, 1);
}

static int check_csr(const char *what, int nrow, int ncol, const int32_t *indptr, const int32_t *indices,
                     const void *values, const Values &V)
{
    MX_REQUIRE(nrow >= 0 && ncol >= 0 && indptr, "%s: bad dimensions or null indptr", what);
    const int64_t nnz = indptr[nrow];
    MX_REQUIRE(nnz >= 0 && (nnz == 0 || (indices && (!V || values))), "%s: null pointer", what);
    return 0;
}

}  // namespace

extern "C" int mx_csr_margin_reduce(int nrow, int ncol, const int32_t *indptr, const int32_t *indices,
                                    const void *values, int value_dtype, int axis, int op, int na_rm, int mean,
                                    double *out)
{
    if (admit_values("mx_csr_margin_reduce", value_dtype)) return 1;
    const Values V(value_dtype);
    if (check_csr("mx_csr_margin_reduce", nrow, ncol, indptr, indices, values, V)) return 1;
    MX_REQUIRE(axis == 0 || axis == 1, "mx_csr_margin_reduce: axis must be 0 (rows) or 1 (columns), got %d", axis);
    MX_REQUIRE(op >= MX_RED_SUM && op <= MX_RED_ABS_MAX, "mx_csr_margin_reduce: unknown operation %d", op);
    const int64_t n_out = axis == 0 ? nrow : ncol;
    if (n_out == 0) return 0;
    MX_REQUIRE(out, "mx_csr_margin_reduce: null output");
    Csr A;
    if (A.upload(indptr, indices, values, nrow, V.bytes)) return 1;
    Dev<double> dout;
    Dev<int32_t> dskip;
    if (dout.alloc(n_out) || (na_rm && dskip.alloc(n_out))) return 1;
    int32_t *skipped = na_rm ? (int32_t *)dskip : nullptr;
    if (margin(A, V, nrow, ncol, axis, op, na_rm, dout, skipped)) return 1;
    if (mean && reduce_mean_divide(dout, skipped, n_out, axis == 0 ? (double)ncol : (double)nrow, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    return dout.download(out, n_out);
}

extern "C" int mx_csr_norm(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                           int value_dtype, int type, double *out)
{
    if (admit_values("mx_csr_norm", value_dtype)) return 1;
    const Values V(value_dtype);
    if (check_csr("mx_csr_norm", nrow, ncol, indptr, indices, values, V)) return 1;
    MX_REQUIRE(type == 'O' || type == 'I' || type == 'F' || type == 'M',
               "mx_csr_norm: type must be one of 'O', 'I', 'F', 'M'");
    MX_REQUIRE(out, "mx_csr_norm: null output");
    *out = 0.0;
    if (nrow == 0 || ncol == 0 || indptr[nrow] == 0) return 0;
    Csr A;
    if (A.upload(indptr, indices, values, nrow, V.bytes)) return 1;
    if (type == 'F') {
        double sq = 0.0;
        if (whole(MX_RED_SQ_SUM, A.x, V.dtype, A.nnz, &sq)) return 1;
        *out = std::sqrt(sq);
        return 0;
    }
    if (type == 'M') return whole(MX_RED_ABS_MAX, A.x, V.dtype, A.nnz, out);
    const int axis = type == 'I' ? 0 : 1;
    const int64_t n = axis == 0 ? nrow : ncol;
    Dev<double> sums;
    if (sums.alloc(n) || margin(A, V, nrow, ncol, axis, MX_RED_ABS_SUM, 0, sums, nullptr)) return 1;
    return whole(MX_RED_ABS_MAX, (const double *)sums, MX_F64, n, out);
}

extern "C" int mx_csr_diag(int nrow, int ncol, const int32_t *indptr, const int32_t *indices, const void *values,
                           int value_dtype, void *out)
{
    if (admit_values("mx_csr_diag", value_dtype)) return 1;
    const Values V(value_dtype);
    if (check_csr("mx_csr_diag", nrow, ncol, indptr, indices, values, V)) return 1;
    const int64_t d = nrow < ncol ? nrow : ncol;
    if (d == 0) return 0;
    MX_REQUIRE(out, "mx_csr_diag: null output");
    Csr A;
    if (A.upload(indptr, indices, values, nrow, V.bytes)) return 1;
    Dev<int32_t> flag_ws;
    int sorted = 0;
    if (flag_ws.alloc(4) || mxd_csr_rows_sorted(nrow, A.p, A.j, flag_ws, &sorted, nullptr)) return 1;
    const size_t out_bytes = value_dtype == MX_F64 ? 8 : 4;
    DevBuf dout;
    if (dout.alloc(d, out_bytes)) return 1;
    if (mxd_csr_diag(nrow, ncol, A.p, A.j, A.x, V.dtype, A.nnz, sorted, dout, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    return dout.download(out, d, out_bytes);
}

// api_bind.hip — export level (host pointers) of what rbind / cbind add to the batched row concat of api.hip: the COO
// concat, a sparse vector as a column of a CSR, and a dense vector as a sparse vector, over the kernels of bind.hip and
// compact.hip.  Arguments are checked before any device call.
#include "mx_export.h"

#include <algorithm>

using namespace mx;

extern "C" {

// rbind2_coo / rbind2_coo_vec (R/rbind.R:405-520): triplets one after the other, through mxd_coo_rbind_append
int mx_rbind_coo_begin(const mx_rbind_input *objs, int n_inputs, const int32_t *row_offsets, int out_kind,
                       mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && n_inputs >= 0 && out_kind >= 0 && out_kind <= 2, "mx_rbind_coo_begin: bad arguments");
    *res_out = nullptr;
    int64_t nrows = 0, nnz = 0;
    for (int k = 0; k < n_inputs; k++) {
        MX_REQUIRE(objs[k].kind >= 0 && objs[k].kind <= 6, "Invalid vector type in argument %d.", k);
        MX_REQUIRE(objs[k].nnz >= 0 && (objs[k].kind >= 3 || objs[k].nrows >= 0),
                   "mx_rbind_coo_begin: negative size in argument %d", k);
        MX_REQUIRE(!row_offsets || row_offsets[k] >= 0, "mx_rbind_coo_begin: negative row offset in argument %d", k);
        nrows += objs[k].kind <= 2 ? objs[k].nrows : 1;
        nnz += objs[k].nnz;
    }
    MX_REQUIRE(nrows <= INT_MAX - 1 && nnz <= INT_MAX, "rbind result exceeds R's int32 index range");
    const size_t vb = out_kind == 0 ? 8 : out_kind == 1 ? 4 : 0;
    return begin_result(res_out, info, out_kind == 0 ? MX_F64 : out_kind == 1 ? MX_LGL : MX_NONE, [&](mx_result &res) {
        if (res.alloc_indptr(nnz)) return 1;                      // a COO carries its row ids there
        if (res.alloc_entries(nnz, vb)) return 1;
        int row = 0;
        int64_t pos = 0;
        for (int k = 0; k < n_inputs; k++) {
            const mx_rbind_input &o = objs[k];
            const bool vec = o.kind >= 3;
            const size_t ivb = (o.kind == 0 || o.kind == 3) ? 8 : (o.kind == 2 || o.kind == 6) ? 0 : 4;
            Dev<int32_t> i, j;                            // i stays null for a vector, x without values
            DevBuf x;
            if (!vec && i.upload(o.indptr, o.nnz)) return 1;
            if (j.upload(o.indices, o.nnz)) return 1;
            if (ivb && x.upload(o.values, o.nnz, ivb)) return 1;
            if (mxd_coo_rbind_append(o.kind, i, j, x, o.nnz, out_kind, row_offsets ? row_offsets[k] : row, pos,
                                     res.indptr, res.indices, res.values, nullptr)) return 1;
            MX_HIP(hipStreamSynchronize(nullptr));        // the operand's buffers are freed at the end of the turn
            row += vec ? 1 : o.nrows;
            pos += o.nnz;
        }
        return 0;
    });
}

int mx_cbind_csr_svec_begin(const int32_t *Xp, int nX, int ncolX, const int32_t *Xj, const void *Xx, int x_kind,
                            const int32_t *vi, const void *vx, int v_kind, int nv, int length, int first, int out_kind,
                            mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_cbind_csr_svec_begin";
    MX_REQUIRE(res_out && info && nX >= 0 && ncolX >= 0 && nv >= 0 && length >= 0, "%s: bad arguments", what);
    MX_REQUIRE(x_kind >= 0 && x_kind <= 2 && v_kind >= 3 && v_kind <= 6 && out_kind >= 0 && out_kind <= 2,
               "%s: bad kind", what);
    MX_REQUIRE(nv == 0 || vi, "%s: null indices", what);
    for (int k = 0; k < nv; k++)
        MX_REQUIRE(vi[k] >= 1 && vi[k] <= length, "%s: index %d of the vector outside 1..length", what, k);
    {   // a row can gain one entry only: the kernel's offsets count each position once
        std::vector<int32_t> sorted(vi, vi + nv);
        std::sort(sorted.begin(), sorted.end());
        MX_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(),
                   "%s: the vector stores a position twice", what);
    }
    *res_out = nullptr;
    const size_t xb = x_kind == 0 ? 8 : x_kind == 1 ? 4 : 0, ivb = v_kind == 3 ? 8 : v_kind == 6 ? 0 : 4;
    const size_t vb = out_kind == 0 ? 8 : out_kind == 1 ? 4 : 0;
    return begin_result(res_out, info, out_kind == 0 ? MX_F64 : out_kind == 1 ? MX_LGL : MX_NONE, [&](mx_result &res) {
        Csr X;
        if (X.upload(Xp, Xj, Xx, nX, xb)) return 1;
        Dev<int32_t> di;
        DevBuf dx, ws;
        if (di.upload(vi, nv)) return 1;
        if (ivb && dx.upload(vx, nv, ivb)) return 1;
        if (nv > 1) {                                     // the kernel searches the indices: sort_vector_indices first
            if (ws.alloc_bytes(mxd_sort_vector_indices_workspace_bytes(nv))) return 1;
            int was_sorted = 1;
            if (mxd_sort_vector_indices(di, dx, nv, v_kind == 3 ? MX_F64 : v_kind == 6 ? MX_NONE : MX_I32, ws,
                                        &was_sorted, nullptr)) return 1;
        }
        const int nrows = nX > length ? nX : length;
        const int64_t nnz = X.nnz + nv;
        MX_REQUIRE(nnz <= INT_MAX && ncolX < INT_MAX, "cbind result exceeds R's int32 index range");
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        if (res.alloc_entries(nnz, vb)) return 1;
        return mxd_csr_cbind_svec(nX, ncolX, X.p, X.j, X.x, x_kind, di, dx, v_kind, nv, length, first, out_kind,
                                  res.indptr, res.indices, res.values, nullptr);
    });
}

int mx_dense_to_svec_begin(const void *dense, int64_t n, int dtype, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && n >= 0 && n < INT_MAX && (dense || n == 0), "mx_dense_to_svec_begin: bad arguments");
    MX_REQUIRE(dtype == MX_F64 || dtype == MX_I32 || dtype == MX_LGL, "mx_dense_to_svec_begin: unsupported dtype %d",
               dtype);
    *res_out = nullptr;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        DevBuf d, ws;
        if (d.upload(dense, n, dtype_bytes(dtype))) return 1;
        if (ws.alloc_bytes(mxd_compact_workspace_bytes(n))) return 1;
        int64_t kept = 0;
        if (mxd_dense_to_svec_count(n, d, dtype, ws, &kept, nullptr)) return 1;
        if (res.alloc_indptr(0)) return 1;
        if (res.alloc_entries(kept, sizeof(double))) return 1;
        return mxd_dense_to_svec_fill(n, d, dtype, ws, res.indices, res.values, nullptr);
    });
}

}  // extern "C"

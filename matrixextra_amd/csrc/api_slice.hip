// api_slice.hip — export level of what finishes `[` (host pointers): NA injection into a COO, the CSR scalar lookup,
// the recycled indices of a sparseVector selector and the drop to a dense vector, over the kernels of coona.hip.
// Arguments are checked before any device call.
#include "mx_export.h"

using namespace mx;

extern "C" {

// inject_NAs_inplace_coo_{numeric,logical}  src/slice_coo.cpp:902-946
int mx_inject_NAs_inplace_coo_begin(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype,
                                    int64_t nnz, const int32_t *rows_na, int64_t n_rows_na, const int32_t *cols_na,
                                    int64_t n_cols_na, int nrows, int ncols, mx_result **res_out,
                                    mx_result_info *info)
{
    const char *what = "mx_inject_NAs_inplace_coo_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0 && n_rows_na >= 0 && n_cols_na >= 0, "%s: negative size", what);
    MX_REQUIRE(nnz <= INT_MAX, "%s: %lld entries exceed R's int32 index range", what, (long long)nnz);
    if (admit_values(what, value_dtype, kNumeric | kLogical)) return 1;
    MX_REQUIRE((nnz == 0 || (ii && jj && xx)) && (n_rows_na == 0 || rows_na) && (n_cols_na == 0 || cols_na),
               "%s: null pointer", what);
    *res_out = nullptr;
    const Values vals(value_dtype);
    return begin_result(res_out, info, value_dtype, [&](mx_result &res) {
        if (n_rows_na == 0 && n_cols_na == 0) return 0;             // three empty vectors: R leaves the matrix alone
        Dev<int32_t> r, c, rna, cna, maps;
        DevBuf x, ws;
        if (r.upload(ii, nnz) || c.upload(jj, nnz) || x.upload(xx, nnz, vals.bytes)) return 1;
        if (rna.upload(rows_na, n_rows_na) || cna.upload(cols_na, n_cols_na)) return 1;
        if (ws.alloc_bytes(mxd_compact_workspace_bytes(nnz))) return 1;
        if (maps.alloc(4 + (int64_t)nrows + ncols + (nrows > ncols ? nrows : ncols))) return 1;
        int64_t nnz_out = 0;
        if (mxd_coo_inject_na_count(nrows, ncols, r, c, nnz, rna, n_rows_na, cna, n_cols_na, ws, maps, &nnz_out,
                                    nullptr))
            return 1;
        if (res.alloc_indptr(nnz_out)) return 1;                      // row ids travel in the indptr vector
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        if (nnz_out == 0) return 0;
        return mxd_coo_inject_na_fill(nrows, ncols, r, c, x, value_dtype, nnz, rna, n_rows_na, cna, n_cols_na, ws,
                                      maps, res.indptr, res.indices, res.values, nullptr);
    });
}

// extract_single_val_csr_{numeric,logical,binary}  src/slice.cpp:737-785
int mx_extract_single_val_csr(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                              int value_dtype, int row, int col, int *found, void *value_out)
{
    const char *what = "mx_extract_single_val_csr";
    MX_REQUIRE(found && indptr && nrows >= 0, "%s: bad arguments", what);
    if (admit_values(what, value_dtype)) return 1;
    MX_REQUIRE(row >= 0 && row < nrows, "%s: row index %d outside [0, %d)", what, row, nrows);
    *found = 0;
    const int s = indptr[row], e = indptr[row + 1];                   // the caller's own vector: only the row goes up
    MX_REQUIRE(s >= 0 && e >= s, "%s: bad index pointer", what);
    if (e == s) return 0;
    MX_REQUIRE(indices && (value_dtype == MX_NONE || values), "%s: null pointer", what);
    const size_t vb = dtype_bytes(value_dtype);
    const int32_t p[2] = {0, e - s};
    Dev<int32_t> dp, dj;
    DevBuf x, ws;
    if (dp.upload(p, 2) || dj.upload(indices + s, (int64_t)e - s)) return 1;
    if (vb && x.upload((const char *)values + (size_t)s * vb, (int64_t)e - s, vb)) return 1;
    if (ws.alloc_bytes(16)) return 1;
    int64_t k = -1;
    if (mxd_csr_single(1, dp, dj, x, value_dtype, (int64_t)e - s, 0, col, ws, &k, value_out, nullptr)) return 1;
    *found = k >= 0;
    return 0;
}

// repeat_indices_n_times  src/slice.cpp:636-659; out holds n_indices * (desired_length / ix_length) + n_remainder
int mx_repeat_indices_n_times(const int32_t *indices, int64_t n_indices, const int32_t *remainder,
                              int64_t n_remainder, int ix_length, int desired_length, int32_t *out)
{
    const char *what = "mx_repeat_indices_n_times";
    MX_REQUIRE(n_indices >= 0 && n_remainder >= 0 && desired_length >= 0, "%s: negative size", what);
    MX_REQUIRE(ix_length > 0, "%s: the indexing vector's length %d is not positive", what, ix_length);
    const int64_t total = n_indices * (desired_length / ix_length) + n_remainder;
    MX_REQUIRE(n_indices <= INT_MAX && n_remainder <= INT_MAX && total <= (int64_t)INT_MAX,
               "%s: %lld indices exceed R's int32 index range", what, (long long)total);
    if (total == 0) return 0;
    MX_REQUIRE(out && (n_indices == 0 || indices) && (n_remainder == 0 || remainder), "%s: null pointer", what);
    Dev<int32_t> ix, rem, o;
    if (ix.upload(indices, n_indices) || rem.upload(remainder, n_remainder) || o.alloc(total)) return 1;
    if (mxd_repeat_indices(ix, n_indices, rem, n_remainder, ix_length, desired_length, o, nullptr)) return 1;
    return o.download(out, total);
}

// as.vector() of a one-row / one-column result (drop_slice, R/slice.R:210-236): out[len], f64 or int32 R logicals
int mx_entries_to_dense_vector(const int32_t *pos, const void *values, int value_dtype, int64_t n, void *out,
                               int out_dtype, int64_t len)
{
    const char *what = "mx_entries_to_dense_vector";
    MX_REQUIRE(n >= 0 && len >= 0, "%s: negative size", what);
    if (admit_values(what, value_dtype) || admit_values(what, out_dtype, kNumeric | kLogical)) return 1;
    MX_REQUIRE(value_dtype == MX_NONE || value_dtype == out_dtype, "%s: values of dtype %d into a vector of dtype %d",
               what, value_dtype, out_dtype);
    if (len == 0) return 0;
    MX_REQUIRE(out && (n == 0 || (pos && (value_dtype == MX_NONE || values))), "%s: null pointer", what);
    for (int64_t k = 0; k < n; k++)
        MX_REQUIRE(pos[k] >= 0 && pos[k] < len, "%s: position %d outside [0, %lld)", what, pos[k], (long long)len);
    Dev<int32_t> dpos;
    DevBuf x, o;
    if (dpos.upload(pos, n) || o.alloc(len, dtype_bytes(out_dtype))) return 1;
    if (value_dtype != MX_NONE && x.upload(values, n, dtype_bytes(value_dtype))) return 1;
    if (mxd_entries_to_dense_vector(dpos, x, value_dtype, n, o, out_dtype, len, nullptr)) return 1;
    return o.download(out, len, dtype_bytes(out_dtype));
}

}  // extern "C"

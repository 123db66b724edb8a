// api.hip — export-level C-ABI (host pointers) of libmxgpu: one entry point per
// Rcpp export of the reference's hot path, marshalling host vectors to the
// device, running the HIP kernels and bringing the result back.  There is no
// CPU fallback: without a usable GPU every call fails with an error.
#include "mx_dispatch.h"
#include "mx_export.h"

#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>

namespace mx {

static thread_local char g_err[512] = "";

int set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

static thread_local const char *g_row_what = "none";
static thread_local int g_row_group = 0;

void note_row_launch(const char *what, int G)
{
    g_row_what = what;
    g_row_group = G;
}

// MXGPU_TRACE=1: wall-clock phases of an export-level call on stderr
struct Trace {
    bool on;
    const char *what;
    std::chrono::steady_clock::time_point t0, last;
    explicit Trace(const char *w) : on(getenv("MXGPU_TRACE") != nullptr), what(w)
    {
        if (on) t0 = last = std::chrono::steady_clock::now();
    }
    ~Trace() { mark("release"); }                   // declared before the device buffers: runs after their hipFree
    void mark(const char *phase)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mxgpu] %s: %-10s %8.3f ms (total %8.3f)\n", what, phase,
                std::chrono::duration<double, std::milli>(now - last).count(),
                std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// C(m x n) = A(CSR, m rows) * B(row-major rows of length ldb); host in, host out
template <typename real_t>
static int spmm_host(int m, int n, int K_rows, const int32_t *indptr, const int32_t *indices, const double *values,
                     const real_t *B_host, int ldb, real_t *C_host, int ldc, bool colmajor)
{
    MX_REQUIRE(m >= 0 && n >= 0 && K_rows >= 0, "negative dimension");
    const int64_t c_elems = (int64_t)m * n;
    if (c_elems == 0) return 0;
    // reference early-out (matmul.cpp:128-129,160-161): result stays the zero-initialised matrix
    if (indptr[0] == indptr[m]) { std::fill_n(C_host, c_elems, real_t(0)); return 0; }
    Trace tr("spmm export");
    Csr A;
    if (A.upload(indptr, indices, values, m, sizeof(double))) return 1;
    tr.mark("H2D csr");
    Dev<real_t> B, C;
    if (B.upload(B_host, (int64_t)K_rows * ldb)) return 1;
    tr.mark("H2D dense");
    if (C.alloc(c_elems)) return 1;
    tr.mark("alloc C");
    const int dt = sizeof(real_t) == 8 ? MX_F64 : MX_F32;
    // kernel choice: AUTO unless the MXGPU_SPMM_ALGO / MXGPU_SPMM_PANELS tuning knobs say otherwise
    int algo = MX_SPMM_AUTO, npanels = 0;
    if (const char *e = getenv("MXGPU_SPMM_ALGO")) algo = atoi(e);
    if (const char *e = getenv("MXGPU_SPMM_PANELS")) npanels = atoi(e);
    int sorted = 0;
    if (algo == MX_SPMM_SLAB) {
        // column panels need rows sorted by column id: one pass over the indices on the device
        Dev<int32_t> flag;
        if (flag.alloc(4)) return 1;
        if (mxd_csr_rows_sorted(m, A.p, A.j, flag, &sorted, nullptr)) return 1;
    }
    if (mxd_spmm_csr_dense_ex(m, n, K_rows, A.p, A.j, A.x, B, ldb, C, ldc,
                              dt, colmajor ? 1 : 0, algo, sorted, npanels, 0, nullptr)) return 1;
    if (tr.on) { MX_HIP(hipDeviceSynchronize()); tr.mark("kernels"); }
    const int rc = C.download(C_host, c_elems);
    tr.mark("D2H C");
    return rc;
}

template <typename vec_t, typename out_t>
static int spmv_host(int m, const int32_t *indptr, const int32_t *indices, const double *values, const vec_t *y,
                     int len_y, int v_dtype, out_t *out)
{
    MX_REQUIRE(m >= 0 && len_y >= 0, "negative dimension");
    if (m == 0) return 0;
    Csr A;
    if (A.upload(indptr, indices, values, m, sizeof(double))) return 1;
    Dev<vec_t> v;
    Dev<out_t> o;
    if (v.upload(y, len_y)) return 1;
    if (o.alloc(m)) return 1;
    if (spmv_launch(m, A.nnz, A.p, A.j, A.x, v, v_dtype, o, nullptr)) return 1;
    return o.download(out, m);
}

}  // namespace mx

using namespace mx;

// The values-only products end alike: one value of value_bytes for each of the sparse operand's n entries, which
// `launch` fills from the operands already on the device, and which goes back to the caller.
template <typename Launch>
static int values_only(int64_t n, size_t value_bytes, void *values_out, Launch &&launch)
{
    DevBuf o;
    if (o.alloc(n, value_bytes)) return 1;
    if (launch(o)) return 1;
    return o.download(values_out, n, value_bytes);
}

extern "C" {

int mxd_last_row_launch(const char **what, int *G)
{
    if (what) *what = mx::g_row_what;
    if (G) *G = mx::g_row_group;
    return 0;
}

const char *mx_last_error(void) { return mx::g_err; }
int mx_abi_version(void) { return MXGPU_ABI_VERSION; }

int mx_device_count(int *count)
{
    MX_REQUIRE(count, "mx_device_count: null pointer");
    *count = 0;
    MX_HIP(hipGetDeviceCount(count));
    return 0;
}
int mx_set_device(int device) { MX_HIP(hipSetDevice(device)); return 0; }
int mx_device_name(char *buf, size_t buflen)
{
    int dev = 0;
    MX_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    MX_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
}
int mx_dev_malloc(void **dptr, size_t bytes) { MX_HIP(hipMalloc(dptr, bytes ? bytes : 16)); return 0; }
int mx_dev_free(void *dptr) { MX_HIP(hipFree(dptr)); return 0; }
int mx_dev_memset(void *dptr, int value, size_t bytes, void *stream)
{
    MX_HIP(hipMemsetAsync(dptr, value, bytes, as_stream(stream)));
    return 0;
}
int mx_memcpy_h2d(void *dptr, const void *hptr, size_t bytes, void *stream)
{
    MX_HIP(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, as_stream(stream)));
    return 0;
}
int mx_memcpy_d2h(void *hptr, const void *dptr, size_t bytes, void *stream)
{
    MX_HIP(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    return 0;
}
int mx_stream_sync(void *stream) { MX_HIP(hipStreamSynchronize(as_stream(stream))); return 0; }
int mx_host_register(void *hptr, size_t bytes) { MX_HIP(hipHostRegister(hptr, bytes, hipHostRegisterDefault)); return 0; }
int mx_host_unregister(void *hptr) { MX_HIP(hipHostUnregister(hptr)); return 0; }

// ---- SpMM exports ------------------------------------------------------------------------------
int mx_tcrossprod_csr_dense_numeric(const int32_t *X_indptr, const int32_t *X_indices, const double *X_values,
                                    int nrows_X, const double *Y_colmajor, int nrow_Y, int ncol_Y, int nthreads,
                                    double *out_colmajor)
{
    (void)nthreads;
    // gemm_csr_drm_as_dcm(m = nrow X, n = nrow Y, B = Y, ldb = nrow Y, C, ldc = m)   matmul.cpp:326-332
    return spmm_host<double>(nrows_X, nrow_Y, ncol_Y, X_indptr, X_indices, X_values, Y_colmajor, nrow_Y,
                             out_colmajor, nrows_X, true);
}
int mx_tcrossprod_csr_dense_float32(const int32_t *X_indptr, const int32_t *X_indices, const double *X_values,
                                    int nrows_X, const float *Y_colmajor, int nrow_Y, int ncol_Y, int nthreads,
                                    float *out_colmajor)
{
    (void)nthreads;
    return spmm_host<float>(nrows_X, nrow_Y, ncol_Y, X_indptr, X_indices, X_values, Y_colmajor, nrow_Y,
                            out_colmajor, nrows_X, true);
}
int mx_matmul_dense_csc_numeric(const double *X_colmajor, int nrows_X, int ncols_X, const int32_t *Y_indptr,
                                const int32_t *Y_indices, const double *Y_values, int ncols_Y, int nthreads,
                                double *out_colmajor)
{
    (void)nthreads;
    // gemm_csr_drm_as_drm(m = ncol Y, n = nrow X, CSC-as-CSR, B = X, ldb = nrow X, C, ldc = nrow X)  matmul.cpp:201-208
    return spmm_host<double>(ncols_Y, nrows_X, ncols_X, Y_indptr, Y_indices, Y_values, X_colmajor, nrows_X,
                             out_colmajor, nrows_X, false);
}
int mx_matmul_dense_csc_float32(const float *X_colmajor, int nrows_X, int ncols_X, const int32_t *Y_indptr,
                                const int32_t *Y_indices, const double *Y_values, int ncols_Y, int nthreads,
                                float *out_colmajor)
{
    (void)nthreads;
    return spmm_host<float>(ncols_Y, nrows_X, ncols_X, Y_indptr, Y_indices, Y_values, X_colmajor, nrows_X,
                            out_colmajor, nrows_X, false);
}
int mx_tcrossprod_dense_csr_numeric(const double *X_colmajor, int nrows_X, int ncols_X, const int32_t *Y_indptr,
                                    const int32_t *Y_indices, const double *Y_values, int nrows_Y, int nthreads,
                                    int ncols_Y, double *out_colmajor)
{
    (void)nthreads; (void)ncols_Y;
    // gemm_csr_drm_as_drm(m = nrow Y, n = nrow X, Y, B = X, ldb = nrow X, C, ldc = nrow X)  matmul.cpp:263-270
    return spmm_host<double>(nrows_Y, nrows_X, ncols_X, Y_indptr, Y_indices, Y_values, X_colmajor, nrows_X,
                             out_colmajor, nrows_X, false);
}
int mx_tcrossprod_dense_csr_float32(const float *X_colmajor, int nrows_X, int ncols_X, const int32_t *Y_indptr,
                                    const int32_t *Y_indices, const double *Y_values, int nrows_Y, int nthreads,
                                    int ncols_Y, float *out_colmajor)
{
    (void)nthreads; (void)ncols_Y;
    return spmm_host<float>(nrows_Y, nrows_X, ncols_X, Y_indptr, Y_indices, Y_values, X_colmajor, nrows_X,
                            out_colmajor, nrows_X, false);
}

// ---- SpMV exports ------------------------------------------------------------------------------
int mx_matmul_csr_dvec_numeric(const int32_t *p, const int32_t *j, const double *x, int nrows_X, const double *y,
                               int len_y, int nthreads, double *out)
{
    (void)nthreads;
    return spmv_host<double, double>(nrows_X, p, j, x, y, len_y, MX_F64, out);
}
int mx_matmul_csr_dvec_integer(const int32_t *p, const int32_t *j, const double *x, int nrows_X, const int32_t *y,
                               int len_y, int nthreads, double *out)
{
    (void)nthreads;
    return spmv_host<int32_t, double>(nrows_X, p, j, x, y, len_y, MX_I32, out);
}
int mx_matmul_csr_dvec_logical(const int32_t *p, const int32_t *j, const double *x, int nrows_X, const int32_t *y,
                               int len_y, int nthreads, double *out)
{
    (void)nthreads;
    return spmv_host<int32_t, double>(nrows_X, p, j, x, y, len_y, MX_LGL, out);
}
int mx_matmul_csr_dvec_float32(const int32_t *p, const int32_t *j, const double *x, int nrows_X, const float *y,
                               int len_y, int nthreads, float *out)
{
    (void)nthreads;
    return spmv_host<float, float>(nrows_X, p, j, x, y, len_y, MX_F32, out);
}

// ---- CSR (+) CSR -------------------------------------------------------------------------------
int mx_csr_elemwise_begin(int op, int nrows, const int32_t *indptr1, const int32_t *indptr2,
                          const int32_t *indices1, const int32_t *indices2, const void *values1,
                          const void *values2, int64_t nnz1, int64_t nnz2, mx_result **res_out,
                          mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_csr_elemwise_begin: null output pointer");
    MX_REQUIRE(op >= MX_OP_ADD && op <= MX_OP_AND, "mx_csr_elemwise_begin: unknown op %d", op);
    MX_REQUIRE(nrows >= 0 && nnz1 >= 0 && nnz2 >= 0, "mx_csr_elemwise_begin: negative size");
    *res_out = nullptr;
    const bool lgl = op == MX_OP_OR || op == MX_OP_XOR || op == MX_OP_AND;
    const size_t vb = lgl ? 4 : 8;
    return begin_result(res_out, info, lgl ? MX_LGL : MX_F64, [&](mx_result &res) {
        // identical-structure fast paths: pointer identity, as operators.cpp:104-108 / :343-346 test it
        if (nnz1 == nnz2 && indptr1 == indptr2 && indices1 == indices2) {
            if (op == MX_OP_SUB && values1 == values2) {
                // operators.cpp:348-355: IntegerVector(indptr.size()) zeros, empty indices / values
                if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
                return res.indptr.zero((int64_t)nrows + 1);
            }
            res.alias(1, (int64_t)nrows + 1, nnz1);
            DevBuf a, b;
            if (a.upload(values1, nnz1, vb)) return 1;
            if (b.upload(values2, nnz2, vb)) return 1;
            if (res.alloc_values(nnz1, vb)) return 1;
            return mxd_values_elemwise(op, nnz1, a, b, res.values, nullptr);
        }
        Csr A, B;
        if (A.upload(indptr1, indices1, values1, nrows, vb)) return 1;
        if (B.upload(indptr2, indices2, values2, nrows, vb)) return 1;
        DevBuf ws;
        if (ws.alloc_bytes(mxd_merge_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_merge_count(op, nrows, A.p, A.j, A.nnz, B.p, B.j, B.nnz, res.indptr, ws, &nnz_out, nullptr))
            return 1;
        if (res.alloc_entries(nnz_out, vb)) return 1;
        return mxd_csr_merge_fill(op, nrows, A.p, A.j, A.x, A.nnz, B.p, B.j, B.x, B.nnz, res.indptr, res.indices,
                                  res.values, nullptr);
    });
}

// ---- row gather --------------------------------------------------------------------------------
int mx_copy_csr_rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                           int value_dtype, int64_t n_values, const int32_t *rows_take, int64_t n_take,
                           mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_copy_csr_rows_begin: null output pointer");
    MX_REQUIRE(nrows >= 0 && n_take >= 0 && n_take <= INT_MAX, "mx_copy_csr_rows_begin: bad size");
    if (admit_values("mx_copy_csr_rows_begin", value_dtype)) return 1;
    *res_out = nullptr;
    const Values vals(value_dtype, n_values);                         // slice.cpp:246,257
    return begin_result(res_out, info, value_dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
        Dev<int32_t> rows;
        DevBuf ws;
        if (rows.upload(rows_take, n_take)) return 1;
        if (ws.alloc_bytes(mxd_gather_workspace_bytes((int)n_take))) return 1;
        if (res.alloc_indptr(n_take + 1)) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_gather_count((int)n_take, A.p, rows, res.indptr, ws, &nnz_out, nullptr)) return 1;
        if (nnz_out == 0) {          // slice.cpp:236-240: three EMPTY vectors (even the indptr)
            res.set_sizes(0, 0, 0);
            return 0;
        }
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        if (!vals) res.info.values_dtype = MX_NONE;
        return mxd_csr_gather_fill((int)n_take, A.p, A.j, A.x, rows, res.indptr, res.indices, res.values, vals.dtype,
                                   nnz_out, nullptr);
    });
}

// ---- column-filtering slices (§8f rank 2) ----------------------------------------------------------------
int mx_copy_csr_rows_col_seq_begin(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                                   int value_dtype, int64_t n_values, const int32_t *rows_take, int64_t n_take,
                                   const int32_t *cols_take, int64_t n_cols_take, int index1,
                                   mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_copy_csr_rows_col_seq_begin: null output pointer");
    MX_REQUIRE(nrows >= 0 && n_take >= 0 && n_take <= INT_MAX && n_cols_take > 0, "mx_copy_csr_rows_col_seq_begin: bad size");
    if (admit_values("mx_copy_csr_rows_col_seq_begin", value_dtype)) return 1;
    *res_out = nullptr;
    int min_col = cols_take[0], max_col = cols_take[0];                      // slice.cpp:337-338
    for (int64_t c = 1; c < n_cols_take; c++) { if (cols_take[c] < min_col) min_col = cols_take[c]; if (cols_take[c] > max_col) max_col = cols_take[c]; }
    min_col -= index1 ? 1 : 0; max_col -= index1 ? 1 : 0;
    const Values vals(value_dtype, n_values);
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {   // always a NumericVector (slice.cpp:363)
        Csr A;
        if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
        Dev<int32_t> rows;
        DevBuf ws;
        if (rows.upload(rows_take, n_take)) return 1;
        if (ws.alloc_bytes(mxd_gather_workspace_bytes((int)n_take))) return 1;
        if (res.alloc_indptr(n_take + 1)) return 1;                           // full-length indptr even when empty
        const double avg = nrows > 0 ? (double)A.nnz / nrows : 0.0;
        int64_t nnz_out = 0;
        if (mxd_csr_colrange_count((int)n_take, A.p, A.j, rows, min_col, max_col, avg, res.indptr, ws, &nnz_out,
                                   nullptr)) return 1;
        if (res.alloc_entries(nnz_out, vals ? sizeof(double) : 0)) return 1;
        if (nnz_out == 0) return 0;                                           // slice.cpp:355-359
        return mxd_csr_colrange_fill((int)n_take, A.p, A.j, A.x, vals.dtype, rows, min_col, max_col, avg, res.indptr,
                                     res.indices, res.values, nullptr);
    });
}

int mx_copy_csr_arbitrary_begin(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                                int value_dtype, int64_t n_values, const int32_t *rows_take, int64_t n_take,
                                const int32_t *cols_take, int64_t n_cols_take, mx_result **res_out,
                                mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_copy_csr_arbitrary_begin: null output pointer");
    MX_REQUIRE(nrows >= 0 && n_take >= 0 && n_take <= INT_MAX && n_cols_take >= 0 && n_cols_take <= INT_MAX,
               "mx_copy_csr_arbitrary_begin: bad size");
    if (admit_values("mx_copy_csr_arbitrary_begin", value_dtype)) return 1;
    *res_out = nullptr;
    const Values vals(value_dtype, n_values);                                 // `if (values.size())`, slice.cpp:565
    int max_j = -1;
    bool cols_sorted = true;                                                  // slice.cpp:487-493
    for (int64_t c = 0; c < n_cols_take; c++) {
        MX_REQUIRE(cols_take[c] >= 0, "mx_copy_csr_arbitrary_begin: negative column index");
        if (cols_take[c] > max_j) max_j = cols_take[c];
        if (c && cols_take[c] < cols_take[c - 1]) cols_sorted = false;
    }
    const int ncol_map = max_j + 1;
    return begin_result(res_out, info, vals.dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
        Dev<int32_t> rows, cols, start, pos;
        DevBuf ws, mws;
        if (rows.upload(rows_take, n_take)) return 1;
        if (cols.upload(cols_take, n_cols_take)) return 1;
        if (start.alloc((int64_t)ncol_map + 1)) return 1;
        if (pos.alloc(n_cols_take)) return 1;
        if (mws.alloc_bytes(mxd_colmap_workspace_bytes(ncol_map))) return 1;
        if (ws.alloc_bytes(mxd_gather_workspace_bytes((int)n_take))) return 1;
        if (res.alloc_indptr(n_take + 1)) return 1;
        if (mxd_colmap_build(cols, n_cols_take, ncol_map, start, pos, mws, nullptr)) return 1;
        const double avg = nrows > 0 ? (double)A.nnz / nrows : 0.0;
        int64_t nnz_out = 0;
        if (mxd_csr_colmap_count((int)n_take, A.p, A.j, rows, ncol_map, start, avg, res.indptr, ws, &nnz_out,
                                 nullptr)) return 1;
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        if (nnz_out == 0) return 0;
        if (mxd_csr_colmap_fill((int)n_take, A.p, A.j, A.x, vals.dtype, rows, ncol_map, start, pos, avg, res.indptr,
                                res.indices, res.values, nullptr)) return 1;
        if (cols_sorted) return 0;
        Dev<int32_t> tj;                                                      // slice.cpp:540-560
        DevBuf tx;
        if (tj.alloc(nnz_out)) return 1;
        if (vals && tx.alloc(nnz_out, vals.bytes)) return 1;
        return mxd_csr_sort_rows((int)n_take, nnz_out, res.indptr, res.indices, res.values, vals.dtype, tj, tx,
                                 nullptr);
    });
}

int mx_reverse_rows_begin(const int32_t *indptr, int nrows, const int32_t *indices, const void *values,
                          int value_dtype, int64_t n_values, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_reverse_rows_begin: null output pointer");
    MX_REQUIRE(nrows >= 0, "mx_reverse_rows_begin: negative size");
    *res_out = nullptr;
    const Values vals(value_dtype, n_values);                                 // slice.cpp:66
    return begin_result(res_out, info, vals.dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
        Dev<int32_t> rows;
        DevBuf ws;
        if (rows.alloc(nrows)) return 1;
        if (ws.alloc_bytes(mxd_gather_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;                   // always full length (slice.cpp:57)
        if (mxd_reversed_iota(nrows, rows, nullptr)) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_gather_count(nrows, A.p, rows, res.indptr, ws, &nnz_out, nullptr)) return 1;
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        if (nnz_out == 0) return 0;
        return mxd_csr_gather_fill(nrows, A.p, A.j, A.x, rows, res.indptr, res.indices, res.values, vals.dtype,
                                   nnz_out, nullptr);
    });
}

int mx_reverse_columns_inplace(const int32_t *indptr, int nrows, int32_t *indices, void *values, int value_dtype,
                               int64_t n_values, int ncol)
{
    if (nrows <= 0) return 0;
    const Values vals(value_dtype, values ? n_values : 0);
    Csr A;
    if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
    if (A.nnz == 0) return 0;
    if (mxd_csr_reverse_columns(nrows, A.nnz, A.p, A.j, A.x, vals.dtype, ncol, nullptr)) return 1;
    if (A.j.download(indices, A.nnz)) return 1;
    if (vals && A.x.download(values, A.nnz, vals.bytes)) return 1;
    return 0;
}

// ---- CSR x sparse vector, CSR (.) dense (§8f rank 4) ---------------------------------------------------------
int mx_matmul_csr_svec(const int32_t *Xp, const int32_t *Xj, const double *Xx, int nrows, const int32_t *yi, int64_t ny,
                       const void *yv, int kind, int nthreads, double *out)
{
    (void)nthreads;
    MX_REQUIRE(nrows >= 0 && ny >= 0 && ny <= INT_MAX && kind >= 0 && kind <= 4, "mx_matmul_csr_svec: bad arguments");
    if (nrows == 0) return 0;
    if (ny == 0) { std::fill_n(out, nrows, 0.0); return 0; }
    Csr A;
    if (A.upload(Xp, Xj, Xx, nrows, sizeof(double))) return 1;
    Dev<int32_t> di;
    DevBuf dv;
    Dev<double> o;
    if (di.upload(yi, ny)) return 1;
    const size_t vb = kind == 0 ? 8 : kind == 3 ? 0 : 4;
    if (vb && dv.upload(yv, ny, vb)) return 1;
    if (o.alloc(nrows)) return 1;
    if (mxd_spmv_csr_svec(nrows, A.nnz, A.p, A.j, A.x, di, (int)ny, dv, kind, o, nullptr)) return 1;
    return o.download(out, nrows);
}

int mx_multiply_csr_by_dense_elemwise(const int32_t *indptr, const int32_t *indices, const void *values, int nrows,
                                      const void *dense_mat, int64_t ncols, int kind, void *values_out)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && kind >= 0 && kind <= 4, "mx_multiply_csr_by_dense_elemwise: bad arguments");
    if (nrows == 0) return 0;
    const size_t vb = kind == 4 ? 4 : 8, db = kind == 0 ? 8 : 4;
    Csr A;
    if (A.upload(indptr, indices, values, nrows, vb)) return 1;
    if (A.nnz == 0) return 0;
    DevBuf D;
    if (D.upload(dense_mat, nrows * ncols, db)) return 1;
    return values_only(A.nnz, vb, values_out, [&](DevBuf &o) {
        return mxd_csr_by_dense_elemwise(nrows, A.nnz, A.p, A.j, A.x, D, kind, o, nullptr);
    });
}

// ---- CSC (.) dense (svec.hip, cscdense.hip) -------------------------------------------------
// values only (multiply_csc_by_dense_ignore_NAs<>, operators.cpp:1061-1122): the structure stays the caller's
static int csc_by_dense_ignore(const int32_t *indptr, int ncols, const int32_t *indices, const void *values,
                               const void *dense, int nrows, int kind, void *values_out)
{
    MX_REQUIRE(indptr && ncols >= 0 && nrows >= 0 && kind >= 0 && kind <= 4, "csc (.) dense: bad arguments");
    if (ncols == 0) return 0;
    const size_t vb = kind == 4 ? 4 : 8, db = kind == 0 ? 8 : 4;
    Csr A;
    if (A.upload(indptr, indices, values, ncols, vb)) return 1;
    if (A.nnz == 0) return 0;
    MX_REQUIRE(nrows > 0 && dense && values_out, "csc (.) dense: entries in a matrix without rows");
    DevBuf D;
    if (D.upload(dense, (int64_t)nrows * ncols, db)) return 1;
    return values_only(A.nnz, vb, values_out, [&](DevBuf &o) {
        return mxd_csc_by_dense_elemwise(ncols, nrows, A.nnz, A.p, A.j, A.x, D, kind, o, nullptr);
    });
}

// NA-keeping (multiply_csc_by_dense_keep_NAs_template<>, operators.cpp:1207-1386): count -> scan -> read-back, then
// the fill, or the values-only kernel when the structure does not change
static int csc_by_dense_keep(const int32_t *indptr, int ncols, const int32_t *indices, const double *values,
                             const void *dense, int nrows, int kind, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && indptr && ncols >= 0 && nrows >= 0, "csc (.) dense: bad arguments");
    MX_REQUIRE(indptr[0] == 0 && indptr[ncols] >= 0, "csc (.) dense: bad index pointer");
    *res_out = nullptr;
    const size_t db = kind == 0 ? 8 : 4;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, ncols, sizeof(double))) return 1;
        DevBuf D, ws;
        if (D.upload(dense, (int64_t)nrows * ncols, db)) return 1;
        if (ws.alloc_bytes(mxd_csc_dense_na_workspace_bytes(nrows, ncols))) return 1;
        int64_t total = 0, outside = 0;
        if (mxd_csc_dense_na_count(nrows, ncols, A.nnz, A.p, A.j, D, kind, ws, &total, &outside, nullptr)) return 1;
        if (res.alloc_indptr((int64_t)ncols + 1)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        if (outside == 0 && total == A.nnz) {           // no NA cell outside the pattern, no repeated row
            if (res.indptr.copy_from(A.p, (int64_t)ncols + 1)) return 1;
            if (res.indices.copy_from(A.j, total)) return 1;
            return mxd_csc_by_dense_elemwise(ncols, nrows, A.nnz, A.p, A.j, A.x, D, kind, res.values, nullptr);
        }
        return mxd_csc_dense_na_fill(nrows, ncols, A.nnz, A.p, A.j, A.x, D, kind, ws, res.indptr, res.indices,
                                     res.values, nullptr);
    });
}

// multiply_csc_by_dense_ignore_NAs_numeric  src/operators.cpp:1125-1139
int mx_multiply_csc_by_dense_ignore_NAs_numeric(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const double *dense, int nrows,
                                                double *values_out)
{
    return csc_by_dense_ignore(indptr, ncols, indices, values, dense, nrows, 0, values_out);
}
// multiply_csc_by_dense_ignore_NAs_float32  :1140-1155 (float32@Data bit patterns)
int mx_multiply_csc_by_dense_ignore_NAs_float32(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const float *dense, int nrows,
                                                double *values_out)
{
    return csc_by_dense_ignore(indptr, ncols, indices, values, dense, nrows, 1, values_out);
}
// multiply_csc_by_dense_ignore_NAs_integer  :1157-1172
int mx_multiply_csc_by_dense_ignore_NAs_integer(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const int32_t *dense, int nrows,
                                                double *values_out)
{
    return csc_by_dense_ignore(indptr, ncols, indices, values, dense, nrows, 2, values_out);
}
// multiply_csc_by_dense_ignore_NAs_logical  :1174-1189
int mx_multiply_csc_by_dense_ignore_NAs_logical(const int32_t *indptr, int ncols, const int32_t *indices,
                                                const double *values, const int32_t *dense, int nrows,
                                                double *values_out)
{
    return csc_by_dense_ignore(indptr, ncols, indices, values, dense, nrows, 3, values_out);
}
// logicaland_csc_by_dense_ignore_NAs  :1191-1206
int mx_logicaland_csc_by_dense_ignore_NAs(const int32_t *indptr, int ncols, const int32_t *indices,
                                          const int32_t *values, const int32_t *dense, int nrows,
                                          int32_t *values_out)
{
    return csc_by_dense_ignore(indptr, ncols, indices, values, dense, nrows, 4, values_out);
}
// multiply_csc_by_dense_keep_NAs_numeric  :1388-1404
int mx_multiply_csc_by_dense_keep_NAs_numeric(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const double *dense, int nrows,
                                              mx_result **res, mx_result_info *info)
{
    return csc_by_dense_keep(indptr, ncols, indices, values, dense, nrows, 0, res, info);
}
// multiply_csc_by_dense_keep_NAs_integer  :1406-1422
int mx_multiply_csc_by_dense_keep_NAs_integer(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const int32_t *dense, int nrows,
                                              mx_result **res, mx_result_info *info)
{
    return csc_by_dense_keep(indptr, ncols, indices, values, dense, nrows, 2, res, info);
}
// multiply_csc_by_dense_keep_NAs_logical  :1424-1440
int mx_multiply_csc_by_dense_keep_NAs_logical(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const int32_t *dense, int nrows,
                                              mx_result **res, mx_result_info *info)
{
    return csc_by_dense_keep(indptr, ncols, indices, values, dense, nrows, 3, res, info);
}
// multiply_csc_by_dense_keep_NAs_float32  :1442-1458
int mx_multiply_csc_by_dense_keep_NAs_float32(const int32_t *indptr, int ncols, const int32_t *indices,
                                              const double *values, const float *dense, int nrows,
                                              mx_result **res, mx_result_info *info)
{
    return csc_by_dense_keep(indptr, ncols, indices, values, dense, nrows, 1, res, info);
}

// ---- CSR * sparse vector (svecmul.hip) --------------------------------------------------------
// multiply_csr_by_svec_no_NAs (operators.cpp:3426-3498, keep_NAs = 0) and multiply_csr_by_svec_keep_NAs
// (:3500-3697): ii_base1 sorted, xx NULL for an nsparseVector; the rows of X sorted
int mx_multiply_csr_by_svec_begin(const int32_t *indptr, int nrows, const int32_t *indices, const double *values,
                                  const int32_t *ii_base1, const double *xx, int64_t nnz_v, int ncols, int length,
                                  int keep_NAs, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && indptr && nrows >= 0 && ncols >= 0 && nnz_v >= 0,
               "mx_multiply_csr_by_svec_begin: bad arguments");
    MX_REQUIRE(indptr[0] == 0 && indptr[nrows] >= 0, "mx_multiply_csr_by_svec_begin: bad index pointer");
    // :3532-3533 (throw_internal_err), asked of both routes here
    MX_REQUIRE(nrows == 0 || (length > 0 && nnz_v <= length && length <= nrows && nrows % length == 0),
               "mx_multiply_csr_by_svec_begin: the vector's length must divide the number of rows");
    *res_out = nullptr;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        Dev<int32_t> vi;
        Dev<double> vx;                                   // stays null for an nsparseVector
        DevBuf ws;
        if (vi.upload(ii_base1, nnz_v)) return 1;
        if (xx && vx.upload(xx, nnz_v)) return 1;
        if (ws.alloc_bytes(mxd_csr_by_svec_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t total = 0, x_na = 0;
        if (mxd_csr_by_svec_count(nrows, ncols, A.nnz, A.p, A.x, vi, nnz_v, vx, length, keep_NAs, ws, res.indptr,
                                  &total, &x_na, nullptr)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        if (total == 0) return 0;
        return mxd_csr_by_svec_fill(nrows, ncols, A.nnz, A.p, A.j, A.x, vi, nnz_v, vx, length, keep_NAs, ws,
                                    res.indptr, res.indices, res.values, nullptr);
    });
}

// ---- dense matrix * sparse vector, COO * dense matrix (densevec.hip) ---------------------------
// the route of multiply_elemwise_dense_by_svec_template<> (operators.cpp:3720, :3765, :3984, :4235)
int mx_dense_by_svec_route(int nrows, int ncols, int length)
{
    if (nrows < 0 || ncols < 0 || length < 0 || (length == 0 && (int64_t)nrows * ncols != 0)) {
        set_error("mx_dense_by_svec_route: bad arguments");
        return -1;
    }
    if ((int64_t)length == (int64_t)nrows * (int64_t)ncols) return MX_DSV_ROUTE_A;
    if (length == nrows) return MX_DSV_ROUTE_B;
    if (length < nrows && nrows % length == 0) return MX_DSV_ROUTE_C;
    return MX_DSV_ROUTE_D;
}

// what the reference does not check (operators.cpp:3709-3712): the vector against its own length
static int dense_by_svec_check(const char *what, const void *X, int kind, int nrows, int ncols, const int32_t *ii,
                               const double *xx, int64_t nnz_v, int length)
{
    MX_REQUIRE(kind >= 0 && kind <= 3 && nnz_v >= 0 && mx_dense_by_svec_route(nrows, ncols, length) >= 0,
               "%s: bad arguments", what);
    MX_REQUIRE(((int64_t)nrows * ncols == 0 || X) && (nnz_v == 0 || (ii && xx)), "%s: null pointer", what);
    MX_REQUIRE(nnz_v <= (int64_t)length, "%s: the vector stores %lld positions, more than its length %d", what,
               (long long)nnz_v, length);
    for (int64_t k = 0; k < nnz_v; k++)
        MX_REQUIRE(ii[k] >= 1 && ii[k] <= length, "%s: position %d lies outside 1..%d", what, ii[k], length);
    return 0;
}

// multiply_elemwise_dense_by_svec_{numeric,float32,integer,logical}, routes B and C  src/operators.cpp:3765-4233
int mx_multiply_elemwise_dense_by_svec_begin(const void *X_colmajor, int kind, int nrows, int ncols,
                                             const int32_t *ii_base1, const double *xx, int64_t nnz_v, int length,
                                             int keep_NAs, mx_result **res_out, mx_result_info *info)
{
    const char *what = "mx_multiply_elemwise_dense_by_svec_begin";
    MX_REQUIRE(res_out && info, "%s: null output pointer", what);
    *res_out = nullptr;
    if (dense_by_svec_check(what, X_colmajor, kind, nrows, ncols, ii_base1, xx, nnz_v, length)) return 1;
    const int route = mx_dense_by_svec_route(nrows, ncols, length);
    MX_REQUIRE(route == MX_DSV_ROUTE_B || route == MX_DSV_ROUTE_C,
               "%s: a vector of length %d against %d x %d gives a dense result", what, length, nrows, ncols);
    const size_t cell = kind == 0 ? 8 : 4;
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        DevBuf X, ws;
        Dev<int32_t> vi;
        Dev<double> vx;
        if (X.upload(X_colmajor, (int64_t)nrows * ncols, cell)) return 1;
        if (vi.upload(ii_base1, nnz_v)) return 1;
        if (vx.upload(xx, nnz_v)) return 1;
        if (ws.alloc_bytes(mxd_dense_by_svec_workspace_bytes(nrows, length))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t total = 0;
        if (mxd_dense_by_svec_count(nrows, ncols, X, kind, vi, nnz_v, length, keep_NAs, ws, res.indptr, &total,
                                    nullptr)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        if (total == 0) return 0;
        return mxd_dense_by_svec_fill(nrows, ncols, X, kind, vx, length, keep_NAs, ws, res.indptr, res.indices,
                                      res.values, nullptr);
    });
}

// multiply_elemwise_dense_by_svec_{numeric,float32,integer,logical}, routes A and D  :3720-3763, :4235-4300
int mx_multiply_elemwise_dense_by_svec_dense(const void *X_colmajor, int kind, int nrows, int ncols,
                                             const int32_t *ii_base1, const double *xx, int64_t nnz_v, int length,
                                             int keep_NAs, double *out_colmajor)
{
    const char *what = "mx_multiply_elemwise_dense_by_svec_dense";
    if (dense_by_svec_check(what, X_colmajor, kind, nrows, ncols, ii_base1, xx, nnz_v, length)) return 1;
    const int route = mx_dense_by_svec_route(nrows, ncols, length);
    MX_REQUIRE(route == MX_DSV_ROUTE_A || route == MX_DSV_ROUTE_D,
               "%s: a vector of length %d against %d x %d gives a CSR result", what, length, nrows, ncols);
    const int64_t cells = (int64_t)nrows * ncols;
    if (cells == 0) return 0;
    MX_REQUIRE(out_colmajor, "%s: null pointer", what);
    DevBuf X, ws;
    Dev<int32_t> vi;
    Dev<double> vx, out;
    if (X.upload(X_colmajor, cells, kind == 0 ? 8 : 4)) return 1;
    if (vi.upload(ii_base1, nnz_v)) return 1;
    if (vx.upload(xx, nnz_v)) return 1;
    if (ws.alloc_bytes(mxd_dense_by_svec_workspace_bytes(0, length))) return 1;
    if (out.alloc(cells)) return 1;
    if (mxd_dense_by_svec_dense(nrows, ncols, X, kind, vi, nnz_v, vx, length, keep_NAs, ws, out, nullptr)) return 1;
    return out.download(out_colmajor, cells);
}

// multiply_coo_by_dense<> (operators.cpp:721-770): values only; kind 4 is the logical and
static int coo_by_dense(const char *what, const void *X, int nrows, int ncols, const int32_t *ii, const int32_t *jj,
                        const void *xx, int64_t nnz, int kind, void *values_out)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0 && nnz <= (int64_t)INT_MAX, "%s: bad arguments", what);
    if (nnz == 0) return 0;
    MX_REQUIRE(ii && jj && xx && values_out, "%s: null pointer", what);
    for (int64_t k = 0; k < nnz; k++)             // the reference reads X wherever the entry points (:740)
        MX_REQUIRE(ii[k] >= 0 && ii[k] < nrows && jj[k] >= 0 && jj[k] < ncols,
                   "%s: entry %lld (%d, %d) lies outside the %d x %d matrix", what, (long long)k, ii[k], jj[k], nrows,
                   ncols);
    MX_REQUIRE(X, "%s: null pointer", what);
    const size_t vb = kind == 4 ? 4 : 8;
    DevBuf D, x;
    Dev<int32_t> i, j;
    if (D.upload(X, (int64_t)nrows * ncols, kind == 0 ? 8 : 4)) return 1;
    if (i.upload(ii, nnz)) return 1;
    if (j.upload(jj, nnz)) return 1;
    if (x.upload(xx, nnz, vb)) return 1;
    return values_only(nnz, vb, values_out, [&](DevBuf &o) {
        return mxd_coo_by_dense(nnz, i, j, x, D, nrows, ncols, kind, o, nullptr);
    });
}
// multiply_coo_by_dense_numeric  src/operators.cpp:772-787
int mx_multiply_coo_by_dense_numeric(const double *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out)
{
    return coo_by_dense("mx_multiply_coo_by_dense_numeric", X_colmajor, nrows, ncols, ii, jj, xx, nnz, 0, values_out);
}
// multiply_coo_by_dense_integer  :789-804
int mx_multiply_coo_by_dense_integer(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out)
{
    return coo_by_dense("mx_multiply_coo_by_dense_integer", X_colmajor, nrows, ncols, ii, jj, xx, nnz, 2, values_out);
}
// multiply_coo_by_dense_logical  :806-821
int mx_multiply_coo_by_dense_logical(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out)
{
    return coo_by_dense("mx_multiply_coo_by_dense_logical", X_colmajor, nrows, ncols, ii, jj, xx, nnz, 3, values_out);
}
// multiply_coo_by_dense_float32  :823-838 (float32@Data bit patterns)
int mx_multiply_coo_by_dense_float32(const float *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                     const int32_t *jj, const double *xx, int64_t nnz, double *values_out)
{
    return coo_by_dense("mx_multiply_coo_by_dense_float32", X_colmajor, nrows, ncols, ii, jj, xx, nnz, 1, values_out);
}
// logicaland_coo_by_dense_logical  :840-855
int mx_logicaland_coo_by_dense_logical(const int32_t *X_colmajor, int nrows, int ncols, const int32_t *ii,
                                       const int32_t *jj, const int32_t *xx, int64_t nnz, int32_t *values_out)
{
    return coo_by_dense("mx_logicaland_coo_by_dense_logical", X_colmajor, nrows, ncols, ii, jj, xx, nnz, 4, values_out);
}

// ---- outer products with a one-column CSR, float32 row vector x CSC (outer.hip) ----------------
// non-empty rows of a host indptr, and the refusal of an outer product beyond R's int32 index range before
// anything is allocated for it (the reference does not check)
static int outer_entries_ok(const char *what, const int32_t *indptr, int nrows, int64_t per_row)
{
    int64_t nonempty = 0;
    for (int r = 0; r < nrows; r++) nonempty += indptr[r] < indptr[r + 1];
    MX_REQUIRE(nonempty * per_row <= (int64_t)INT_MAX,
               "%s: the outer product has %lld entries: exceeds R's int32 index range", what,
               (long long)(nonempty * per_row));
    return 0;
}

int mx_matmul_colvec_by_scolvecascsr_begin(const void *colvec, int colvec_dtype, int dim, const int32_t *indptr,
                                           int nrows, const int32_t *indices, const double *values,
                                           mx_result **res_out, mx_result_info *info)
{
    (void)indices;                                          // never read (matmul.cpp:722-731)
    MX_REQUIRE(res_out && info && indptr && nrows >= 0 && dim >= 0 && (dim == 0 || colvec),
               "mx_matmul_colvec_by_scolvecascsr_begin: bad arguments");
    MX_REQUIRE(colvec_dtype == MX_F64 || colvec_dtype == MX_F32,
               "mx_matmul_colvec_by_scolvecascsr_begin: unsupported dense dtype %d", colvec_dtype);
    MX_REQUIRE(indptr[0] >= 0 && indptr[nrows] >= 0, "mx_matmul_colvec_by_scolvecascsr_begin: bad index pointer");
    *res_out = nullptr;
    if (outer_entries_ok("mx_matmul_colvec_by_scolvecascsr_begin", indptr, nrows, dim)) return 1;
    const int64_t nnz = indptr[nrows];
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Dev<int32_t> p;
        Dev<double> x;
        DevBuf v, ws;
        if (p.upload(indptr, (int64_t)nrows + 1)) return 1;
        if (x.upload(values, nnz)) return 1;
        if (v.upload(colvec, dim, dtype_bytes(colvec_dtype))) return 1;
        if (ws.alloc_bytes(mxd_csr_outer_dense_workspace_bytes(nrows))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        int64_t total = 0;
        if (mxd_csr_outer_dense_count(nrows, dim, p, ws, res.indptr, &total, nullptr)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        if (total == 0) return 0;
        return mxd_csr_outer_dense_fill(nrows, dim, nnz, p, x, v, colvec_dtype, res.indptr, res.indices, res.values,
                                        nullptr);
    });
}

int mx_matmul_spcolvec_by_scolvecascsr_begin(const int32_t *X_indptr, int nrows, const int32_t *X_indices,
                                             const double *X_values, const int32_t *y_indices_base1,
                                             const void *y_values, int value_dtype, int64_t nnz_y, int y_length,
                                             mx_result **res_out, mx_result_info *info)
{
    (void)X_indices;                                        // never read (matmul.cpp:811-833)
    MX_REQUIRE(res_out && info && X_indptr && nrows >= 0 && nnz_y >= 0 && nnz_y <= INT_MAX && y_length >= 0,
               "mx_matmul_spcolvec_by_scolvecascsr_begin: bad arguments");
    if (admit_values("mx_matmul_spcolvec_by_scolvecascsr_begin", value_dtype, kNumeric | kInteger | kLogical | kPattern))
        return 1;
    MX_REQUIRE(nnz_y == 0 || (y_indices_base1 && (value_dtype == MX_NONE || y_values)),
               "mx_matmul_spcolvec_by_scolvecascsr_begin: null pointer");
    MX_REQUIRE(X_indptr[0] >= 0 && X_indptr[nrows] >= 0, "mx_matmul_spcolvec_by_scolvecascsr_begin: bad index pointer");
    *res_out = nullptr;
    if (outer_entries_ok("mx_matmul_spcolvec_by_scolvecascsr_begin", X_indptr, nrows, nnz_y)) return 1;
    const int64_t nnz = X_indptr[nrows];
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Dev<int32_t> p, yi;
        Dev<double> x;
        DevBuf yv, ws;                                    // yv stays null for an nsparseVector
        if (p.upload(X_indptr, (int64_t)nrows + 1)) return 1;
        if (x.upload(X_values, nnz)) return 1;
        if (yi.upload(y_indices_base1, nnz_y)) return 1;
        if (value_dtype != MX_NONE && yv.upload(y_values, nnz_y, dtype_bytes(value_dtype))) return 1;
        if (ws.alloc_bytes(mxd_csr_outer_svec_workspace_bytes(nrows, y_length))) return 1;
        if (res.alloc_indptr((int64_t)y_length + 1)) return 1;
        int64_t nonempty = 0, total = 0;
        if (mxd_csr_outer_svec_count(nrows, nnz, p, x, yi, nnz_y, y_length, ws, res.indptr, &nonempty, &total,
                                     nullptr)) return 1;
        if (res.alloc_entries(total, sizeof(double))) return 1;
        if (total == 0) return 0;
        return mxd_csr_outer_svec_fill(nrows, yi, nnz_y, yv, value_dtype, y_length, nonempty, ws, res.indptr,
                                       res.indices, res.values, nullptr);
    });
}

int mx_matmul_rowvec_by_csc(const float *rowvec, int64_t len_rowvec, const int32_t *indptr, int ncols,
                            const int32_t *indices, const double *values, float *out)
{
    MX_REQUIRE(ncols >= 0 && len_rowvec >= 0, "mx_matmul_rowvec_by_csc: negative size");
    if (ncols == 0) return 0;
    MX_REQUIRE(indptr && out, "mx_matmul_rowvec_by_csc: null pointer");
    Csr A;
    if (A.upload(indptr, indices, values, ncols, values ? sizeof(double) : 0)) return 1;
    for (int64_t k = 0; k < A.nnz; k++)
        MX_REQUIRE(indices[k] >= 0 && indices[k] < len_rowvec,
                   "mx_matmul_rowvec_by_csc: row index %d outside the vector's length", indices[k]);
    Dev<float> v, o;
    if (v.upload(rowvec, len_rowvec)) return 1;
    if (o.alloc(ncols)) return 1;
    if (mxd_rowvec_by_csc(ncols, A.nnz, A.p, A.j, A.x, v, o, nullptr)) return 1;      // A.x is null without values
    return o.download(out, ncols);
}

// ---- CSR (op) dense vector (§8f rank 4) ----------------------------------------------------------------------
static int csr_by_dvec_export(const int32_t *indptr, const int32_t *indices, const void *values, int nrows,
                              const void *dvec, int64_t dvec_len, int ncols, int op, int lhs, void *values_out)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && dvec_len >= 0, "csr (op) vector: negative size");
    if (nrows == 0) return 0;
    const size_t eb = op == MX_DV_LOGICAL_AND ? 4 : 8;
    Csr A;
    if (A.upload(indptr, indices, values, nrows, eb)) return 1;
    if (A.nnz == 0) return 0;
    MX_REQUIRE(dvec_len > 0, "csr (op) vector: empty vector");
    DevBuf D;
    if (D.upload(dvec, dvec_len, eb)) return 1;
    return values_only(A.nnz, eb, values_out, [&](DevBuf &o) {
        return mxd_csr_by_dvec(nrows, ncols, A.nnz, A.p, A.j, A.x, D, dvec_len, op, lhs, o, nullptr);
    });
}

int mx_multiply_csr_by_dvec_no_NAs_numeric(const int32_t *indptr, const int32_t *indices, const double *values,
                                           int nrows, const double *dvec, int64_t dvec_len, int ncols, int multiply,
                                           int powerto, int divide, int divrest, int intdiv, int X_is_LHS,
                                           double *values_out)
{
    int op;
    if (dvec_op_of(multiply, powerto, divide, divrest, intdiv, &op)) return 1;       // operators.cpp:1620-1632
    return csr_by_dvec_export(indptr, indices, values, nrows, dvec, dvec_len, ncols, op, X_is_LHS, values_out);
}

// multiply_csr_by_dvec_with_NAs (operators.cpp:2258-2852; dvecna.hip)
int mx_multiply_csr_by_dvec_with_NAs_begin(const int32_t *indptr, const int32_t *indices, const double *values,
                                           int nrows, const double *dvec, int64_t dvec_len, int ncols, int multiply,
                                           int powerto, int divide, int divrest, int intdiv, int X_is_LHS,
                                           mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && indptr && dvec && nrows >= 0 && ncols >= 0,
               "mx_multiply_csr_by_dvec_with_NAs_begin: bad arguments");
    *res_out = nullptr;
    // :2275-2289
    if ((powerto || divide || divrest) && !X_is_LHS) return set_error("Internal error. Please file an issue in GitHub.");
    int op;
    if (dvec_op_of(multiply, powerto, divide, divrest, intdiv, &op)) return 1;
    MX_REQUIRE(indptr[0] == 0 && indptr[nrows] >= 0, "mx_multiply_csr_by_dvec_with_NAs_begin: bad index pointer");
    MX_REQUIRE(dvec_len >= 1, "mx_multiply_csr_by_dvec_with_NAs_begin: empty vector");   // R/operators.R:961-966
    const bool row_ruled = dvec_len <= nrows && nrows % dvec_len == 0;                    // :2314
    MX_REQUIRE(row_ruled || dvec_len <= (int64_t)nrows * ncols,
               "mx_multiply_csr_by_dvec_with_NAs_begin: the vector has more entries than the matrix");
    return begin_result(res_out, info, MX_F64, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, sizeof(double))) return 1;
        Dev<double> D;
        if (D.upload(dvec, dvec_len)) return 1;
        if (row_ruled) {
            DevBuf ws;
            if (ws.alloc_bytes(mxd_csr_by_dvec_na_rows_workspace_bytes(nrows))) return 1;
            if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
            int64_t total = 0;
            if (mxd_csr_by_dvec_na_rows_count(nrows, ncols, A.nnz, A.p, D, dvec_len, op, ws, res.indptr, &total,
                                              nullptr)) return 1;
            if (res.alloc_entries(total, sizeof(double))) return 1;
            if (total == 0) return 0;
            return mxd_csr_by_dvec_na_rows_fill(nrows, ncols, A.nnz, A.p, A.j, A.x, D, dvec_len, op, res.indptr,
                                                res.indices, res.values, nullptr);
        }
        // the flat regime: the new cells first, as COO triplets
        int64_t nspecial = 0, candidates = 0, n_new = 0;
        Dev<int32_t> nr, nc;
        Dev<double> nx;
        {
            DevBuf sws, cws;
            if (sws.alloc_bytes(mxd_dvec_na_special_workspace_bytes(dvec_len))) return 1;
            if (mxd_dvec_na_special(nrows, ncols, D, dvec_len, op, sws, &nspecial, &candidates, nullptr)) return 1;
            if (candidates > 0) {
                if (cws.alloc_bytes(mxd_dvec_na_cells_workspace_bytes(candidates))) return 1;
                if (mxd_dvec_na_cells_count(nrows, ncols, A.nnz, A.p, A.j, dvec_len, sws, nspecial, candidates, cws,
                                            &n_new, nullptr)) return 1;
            }
            if (n_new > 0) {
                if (nr.alloc(n_new) || nc.alloc(n_new) || nx.alloc(n_new)) return 1;
                if (mxd_dvec_na_cells_fill(nrows, ncols, D, dvec_len, op, sws, nspecial, candidates, cws, nr, nc, nx,
                                           nullptr)) return 1;
            }
        }
        if (n_new == 0) {
            // :2643-2651: the input structure itself and the values-only product, with X on the side it was given
            res.alias(1, (int64_t)nrows + 1, A.nnz);
            if (res.alloc_values(A.nnz, sizeof(double))) return 1;
            return mxd_csr_by_dvec(nrows, ncols, A.nnz, A.p, A.j, A.x, D, dvec_len, op, X_is_LHS, res.values, nullptr);
        }
        Dev<int32_t> Bp, Bj;
        Dev<double> Bx, Ax;
        {
            DevBuf ws;
            if (ws.alloc_bytes(mxd_coo_to_csr_workspace_bytes(n_new, ncols))) return 1;
            if (Bp.alloc((int64_t)nrows + 1) || Bj.alloc(n_new) || Bx.alloc(n_new)) return 1;
            int64_t kept = 0;
            if (mxd_coo_to_csr(nrows, ncols, nr, nc, nx, MX_F64, n_new, Bp, Bj, Bx, ws, &kept, nullptr)) return 1;
            MX_REQUIRE(kept == n_new, "mx_multiply_csr_by_dvec_with_NAs_begin: repeated new cells");
        }
        // :2705-2743: the stored entries, always with X on the left
        if (Ax.alloc(A.nnz)) return 1;
        if (mxd_csr_by_dvec(nrows, ncols, A.nnz, A.p, A.j, A.x, D, dvec_len, op, 1, Ax, nullptr)) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        if (res.alloc_entries(A.nnz + n_new, sizeof(double))) return 1;
        return mxd_csr_join_disjoint(nrows, A.p, A.j, Ax, A.nnz, Bp, Bj, Bx, n_new, res.indptr, res.indices,
                                     res.values, nullptr);
    });
}

int mx_logicaland_csr_by_dvec_internal(const int32_t *indptr, const int32_t *indices, const int32_t *values,
                                       int nrows, const int32_t *dvec, int64_t dvec_len, int ncols,
                                       int32_t *values_out)
{
    return csr_by_dvec_export(indptr, indices, values, nrows, dvec, dvec_len, ncols, MX_DV_LOGICAL_AND, 1, values_out);
}

// ---- cbind / rbind (§8f rank 3) ----------------------------------------------------------------------------
int mx_cbind_csr_begin(const int32_t *Xp, int nX, const int32_t *Xj, const void *Xx, int64_t nvX, const int32_t *Yp,
                       int nY, const int32_t *Yj, const void *Yx, int64_t nvY, int value_dtype, mx_result **res_out,
                       mx_result_info *info)
{
    MX_REQUIRE(res_out && info && nX >= 0 && nY >= 0, "mx_cbind_csr_begin: bad arguments");
    *res_out = nullptr;
    const Values vals(value_dtype, nvX > nvY ? nvX : nvY);            // either operand has values: cbind.cpp:19-20
    // binary: an empty NumericVector
    return begin_result(res_out, info, value_dtype == MX_NONE ? MX_F64 : value_dtype, [&](mx_result &res) {
        Csr X, Y;
        if (X.upload(Xp, Xj, Xx, nX, vals.bytes)) return 1;
        if (Y.upload(Yp, Yj, Yx, nY, vals.bytes)) return 1;
        const int nrows = nX > nY ? nX : nY;
        const int64_t nnz = X.nnz + Y.nnz;
        MX_REQUIRE(nnz <= INT_MAX, "cbind result exceeds R's int32 index range");
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        if (nnz == 0) return res.indptr.zero((int64_t)nrows + 1);                      // cbind.cpp:22-29: zeros
        if (res.alloc_entries(nnz, vals.bytes)) return 1;
        return mxd_csr_cbind(nX, nY, X.p, X.j, X.x, Y.p, Y.j, Y.x, vals.dtype, nnz, res.indptr, res.indices,
                             res.values, nullptr);
    });
}

int mx_concat_csr_batch_begin(const mx_rbind_input *objs, int n_inputs, int out_kind, mx_result **res_out,
                              mx_result_info *info)
{
    MX_REQUIRE(res_out && info && n_inputs >= 0 && out_kind >= 0 && out_kind <= 2, "mx_concat_csr_batch_begin: bad arguments");
    *res_out = nullptr;
    int64_t nrows = 0, nnz = 0;
    for (int k = 0; k < n_inputs; k++) {
        MX_REQUIRE(objs[k].kind >= 0 && objs[k].kind <= 6, "Invalid vector type in argument %d.", k);   // rbind.cpp:131-135
        nrows += objs[k].kind <= 2 ? objs[k].nrows : 1;
        nnz += objs[k].nnz;
    }
    MX_REQUIRE(nrows <= INT_MAX - 1 && nnz <= INT_MAX, "rbind result exceeds R's int32 index range");
    const size_t vb = out_kind == 0 ? 8 : out_kind == 1 ? 4 : 0;
    return begin_result(res_out, info, out_kind == 0 ? MX_F64 : out_kind == 1 ? MX_LGL : MX_NONE, [&](mx_result &res) {
        if (res.alloc_indptr(nrows + 1)) return 1;
        if (res.alloc_entries(nnz, vb)) return 1;
        // every operand's arrays in ONE device buffer, sent up as one stream (a small batch is packed on the host and
        // goes up in one copy, a large one is gathered chunk by chunk into the pinned transfer slots), then the table,
        // two launches, and begin_result's one synchronisation
        BindStaging in;
        std::vector<mx_rbind_item> items((size_t)n_inputs);
        int row = 0;
        int64_t pos = 0;
        for (int k = 0; k < n_inputs; k++) {
            const mx_rbind_input &o = objs[k];
            const bool vec = o.kind >= 3;
            const size_t ivb = (o.kind == 0 || o.kind == 3) ? 8 : (o.kind == 2 || o.kind == 6) ? 0 : 4;
            MX_REQUIRE(o.nnz >= 0 && (vec || o.nrows >= 0), "mx_concat_csr_batch_begin: negative size in argument %d", k);
            mx_rbind_item &it = items[(size_t)k];
            it.kind = o.kind;
            it.nrows = vec ? 1 : o.nrows;
            it.nnz = o.nnz;
            it.row_offset = row;
            it.entry_offset = pos;
            in.add(vec ? nullptr : o.indptr, vec ? 0 : ((size_t)o.nrows + 1) * sizeof(int32_t), (const void **)&it.indptr);
            in.add(o.indices, (size_t)o.nnz * sizeof(int32_t), (const void **)&it.indices);
            in.add(ivb ? o.values : nullptr, (size_t)o.nnz * ivb, &it.values);
            row += it.nrows;
            pos += o.nnz;
        }
        if (in.upload()) return 1;
        Dev<mx_rbind_item> table;
        if (table.upload(items.data(), n_inputs)) return 1;
        return mxd_csr_rbind_batch(table, n_inputs, out_kind, (int)nrows, nnz, res.indptr, res.indices, res.values,
                                   nullptr);
    });
}

// ---- transpose: t_deep / CSR <-> CSC -------------------------------------------------------------------
int mx_csr_transpose_begin(const int32_t *indptr, int nrows, int ncols, const int32_t *indices, const void *values,
                           int value_dtype, int64_t n_values, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && indptr, "mx_csr_transpose_begin: null pointer");
    MX_REQUIRE(nrows >= 0 && ncols >= 0, "mx_csr_transpose_begin: negative dimension");
    if (admit_values("mx_csr_transpose_begin", value_dtype)) return 1;
    MX_REQUIRE(indptr[0] == 0 && indptr[nrows] >= 0, "mx_csr_transpose_begin: bad index pointer");
    *res_out = nullptr;
    const Values vals(value_dtype, n_values);
    MX_REQUIRE(!vals || n_values == indptr[nrows], "mx_csr_transpose_begin: lengths of indices and values differ");
    return begin_result(res_out, info, vals.dtype, [&](mx_result &res) {
        Csr A;
        if (A.upload(indptr, indices, values, nrows, vals.bytes)) return 1;
        DevBuf ws;
        if (ws.alloc_bytes(mxd_csr_transpose_workspace_bytes(A.nnz))) return 1;
        if (res.alloc_indptr((int64_t)ncols + 1)) return 1;
        if (res.alloc_entries(A.nnz, vals.bytes)) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_transpose(nrows, ncols, A.p, A.j, A.x, vals.dtype, A.nnz, res.indptr, res.indices, res.values, ws,
                              &nnz_out, nullptr)) return 1;
        res.set_sizes((int64_t)ncols + 1, nnz_out, vals ? nnz_out : 0);
        return 0;
    });
}

// ---- COO: as.csr.matrix / as.csc.matrix of a TsparseMatrix, as.coo.matrix, CSR (.) COO, COO (op) vector ----
int mx_coo_to_csr_begin(const int32_t *rows, const int32_t *cols, const void *values, int value_dtype,
                        int64_t n_entries, int nrows, int ncols, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_coo_to_csr_begin: null output pointer");
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && n_entries >= 0, "mx_coo_to_csr_begin: negative size");
    MX_REQUIRE(n_entries <= INT_MAX, "mx_coo_to_csr_begin: %lld entries exceed R's int32 index range",
               (long long)n_entries);
    if (admit_values("mx_coo_to_csr_begin", value_dtype)) return 1;
    *res_out = nullptr;
    const Values vals(value_dtype);
    return begin_result(res_out, info, value_dtype, [&](mx_result &res) {
        Dev<int32_t> r, c;
        DevBuf x, ws;
        if (r.upload(rows, n_entries)) return 1;
        if (c.upload(cols, n_entries)) return 1;
        if (vals && x.upload(values, n_entries, vals.bytes)) return 1;
        if (ws.alloc_bytes(mxd_coo_to_csr_workspace_bytes(n_entries, ncols))) return 1;
        if (res.alloc_indptr((int64_t)nrows + 1)) return 1;
        if (res.alloc_entries(n_entries, vals.bytes)) return 1;
        int64_t nnz_out = 0;
        if (mxd_coo_to_csr(nrows, ncols, r, c, x, value_dtype, n_entries, res.indptr, res.indices, res.values, ws,
                           &nnz_out, nullptr)) return 1;
        res.set_sizes((int64_t)nrows + 1, nnz_out, vals ? nnz_out : 0);
        return 0;
    });
}

int mx_csr_to_coo(const int32_t *indptr, int nrows, int32_t *out_rows)
{
    MX_REQUIRE(indptr && nrows >= 0, "mx_csr_to_coo: bad arguments");
    MX_REQUIRE(indptr[0] == 0 && indptr[nrows] >= 0, "mx_csr_to_coo: bad index pointer");
    const int64_t nnz = indptr[nrows];
    if (nnz == 0) return 0;
    MX_REQUIRE(out_rows, "mx_csr_to_coo: null pointer");
    Dev<int32_t> p, o;
    if (p.upload(indptr, (int64_t)nrows + 1)) return 1;
    if (o.alloc(nnz)) return 1;
    if (mxd_csr_to_coo(nrows, nnz, p, o, nullptr)) return 1;
    return o.download(out_rows, nnz);
}

int mx_multiply_csr_by_coo_begin(int logical, const int32_t *X_indptr, const int32_t *X_indices,
                                 const void *X_values, const int32_t *Y_rows, const int32_t *Y_cols,
                                 const void *Y_values, int64_t nnz_Y, int max_row_X, int max_col_X,
                                 mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info && X_indptr, "mx_multiply_csr_by_coo_begin: null pointer");
    MX_REQUIRE(max_row_X >= 0 && max_col_X >= 0 && nnz_Y >= 0, "mx_multiply_csr_by_coo_begin: negative size");
    MX_REQUIRE(nnz_Y <= INT_MAX, "mx_multiply_csr_by_coo_begin: %lld entries exceed R's int32 index range",
               (long long)nnz_Y);
    *res_out = nullptr;
    const size_t vb = logical ? 4 : 8;
    return begin_result(res_out, info, logical ? MX_LGL : MX_F64, [&](mx_result &res) {
        Csr X;
        if (X.upload(X_indptr, X_indices, X_values, max_row_X, vb)) return 1;
        Dev<int32_t> r, c;
        DevBuf y, ws;
        if (r.upload(Y_rows, nnz_Y)) return 1;
        if (c.upload(Y_cols, nnz_Y)) return 1;
        if (y.upload(Y_values, nnz_Y, vb)) return 1;
        if (ws.alloc_bytes(mxd_csr_by_coo_workspace_bytes(nnz_Y))) return 1;
        int64_t nnz_out = 0;
        if (mxd_csr_by_coo_count(logical, max_row_X, max_col_X, X.p, X.j, X.x, r, c, y, nnz_Y, ws, &nnz_out, nullptr))
            return 1;
        if (res.alloc_indptr(nnz_out)) return 1;                    // row ids travel in the indptr vector
        if (res.alloc_entries(nnz_out, vb)) return 1;
        if (nnz_out == 0) return 0;
        return mxd_csr_by_coo_fill(logical, max_row_X, max_col_X, X.p, X.j, X.x, r, c, y, nnz_Y, ws, res.indptr,
                                   res.indices, res.values, nullptr);
    });
}

static int coo_by_dvec_export(const int32_t *ii, const int32_t *jj, const void *xx, int64_t nnz, const void *dvec,
                              int64_t dvec_len, int nrows, int ncols, int op, int lhs, void *values_out)
{
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0 && dvec_len >= 0, "coo (op) vector: negative size");
    if (nnz == 0) return 0;
    MX_REQUIRE(dvec_len > 0, "coo (op) vector: empty vector");
    const size_t eb = op == MX_DV_LOGICAL_AND ? 4 : 8;
    Dev<int32_t> i, j;
    DevBuf x, D;
    if (i.upload(ii, nnz)) return 1;
    if (j.upload(jj, nnz)) return 1;
    if (x.upload(xx, nnz, eb)) return 1;
    if (D.upload(dvec, dvec_len, eb)) return 1;
    return values_only(nnz, eb, values_out, [&](DevBuf &o) {
        return mxd_coo_by_dvec(nrows, ncols, nnz, i, j, x, D, dvec_len, op, lhs, o, nullptr);
    });
}

int mx_multiply_coo_by_dense_ignore_NAs_numeric(const int32_t *ii, const int32_t *jj, const double *xx, int64_t nnz,
                                                const double *dvec, int64_t dvec_len, int nrows, int ncols,
                                                int multiply, int powerto, int divide, int divrest, int intdiv,
                                                int X_is_LHS, double *values_out)
{
    int op;
    if (dvec_op_of(multiply, powerto, divide, divrest, intdiv, &op)) return 1;       // operators.cpp:2872-2883
    return coo_by_dvec_export(ii, jj, xx, nnz, dvec, dvec_len, nrows, ncols, op, X_is_LHS, values_out);
}

int mx_multiply_coo_by_dense_ignore_NAs_logical(const int32_t *ii, const int32_t *jj, const int32_t *xx, int64_t nnz,
                                                const int32_t *dvec, int64_t dvec_len, int nrows, int ncols,
                                                int32_t *values_out)
{
    return coo_by_dvec_export(ii, jj, xx, nnz, dvec, dvec_len, nrows, ncols, MX_DV_LOGICAL_AND, 1, values_out);
}

// ---- X[i, j] of a COO: slice_coo_arbitrary_* / slice_coo_single_* (src/slice_coo.cpp) ----
// One axis of a slice from get_ij_properties' flags (R/slice.R:59-143): all / seq / rev-seq are affine
// (process_i_arbitrary, src/slice_coo.cpp:73-114, and post_process_seq, :120-150); anything else becomes the dense
// map of the 1-based selector (the reference's robin_map + i_indices_rep), in mxd_colmap_build's layout.
static int coo_axis_setup(const int32_t *take_base1, int64_t n_take, int all, int is_seq, int is_rev_seq, int n,
                          const char *what, mx_coo_axis *ax, Dev<int32_t> &start, Dev<int32_t> &pos)
{
    *ax = mx_coo_axis{MX_AXIS_AFFINE, 0, n - 1, 0, 0, nullptr, nullptr};
    if (all) return 0;
    const int first = take_base1[0] - 1, last = take_base1[n_take - 1] - 1;
    if (is_seq || is_rev_seq) {
        MX_REQUIRE(first >= 0 && first < n && last >= 0 && last < n, "slice of a COO: %s index outside [1, %d]", what,
                   n);
        MX_REQUIRE(is_seq ? first <= last : first >= last, "slice of a COO: %s selector is not a %s sequence", what,
                   is_seq ? "ascending" : "descending");
        ax->lo = is_seq ? first : last;
        ax->hi = is_seq ? last : first;
        ax->reversed = is_seq ? 0 : 1;
        return 0;
    }
    int max_v = 0;
    for (int64_t t = 0; t < n_take; t++) {
        MX_REQUIRE(take_base1[t] >= 1 && take_base1[t] <= n, "slice of a COO: %s index outside [1, %d]", what, n);
        if (take_base1[t] > max_v) max_v = take_base1[t];
    }
    const int nmap = max_v + 1;
    // mxd_colmap_build's layout, made here by a stable counting sort while the selector is checked anyway: its
    // device build orders repeated positions by an insertion sort in one lane per index, which is quadratic in the
    // repeats of one index (minutes for 50 000 repeats)
    std::unique_ptr<int32_t[]> h_start(new (std::nothrow) int32_t[(size_t)nmap + 1]());      // zeros
    std::unique_ptr<int32_t[]> h_pos(new (std::nothrow) int32_t[(size_t)n_take]);
    MX_REQUIRE(h_start && h_pos, "out of host memory");
    for (int64_t t = 0; t < n_take; t++) h_start[take_base1[t] + 1]++;  // key v counted at v + 1 <= nmap
    for (int v = 1; v <= nmap; v++) h_start[v] += h_start[v - 1];            // start[v] = entries with key < v
    for (int64_t t = 0; t < n_take; t++) h_pos[h_start[take_base1[t]]++] = (int32_t)t;
    for (int v = nmap; v > 0; v--) h_start[v] = h_start[v - 1];             // undo the cursor shift
    h_start[0] = 0;
    if (start.upload(h_start.get(), (int64_t)nmap + 1)) return 1;
    if (pos.upload(h_pos.get(), n_take)) return 1;
    *ax = mx_coo_axis{MX_AXIS_MAP, 0, 0, 0, nmap, start, pos};
    return 0;
}

int mx_slice_coo_arbitrary_begin(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype,
                                 int64_t nnz, const int32_t *rows_take_base1, int64_t n_rows_take,
                                 const int32_t *cols_take_base1, int64_t n_cols_take, int all_i, int all_j,
                                 int i_is_seq, int j_is_seq, int i_is_rev_seq, int j_is_rev_seq, int nrows,
                                 int ncols, mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "mx_slice_coo_arbitrary_begin: null output pointer");
    MX_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0 && n_rows_take >= 0 && n_cols_take >= 0,
               "mx_slice_coo_arbitrary_begin: negative size");
    MX_REQUIRE(nnz <= INT_MAX, "mx_slice_coo_arbitrary_begin: %lld entries exceed R's int32 index range",
               (long long)nnz);
    if (admit_values("mx_slice_coo_arbitrary_begin", value_dtype)) return 1;
    MX_REQUIRE((nnz == 0 || (ii && jj && (value_dtype == MX_NONE || xx))) && (n_rows_take == 0 || rows_take_base1) &&
               (n_cols_take == 0 || cols_take_base1), "mx_slice_coo_arbitrary_begin: null pointer");
    *res_out = nullptr;
    const Values vals(value_dtype);
    return begin_result(res_out, info, value_dtype, [&](mx_result &res) {
        // the reference reads rows_take_base1[0] unguarded; the R caller never passes an empty selector (:108-125)
        if (nnz == 0 || n_rows_take == 0 || n_cols_take == 0) return 0;       // three empty vectors
        Dev<int32_t> sti, psi, stj, psj;
        mx_coo_axis ai, aj;
        if (coo_axis_setup(rows_take_base1, n_rows_take, all_i, i_is_seq, i_is_rev_seq, nrows, "row", &ai, sti, psi))
            return 1;
        if (coo_axis_setup(cols_take_base1, n_cols_take, all_j, j_is_seq, j_is_rev_seq, ncols, "column", &aj, stj,
                           psj)) return 1;
        Dev<int32_t> r, c;
        DevBuf x, ws;
        if (r.upload(ii, nnz)) return 1;
        if (c.upload(jj, nnz)) return 1;
        if (vals && x.upload(xx, nnz, vals.bytes)) return 1;
        if (ws.alloc_bytes(mxd_coo_slice_workspace_bytes(nnz))) return 1;
        int64_t nnz_out = 0;
        if (mxd_coo_slice_count(nrows, ncols, r, c, nnz, &ai, &aj, ws, &nnz_out, nullptr)) return 1;
        if (res.alloc_indptr(nnz_out)) return 1;                      // row ids travel in the indptr vector
        if (res.alloc_entries(nnz_out, vals.bytes)) return 1;
        if (nnz_out == 0) return 0;
        return mxd_coo_slice_fill(nrows, ncols, r, c, x, value_dtype, nnz, &ai, &aj, ws, res.indptr, res.indices,
                                  res.values, nullptr);
    });
}

int mx_slice_coo_single(const int32_t *ii, const int32_t *jj, const void *xx, int value_dtype, int64_t nnz, int i,
                        int j, int *found, void *value_out)
{
    MX_REQUIRE(found && nnz >= 0, "mx_slice_coo_single: bad arguments");
    if (admit_values("mx_slice_coo_single", value_dtype)) return 1;
    *found = 0;
    if (nnz == 0) return 0;
    MX_REQUIRE(ii && jj && (value_dtype == MX_NONE || xx), "mx_slice_coo_single: null pointer");
    Dev<int32_t> r, c;
    DevBuf x, ws;
    if (r.upload(ii, nnz)) return 1;
    if (c.upload(jj, nnz)) return 1;
    if (value_dtype != MX_NONE && x.upload(xx, nnz, dtype_bytes(value_dtype))) return 1;
    if (ws.alloc_bytes(mxd_coo_single_workspace_bytes())) return 1;
    int64_t k = -1;
    if (mxd_coo_single(r, c, x, value_dtype, nnz, i, j, ws, &k, value_out, nullptr)) return 1;
    *found = k >= 0;
    return 0;
}

// ---- remove_sparse_zeros / filterSparse / check_sparse_matrix (compact.hip) ----------------------------
// One compaction for every layout: 0 CSR / CSC (indptr, idx0), 1 COO (idx0, idx1; the result's ii travels in the
// indptr vector), 2 sparse vector (idx0).  Only the values (or the mask) go up before the count; when a zero rule
// removes nothing the result aliases the inputs and nothing else is moved.
static int compact_begin(int layout, const int32_t *indptr, int nrows, const int32_t *idx0, const int32_t *idx1,
                         const void *values, int value_dtype, int64_t nnz, int rule, const int32_t *mask,
                         mx_result **res_out, mx_result_info *info)
{
    MX_REQUIRE(res_out && info, "compaction: null output pointer");
    MX_REQUIRE(layout >= 0 && layout <= 2 && nrows >= 0 && nrows < INT_MAX, "compaction: bad arguments");
    if (admit_values("compaction", value_dtype, kNumeric | kLogical | kInteger)) return 1;
    if (layout == 0) {
        MX_REQUIRE(indptr && indptr[0] == 0 && indptr[nrows] >= 0, "compaction: bad index pointer");
        nnz = indptr[nrows];
    }
    MX_REQUIRE(nnz >= 0 && nnz <= INT_MAX, "compaction: bad number of entries");
    MX_REQUIRE(nnz == 0 || (idx0 && (layout != 1 || idx1) && values && (rule != MX_KEEP_MASK || mask)),
               "compaction: null pointer");
    *res_out = nullptr;
    const size_t vb = dtype_bytes(value_dtype);
    return begin_result(res_out, info, value_dtype, [&](mx_result &res) {
        DevBuf x, ws;
        Dev<int32_t> mk;                                  // stays null without a mask
        if (x.upload(values, nnz, vb)) return 1;
        if (rule == MX_KEEP_MASK && mk.upload(mask, nnz)) return 1;
        if (ws.alloc_bytes(mxd_compact_workspace_bytes(nnz))) return 1;
        int64_t kept = 0;
        if (mxd_compact_count(nnz, x, value_dtype, rule, mk, ws, &kept, nullptr)) return 1;
        if (kept == nnz && rule != MX_KEEP_MASK) {                  // misc.cpp:586-590, :735-739, :864-867
            res.alias(MX_ALIAS_ALL, layout == 0 ? (int64_t)nrows + 1 : layout == 1 ? nnz : 0, nnz);
            return 0;
        }
        Dev<int32_t> p, i0, i1;                           // p: layout 0 only, i1: layout 1 only, else null
        if (layout == 0 && p.upload(indptr, (int64_t)nrows + 1)) return 1;
        if (i0.upload(idx0, nnz)) return 1;
        if (layout == 1 && i1.upload(idx1, nnz)) return 1;
        if (layout != 2 && res.alloc_indptr(layout == 0 ? (int64_t)nrows + 1 : kept)) return 1;
        if (res.alloc_entries(kept, vb)) return 1;
        int32_t *const rp = res.indptr, *const rj = res.indices;
        return mxd_compact_fill(nnz, x, value_dtype, rule, mk, i0, i1, layout == 0 ? nrows : 0, p, ws,
                                layout == 1 ? rp : rj, layout == 1 ? rj : nullptr, res.values,
                                layout == 0 ? rp : nullptr, nullptr);
    });
}

// the reference's loops (misc.cpp:600-646) as keep rules: a logical CSR with na.rm removes only NA (:637-648)
static int csr_rule(int value_dtype, int remove_NAs)
{
    if (!remove_NAs) return MX_KEEP_NONZERO;
    return value_dtype == MX_F64 ? MX_KEEP_NONZERO_NOT_NA : MX_KEEP_NOT_NA;
}

int mx_remove_zero_valued_csr_numeric(const int32_t *indptr, const int32_t *indices, const double *values, int nrows,
                                      int remove_NAs, mx_result **res, mx_result_info *info)
{
    return compact_begin(0, indptr, nrows, indices, nullptr, values, MX_F64, 0, csr_rule(MX_F64, remove_NAs), nullptr,
                         res, info);
}
int mx_remove_zero_valued_csr_logical(const int32_t *indptr, const int32_t *indices, const int32_t *values,
                                      int nrows, int remove_NAs, mx_result **res, mx_result_info *info)
{
    return compact_begin(0, indptr, nrows, indices, nullptr, values, MX_LGL, 0, csr_rule(MX_LGL, remove_NAs), nullptr,
                         res, info);
}
int mx_remove_zero_valued_coo_numeric(const int32_t *ii, const int32_t *jj, const double *xx, int64_t nnz,
                                      int remove_NAs, mx_result **res, mx_result_info *info)
{
    return compact_begin(1, nullptr, 0, ii, jj, xx, MX_F64, nnz, remove_NAs ? MX_KEEP_NONZERO_NOT_NA : MX_KEEP_NONZERO,
                         nullptr, res, info);
}
int mx_remove_zero_valued_coo_logical(const int32_t *ii, const int32_t *jj, const int32_t *xx, int64_t nnz,
                                      int remove_NAs, mx_result **res, mx_result_info *info)
{
    return compact_begin(1, nullptr, 0, ii, jj, xx, MX_LGL, nnz, remove_NAs ? MX_KEEP_NONZERO_NOT_NA : MX_KEEP_NONZERO,
                         nullptr, res, info);
}
int mx_remove_zero_valued_svec_numeric(const int32_t *ii, const double *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info)
{
    (void)remove_NAs;                                  // misc.cpp:882-886: with na.rm, NaN is still kept (quirk)
    return compact_begin(2, nullptr, 0, ii, nullptr, xx, MX_F64, nnz, MX_KEEP_NONZERO, nullptr, res, info);
}
int mx_remove_zero_valued_svec_integer(const int32_t *ii, const int32_t *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info)
{
    return compact_begin(2, nullptr, 0, ii, nullptr, xx, MX_I32, nnz,
                         remove_NAs ? MX_KEEP_NONZERO_NOT_NA : MX_KEEP_NONZERO, nullptr, res, info);
}
int mx_remove_zero_valued_svec_logical(const int32_t *ii, const int32_t *xx, int64_t nnz, int remove_NAs,
                                       mx_result **res, mx_result_info *info)
{
    return compact_begin(2, nullptr, 0, ii, nullptr, xx, MX_LGL, nnz,
                         remove_NAs ? MX_KEEP_NONZERO_NOT_NA : MX_KEEP_NONZERO, nullptr, res, info);
}

int mx_filter_sparse_begin(int layout, const int32_t *indptr, int nrows, const int32_t *idx0, const int32_t *idx1,
                           const void *values, int value_dtype, int64_t nnz, const int32_t *mask, mx_result **res,
                           mx_result_info *info)
{
    return compact_begin(layout, indptr, nrows, idx0, idx1, values, value_dtype, nnz, MX_KEEP_MASK, mask, res, info);
}

int mx_rebuild_indptr_after_filter(const int32_t *indptr, int64_t indptr_len, const int32_t *filter,
                                   int32_t *out_indptr)
{
    MX_REQUIRE(indptr_len >= 0 && indptr_len <= INT_MAX, "rebuild_indptr_after_filter: bad size");
    if (indptr_len == 0) return 0;                     // nrows = -1: an empty vector (misc.cpp:1105-1106)
    MX_REQUIRE(indptr && out_indptr, "rebuild_indptr_after_filter: null pointer");
    const int m = (int)(indptr_len - 1);
    MX_REQUIRE(indptr[0] == 0 && indptr[m] >= 0, "rebuild_indptr_after_filter: bad index pointer");
    const int64_t nnz = indptr[m];
    MX_REQUIRE(nnz == 0 || filter, "rebuild_indptr_after_filter: null pointer");
    Dev<int32_t> p, f, o;
    DevBuf ws;
    if (p.upload(indptr, indptr_len)) return 1;
    if (f.upload(filter, nnz)) return 1;
    if (ws.alloc_bytes(mxd_compact_workspace_bytes(nnz))) return 1;
    if (o.alloc(indptr_len)) return 1;
    int64_t kept = 0;
    if (mxd_compact_count(nnz, nullptr, MX_NONE, MX_KEEP_MASK, f, ws, &kept, nullptr)) return 1;
    if (mxd_compact_fill(nnz, nullptr, MX_NONE, MX_KEEP_MASK, f, nullptr, nullptr, m, p, ws, nullptr, nullptr, nullptr,
                         o, nullptr)) return 1;
    MX_HIP(hipStreamSynchronize(nullptr));
    return o.download(out_indptr, indptr_len);
}

// check_valid_*: the first failing check in the reference's order, with its message (misc.cpp:978-1013)
static const char *first_failure(int f)
{
    if (f & MX_BAD_NEGATIVE) return "Matrix has negative indices.";
    if (f & MX_BAD_BOUND) return "Matrix has invalid column indices.";     // also for row indices (sic)
    if (f & MX_BAD_NA) return "Matrix has indices with missing values.";   // NA_INTEGER < 0: never reached
    if (f & MX_BAD_PTR_NA) return "Matrix has missing values in the index pointer.";
    if (f & MX_BAD_PTR_ORDER) return "Matrix index pointer is not monotonicaly increasing.";
    return nullptr;
}

static int validate_host(const int32_t *idx, int64_t n, int bound, const int32_t *indptr, int64_t n_ptr,
                         int64_t n_mono, int *flags)
{
    Dev<int32_t> d, p, ws;
    if (d.upload(idx, n)) return 1;
    if (p.upload(indptr, n_ptr)) return 1;
    if (ws.alloc(4)) return 1;
    return mxd_validate_indices(d, n, bound, p, n_ptr, n_mono, ws, flags, nullptr);
}

int mx_check_valid_csr_matrix(const int32_t *indptr, int64_t indptr_len, const int32_t *indices, int64_t nnz,
                              int nrows, int ncols, const char **err)
{
    MX_REQUIRE(err && indptr_len >= 0 && nnz >= 0 && (indptr_len == 0 || indptr) && (nnz == 0 || indices),
               "check_valid_csr_matrix: bad arguments");
    *err = nullptr;
    int64_t mono = (int64_t)nrows < indptr_len - 1 ? (int64_t)nrows : indptr_len - 1;
    if (mono < 0) mono = 0;
    int f = 0;
    if (validate_host(indices, nnz, ncols, indptr, indptr_len, mono, &f)) return 1;
    *err = first_failure(f);
    return 0;
}

int mx_check_valid_coo_matrix(const int32_t *ii, const int32_t *jj, int64_t nnz, int nrows, int ncols,
                              const char **err)
{
    MX_REQUIRE(err && nnz >= 0 && (nnz == 0 || (ii && jj)), "check_valid_coo_matrix: bad arguments");
    *err = nullptr;
    int f = 0;
    if (validate_host(ii, nnz, nrows, nullptr, 0, 0, &f)) return 1;
    if ((*err = first_failure(f)) != nullptr) return 0;
    if (validate_host(jj, nnz, ncols, nullptr, 0, 0, &f)) return 1;
    *err = first_failure(f);
    return 0;
}

int mx_check_valid_svec(const int32_t *ii, int64_t nnz, int nrows, const char **err)
{
    MX_REQUIRE(err && nnz >= 0 && (nnz == 0 || ii), "check_valid_svec: bad arguments");
    *err = nullptr;
    int f = 0;
    if (validate_host(ii, nnz, nrows, nullptr, 0, 0, &f)) return 1;
    *err = first_failure(f);
    return 0;
}

int mx_result_finish(mx_result *res, int32_t *out_indptr, int32_t *out_indices, void *out_values)
{
    MX_REQUIRE(res, "mx_result_finish: null handle");
    const std::unique_ptr<mx_result> owned(res);
    const mx_result_info &inf = res->info;
    if (!inf.alias_structure) {
        if (inf.indptr_len > 0 && out_indptr && res->indptr.download(out_indptr, inf.indptr_len) != 0)
            return set_error("D2H copy of indptr failed");
        if (inf.nnz > 0 && out_indices && res->indices.download(out_indices, inf.nnz) != 0)
            return set_error("D2H copy of indices failed");
    }
    const size_t vb = dtype_bytes(inf.values_dtype);
    if (vb && inf.values_len > 0 && out_values && res->values.p &&
        res->values.download(out_values, inf.values_len, vb) != 0)
        return set_error("D2H copy of values failed");
    return 0;
}

int mx_result_discard(mx_result *res) { delete res; return 0; }

// ---- index-vector classification -------------------------------------------------------------------
static int check_seq_host(const int32_t *indices, int64_t n, int reversed, int *result)
{
    MX_REQUIRE(result, "check_is_seq: null result pointer");
    if (n < 2) { *result = 1; return 0; }
    // slice.cpp:28,40: end-point test first — avoids the transfer for the common negative
    const int64_t span = reversed ? (int64_t)indices[0] - indices[n - 1] : (int64_t)indices[n - 1] - indices[0];
    if (span != n - 1) { *result = 0; return 0; }
    Dev<int32_t> d, flag;
    if (d.upload(indices, n)) return 1;
    if (flag.alloc(4)) return 1;
    return mxd_check_is_seq(d, n, reversed, flag, result, nullptr);
}
int mx_check_is_seq(const int32_t *indices, int64_t n, int *result) { return check_seq_host(indices, n, 0, result); }
int mx_check_is_rev_seq(const int32_t *indices, int64_t n, int *result) { return check_seq_host(indices, n, 1, result); }

// ---- sort precondition (§8f rank 1) ------------------------------------------------------------------
int mx_check_indices_are_sorted(const int32_t *indptr, const int32_t *indices, int nrows, int *result)
{
    MX_REQUIRE(result, "mx_check_indices_are_sorted: null result pointer");
    if (nrows <= 0) { *result = 1; return 0; }
    Csr A;
    if (A.upload(indptr, indices, nullptr, nrows, 0)) return 1;
    Dev<int32_t> flag;
    if (flag.alloc(4)) return 1;
    return mxd_csr_rows_sorted(nrows, A.p, A.j, flag, result, nullptr);
}

int mx_sort_sparse_indices(const int32_t *indptr, int32_t *indices, void *values, int value_dtype, int nrows)
{
    if (nrows <= 0) return 0;
    const size_t vb = values ? dtype_bytes(value_dtype) : 0;
    Csr A;
    if (A.upload(indptr, indices, values, nrows, vb)) return 1;
    if (A.nnz < 2) return 0;
    Dev<int32_t> flag, tj;
    DevBuf tx;
    if (flag.alloc(4)) return 1;
    int sorted = 0;
    if (mxd_csr_rows_sorted(nrows, A.p, A.j, flag, &sorted, nullptr)) return 1;
    if (sorted) return 0;                      // nothing to do, inputs untouched
    if (tj.alloc(A.nnz)) return 1;
    if (vb && tx.alloc(A.nnz, vb)) return 1;
    if (mxd_csr_sort_rows(nrows, A.nnz, A.p, A.j, A.x, vb ? value_dtype : MX_NONE, tj, tx, nullptr)) return 1;
    if (A.j.download(indices, A.nnz)) return 1;
    if (vb && A.x.download(values, A.nnz, vb)) return 1;
    return 0;
}

// sort_vector_indices_{numeric,integer,logical,binary}  src/misc.cpp:460-527: sorts ii (and xx) in place
int mx_sort_vector_indices(int32_t *ii, void *xx, int64_t n, int value_dtype)
{
    MX_REQUIRE(n >= 0 && n <= INT_MAX, "mx_sort_vector_indices: bad size");
    if (n < 2) return 0;
    const size_t vb = value_dtype == MX_NONE ? 0 : dtype_bytes(value_dtype);
    MX_REQUIRE(ii && (vb || value_dtype == MX_NONE) && (!vb || xx), "mx_sort_vector_indices: bad arguments");
    Dev<int32_t> di;
    DevBuf dx, ws;                             // dx stays null without values
    if (di.upload(ii, n)) return 1;
    if (vb && dx.upload(xx, n, vb)) return 1;
    if (ws.alloc_bytes(mxd_sort_vector_indices_workspace_bytes(n))) return 1;
    int was_sorted = 1;
    if (mxd_sort_vector_indices(di, dx, n, value_dtype, ws, &was_sorted, nullptr)) return 1;
    if (was_sorted) return 0;                  // nothing to do, inputs untouched
    if (di.download(ii, n)) return 1;
    if (vb && dx.download(xx, n, vb)) return 1;
    return 0;
}

// sort_coo_indices_{numeric,logical,binary}  src/misc.cpp:387-457: sorts ii, jj (and xx) in place by (ii, jj)
int mx_sort_coo_indices(int32_t *ii, int32_t *jj, void *xx, int64_t nnz, int value_dtype)
{
    MX_REQUIRE(nnz >= 0, "mx_sort_coo_indices: negative size");
    MX_REQUIRE(nnz <= INT_MAX, "mx_sort_coo_indices: %lld entries exceed R's int32 index range", (long long)nnz);
    if (admit_values("mx_sort_coo_indices", value_dtype)) return 1;
    if (nnz == 0) return 0;
    const size_t vb = value_dtype == MX_NONE ? 0 : dtype_bytes(value_dtype);
    MX_REQUIRE(ii && jj && (!vb || xx), "mx_sort_coo_indices: bad arguments");
    Dev<int32_t> di, dj;
    DevBuf dx, ws;                             // dx stays null without values
    if (di.upload(ii, nnz)) return 1;
    if (dj.upload(jj, nnz)) return 1;
    if (vb && dx.upload(xx, nnz, vb)) return 1;
    if (ws.alloc_bytes(mxd_coo_sort_workspace_bytes(nnz))) return 1;
    int was_sorted = 1;
    if (mxd_coo_sort(di, dj, dx, nnz, value_dtype, ws, &was_sorted, nullptr)) return 1;
    if (was_sorted) return 0;                  // nothing to do, inputs untouched
    MX_HIP(hipStreamSynchronize(nullptr));     // a failed sort shows here, before any of the caller's arrays is written
    if (di.download(ii, nnz)) return 1;
    if (dj.download(jj, nnz)) return 1;
    if (vb && dx.download(xx, nnz, vb)) return 1;
    return 0;
}

}  // extern "C"

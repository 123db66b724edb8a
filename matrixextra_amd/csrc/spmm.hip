// spmm.hip — CSR x dense SpMM for gfx950 (MI355X): the policy.  The kernels and their launchers are in
// spmm_rowwave.hip (v1), spmm_slab.hip (v2) and spmm_plan.hip (v3); here are mxd_spmm_csr_dense_ex, which picks one
// (AUTO), and the per-thread host state they share: AUTO's plan, the per-device workspaces, the kernel timer and the
// name of the last kernel.
#include "spmm_common.h"
#include <new>

namespace mx {

static thread_local mx_spmm_plan *g_auto_plan = nullptr;
static thread_local const char *g_last_spmm_kernel = "none";
void note_spmm_kernel(const char *name) { g_last_spmm_kernel = name; }

// wg_per_cu workgroups per CU, no more than the items need (+7: the rounding below), a multiple of 8, at least 8
unsigned persistent_grid(int wg_per_cu, long long total_items)
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    long long grid = (long long)cus * wg_per_cu;
    if (grid > total_items + 7) grid = total_items + 7;
    grid = (grid / 8) * 8;
    if (grid < 8) grid = 8;
    return (unsigned)grid;
}

// grow-only scratch of the calling thread, one buffer per device; get() serves the current device
struct DeviceWorkspace {
    void *ws[64] = {};
    size_t cap[64] = {};
    void *get(size_t bytes, bool release = false)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
        if (release || cap[dev] < bytes) {
            if (ws[dev]) (void)hipFree(ws[dev]);
            ws[dev] = nullptr; cap[dev] = 0;
            if (release || hipMalloc(&ws[dev], bytes) != hipSuccess) return ws[dev] = nullptr;
            cap[dev] = bytes;
        }
        return ws[dev];
    }
    void release() { (void)get(0, true); }
};
static thread_local DeviceWorkspace g_pack_ws, g_sync_ws;
void *pack_workspace(size_t bytes) { return g_pack_ws.get(bytes); }
unsigned *sync_workspace() { return (unsigned *)g_sync_ws.get(SYNC_BYTES); }

// Optional HIP-event ring around the dominant kernel of every SpMM launch (bench.py's roofline figure): events sit
// on the launch stream right before / after the kernel, nothing else in between.
struct KernelTimer {
    static constexpr int N = 256;
    hipEvent_t a[N], b[N];
    bool made = false, on = false;
    int count = 0;
};
static thread_local KernelTimer g_kt;
void kt_begin(hipStream_t st)
{
    if (!g_kt.on || g_kt.count >= KernelTimer::N) return;
    if (!g_kt.made) { for (int i = 0; i < KernelTimer::N; i++) { (void)hipEventCreate(&g_kt.a[i]); (void)hipEventCreate(&g_kt.b[i]); } g_kt.made = true; }
    (void)hipEventRecord(g_kt.a[g_kt.count], st);
}
void kt_end(hipStream_t st)
{
    if (!g_kt.on || g_kt.count >= KernelTimer::N) return;
    (void)hipEventRecord(g_kt.b[g_kt.count], st);
    g_kt.count++;
}

}  // namespace mx

// frees this thread's grow-only scratch (AUTO's plan, the slab-major copy of B, the timing barrier's counters); they
// are re-created on demand
extern "C" int mxd_release_workspaces(void)
{
    if (mx::g_auto_plan) { mxd_spmm_plan_destroy(mx::g_auto_plan); mx::g_auto_plan = nullptr; }
    mx::g_pack_ws.release();
    mx::g_sync_ws.release();
    return 0;
}

extern "C" int mxd_spmm_kernel_timing(int enable)
{
    mx::g_kt.on = enable != 0;
    mx::g_kt.count = 0;
    return 0;
}
// elapsed ms of the dominant kernel of each SpMM launch since mxd_spmm_kernel_timing(1) (synchronises on the events)
extern "C" int mxd_spmm_kernel_times(float *out_ms, int max_out, int *count)
{
    MX_REQUIRE(count, "mxd_spmm_kernel_times: null count pointer");
    const int n = mx::g_kt.count < max_out ? mx::g_kt.count : max_out;
    for (int i = 0; i < n; i++) {
        MX_HIP(hipEventSynchronize(mx::g_kt.b[i]));
        MX_HIP(hipEventElapsedTime(&out_ms[i], mx::g_kt.a[i], mx::g_kt.b[i]));
    }
    *count = n;
    mx::g_kt.count = 0;
    return 0;
}

extern "C" const char *mxd_spmm_last_kernel(void) { return mx::g_last_spmm_kernel; }

extern "C" int mxd_spmm_csr_dense_ex(int m, int n, int K,
                                     const int32_t *indptr, const int32_t *indices, const double *values,
                                     const void *B, size_t ldb, void *C, size_t ldc,
                                     int dense_dtype, int colmajor_out, int algo, int rows_sorted,
                                     int npanels, int wg_per_cu, void *stream)
{
    MX_REQUIRE(m >= 0 && n >= 0 && K >= 0, "mxd_spmm_csr_dense_ex: negative dimension");
    if (m == 0 || n == 0) return 0;
    MX_REQUIRE(indptr && B && C, "mxd_spmm_csr_dense_ex: null pointer");
    hipStream_t st = mx::as_stream(stream);
    bool ok = false;                        // can the slab and planned kernels take these operands?
    if (mx::dispatch_dense("mxd_spmm_csr_dense_ex", dense_dtype, [&](auto t) {
            using real_t = typename decltype(t)::type;
            ok = mx::slab_ok<real_t>(n, (const real_t *)B, ldb, (const real_t *)C, ldc, colmajor_out);
            return 0;
        })) return 1;
    bool auto_pick_planned = false;
    if (algo == MX_SPMM_AUTO) {
        // Measured on MI355X, headline config (profiles/r01_*, r02_*): row-wave 4.45 ms; one-panel slab kernel on the
        // slab-major copy of B 4.05 ms; planned panel sweep 1.87 ms + 0.24 ms to build the plan from plain CSR.
        // AUTO = planned (plan rebuilt on every call: nothing is assumed about A between calls) when B outgrows
        // one XCD's L2 and there is enough work to fill the persistent grid, else the row-wave kernel.
        const size_t b_bytes = (size_t)K * (size_t)n * (dense_dtype == MX_F64 ? 8 : 4);
        const bool big = ok && b_bytes > ((size_t)8 << 20) && (long long)m * n >= (1LL << 24);
        algo = big ? (K < (1 << 25) ? MX_SPMM_PLANNED : MX_SPMM_SLAB) : MX_SPMM_ROWWAVE;
        auto_pick_planned = algo == MX_SPMM_PLANNED;
        if (algo == MX_SPMM_SLAB) { npanels = 1; if (wg_per_cu <= 0) wg_per_cu = 4; }
    }
    if (algo == MX_SPMM_PLANNED) {
        MX_REQUIRE(ok, "mxd_spmm_csr_dense_ex: operands do not meet the planned kernel's 16-byte alignment rules");
        mx_spmm_plan *&auto_plan = mx::g_auto_plan;                  // buffers re-used from call to call (grow-only)
        if (!auto_plan) auto_plan = new (std::nothrow) mx_spmm_plan();
        MX_REQUIRE(auto_plan, "out of host memory");
        // Measured with log-normal row lengths (tools/skew_probe.py): up to ~1.8x the CSR the planned sweep still
        // beats the row-wave kernel even with the plan built per call; beyond that AUTO stops after the sizing pass
        // (from indptr alone, plus the scan) and uses the row-wave kernel.
        if (mx::plan_begin(auto_plan, m, K, indptr, indices, values, npanels, st, auto_pick_planned ? 1 : 0)) return 1;
        // B is packed behind the fill (and skipped with it) while the host waits for the plan's size: the GPU does not
        // idle through the round trip, and B is still packed after the fill, right before the sweep (the fill's
        // traffic would push a B packed earlier out of the Infinity Cache: sweep 2.75 ms instead of 2.05 ms)
        void *Bp = nullptr;
        if (mx::plan_repack(K, n, B, ldb, dense_dtype, st, &Bp, auto_plan->go)) return 1;
        bool refilled = false;
        if (mx::plan_end(auto_plan, st, &refilled)) return 1;
        if (auto_plan->ready) {
            // buffers grown: filled again, pack B behind it
            if (refilled && mx::plan_repack(K, n, B, ldb, dense_dtype, st, &Bp)) return 1;
            mx::g_last_spmm_kernel = "spmm_plan_kernel";
            return mx::plan_run(auto_plan, n, B, ldb, C, ldc, dense_dtype, colmajor_out, 0, 1, st, Bp);
        }
        algo = MX_SPMM_ROWWAVE;
    }
    if (algo == MX_SPMM_SLAB) {
        MX_REQUIRE(ok, "mxd_spmm_csr_dense_ex: operands do not meet the slab kernel's 16-byte alignment rules");
        mx::g_last_spmm_kernel = "spmm_slab_kernel";
        if (npanels <= 0) npanels = rows_sorted ? mx::pick_panels(K, (size_t)2560 << 10) : 1;
        if (!rows_sorted) npanels = 1;                 // panels need column-sorted rows
        if (wg_per_cu <= 0) wg_per_cu = 4;
        return mx::launch_spmm_slab(m, n, K, indptr, indices, values, B, ldb, C, ldc, dense_dtype, colmajor_out, npanels,
                                    wg_per_cu, st);
    }
    mx::g_last_spmm_kernel = "spmm_rowwave_kernel";
    return mxd_spmm_csr_dense(m, n, indptr, indices, values, B, ldb, C, ldc, dense_dtype, colmajor_out, stream);
}

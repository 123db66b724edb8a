// spmm_common.h — what the SpMM units share and nothing else includes (spmm.hip: the policy; spmm_rowwave.hip,
// spmm_slab.hip, spmm_plan.hip: one kernel each): the kernels' vector access helpers, the slab geometry, the plan
// handle, and the host helpers every SpMM launcher goes through.
#pragma once
#include "mx_dispatch.h"

// device-resident plan of one CSR matrix (see spmm_plan.hip)
struct mx_spmm_plan {
    int m = 0, K = 0, npanels = 0, panel_cols = 0, noct = 0;
    long long total_steps = 0;
    long long nnz = 0;
    int32_t *step_off = nullptr; size_t step_off_cap = 0;
    int32_t *pcol = nullptr;     size_t pcol_cap = 0;
    double *pval = nullptr;      size_t pval_cap = 0;
    void *scratch = nullptr;     size_t scratch_cap = 0;       // steps + read-back block (build only)
    bool ready = false;                                            // false: sized but not filled (rejected by AUTO)
    // a build between plan_begin and plan_end: the CSR it reads, what the sizing pass wrote (steps per octet, the sum
    // of every tile of tile_octs octets, nnz), the go flag, the capacity the fill saw
    bool pending = false;
    const int32_t *indptr = nullptr, *indices = nullptr;
    const double *values = nullptr;
    const int32_t *steps = nullptr;
    const unsigned *tile_sums = nullptr;
    int ntiles = 0, tile_octs = 0;
    const long long *nnz_dev = nullptr;
    int *go = nullptr;
    long long fill_cap = 0;
    int pad_rule = 0;
};

namespace mx {

template <typename T, int N> struct VecT;
template <> struct VecT<double, 1> { using type = double; };
template <> struct VecT<double, 2> { using type = double __attribute__((ext_vector_type(2))); };
template <> struct VecT<float, 1>  { using type = float; };
template <> struct VecT<float, 2>  { using type = float __attribute__((ext_vector_type(2))); };
template <> struct VecT<float, 4>  { using type = float __attribute__((ext_vector_type(4))); };

template <typename real_t, int VEC>
__device__ __forceinline__ void vload(real_t (&dst)[VEC], const real_t *__restrict__ p)
{
    using V = typename VecT<real_t, VEC>::type;
    if constexpr (VEC == 1) {
        dst[0] = *p;
    } else {
        const V v = *reinterpret_cast<const V *>(p);
#pragma unroll
        for (int i = 0; i < VEC; i++) dst[i] = v[i];
    }
}

template <typename real_t, int VEC>
__device__ __forceinline__ void vstore(real_t *__restrict__ p, const real_t (&src)[VEC])
{
    using V = typename VecT<real_t, VEC>::type;
    if constexpr (VEC == 1) {
        *p = src[0];
    } else {
        V v;
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = src[i];
        *reinterpret_cast<V *>(p) = v;
    }
}

// streaming store: C is written once and not read again by the kernel — keep it from displacing the packed B in L2 /
// the Infinity Cache (measured on the planned kernel: 2.05 -> 1.98 ms)
template <typename real_t, int VEC>
__device__ __forceinline__ void vstore_nt(real_t *__restrict__ p, const real_t (&src)[VEC])
{
    using V = typename VecT<real_t, VEC>::type;
    if constexpr (VEC == 1) {
        __builtin_nontemporal_store(src[0], p);
    } else {
        V v;
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = src[i];
        __builtin_nontemporal_store(v, reinterpret_cast<V *>(p));
    }
}

__device__ __forceinline__ double mx_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float mx_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

constexpr int SLAB_GROUP = 8;                       // lanes per row
// a slab is one 128-byte line of a B row: 16 bytes (SLAB_VEC elements) per lane of the group, SLAB_W columns in all
template <typename real_t> constexpr int SLAB_VEC = 16 / (int)sizeof(real_t);
template <typename real_t> constexpr int SLAB_W = SLAB_GROUP * SLAB_VEC<real_t>;

// Timing-only barrier among the workgroups that share blockIdx % 8 (the XCD group): it keeps them on the same
// column panel so that the panel stays L2-resident.  No data is handed over, so no release/acquire is needed
// and a timeout is harmless: the spin is bounded and falling through only costs locality, never correctness
// (all co-resident by grid sizing; a block that is not resident simply makes the others time out).
__device__ __forceinline__ void xcd_timing_barrier(unsigned *ctr, unsigned target)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && ++spins < 4096)
            __builtin_amdgcn_s_sleep(8);
    }
    __syncthreads();
}

// panels so that one slab-panel (K/npanels rows x 128 B) stays within `l2_budget` bytes
inline int pick_panels(int K, size_t l2_budget)
{
    const size_t slab_bytes = (size_t)K * 128;
    int p = (int)((slab_bytes + l2_budget - 1) / l2_budget);
    if (p < 1) p = 1;
    if (p > 64) p = 64;
    return p;
}

// can the slab kernel take these operands?  (16-B aligned rows of B, whole vectors per row;
// row-major C additionally needs 16-B aligned rows of C)
template <typename real_t>
inline bool slab_ok(int n, const real_t *B, size_t ldb, const real_t *C, size_t ldc, int colmajor)
{
    constexpr int VEC = SLAB_VEC<real_t>;
    if (n < VEC || n % VEC || ldb % VEC || (uintptr_t)B % 16) return false;
    if (!colmajor && (ldc % VEC || (uintptr_t)C % 16)) return false;
    return true;
}

#pragma GCC visibility push(hidden)
// spmm.hip: the optional HIP-event ring around the dominant kernel of a launch, and what mxd_spmm_last_kernel reports
void kt_begin(hipStream_t st);
void kt_end(hipStream_t st);
void note_spmm_kernel(const char *name);
// spmm.hip: grid of a persistent kernel that deals `total_items` work items to the 8 XCD groups (blockIdx % 8)
unsigned persistent_grid(int wg_per_cu, long long total_items);
// spmm.hip: this thread's grow-only per-device buffers (nullptr when they cannot be had): the packed copy of B, and
// the SYNC_BYTES of counters of the timing barrier (8 groups x 256 B)
constexpr size_t SYNC_BYTES = 8 * 64 * sizeof(unsigned);
void *pack_workspace(size_t bytes);
unsigned *sync_workspace();

// spmm_slab.hip: B -> slab-major Bp with Kp >= K rows per slab (repack_slabs_kernel), and the slab kernel
template <typename real_t>
int launch_repack(int K, int Kp, int n, const real_t *B, size_t ldb, real_t *Bp, const int *go, hipStream_t st);
int launch_spmm_slab(int m, int n, int K, const int32_t *indptr, const int32_t *indices, const double *values,
                     const void *B, size_t ldb, void *C, size_t ldc, int dense_dtype, int colmajor, int npanels,
                     int wg_per_cu, hipStream_t stream);

// spmm_plan.hip
int plan_begin(mx_spmm_plan *pl, int m, int K, const int32_t *indptr, const int32_t *indices, const double *values,
               int npanels, hipStream_t st, int pad_rule = 0);
int plan_end(mx_spmm_plan *pl, hipStream_t st, bool *refilled = nullptr);
int plan_repack(int K, int n, const void *B, size_t ldb, int dense_dtype, hipStream_t st, void **Bp_out,
                const int *go = nullptr);
int plan_run(const mx_spmm_plan *pl, int n, const void *B, size_t ldb, void *C, size_t ldc, int dense_dtype,
             int colmajor, int wg_per_cu, int sync_mode, hipStream_t st, const void *Bp = nullptr);
#pragma GCC visibility pop

}  // namespace mx

// spmm.hip — CSR x dense SpMM for gfx950 (MI355X), hand-written HIP.
//
// Replaces the two OpenMP loops of the reference:
//   gemm_csr_drm_as_drm  src/matmul.cpp:118-142  (C row-major)
//   gemm_csr_drm_as_dcm  src/matmul.cpp:150-185  (C column-major, what R needs)
//
// Design (v1, "row-wave"): a workgroup of 4 wavefronts owns a tile of TR
// consecutive rows; each wavefront walks TR/4 rows.  For one row the 64 lanes
// span 64*VEC consecutive columns of the output, so every nonzero a_ij turns
// into ONE fully coalesced read of B[j, slab] (1 KiB for f64 n=128 / f32
// n=256: 16 B per lane) with the row base address in SGPRs (v_readlane of the
// column id), followed by VEC FMAs per lane.  (j, a) of the row are loaded
// coalesced by the wave, kept in one VGPR pair and broadcast lane by lane; the
// next row's first chunk is prefetched while the current row streams B.
// Accumulation runs in CSR storage order, one FMA per nonzero per column —
// the same order as the reference's axpy loop — so results differ from an
// FMA-enabled BLAS in nothing and from a non-FMA one by one rounding per term.
//
// Column-major epilogue: the tile's rows are parked in LDS (row stride odd ->
// conflict-free transposed reads) and written out as TR-row-contiguous
// segments per output column (256 B for f64, TR=32), instead of the
// stride-m scatter the CPU code does with dcopy.
//
// Roofline: HBM-bound.  Algorithmic bytes per launch =
//   4(m+1) + 12 nnz + s*K*n + s*m*n   (SURVEY §8d).  The gather of B rows is
// served by L2 / Infinity Cache (B = 102 MB for the headline config).
#include "mx_common.h"
#include <cstdlib>
#include <new>

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

static void kt_begin(hipStream_t st);
static void kt_end(hipStream_t st);

constexpr int SPMM_WAVES = 4;     // wavefronts per workgroup
constexpr int SPMM_UNROLL = 8;    // B-row reads in flight per wavefront

// one chunk of <=64 nonzeros of the current row: lane k holds (jv, av) of entry k.
// B is wave-uniform and `col` a per-lane element offset, so each read is
// "SGPR row base + VGPR lane offset" (global_load ... s[base], no 64-bit VALU
// address arithmetic per nonzero).  Lanes past the last column read a clamped,
// valid column instead of branching; their results are never stored.
template <typename real_t, int VEC>
__device__ __forceinline__ void spmm_chunk(int cnt, int jv, double av,
                                           const real_t *__restrict__ B, size_t ldb, unsigned col,
                                           real_t (&acc)[VEC])
{
    int k = 0;
    for (; k + SPMM_UNROLL <= cnt; k += SPMM_UNROLL) {
        real_t b[SPMM_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < SPMM_UNROLL; u++) {
            const int j = __builtin_amdgcn_readlane(jv, k + u);
            const real_t *__restrict__ rowp = B + (size_t)j * ldb;
            vload<real_t, VEC>(b[u], rowp + col);
        }
#pragma unroll
        for (int u = 0; u < SPMM_UNROLL; u++) {
            const real_t a = (real_t)readlane_f64(av, k + u);   // narrowed per nonzero for f32 (matmul.cpp:53-57)
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[v] = mx_fma(a, b[u][v], acc[v]);
        }
    }
    for (; k < cnt; k++) {
        const int j = __builtin_amdgcn_readlane(jv, k);
        const real_t a = (real_t)readlane_f64(av, k);
        const real_t *__restrict__ rowp = B + (size_t)j * ldb;
        real_t b[VEC];
        vload<real_t, VEC>(b, rowp + col);
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[v] = mx_fma(a, b[v], acc[v]);
    }
}

// TR rows per workgroup.  COLMAJOR: stage the tile in LDS and write transposed.
// VSTORE (COLMAJOR only): two consecutive rows per lane -> wider stores; needs
// even m, even ldc and 2*sizeof(real_t)-aligned C.
template <typename real_t, int VEC, bool COLMAJOR, bool VSTORE, int TR>
__global__ __launch_bounds__(SPMM_WAVES * MX_WAVE)
void spmm_rowwave_kernel(int m, int n,
                         const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                         const double *__restrict__ values,
                         const real_t *__restrict__ B, size_t ldb,
                         real_t *__restrict__ C, size_t ldc)
{
    constexpr int W = MX_WAVE * VEC;          // output columns per workgroup pass
    constexpr int S = W + 1;                  // odd LDS row stride (elements)
    constexpr int ROWS_PER_WAVE = TR / SPMM_WAVES;
    __shared__ real_t tile[COLMAJOR ? TR * S : 1];

    const int lane = lane_id();
    const int wave = uniform(threadIdx.x / MX_WAVE);
    const int row0 = blockIdx.x * TR;
    const int c0 = blockIdx.y * W;
    const int col = c0 + lane * VEC;
    const bool active = col < n;
    // clamped column for the reads of inactive lanes (n >= VEC always holds here)
    const unsigned lcol = active ? (unsigned)col : (unsigned)(n - VEC);

    const int r_begin = row0 + wave * ROWS_PER_WAVE;
    const int r_end = min(r_begin + ROWS_PER_WAVE, m);

    int s = 0, e = 0, jv = 0;
    double av = 0.0;
    if (r_begin < r_end) {
        s = uniform(indptr[r_begin]);
        e = uniform(indptr[r_begin + 1]);
        if (s + lane < e) { jv = indices[s + lane]; av = values[s + lane]; }
    }
    for (int row = r_begin; row < r_end; row++) {
        // prefetch the first chunk of the next row
        int e2 = e, jv2 = 0;
        double av2 = 0.0;
        if (row + 1 < r_end) {
            e2 = uniform(indptr[row + 2]);
            if (e + lane < e2) { jv2 = indices[e + lane]; av2 = values[e + lane]; }
        }
        real_t acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[v] = 0;

        spmm_chunk<real_t, VEC>(min(MX_WAVE, e - s), jv, av, B, ldb, lcol, acc);
        for (int k0 = s + MX_WAVE; k0 < e; k0 += MX_WAVE) {   // rows longer than one wavefront
            int jc = 0;
            double ac = 0.0;
            if (k0 + lane < e) { jc = indices[k0 + lane]; ac = values[k0 + lane]; }
            spmm_chunk<real_t, VEC>(min(MX_WAVE, e - k0), jc, ac, B, ldb, lcol, acc);
        }

        if constexpr (COLMAJOR) {
            real_t *t = tile + (row - row0) * S + lane * VEC;
#pragma unroll
            for (int v = 0; v < VEC; v++) t[v] = acc[v];
        } else {
            if (active) vstore<real_t, VEC>(C + (size_t)row * ldc + col, acc);
        }
        s = e; e = e2; jv = jv2; av = av2;
    }

    if constexpr (COLMAJOR) {
        __syncthreads();
        const int ncols = min(W, n - c0);
        constexpr int RPL = VSTORE ? 2 : 1;        // rows per lane in the write-out
        constexpr int LPC = TR / RPL;              // lanes per output column
        constexpr int CPW = MX_WAVE / LPC;         // columns per wave-instruction
        const int q = lane % LPC;
        const int r = q * RPL;
        const int grow = row0 + r;
        for (int cb = wave * CPW; cb < ncols; cb += SPMM_WAVES * CPW) {
            const int c = cb + lane / LPC;
            if (c < ncols && grow < m) {
                real_t *dst = C + (size_t)(c0 + c) * ldc + grow;
                if constexpr (VSTORE) {
                    real_t two[2] = { tile[r * S + c], tile[(r + 1) * S + c] };
                    vstore<real_t, 2>(dst, two);   // m even & grow even => grow+1 < m
                } else {
                    *dst = tile[r * S + c];
                }
            }
        }
    }
}

template <typename real_t, int VEC, bool COLMAJOR, bool VSTORE>
static int launch_spmm(int m, int n, const int32_t *indptr, const int32_t *indices, const double *values,
                       const real_t *B, size_t ldb, real_t *C, size_t ldc, hipStream_t stream)
{
    constexpr int TR = 32;
    constexpr int W = MX_WAVE * VEC;
    dim3 grid((unsigned)ceil_div(m, TR), (unsigned)ceil_div(n, W));
    kt_begin(stream);
    hipLaunchKernelGGL((spmm_rowwave_kernel<real_t, VEC, COLMAJOR, VSTORE, TR>), grid,
                       dim3(SPMM_WAVES * MX_WAVE), 0, stream, m, n, indptr, indices, values, B, ldb, C, ldc);
    kt_end(stream);
    MX_LAUNCH_CHECK();
    return 0;
}

template <typename real_t, int VECMAX>
static int dispatch_spmm(int m, int n, const int32_t *indptr, const int32_t *indices, const double *values,
                         const real_t *B, size_t ldb, real_t *C, size_t ldc, int colmajor, hipStream_t stream)
{
    // widest per-lane access the operands allow (16 B when rows of B are 16-B aligned)
    const bool b_vec = (n % VECMAX == 0) && (ldb % VECMAX == 0) && ((uintptr_t)B % (VECMAX * sizeof(real_t)) == 0);
    if (colmajor) {
        // paired stores write rows grow and grow+1 (grow even): with m odd the last pair would write row m, which
        // is the column's ldc padding when ldc > m
        const bool vs = (m % 2 == 0) && (ldc % 2 == 0) && ((uintptr_t)C % (2 * sizeof(real_t)) == 0);
        if (b_vec) return vs ? launch_spmm<real_t, VECMAX, true, true>(m, n, indptr, indices, values, B, ldb, C, ldc, stream)
                             : launch_spmm<real_t, VECMAX, true, false>(m, n, indptr, indices, values, B, ldb, C, ldc, stream);
        return vs ? launch_spmm<real_t, 1, true, true>(m, n, indptr, indices, values, B, ldb, C, ldc, stream)
                  : launch_spmm<real_t, 1, true, false>(m, n, indptr, indices, values, B, ldb, C, ldc, stream);
    }
    const bool c_vec = b_vec && (ldc % VECMAX == 0) && ((uintptr_t)C % (VECMAX * sizeof(real_t)) == 0);
    if (c_vec) return launch_spmm<real_t, VECMAX, false, false>(m, n, indptr, indices, values, B, ldb, C, ldc, stream);
    return launch_spmm<real_t, 1, false, false>(m, n, indptr, indices, values, B, ldb, C, ldc, stream);
}


// =====================================================================================================
// v2 "slab / panel sweep" kernel.
//
// Why: with B = K x n row-major far larger than one XCD's 4 MiB L2 (102 MB for the headline config) the
// row-wave kernel above gets a 7 % L2 hit rate and runs at the Infinity-Cache gather rate (~7 TB/s of
// fabric reads for nnz*n*8 = 32.8 GB -> 4.5 ms; profiles/r01_v1_*).  The same kernel with a 4 MB B runs in
// 1.5 ms.  This kernel restructures the iteration space so that each XCD's *working set* of B fits its L2:
//
//   * column slabs: the n output columns are cut into 128-byte slabs (16 f64 / 32 f32 columns = one cache
//     line of a B row).  Work items (slab, row block) are dealt slab-major to the 8 XCDs (blockIdx % 8 is
//     the XCD a workgroup lands on — a locality heuristic only, never a correctness assumption), so one
//     XCD touches K x 128 B of B (12.8 MB) instead of all of it;
//   * column panels: [0, K) is cut into `npanels` ranges so that one slab-panel (K/npanels x 128 B) fits
//     L2.  A workgroup keeps the accumulators of its RB = 32*RPG rows in registers and sweeps the panels
//     in order, visiting for each of its rows only the entries whose column lies in the current panel
//     (rows are sorted, so a cursor per row suffices).  All workgroups of an XCD start together and do
//     statistically equal work per panel, so they stay on the same panel (soft synchronisation).
//     npanels > 1 requires rows sorted by column; npanels == 1 works for any order.
//   * 8 lanes own one row (x 16 B per lane = the 128-B slab line), so a wave-instruction reads 8 full
//     lines of B for 8 different rows; (j, a) are loaded coalesced 8 entries at a time per row and
//     broadcast inside the 8-lane group with ds_swizzle.
// Summation order inside a row is still CSR storage order (one FMA per entry), as in the reference.
// =====================================================================================================
constexpr int SLAB_BLOCK = 256;
constexpr int SLAB_GROUP = 8;                       // lanes per row
constexpr int SLAB_GROUPS = SLAB_BLOCK / SLAB_GROUP;

template <int T>
__device__ __forceinline__ int group8_bcast(int v)
{
    // ds_swizzle bit-mask mode: src lane = ((lane & and) | or) ^ xor inside each 32-lane half;
    // and = 0b11000 keeps the 8-lane group, or = T picks entry T of the group.
    return __builtin_amdgcn_ds_swizzle(v, 0x18 | (T << 5));
}
template <int T>
__device__ __forceinline__ double group8_bcast(double v)
{
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = group8_bcast<T>(u.i[0]);
    u.i[1] = group8_bcast<T>(u.i[1]);
    return u.d;
}

__device__ __forceinline__ unsigned group8_ballot(bool pred)
{
    const unsigned long long b = __ballot(pred);
    return (unsigned)(b >> (lane_id() & ~(SLAB_GROUP - 1))) & 0xFFu;
}

// One chunk (<= 8 entries, lane t of the group holds entry t) of one row: all B reads are issued before
// the first FMA so that 8 line reads per group are in flight (a branch per entry would serialise them
// behind s_waitcnt vmcnt(0)).  Entries past `cnt` read a valid address (entry 0's row) and are dropped
// by a select, never by arithmetic (0 * Inf would poison the sum).
template <typename real_t, int VEC, int T>
__device__ __forceinline__ void slab_load(int cnt, int jv, const real_t *__restrict__ B, size_t ldb, unsigned lcol,
                                          real_t (&b)[VEC])
{
    int j = group8_bcast<T>(jv);
    j = (T < cnt) ? j : 0;
    vload<real_t, VEC>(b, B + (size_t)j * ldb + lcol);
}
template <typename real_t, int VEC, int T>
__device__ __forceinline__ void slab_fma(int cnt, double av, const real_t (&b)[VEC], real_t (&acc)[VEC])
{
    const real_t a = (real_t)group8_bcast<T>(av);
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        const real_t f = mx_fma(a, b[v], acc[v]);
        acc[v] = (T < cnt) ? f : acc[v];
    }
}
template <typename real_t, int VEC>
__device__ __forceinline__ void slab_chunk(int cnt, int jv, double av, const real_t *__restrict__ B, size_t ldb,
                                           unsigned lcol, real_t (&acc)[VEC])
{
    real_t b0[VEC], b1[VEC], b2[VEC], b3[VEC], b4[VEC], b5[VEC], b6[VEC], b7[VEC];
    slab_load<real_t, VEC, 0>(cnt, jv, B, ldb, lcol, b0);
    slab_load<real_t, VEC, 1>(cnt, jv, B, ldb, lcol, b1);
    slab_load<real_t, VEC, 2>(cnt, jv, B, ldb, lcol, b2);
    slab_load<real_t, VEC, 3>(cnt, jv, B, ldb, lcol, b3);
    slab_load<real_t, VEC, 4>(cnt, jv, B, ldb, lcol, b4);
    slab_load<real_t, VEC, 5>(cnt, jv, B, ldb, lcol, b5);
    slab_load<real_t, VEC, 6>(cnt, jv, B, ldb, lcol, b6);
    slab_load<real_t, VEC, 7>(cnt, jv, B, ldb, lcol, b7);
    slab_fma<real_t, VEC, 0>(cnt, av, b0, acc);
    slab_fma<real_t, VEC, 1>(cnt, av, b1, acc);
    slab_fma<real_t, VEC, 2>(cnt, av, b2, acc);
    slab_fma<real_t, VEC, 3>(cnt, av, b3, acc);
    slab_fma<real_t, VEC, 4>(cnt, av, b4, acc);
    slab_fma<real_t, VEC, 5>(cnt, av, b5, acc);
    slab_fma<real_t, VEC, 6>(cnt, av, b6, acc);
    slab_fma<real_t, VEC, 7>(cnt, av, b7, acc);
}

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

template <typename real_t, int RPG, bool COLMAJOR>
__global__ __launch_bounds__(SLAB_BLOCK)
void spmm_slab_kernel(int m, int n,
                      const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                      const double *__restrict__ values,
                      const real_t *__restrict__ B, size_t ldb,
                      real_t *__restrict__ C, size_t ldc,
                      int npanels, int panel_cols, int nslabs, int nrowblocks, int c_vec_ok,
                      unsigned *__restrict__ sync_ctr, int sync_mode, size_t slab_stride)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;             // columns per slab
    constexpr int RB = SLAB_GROUPS * RPG;           // rows per workgroup step
    const int lg = threadIdx.x & (SLAB_GROUP - 1);
    const int grp = threadIdx.x / SLAB_GROUP;
    const int xcd = blockIdx.x & 7;
    const int wg = blockIdx.x >> 3, nwg = gridDim.x >> 3;
    const long long total = (long long)nslabs * nrowblocks;
    const long long lo = total * xcd / 8, hi = total * (xcd + 1) / 8;

    // every workgroup of the group runs the same number of steps (idle ones only keep the barrier count right)
    const int niter = (int)((hi - lo + nwg - 1) / nwg);
    unsigned *const my_ctr = sync_ctr + xcd * 64;    // one counter per group, 256 B apart
    unsigned step = 0;
    for (int it = 0; it < niter; it++) {
        const long long item_raw = lo + wg + (long long)it * nwg;
        const bool have = item_raw < hi;
        const long long item = have ? item_raw : lo;
        const int slab = (int)(item / nrowblocks);
        const int rb = (int)(item % nrowblocks);
        const int row0 = rb * RB + grp * RPG;
        const int col = slab * W + lg * VEC;
        const bool active = col < n;
        // slab_stride != 0: B was repacked slab-major ([slab][K][W], zero padded) so that a slab is contiguous and
        // spreads over all L2 channels; the caller then passes ldb = W and this adds the slab's base.
        const unsigned lcol = slab_stride ? (unsigned)(lg * VEC) : (active ? (unsigned)col : (unsigned)(n - VEC));
        const real_t *__restrict__ Bs = B + (size_t)slab * slab_stride;

        int cur[RPG], end[RPG];
        real_t acc[RPG][VEC];
#pragma unroll
        for (int r = 0; r < RPG; r++) {
            const int row = row0 + r;
            cur[r] = 0; end[r] = 0;
            if (have && row < m) { cur[r] = indptr[row]; end[r] = indptr[row + 1]; }
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[r][v] = 0;
        }

        for (int p = 0; p < npanels; p++) {
            const int pend = (p == npanels - 1) ? INT_MAX : (p + 1) * panel_cols;
            if (sync_mode == 2 || (sync_mode == 1 && p == 0)) {
                step++;
                xcd_timing_barrier(my_ctr, step * (unsigned)nwg);
            }
            unsigned pending = (1u << RPG) - 1u;          // rows that may still have entries in this panel
            while (__ballot(pending != 0) != 0ULL) {
                int jv[RPG];
                double av[RPG];
#pragma unroll
                for (int r = 0; r < RPG; r++) {
                    // unconditional reads (clamped to entry 0) so that all 2*RPG loads are in flight together
                    const int k = cur[r] + lg;
                    const bool valid = ((pending >> r) & 1u) && k < end[r];
                    const int ks = valid ? k : 0;
                    const int jl = indices[ks];
                    const double al = values[ks];
                    jv[r] = valid ? jl : INT_MAX;
                    av[r] = al;
                }
#pragma unroll
                for (int r = 0; r < RPG; r++) {
                    const unsigned long long inpanel = __ballot(jv[r] < pend);
                    if (inpanel == 0ULL) { pending &= ~(1u << r); continue; }   // no group of this wave has entries here
                    // sorted row: in-panel entries are a prefix of the chunk
                    const int cnt = __popc((unsigned)(inpanel >> (lane_id() & ~(SLAB_GROUP - 1))) & 0xFFu);
                    // entry 0 of an empty chunk may be INT_MAX: slab_load only dereferences entries < cnt (else row 0)
                    slab_chunk<real_t, VEC>(cnt, jv[r], av[r], Bs, ldb, lcol, acc[r]);
                    cur[r] += cnt;
                    if (cnt < SLAB_GROUP) pending &= ~(1u << r);          // panel (or row) exhausted
                }
            }
        }

        // epilogue: lane holds columns col..col+VEC-1 of rows row0..row0+RPG-1
        if (active && have) {
            if constexpr (!COLMAJOR) {
#pragma unroll
                for (int r = 0; r < RPG; r++)
                    if (row0 + r < m) vstore<real_t, VEC>(C + (size_t)(row0 + r) * ldc + col, acc[r]);
            } else {
                constexpr int RV = 16 / (int)sizeof(real_t);               // rows per 16-B store
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    real_t *__restrict__ dst = C + (size_t)(col + v) * ldc + row0;
                    if (c_vec_ok && row0 + RPG <= m) {
#pragma unroll
                        for (int r = 0; r < RPG; r += RV) {
                            real_t tmp[RV];
#pragma unroll
                            for (int q = 0; q < RV; q++) tmp[q] = acc[r + q][v];
                            vstore<real_t, RV>(dst + r, tmp);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < RPG; r++)
                            if (row0 + r < m) dst[r] = acc[r][v];
                    }
                }
            }
        }
    }
}

// panels so that one slab-panel (K/npanels rows x 128 B) stays within `l2_budget` bytes
static int pick_panels(int K, size_t l2_budget)
{
    const size_t slab_bytes = (size_t)K * 128;
    int p = (int)((slab_bytes + l2_budget - 1) / l2_budget);
    if (p < 1) p = 1;
    if (p > 64) p = 64;
    return p;
}

// B (K x n row-major, leading dimension ldb) -> slab-major [nslabs][K][W], zero padded past column n; skipped when
// `go` (a plan fill's verdict, see plan_fill_kernel) is set and 0.  One thread per 16-byte piece; reads are row-contiguous, each 8-lane group writes one full 128-byte line.
template <typename real_t>
__global__ __launch_bounds__(256)
void repack_slabs_kernel(int K, int Kp, int n, int nslabs, const real_t *__restrict__ B, size_t ldb, real_t *__restrict__ Bp,
                         const int *__restrict__ go)
{
    if (go && *go == 0) return;                                      // the plan fill in front of it was skipped
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;
    const long long pieces_per_row = (long long)nslabs * SLAB_GROUP;
    const long long total = (long long)Kp * pieces_per_row;          // rows K..Kp-1 of every slab are zero (plan padding)
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(t / pieces_per_row);
        const int piece = (int)(t % pieces_per_row);
        const int slab = piece / SLAB_GROUP, lg = piece % SLAB_GROUP;
        const int col = slab * W + lg * VEC;
        real_t v[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = 0;
        if (col < n && j < K) vload<real_t, VEC>(v, B + (size_t)j * ldb + col);       // n % VEC == 0 (slab_ok)
        vstore<real_t, VEC>(Bp + ((size_t)slab * Kp + j) * W + lg * VEC, v);
    }
}

// grow-only per-device scratch for the packed copy of B
static void *slab_pack_workspace(size_t bytes, bool release = false)
{
    static thread_local void *ws[64] = {};
    static thread_local size_t cap[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (release) { if (ws[dev]) (void)hipFree(ws[dev]); ws[dev] = nullptr; cap[dev] = 0; return nullptr; }
    if (cap[dev] < bytes) {
        if (ws[dev]) (void)hipFree(ws[dev]);
        ws[dev] = nullptr; cap[dev] = 0;
        if (hipMalloc(&ws[dev], bytes) != hipSuccess) return nullptr;
        cap[dev] = bytes;
    }
    return ws[dev];
}

// per-device counters for the timing barrier (8 groups x 256 B), allocated once
static unsigned *slab_sync_workspace()
{
    static thread_local unsigned *ws[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!ws[dev] && hipMalloc((void **)&ws[dev], 8 * 64 * sizeof(unsigned)) != hipSuccess) ws[dev] = nullptr;
    return ws[dev];
}

template <typename real_t, int RPG>
static int launch_spmm_slab_rpg(int m, int n, int K, const int32_t *indptr, const int32_t *indices,
                                const double *values, const real_t *B, size_t ldb, real_t *C, size_t ldc,
                                int colmajor, int npanels, int wg_per_cu, int sync_mode, hipStream_t stream)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;
    constexpr int RB = SLAB_GROUPS * RPG;
    const int nslabs = (int)ceil_div(n, W);
    const int nrowblocks = (int)ceil_div(m, RB);
    if (npanels < 1) npanels = 1;
    const int panel_cols = (int)ceil_div(K > 0 ? K : 1, npanels);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    long long grid = (long long)cus * wg_per_cu;
    const long long total = (long long)nslabs * nrowblocks;
    if (grid > total + 7) grid = total + 7;
    grid = (grid / 8) * 8;
    if (grid < 8) grid = 8;
    const int c_vec_ok = colmajor && (ldc % VEC == 0) && ((uintptr_t)C % 16 == 0);
    unsigned *sync = slab_sync_workspace();
    if (!sync) sync_mode = 0;
    if (sync_mode) MX_HIP(hipMemsetAsync(sync, 0, 8 * 64 * sizeof(unsigned), stream));
    // slab-major copy of B (MXGPU_SLAB_PACK=0 disables): with B row-major a slab is 128 B out of every ldb*s
    // bytes — a power-of-two stride that lands on a fraction of the L2 channels
    size_t slab_stride = 0;
    int pack = 1;
    if (const char *e = getenv("MXGPU_SLAB_PACK")) pack = atoi(e);
    if (pack) {
        const size_t bytes = (size_t)nslabs * (size_t)K * W * sizeof(real_t);
        real_t *Bp = (real_t *)slab_pack_workspace(bytes);
        if (Bp) {
            const long long pieces = (long long)K * nslabs * SLAB_GROUP;
            const unsigned g = (unsigned)(ceil_div(pieces, 256) < 8192 ? ceil_div(pieces, 256) : 8192);
            hipLaunchKernelGGL((repack_slabs_kernel<real_t>), dim3(g), dim3(256), 0, stream, K, K, n, nslabs, B, ldb, Bp,
                               (const int *)nullptr);
            MX_LAUNCH_CHECK();
            B = Bp; ldb = W; slab_stride = (size_t)K * W;
        }
    }
    kt_begin(stream);
    if (colmajor)
        hipLaunchKernelGGL((spmm_slab_kernel<real_t, RPG, true>), dim3((unsigned)grid), dim3(SLAB_BLOCK), 0, stream,
                           m, n, indptr, indices, values, B, ldb, C, ldc, npanels, panel_cols, nslabs, nrowblocks,
                           c_vec_ok, sync, sync_mode, slab_stride);
    else
        hipLaunchKernelGGL((spmm_slab_kernel<real_t, RPG, false>), dim3((unsigned)grid), dim3(SLAB_BLOCK), 0, stream,
                           m, n, indptr, indices, values, B, ldb, C, ldc, npanels, panel_cols, nslabs, nrowblocks,
                           c_vec_ok, sync, sync_mode, slab_stride);
    kt_end(stream);
    MX_LAUNCH_CHECK();
    return 0;
}

template <typename real_t>
static int launch_spmm_slab(int m, int n, int K, const int32_t *indptr, const int32_t *indices,
                            const double *values, const real_t *B, size_t ldb, real_t *C, size_t ldc,
                            int colmajor, int npanels, int wg_per_cu, hipStream_t stream)
{
    // experiment knobs (tuning only): MXGPU_SLAB_SYNC 0 none / 1 per row-block / 2 per panel; MXGPU_SLAB_RPG 8 / 16
    int sync_mode = 2, rpg = 8;
    if (const char *e = getenv("MXGPU_SLAB_SYNC")) sync_mode = atoi(e);
    if (const char *e = getenv("MXGPU_SLAB_RPG")) rpg = atoi(e);
    if (npanels <= 1) sync_mode = 0;
    if (rpg == 16)
        return launch_spmm_slab_rpg<real_t, 16>(m, n, K, indptr, indices, values, B, ldb, C, ldc, colmajor, npanels,
                                                wg_per_cu, sync_mode, stream);
    return launch_spmm_slab_rpg<real_t, 8>(m, n, K, indptr, indices, values, B, ldb, C, ldc, colmajor, npanels,
                                           wg_per_cu, sync_mode, stream);
}

// =====================================================================================================
// v3 "planned panel sweep".
//
// PMC on v2 (profiles/r01_v2_*): with column panels + the XCD timing barrier the L2 hit rate only reaches
// 60 % because every (row, panel) visit re-reads the row's (j, a) chunk — with P panels the CSR arrays are
// streamed ~2P times per XCD and that traffic, not B, dominates and evicts the panel.  v3 fixes the data
// layout instead of the loop: a *plan* regroups A's entries by (octet of 8 row-bundles, panel) and
// interleaves the 8 bundles of an octet in batches of 8 steps (slot 64*batch + 8*g + u = step 8*batch + u of
// bundle g), so that
//   * one wavefront (8 lane groups = 8 bundles) reads 64 consecutive plan entries per 8 steps — every entry of A
//     is read exactly once per slab, coalesced, and reaches its lane group by a DPP row broadcast;
//   * entries of a bundle inside a panel are ordered by row, the group accumulates the current row in
//     registers and folds it into the bundle's accumulators in LDS when the row changes (only that group
//     touches those LDS rows: plain read-modify-write, no atomics);
//   * all workgroups of an XCD group stay close to the same panel (same code on statistically identical data;
//     optional timing barrier), whose slab-major copy of B
//     (K/P x 128 B, contiguous) fits the XCD's L2.
// Entry = int32 (col | local_row << 27; padding = zero row of the packed B, value 0) + f64 value; plan bytes ~ the CSR arrays (octet lengths rounded to 8 steps).
// Summation order: CSR order inside a (row, panel), panels added in ascending order — a regrouping of the
// reference's sequential sum (tolerance-level difference, not bitwise).  Works for unsorted rows too.
// =====================================================================================================
constexpr int PLAN_RB = 8;                         // rows per bundle (owned by one 8-lane group)
constexpr int PLAN_OCT_ROWS = PLAN_RB * 8;         // rows per octet (one wavefront)
// wavefronts per workgroup (template parameter WAVES): 16 = ONE 1024-thread workgroup with 128 KiB of LDS per CU,
// 8 = two 512-thread workgroups with 64 KiB each (one's epilogue overlaps the other's sweep), 4 = four.
constexpr int PLAN_MAXP = 64;
constexpr int PLAN_DEFAULT_WG_PER_CU = 1;
constexpr int PLAN_CHUNK = 4;                      // batches of 8 steps fetched per plan read (octets are whole chunks)
constexpr int PLAN_TAIL_SLOTS = 512;               // readable padding behind the last octet (2 chunks)
constexpr int PLAN_ROW_SHIFT = 27;                 // col < 2^27

// Plan construction.
// Sizing: an octet is as long as its longest bundle rounded up to whole chunks, and a bundle's length is
// indptr[r0 + 8] - indptr[r0], so the sizes (and the AUTO pad-ratio rule) come from indptr alone.  The scan of the
// octet lengths gives oct_off[] and the step total; the total and nnz go back to the host in one pinned copy.
// Fill: one 512-thread workgroup per octet, one wavefront per bundle.  The wavefront reads its bundle's entries once
// (coalesced, 64 per load, PLAN_LD loads in flight), counts them per panel, takes the prefix over the panels (the
// bundle's panel offsets) and places every entry at (panel offset + rank inside its panel, in CSR order).  Ranks come
// from a multisplit: ceil(log2 P) ballots of the panel's bits give each lane the mask of its peers, so the cost does
// not grow with P.  Octets of up to PLAN_STAGE_STEPS steps are assembled in LDS in their final slot order and
// written out with 16-byte stores; longer ones are scattered straight to global memory.
constexpr int PLAN_LD = 4;
constexpr int PLAN_STAGE_STEPS = 384;              // 384 x 64 slots x 12 B = 36 KiB of LDS: four workgroups per CU
constexpr int PLAN_PAD_NUM = 7, PLAN_PAD_DEN = 4;  // AUTO's pad rule: reject a plan of more than 1.75 x nnz + 65536 slots

// Accept the plan: it fits buffers of cap_slots slots and (pad_rule) is not padded beyond PLAN_PAD_NUM/DEN x nnz.
// The fill kernel takes this decision from the device-side total, the host repeats it from the read-back copy.
__host__ __device__ __forceinline__ bool plan_accept(long long total, long long nnz, long long cap_slots, int pad_rule)
{
    if (total < 0 || total * 8 + PLAN_TAIL_SLOTS > cap_slots) return false;
    return !(pad_rule && total * 8 * PLAN_PAD_DEN > nnz * PLAN_PAD_NUM + 65536LL * PLAN_PAD_DEN);
}

// col / panel_cols without the integer divide: float estimate (col < 2^25 is exact in float up to 2^24, so one
// correction step either way), clamped to the last panel
__device__ __forceinline__ int panel_of(int col, int panel_cols, float inv_pc, int npanels)
{
    int q = (int)((float)col * inv_pc);
    const int r = col - q * panel_cols;
    q += r >= panel_cols ? 1 : (r < 0 ? -1 : 0);
    return q < npanels ? q : npanels - 1;
}

// steps[oct] = longest bundle of the octet rounded up to whole chunks; one thread per bundle, 8 per octet
__global__ __launch_bounds__(256)
void plan_size_kernel(int m, int noct, const int32_t *__restrict__ indptr, int32_t *__restrict__ steps,
                      long long *__restrict__ nnz_out)
{
    const int b = blockIdx.x * 256 + threadIdx.x;                    // bundle; noct * 8 threads are live
    if (b == 0) *nnz_out = indptr[m];                                // rides back with the step total (one copy)
    int len = 0;
    if (b < noct * 8) {
        const int r0 = min(b * PLAN_RB, m), r1 = min(b * PLAN_RB + PLAN_RB, m);
        len = indptr[r1] - indptr[r0];
    }
    len = max(len, __shfl_xor(len, 1, 8));
    len = max(len, __shfl_xor(len, 2, 8));
    len = max(len, __shfl_xor(len, 4, 8));
    if (b < noct * 8 && (b & 7) == 0)
        steps[b >> 3] = (len + 8 * PLAN_CHUNK - 1) & ~(8 * PLAN_CHUNK - 1);    // whole chunks of 4 batches of 8 steps
}

// lanes whose key agrees with `key` on the low nbits bits, among the lanes in `valid` (bal[b] = ballot of key bit b)
__device__ __forceinline__ unsigned long long multisplit_peers(int key, const unsigned long long (&bal)[6], int nbits,
                                                                unsigned long long valid)
{
    unsigned long long peers = valid;
#pragma unroll
    for (int b = 0; b < 6; b++)
        if (b < nbits) peers &= ((key >> b) & 1) ? bal[b] : ~bal[b];
    return peers;
}

// Slot layout inside a batch of 8 steps: [bundle g][step u] — lane 8g+u of the sweep's reading wavefront holds bundle
// g's entry for step u, i.e. inside g's own lane group (intra-group DPP broadcast).  Step t of bundle g of an octet
// lands in slot (t & ~7) * 8 + g * 8 + (t & 7) of the octet.
__global__ __launch_bounds__(512, 8)
void plan_fill_kernel(int m, int npanels, int panel_cols, const int32_t *__restrict__ indptr,
                      const int32_t *__restrict__ indices, const double *__restrict__ values,
                      const int32_t *__restrict__ oct_off, int32_t *__restrict__ pcol, double *__restrict__ pval,
                      int noct, int pad_col, int32_t *__restrict__ step_off,
                      const long long *__restrict__ sizes, long long cap_slots, int pad_rule, int *__restrict__ go)
{
    __shared__ int32_t s_col[PLAN_STAGE_STEPS * 8];
    __shared__ double s_val[PLAN_STAGE_STEPS * 8];
    __shared__ int s_bpo[8][PLAN_MAXP];

    // sizes = [step total, nnz] from the sizing pass; a plan that does not fit (or that AUTO rejects) is not written
    // at all, and the repack of B behind this kernel is skipped with it
    const bool ok = plan_accept(sizes[0], sizes[1], cap_slots, pad_rule);
    if (blockIdx.x == 0 && threadIdx.x == 0) *go = ok ? 1 : 0;
    if (!ok) return;

    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int oct = blockIdx.x;
    const int row0 = oct * PLAN_OCT_ROWS + g * PLAN_RB;
    int rp[PLAN_RB + 1];                                             // the bundle's row pointers (wave-uniform)
#pragma unroll
    for (int r = 0; r <= PLAN_RB; r++) rp[r] = uniform(indptr[min(row0 + r, m)]);
    const int s = rp[0], e = rp[PLAN_RB];
    const int base = oct_off[oct];
    const int steps_oct = oct_off[oct + 1] - base;
    const bool stage = steps_oct <= PLAN_STAGE_STEPS;                // workgroup-uniform
    const float inv_pc = 1.0f / (float)panel_cols;
    const int nbits = npanels > 1 ? 32 - __clz(npanels - 1) : 0;
    const unsigned long long below = (1ULL << lane) - 1ULL;

    // The first PLAN_LD x 64 entries (all of a cfg2 bundle) stay in registers between the two passes; longer bundles
    // read the rest again in pass 2 (from L2: the workgroup read it moments before).
    int col0[PLAN_LD];
    double val0[PLAN_LD];
#pragma unroll
    for (int c = 0; c < PLAN_LD; c++) {
        const int k = s + 64 * c + lane;
        col0[c] = -1; val0[c] = 0.0;
        if (k < e) { col0[c] = indices[k]; val0[c] = values[k]; }
    }
    // ballots of the panel bits of one 64-entry chunk (pan < 0: no entry)
    auto split = [&](int pan, unsigned long long (&bal)[6]) -> unsigned long long {
#pragma unroll
        for (int b = 0; b < 6; b++)
            bal[b] = b < nbits ? __ballot(pan >= 0 && ((pan >> b) & 1)) : 0ULL;
        return __ballot(pan >= 0);
    };

    // pass 1: lane q counts the bundle's entries in panel q
    int mine = 0;
    for (int k0 = s; k0 < e; k0 += 64 * PLAN_LD) {
        int colv[PLAN_LD];
#pragma unroll
        for (int c = 0; c < PLAN_LD; c++) {
            const int k = k0 + 64 * c + lane;
            colv[c] = col0[c];
            if (k0 != s) colv[c] = k < e ? indices[k] : -1;
        }
#pragma unroll
        for (int c = 0; c < PLAN_LD; c++) {
            if (k0 + 64 * c >= e) break;                             // uniform
            const int pan = colv[c] >= 0 ? panel_of(colv[c], panel_cols, inv_pc, npanels) : -1;
            unsigned long long bal[6];
            const unsigned long long valid = split(pan, bal);
            if (lane < npanels) mine += __popcll(multisplit_peers(lane, bal, nbits, valid));
        }
    }
    // exclusive prefix over the panels (lanes 0..npanels-1): where panel q starts in the bundle's stream
    int incl = lane < npanels ? mine : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    int nextstep = incl - mine;                                      // lane q: next free step of panel q
    s_bpo[g][lane] = nextstep;

    auto put = [&](int t, int word, double v) {
        const int slot = (t & ~7) * 8 + g * 8 + (t & 7);
        if (stage) { s_col[slot] = word; s_val[slot] = v; }
        else { pcol[(size_t)base * 8 + slot] = word; pval[(size_t)base * 8 + slot] = v; }
    };

    // pass 2: place every entry at its panel's next step + its rank among the chunk's entries of that panel
    for (int k0 = s; k0 < e; k0 += 64 * PLAN_LD) {
        int colv[PLAN_LD];
        double av[PLAN_LD];
#pragma unroll
        for (int c = 0; c < PLAN_LD; c++) {
            const int k = k0 + 64 * c + lane;
            colv[c] = col0[c]; av[c] = val0[c];
            if (k0 != s) {
                colv[c] = -1; av[c] = 0.0;
                if (k < e) { colv[c] = indices[k]; av[c] = values[k]; }
            }
        }
#pragma unroll
        for (int c = 0; c < PLAN_LD; c++) {
            if (k0 + 64 * c >= e) break;                             // uniform
            const int k = k0 + 64 * c + lane;
            const int col = colv[c];
            int pan = -1, lrow = 0;
            if (col >= 0) {
                pan = panel_of(col, panel_cols, inv_pc, npanels);
#pragma unroll
                for (int r = 1; r < PLAN_RB; r++) lrow += k >= rp[r];
            }
            unsigned long long bal[6];
            const unsigned long long valid = split(pan, bal);
            const int start = __shfl(nextstep, pan < 0 ? 0 : pan, 64);
            if (pan >= 0) put(start + __popcll(multisplit_peers(pan, bal, nbits, valid) & below), col | (lrow << PLAN_ROW_SHIFT), av[c]);
            if (lane < npanels) nextstep += __popcll(multisplit_peers(lane, bal, nbits, valid));
        }
    }
    // Padding up to the octet's length: a no-op entry — value 0, column `pad_col` (the all-zero extra row of the
    // packed B), row = the bundle's last entry's row so that it does not even trigger a row switch.  0 * 0 added to
    // an accumulator that is never -0.0 leaves it unchanged bit for bit.
    int last_lrow = 0;
    if (e > s) {
#pragma unroll
        for (int r = 1; r < PLAN_RB; r++) last_lrow += (e - 1) >= rp[r];
    }
    for (int t = (e - s) + lane; t < steps_oct; t += 64) put(t, pad_col | (last_lrow << PLAN_ROW_SHIFT), 0.0);

    __syncthreads();
    // panel boundaries of the octet for the sweep's panel meetings: mean start of the panel over the 8 bundles
    if (g == 0 && lane < npanels) {
        int sum = 0;
#pragma unroll
        for (int gg = 0; gg < 8; gg++) sum += s_bpo[gg][lane];
        step_off[(size_t)oct * npanels + lane] = base + (lane == 0 ? 0 : sum / 8);
        if (oct == noct - 1 && lane == 0) step_off[(size_t)noct * npanels] = oct_off[noct];
    }
    if (stage) {
        // the octet's image is contiguous: slots [base * 8, (base + steps_oct) * 8), a multiple of 256 slots
        // starting on a 1 KiB (pcol) / 2 KiB (pval) boundary — 16 bytes per lane per store
        const int nslots = steps_oct * 8;
        int4 *gc = reinterpret_cast<int4 *>(pcol + (size_t)base * 8);
        const int4 *lc = reinterpret_cast<const int4 *>(s_col);
        for (int i = threadIdx.x; i < nslots / 4; i += 512) gc[i] = lc[i];
        using d2 = double __attribute__((ext_vector_type(2)));
        d2 *gv = reinterpret_cast<d2 *>(pval + (size_t)base * 8);
        const d2 *lv = reinterpret_cast<const d2 *>(s_val);
        for (int i = threadIdx.x; i < nslots / 2; i += 512) gv[i] = lv[i];
    }
    // PLAN_TAIL_SLOTS padding slots behind the last octet: the kernel's read-ahead runs two batches past an octet
    if (oct == noct - 1) {
        static_assert(PLAN_TAIL_SLOTS == 512, "one slot per thread of the last block");
        const size_t dst = (size_t)oct_off[noct] * 8 + threadIdx.x;
        pcol[dst] = pad_col;
        pval[dst] = 0.0;
    }
}

// broadcast lane U of every 8-lane group: row_newbcast takes lane n of each 16-lane DPP row; bank_mask restricts the
// write to the low / high half of the row (banks of 4 lanes), so two moves serve the two groups of a row
template <int U>
__device__ __forceinline__ int group8_dpp_bcast(int v)
{
    int t = __builtin_amdgcn_mov_dpp(v, 0x150 + U, 0xF, 0x3, false);      // lanes of the other half: don't care
    return __builtin_amdgcn_update_dpp(t, v, 0x150 + 8 + U, 0xF, 0xC, false);
}
template <int U>
__device__ __forceinline__ void plan_bcast(int pcw, double pvw, int &pc, double &pv)
{
    union { double d; int i[2]; } a, b;
    a.d = pvw;
    pc = group8_dpp_bcast<U>(pcw);
    b.i[0] = group8_dpp_bcast<U>(a.i[0]);
    b.i[1] = group8_dpp_bcast<U>(a.i[1]);
    pv = b.d;
}

// Fold a finished row's partial sums into its LDS accumulators.  Only this lane ever touches these words and one
// wavefront's LDS operations execute in order, so both forms are the same sequence of additions.  f64: two
// fire-and-forget ds_add_f64 (no return value, nothing to wait for; the read-modify-write cost an LDS round trip on
// ~70 % of the steps).  f32: read-modify-write of one 16-byte word (four ds_add_f32 measured 2.4x slower overall).
template <int VEC>
__device__ __forceinline__ void lds_fold(double *d, double (&acc)[VEC])
{
#pragma unroll
    for (int v = 0; v < VEC; v++) __hip_atomic_fetch_add(d + v, acc[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int VEC>
__device__ __forceinline__ void lds_fold(float *d, float (&acc)[VEC])
{
#pragma unroll
    for (int v = 0; v < VEC; v++) d[v] += acc[v];
}

// Profiling build only (make PROBE=1, never the library that ships): lane 0 of every wavefront sums wall_clock64()
// ticks (100 MHz) from the end of a batch to the completion of consume(0) of the next batch, separately for batches
// that ended (0) without and (1) with a panel meeting (then from leaving the meeting's barrier), and (2) from the end of a generation's stream loop to the
// first consume(0) of the next generation that waits for a B line.  Per XCD: [sum, count] x 3, then the wavefronts.
// The clock reads wait for lgkmcnt(0) twice per batch, so a probe build is a few percent slower than the real one.
#ifdef MX_SWEEP_PROBE
__device__ unsigned long long g_sweep_probe[8][8];
#define MX_PROBE(...) __VA_ARGS__
#else
#define MX_PROBE(...)
#endif

// main kernel
template <typename real_t, bool COLMAJOR, int PLAN_WAVES>
__global__ __launch_bounds__(PLAN_WAVES * 64)
void spmm_plan_kernel(int m, int n, int npanels, const int32_t *__restrict__ step_off,
                      const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                      const real_t *__restrict__ Bp, size_t slab_stride,
                      real_t *__restrict__ C, size_t ldc, int nslabs, int ngens, int noct, int pad_col,
                      unsigned *__restrict__ sync_ctr, int sync_mode)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;
    constexpr int U = 8;                                            // plan steps in flight per wavefront
    constexpr int PLAN_WG_ROWS = PLAN_OCT_ROWS * PLAN_WAVES;        // rows per workgroup generation
    // accumulator rows are padded by 8 (f64) / 16 (f32) bytes: the column-major epilogue reads one column of 64
    // consecutive rows per instruction, which at a 128-byte stride would hit a single LDS bank pair
    constexpr int S = W + 16 / (int)sizeof(real_t) / 2;
    __shared__ real_t accs[PLAN_WG_ROWS * S];                       // 16 waves: 1024 rows x 136 B = 136 KiB

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 3, lg = lane & 7;
    const int xcd = blockIdx.x & 7, wg = blockIdx.x >> 3, nwg = gridDim.x >> 3;
    const long long total = (long long)nslabs * ngens;
    const long long lo = total * xcd / 8, hi = total * (xcd + 1) / 8;
    const int niter = (int)((hi - lo + nwg - 1) / nwg);
    unsigned *const my_ctr = sync_ctr + xcd * 64;
    real_t *const my_oct = accs + (size_t)wave * PLAN_OCT_ROWS * S;                     // this wavefront's 64 rows
    real_t *const my_rows = my_oct + (size_t)g * PLAN_RB * S + lg * VEC;                // this group's bundle
    MX_PROBE(long long pr_t = 0; int pr_kind = 0; unsigned long long pr_sum[3] = {0, 0, 0}; unsigned pr_cnt[3] = {0, 0, 0};)

    for (int it = 0; it < niter; it++) {
        const long long item_raw = lo + wg + (long long)it * nwg;
        const bool have = item_raw < hi;
        const long long item = have ? item_raw : lo;
        const int slab = (int)(item / ngens), gen = (int)(item % ngens);
        const int oct = gen * PLAN_WAVES + wave;
        const bool oct_ok = have && oct < noct;
        // slab base is wave-uniform (scalar registers), the per-lane part is a 32-bit byte offset: one VALU op per
        // address.  A slab is K x 128 B < 4 GiB because K < 2^27... checked on the host (K * 128 < 2^32).
        const char *__restrict__ Bbase = reinterpret_cast<const char *>(Bp + (size_t)slab * slab_stride);
        const unsigned lane_off = (unsigned)(lg * VEC * sizeof(real_t));

        // A wavefront's accumulator rows are touched by that wavefront only (zeroing, folds, epilogue): no
        // workgroup-wide synchronisation around a generation, the wavefronts only meet at the panel boundaries.
        for (int i = lane; i < PLAN_OCT_ROWS * S; i += 64) my_oct[i] = 0;
        if (sync_mode > 0) __syncthreads();                          // locality only: start the first panel together

        // One continuous, software-pipelined stream over the octet's entries of ALL panels (they are contiguous in
        // the plan).  Panel boundaries only matter for locality: when the stream crosses one, the 16 waves of the
        // CU's single workgroup meet at a __syncthreads: a bare s_barrier, nothing is loaded or waited for there, so
        // the B lines and the plan chunk in flight stay in flight (the boundaries come out of a register, see
        // so_row below).  Across the 32 CUs of the XCD group there is ONE global timing barrier per
        // generation (32 pollers per counter); in between the CUs run identical code on statistically identical
        // data and drift by a fraction of a panel.
        {
            if (sync_mode >= 2) xcd_timing_barrier(my_ctr, (unsigned)(it + 1) * (unsigned)nwg);
            // The octet's whole row of step_off is read here, once: lane p holds the start of panel p (npanels <= 64
            // lanes), the end of the last panel sits in a second register.  Every panel boundary the stream meets
            // later is a v_readlane of that register: a load at the meeting would have to be waited for with
            // vmcnt(0), and vector loads return in order, so that wait would drain the B lines and the plan chunk in
            // flight.
            int so_row = 0, so_end = 0;
            if (oct_ok) {
                if (lane < npanels) so_row = step_off[(size_t)oct * npanels + lane];
                so_end = step_off[(size_t)oct * npanels + npanels];
            }
            const int sbeg = __builtin_amdgcn_readfirstlane(so_row);   // wave-uniform: keep the loop control scalar
            const int send = __builtin_amdgcn_readfirstlane(so_end);
            int next_b = npanels > 1 ? __builtin_amdgcn_readlane(so_row, 1) : send;
            int p = 0;
            int cur = 0;
            real_t acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[v] = 0;
            // A batch = U = 8 steps = 64 consecutive plan slots, laid out [bundle g][step u]: lane l reads slot
            // (8 s + l) — one fully coalesced 256 B + 512 B read per batch — and step u's entry is broadcast from
            // lane u of each group.  (Reading the slot from all 8 lanes of a group instead costs the texture
            // addresser 8x the lane-bytes: PMC showed TA_BUSY 71 % and the kernel TA-bound.)
            // Every slot is a valid entry: padding is (zero row of B, value 0, current row) — no per-step validity
            // test, no clamp.
            static_assert(U == 8, "one batch = one wavefront of plan slots");
            static_assert(W * sizeof(real_t) == 128, "slab line");
            auto b_offset = [&](int c) -> unsigned {                // the row bits (27..29) fall off the 32-bit shift
                return ((unsigned)c * (unsigned)(W * sizeof(real_t))) + lane_off;
            };
            // The plan slots are fetched a CHUNK (PLAN_CHUNK = 4 batches = 32 steps) at a time, one chunk ahead.
            // Vector loads return in order, so a slot read that misses to HBM (the plan is a pure stream) holds back
            // every younger B-line load behind it; fetching one batch per iteration put that full latency into every
            // iteration (measured: 1.95 us per 8 steps per wave, whatever the locality of B).  Now it is paid once
            // per 32 steps.  The last read-ahead of an octet runs one chunk past it (the next octet's slots / the
            // padding behind the last octet): it is fetched and dropped, never used.  Nothing of the NEXT generation
            // is in flight when this one's stream ends: the turnover (last batch, epilogue, zeroing, step_off row,
            // first chunk, first batch of B lines, each waited for in turn) measures 11 us per generation and
            // wavefront, see DESIGN.md 4.1.
            int rc[PLAN_CHUNK], rn[PLAN_CHUNK];
            double rv[PLAN_CHUNK], rvn[PLAN_CHUNK];
            auto load_chunk = [&](int step, int (&c)[PLAN_CHUNK], double (&v)[PLAN_CHUNK]) {
                const long long e = (long long)step * 8 + lane;
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) { c[k] = pcol[e + 64 * k]; v[k] = pval[e + 64 * k]; }
            };
            int pc[U];
            double pv[U];
            real_t b[U][VEC];
#pragma unroll
            for (int u = 0; u < U; u++) {
                pc[u] = 0;
                pv[u] = 0.0;
#pragma unroll
                for (int v = 0; v < VEC; v++) b[u][v] = 0;
            }
            // consume step u of the batch in (pc, pv, b): row switch -> fold the finished row into LDS, then FMA
            auto consume = [&](int u) {
                const int lrow = (int)((unsigned)pc[u] >> PLAN_ROW_SHIFT);
                if (lrow != cur) {
                    lds_fold<VEC>(my_rows + cur * S, acc);
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[v] = 0;
                    cur = lrow;
                }
                const real_t a = (real_t)pv[u];
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[v] = mx_fma(a, b[u][v], acc[v]);
                // keep the reload BEHIND the FMAs that read the old line (and the FMAs where they are): letting the two
                // cross renames b[u] and ends in a register copy at the back edge that waits for every load in flight
#pragma unroll
                for (int v = 0; v < VEC; v++) asm volatile("" : "+v"(acc[v]));
                __builtin_amdgcn_sched_barrier(0);
            };
            if (send > sbeg) {
                load_chunk(sbeg, rc, rv);
                // the first chunk has to be there before anything can start; with it complete at loop entry the
                // compiler's vmcnt bookkeeping is exact on both edges of the loop
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) asm volatile("" : "+v"(rc[k]), "+v"(rv[k]));
            }
            // Consumption lags one batch behind the broadcast + B-line load: while batch t is consumed step by step,
            // the line of the same step of batch t+1 is requested into the registers the FMA just released, so 8
            // B-line loads per wavefront are in flight all the time.  The first pass consumes the no-op batch set up
            // above, the last batch is consumed after the loop.
            for (int s = sbeg; s < send; s += U * PLAN_CHUNK) {      // sbeg, send are wave-uniform
                load_chunk(s + U * PLAN_CHUNK, rn, rvn);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) {
#define MX_PLAN_STEP(UU)                                                                                              \
                    consume(UU);                                                                                      \
                    plan_bcast<UU>(rc[k], rv[k], pc[UU], pv[UU]);                                                     \
                    vload<real_t, VEC>(b[UU], reinterpret_cast<const real_t *>(Bbase + b_offset(pc[UU])));            \
                    __builtin_amdgcn_sched_barrier(0);
                    MX_PLAN_STEP(0)
                    MX_PROBE(if (pr_kind && !(pr_kind == 3 && s == sbeg && k == 0)) {   // that first batch is the no-op one
                        const unsigned long long dt = (unsigned long long)(wall_clock64() - pr_t);
                        _Pragma("unroll") for (int j = 0; j < 3; j++)
                            if (pr_kind == j + 1) { pr_sum[j] += dt; pr_cnt[j]++; }
                        pr_kind = 0;
                    })
                    MX_PLAN_STEP(1) MX_PLAN_STEP(2) MX_PLAN_STEP(3)
                    MX_PLAN_STEP(4) MX_PLAN_STEP(5) MX_PLAN_STEP(6) MX_PLAN_STEP(7)
#undef MX_PLAN_STEP
                    MX_PROBE(bool pr_met = false;)
                    if (sync_mode > 0) {
                        const int sn = s + U * k;                   // steps consumed so far
                        while (p < npanels - 1 && sn >= next_b) {   // the stream moved into the next panel
                            p++;
                            __syncthreads();
                            MX_PROBE(pr_met = true; if (pr_kind != 3) pr_t = wall_clock64();)
                            next_b = p < npanels - 1 ? __builtin_amdgcn_readlane(so_row, p + 1) : send;
                        }
                    }
                    MX_PROBE(if (pr_kind != 3) { pr_kind = pr_met ? 2 : 1; if (!pr_met) pr_t = wall_clock64(); })
                }
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) { rc[k] = rn[k]; rv[k] = rvn[k]; }
            }
            MX_PROBE(if (send > sbeg) { pr_kind = 3; pr_t = wall_clock64(); })
#pragma unroll
            for (int u = 0; u < U; u++) consume(u);
            lds_fold<VEC>(my_rows + cur * S, acc);
            if (sync_mode > 0)
                for (; p < npanels - 1; p++) __syncthreads();           // every wave meets npanels-1 times per generation
        }

        // each wavefront writes the 64 x W tile of C it accumulated (streaming stores: C is not read again)
        if (oct_ok) {
            const int row_base = gen * PLAN_WG_ROWS + wave * PLAN_OCT_ROWS;
            const int ncols = min(W, n - slab * W);
            if constexpr (!COLMAJOR) {
#pragma unroll
                for (int rr = 0; rr < PLAN_OCT_ROWS / 8; rr++) {
                    const int r = rr * 8 + g;
                    const int row = row_base + r;
                    if (row < m && lg * VEC < ncols) {
                        real_t t[VEC];
#pragma unroll
                        for (int v = 0; v < VEC; v++) t[v] = my_oct[(size_t)r * S + lg * VEC + v];
                        vstore_nt<real_t, VEC>(C + (size_t)row * ldc + slab * W + lg * VEC, t);
                    }
                }
            } else {
                // lane = row: one 512-byte (f64) segment of an output column per store instruction
                const int row = row_base + lane;
                if (row < m) {
                    for (int c = 0; c < ncols; c++)
                        __builtin_nontemporal_store(my_oct[(size_t)lane * S + c], &C[(size_t)(slab * W + c) * ldc + row]);
                }
            }
        }
    }
    MX_PROBE(if (lane == 0) {
        for (int j = 0; j < 3; j++) {
            atomicAdd(&g_sweep_probe[xcd][2 * j], pr_sum[j]);
            atomicAdd(&g_sweep_probe[xcd][2 * j + 1], (unsigned long long)pr_cnt[j]);
        }
        atomicAdd(&g_sweep_probe[xcd][6], 1ULL);
    })
}

}  // namespace mx

// device-resident plan of one CSR matrix (see the v3 comment above)
struct mx_spmm_plan {
    int m = 0, K = 0, npanels = 0, panel_cols = 0, noct = 0;
    long long total_steps = 0;
    long long nnz = 0;
    int32_t *step_off = nullptr; size_t step_off_cap = 0;
    int32_t *pcol = nullptr;     size_t pcol_cap = 0;
    double *pval = nullptr;      size_t pval_cap = 0;
    void *scratch = nullptr;     size_t scratch_cap = 0;       // steps + oct_off + read-back + scan workspace (build only)
    bool ready = false;                                            // false: sized but not filled (rejected by AUTO)
    // a build between plan_begin and plan_end: the CSR it reads, device-side sizes / go flag, the capacity the fill saw
    bool pending = false;
    const int32_t *indptr = nullptr, *indices = nullptr;
    const double *values = nullptr;
    const int32_t *oct_off = nullptr;
    const long long *sizes = nullptr;
    int *go = nullptr;
    long long fill_cap = 0;
    int pad_rule = 0;
};

namespace mx {

static thread_local mx_spmm_plan *g_auto_plan = nullptr;

static int grow(void **p, size_t *cap, size_t bytes)
{
    if (*cap >= bytes && *p) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    MX_HIP(hipMalloc(p, bytes ? bytes : 16));
    *cap = bytes;
    return 0;
}

// pinned landing zone + event for the one host read-back of a plan build
struct PlanReadback {
    long long *host = nullptr;                                      // [0] total steps, [1] nnz (int32 in the low half)
    hipEvent_t ev = nullptr;
};
static PlanReadback *plan_readback()
{
    static thread_local PlanReadback rb;
    if (!rb.host) {
        if (hipHostMalloc((void **)&rb.host, 2 * sizeof(long long), hipHostMallocDefault) != hipSuccess) { rb.host = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(rb.host); rb.host = nullptr; return nullptr; }
    }
    return &rb;
}

// Building a plan is split in two so that the GPU never waits for the host.  plan_begin enqueues the sizing pass, the
// scan, the one read-back of [step total, nnz] and the fill, which decides on the device-side total whether the plan
// fits the current (grow-only) buffers; the caller may enqueue more work behind it (AUTO packs B).  plan_end waits for
// the read-back, takes the same decision on the host and, when the buffers were too small (typically the first call),
// grows them and fills again (*refilled = true).
// pad_rule: AUTO's rejection of plans that would hold more than 1.75 x nnz slots (rows of very uneven length pad the
// 8-way interleave: an octet is as long as its longest bundle) — pl->ready then stays false and nothing is written.
static int plan_begin(mx_spmm_plan *pl, int m, int K, const int32_t *indptr, const int32_t *indices,
                      const double *values, int npanels, hipStream_t st, int pad_rule = 0)
{
    pl->ready = false;
    pl->pending = false;
    MX_REQUIRE(K < (1 << 25), "spmm plan: more than 2^25 columns (32-bit slab offsets)");
    // measured (cfg2, whole call): P = 8 (1.6 MB panels) 2.10 ms, P = 6 2.12 ms, P = 5 2.13 ms — the build no longer
    // depends on P, so the sweep's best panel size is the default
    if (npanels <= 0) npanels = pick_panels(K, (size_t)1600 << 10);
    if (npanels > PLAN_MAXP) npanels = PLAN_MAXP;
    pl->m = m; pl->K = K; pl->npanels = npanels;
    pl->panel_cols = (int)ceil_div(K > 0 ? K : 1, npanels);
    pl->noct = (int)ceil_div(m, PLAN_OCT_ROWS);
    pl->total_steps = 0; pl->nnz = 0;
    if (m == 0) { pl->ready = true; return 0; }                     // nothing to plan (and no zero-sized launches)
    const size_t nop = (size_t)pl->noct * npanels;
    const size_t al = 255;
    const size_t steps_b = (((size_t)pl->noct * 4) + al) & ~al;
    const size_t octoff_b = ((((size_t)pl->noct + 1) * 4) + al) & ~al;
    const size_t rb_b = 256;                                        // [total steps][nnz][go flag], read back in one copy
    if (grow(&pl->scratch, &pl->scratch_cap, steps_b + octoff_b + rb_b + scan_workspace_bytes((int64_t)pl->noct))) return 1;
    if (grow((void **)&pl->step_off, &pl->step_off_cap, (nop + 1) * 4)) return 1;
    int32_t *steps = (int32_t *)pl->scratch;
    int32_t *oct_off = (int32_t *)((char *)steps + steps_b);
    long long *rb_dev = (long long *)((char *)oct_off + octoff_b);
    void *scan_ws = (char *)rb_dev + rb_b;
    const unsigned sblocks = (unsigned)ceil_div((long long)pl->noct * 8, 256);
    hipLaunchKernelGGL(plan_size_kernel, dim3(sblocks), dim3(256), 0, st, m, pl->noct, indptr, steps, rb_dev + 1);
    MX_LAUNCH_CHECK();
    if (exclusive_scan_i32(steps, (int64_t)pl->noct, oct_off, (int64_t *)rb_dev, scan_ws, st)) return 1;
    PlanReadback *rb = plan_readback();
    MX_REQUIRE(rb, "spmm plan: cannot allocate the pinned read-back buffer");
    MX_HIP(hipMemcpyAsync(rb->host, rb_dev, 2 * sizeof(long long), hipMemcpyDeviceToHost, st));
    MX_HIP(hipEventRecord(rb->ev, st));
    pl->indptr = indptr; pl->indices = indices; pl->values = values;
    pl->oct_off = oct_off; pl->sizes = rb_dev; pl->go = (int *)(rb_dev + 2);
    pl->pad_rule = pad_rule;
    pl->fill_cap = (long long)std::min(pl->pcol_cap / 4, pl->pval_cap / 8);
    hipLaunchKernelGGL(plan_fill_kernel, dim3((unsigned)pl->noct), dim3(512), 0, st, m, npanels, pl->panel_cols, indptr,
                       indices, values, oct_off, pl->pcol, pl->pval, pl->noct, K, pl->step_off, pl->sizes, pl->fill_cap,
                       pad_rule, pl->go);
    MX_LAUNCH_CHECK();
    pl->pending = true;
    return 0;
}

static int plan_end(mx_spmm_plan *pl, hipStream_t st, bool *refilled = nullptr)
{
    if (refilled) *refilled = false;
    if (!pl->pending) return 0;                                     // m == 0 (ready) or plan_begin failed
    pl->pending = false;
    PlanReadback *rb = plan_readback();
    MX_HIP(hipEventSynchronize(rb->ev));
    const long long total = rb->host[0];
    pl->nnz = (int32_t)rb->host[1];
    MX_REQUIRE(total >= 0 && total * 8 <= (long long)INT_MAX * 4LL, "spmm plan: too many steps (%lld)", total);
    MX_REQUIRE(total <= (long long)INT_MAX, "spmm plan: step offsets exceed int32");
    pl->total_steps = total;
    if (plan_accept(total, pl->nnz, pl->fill_cap, pl->pad_rule)) { pl->ready = true; return 0; }   // the fill wrote it
    if (plan_accept(total, pl->nnz, LLONG_MAX, pl->pad_rule) == false) return 0;                    // rejected by AUTO
    const size_t slots = (size_t)total * 8 + PLAN_TAIL_SLOTS;
    if (grow((void **)&pl->pcol, &pl->pcol_cap, slots * 4)) return 1;
    if (grow((void **)&pl->pval, &pl->pval_cap, slots * 8)) return 1;
    pl->fill_cap = (long long)std::min(pl->pcol_cap / 4, pl->pval_cap / 8);
    hipLaunchKernelGGL(plan_fill_kernel, dim3((unsigned)pl->noct), dim3(512), 0, st, pl->m, pl->npanels, pl->panel_cols,
                       pl->indptr, pl->indices, pl->values, pl->oct_off, pl->pcol, pl->pval, pl->noct, pl->K, pl->step_off,
                       pl->sizes, pl->fill_cap, pl->pad_rule, pl->go);
    MX_LAUNCH_CHECK();
    pl->ready = true;
    if (refilled) *refilled = true;
    return 0;
}

// Optional HIP-event ring around the dominant kernel of every SpMM launch (bench.py's roofline figure): events sit
// on the launch stream right before / after the kernel, nothing else in between.
struct KernelTimer {
    static constexpr int N = 256;
    hipEvent_t a[N], b[N];
    bool made = false, on = false;
    int count = 0;
};
static thread_local KernelTimer g_kt;
static void kt_begin(hipStream_t st)
{
    if (!g_kt.on || g_kt.count >= KernelTimer::N) return;
    if (!g_kt.made) { for (int i = 0; i < KernelTimer::N; i++) { (void)hipEventCreate(&g_kt.a[i]); (void)hipEventCreate(&g_kt.b[i]); } g_kt.made = true; }
    (void)hipEventRecord(g_kt.a[g_kt.count], st);
}
static void kt_end(hipStream_t st)
{
    if (!g_kt.on || g_kt.count >= KernelTimer::N) return;
    (void)hipEventRecord(g_kt.b[g_kt.count], st);
    g_kt.count++;
}

// slab-major copy of B with one extra all-zero row (index K) per slab: the plan's padding slots point at it
template <typename real_t>
static int plan_repack(int K, int n, const real_t *B, size_t ldb, hipStream_t st, real_t **Bp_out, const int *go = nullptr)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;
    const int nslabs = (int)ceil_div(n, W);
    const int Kp = K + 1;
    real_t *Bp = (real_t *)slab_pack_workspace((size_t)nslabs * (size_t)Kp * W * sizeof(real_t));
    MX_REQUIRE(Bp, "spmm plan: cannot allocate the packed copy of B");
    const long long pieces = (long long)Kp * nslabs * SLAB_GROUP;
    const unsigned gsz = (unsigned)(ceil_div(pieces, 256) < 8192 ? ceil_div(pieces, 256) : 8192);
    hipLaunchKernelGGL((repack_slabs_kernel<real_t>), dim3(gsz), dim3(256), 0, st, K, Kp, n, nslabs, B, ldb, Bp, go);
    MX_LAUNCH_CHECK();
    *Bp_out = Bp;
    return 0;
}

template <typename real_t>
static int plan_run(const mx_spmm_plan *pl, int n, const real_t *B, size_t ldb, real_t *C, size_t ldc, int colmajor,
                    int wg_per_cu, int sync_mode, hipStream_t st, const real_t *Bp = nullptr)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    constexpr int W = SLAB_GROUP * VEC;
    const int m = pl->m, K = pl->K;
    const int nslabs = (int)ceil_div(n, W);
    const int Kp = K + 1;
    if (!Bp) {                                                       // else the caller packed B (AUTO, behind the fill)
        real_t *packed = nullptr;
        if (plan_repack<real_t>(K, n, B, ldb, st, &packed)) return 1;
        Bp = packed;
    }
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    if (wg_per_cu != 1 && wg_per_cu != 2 && wg_per_cu != 4) wg_per_cu = PLAN_DEFAULT_WG_PER_CU;
    const int waves = 16 / wg_per_cu;
    const int ngens = (int)ceil_div(m, PLAN_OCT_ROWS * waves);
    long long grid = (long long)cus * wg_per_cu;
    const long long total = (long long)nslabs * ngens;
    if (grid > total + 7) grid = total + 7;
    grid = (grid / 8) * 8;
    if (grid < 8) grid = 8;
    unsigned *sync = slab_sync_workspace();
    if (!sync || pl->npanels <= 1) sync_mode = 0;
    if (sync_mode >= 2) MX_HIP(hipMemsetAsync(sync, 0, 8 * 64 * sizeof(unsigned), st));   // counters of the XCD timing barrier
    kt_begin(st);
#define MX_PLAN_LAUNCH(CM, WV)                                                                                           \
    hipLaunchKernelGGL((spmm_plan_kernel<real_t, CM, WV>), dim3((unsigned)grid), dim3(WV * 64), 0, st, m, n, pl->npanels, \
                       pl->step_off, pl->pcol, pl->pval, Bp, (size_t)Kp * W, C, ldc, nslabs, ngens, pl->noct, K,         \
                       sync, sync_mode)
    if (colmajor) {
        if (waves == 16) MX_PLAN_LAUNCH(true, 16); else if (waves == 8) MX_PLAN_LAUNCH(true, 8); else MX_PLAN_LAUNCH(true, 4);
    } else {
        if (waves == 16) MX_PLAN_LAUNCH(false, 16); else if (waves == 8) MX_PLAN_LAUNCH(false, 8); else MX_PLAN_LAUNCH(false, 4);
    }
#undef MX_PLAN_LAUNCH
    kt_end(st);
    MX_LAUNCH_CHECK();
    return 0;
}

// can the slab kernel take these operands?  (16-B aligned rows of B, whole vectors per row;
// row-major C additionally needs 16-B aligned rows of C)
template <typename real_t>
static bool slab_ok(int n, const real_t *B, size_t ldb, const real_t *C, size_t ldc, int colmajor)
{
    constexpr int VEC = 16 / (int)sizeof(real_t);
    if (n < VEC || n % VEC || ldb % VEC || (uintptr_t)B % 16) return false;
    if (!colmajor && (ldc % VEC || (uintptr_t)C % 16)) return false;
    return true;
}

}  // namespace mx

extern "C" int mxd_spmm_plan_create(int m, int K, const int32_t *indptr, const int32_t *indices, const double *values,
                                    int npanels, void *stream, mx_spmm_plan **plan_out)
{
    MX_REQUIRE(plan_out && m >= 0 && K >= 0, "mxd_spmm_plan_create: bad arguments");
    mx_spmm_plan *pl = *plan_out ? *plan_out : new (std::nothrow) mx_spmm_plan();      // pass an old plan to reuse its buffers
    MX_REQUIRE(pl, "out of host memory");
    const hipStream_t st = mx::as_stream(stream);
    if (mx::plan_begin(pl, m, K, indptr, indices, values, npanels, st) || mx::plan_end(pl, st)) {
        if (!*plan_out) { mxd_spmm_plan_destroy(pl); }
        return 1;
    }
    *plan_out = pl;
    return 0;
}

extern "C" int mxd_spmm_plan_destroy(mx_spmm_plan *pl)
{
    if (!pl) return 0;
    if (pl->step_off) (void)hipFree(pl->step_off);
    if (pl->pcol) (void)hipFree(pl->pcol);
    if (pl->pval) (void)hipFree(pl->pval);
    if (pl->scratch) (void)hipFree(pl->scratch);
    delete pl;
    return 0;
}

extern "C" int mxd_spmm_plan_info(const mx_spmm_plan *pl, int *npanels, int64_t *padded_entries)
{
    MX_REQUIRE(pl, "mxd_spmm_plan_info: null plan");
    if (npanels) *npanels = pl->npanels;
    if (padded_entries) *padded_entries = pl->total_steps * 8;
    return 0;
}

// the plan's arrays as the sweep reads them: step_off[noct * npanels + 1], pcol / pval[padded_entries + 512 tail slots]
extern "C" int mxd_spmm_plan_copy_to_host(const mx_spmm_plan *pl, int32_t *step_off, int32_t *pcol, double *pval,
                                          void *stream)
{
    MX_REQUIRE(pl && step_off && pcol && pval, "mxd_spmm_plan_copy_to_host: null pointer");
    MX_REQUIRE(pl->ready, "mxd_spmm_plan_copy_to_host: the plan was sized but not built");
    if (pl->m == 0) return 0;
    const hipStream_t st = mx::as_stream(stream);
    const size_t nso = (size_t)pl->noct * pl->npanels + 1;
    const size_t slots = (size_t)pl->total_steps * 8 + mx::PLAN_TAIL_SLOTS;
    MX_HIP(hipMemcpyAsync(step_off, pl->step_off, nso * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipMemcpyAsync(pcol, pl->pcol, slots * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipMemcpyAsync(pval, pl->pval, slots * sizeof(double), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    return 0;
}

static thread_local const char *g_last_spmm_kernel = "none";

// frees this thread's grow-only scratch (AUTO's plan, the slab-major copy of B); they are re-created on demand
extern "C" int mxd_release_workspaces(void)
{
    if (mx::g_auto_plan) { mxd_spmm_plan_destroy(mx::g_auto_plan); mx::g_auto_plan = nullptr; }
    mx::slab_pack_workspace(0, true);
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

extern "C" int mxd_spmm_plan_run(const mx_spmm_plan *pl, int n, const void *B, size_t ldb, void *C, size_t ldc,
                                 int dense_dtype, int colmajor_out, int wg_per_cu, int sync_mode, void *stream)
{
    MX_REQUIRE(pl && n >= 0, "mxd_spmm_plan_run: bad arguments");
    MX_REQUIRE(pl->ready, "mxd_spmm_plan_run: the plan was sized but not built");
    if (pl->m == 0 || n == 0) return 0;
    MX_REQUIRE(B && C, "mxd_spmm_plan_run: null pointer");
    hipStream_t st = mx::as_stream(stream);
    if (sync_mode < 0) sync_mode = 1;       // panel meetings inside the CU's workgroup; 2 adds one XCD barrier per generation
    g_last_spmm_kernel = "spmm_plan_kernel";
    if (dense_dtype == MX_F64) {
        MX_REQUIRE(mx::slab_ok<double>(n, (const double *)B, ldb, (const double *)C, ldc, colmajor_out),
                   "mxd_spmm_plan_run: operands do not meet the 16-byte alignment rules");
        return mx::plan_run<double>(pl, n, (const double *)B, ldb, (double *)C, ldc, colmajor_out, wg_per_cu, sync_mode, st);
    }
    if (dense_dtype == MX_F32) {
        MX_REQUIRE(mx::slab_ok<float>(n, (const float *)B, ldb, (const float *)C, ldc, colmajor_out),
                   "mxd_spmm_plan_run: operands do not meet the 16-byte alignment rules");
        return mx::plan_run<float>(pl, n, (const float *)B, ldb, (float *)C, ldc, colmajor_out, wg_per_cu, sync_mode, st);
    }
    return mx::set_error("mxd_spmm_plan_run: unsupported dense dtype %d", dense_dtype);
}

extern "C" const char *mxd_spmm_last_kernel(void) { return g_last_spmm_kernel; }

#ifdef MX_SWEEP_PROBE
// probe builds only (tools/sweep_probe.py): copies the 8 x 8 counters of spmm_plan_kernel out and clears them
extern "C" int mxd_spmm_sweep_probe(unsigned long long *out64)
{
    static const unsigned long long zeros[64] = {};
    MX_HIP(hipDeviceSynchronize());
    MX_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(mx::g_sweep_probe), sizeof(zeros)));
    MX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mx::g_sweep_probe), zeros, sizeof(zeros)));
    return 0;
}
#endif

extern "C" int mxd_spmm_csr_dense_ex(int m, int n, int K,
                                     const int32_t *indptr, const int32_t *indices, const double *values,
                                     const void *B, size_t ldb, void *C, size_t ldc,
                                     int dense_dtype, int colmajor_out, int algo, int rows_sorted,
                                     int npanels, int wg_per_cu, void *stream)
{
    MX_REQUIRE(m >= 0 && n >= 0 && K >= 0, "mxd_spmm_csr_dense_ex: negative dimension");
    if (m == 0 || n == 0) return 0;
    MX_REQUIRE(indptr && B && C, "mxd_spmm_csr_dense_ex: null pointer");
    MX_REQUIRE(dense_dtype == MX_F64 || dense_dtype == MX_F32, "mxd_spmm_csr_dense_ex: unsupported dense dtype %d", dense_dtype);
    hipStream_t st = mx::as_stream(stream);
    const bool ok = dense_dtype == MX_F64
        ? mx::slab_ok<double>(n, (const double *)B, ldb, (const double *)C, ldc, colmajor_out)
        : mx::slab_ok<float>(n, (const float *)B, ldb, (const float *)C, ldc, colmajor_out);
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
        const bool f64 = dense_dtype == MX_F64;
        void *Bp = nullptr;
        auto pack = [&](const int *go) {
            return f64 ? mx::plan_repack<double>(K, n, (const double *)B, ldb, st, (double **)&Bp, go)
                       : mx::plan_repack<float>(K, n, (const float *)B, ldb, st, (float **)&Bp, go);
        };
        if (pack(auto_plan->go)) return 1;
        bool refilled = false;
        if (mx::plan_end(auto_plan, st, &refilled)) return 1;
        if (auto_plan->ready) {
            if (refilled && pack(nullptr)) return 1;                    // buffers grown: filled again, pack B behind it
            g_last_spmm_kernel = "spmm_plan_kernel";
            return f64 ? mx::plan_run<double>(auto_plan, n, (const double *)B, ldb, (double *)C, ldc, colmajor_out, 0, 1,
                                              st, (const double *)Bp)
                       : mx::plan_run<float>(auto_plan, n, (const float *)B, ldb, (float *)C, ldc, colmajor_out, 0, 1, st,
                                             (const float *)Bp);
        }
        algo = MX_SPMM_ROWWAVE;
    }
    if (algo == MX_SPMM_SLAB) {
        MX_REQUIRE(ok, "mxd_spmm_csr_dense_ex: operands do not meet the slab kernel's 16-byte alignment rules");
        g_last_spmm_kernel = "spmm_slab_kernel";
        if (npanels <= 0) npanels = rows_sorted ? mx::pick_panels(K, (size_t)2560 << 10) : 1;
        if (!rows_sorted) npanels = 1;                 // panels need column-sorted rows
        if (wg_per_cu <= 0) wg_per_cu = 4;
        if (dense_dtype == MX_F64)
            return mx::launch_spmm_slab<double>(m, n, K, indptr, indices, values, (const double *)B, ldb, (double *)C,
                                                ldc, colmajor_out, npanels, wg_per_cu, st);
        return mx::launch_spmm_slab<float>(m, n, K, indptr, indices, values, (const float *)B, ldb, (float *)C, ldc,
                                           colmajor_out, npanels, wg_per_cu, st);
    }
    g_last_spmm_kernel = "spmm_rowwave_kernel";
    return mxd_spmm_csr_dense(m, n, indptr, indices, values, B, ldb, C, ldc, dense_dtype, colmajor_out, stream);
}

extern "C" int mxd_spmm_csr_dense(int m, int n,
                                  const int32_t *indptr, const int32_t *indices, const double *values,
                                  const void *B, size_t ldb, void *C, size_t ldc,
                                  int dense_dtype, int colmajor_out, void *stream)
{
    MX_REQUIRE(m >= 0 && n >= 0, "mxd_spmm_csr_dense: negative dimension (m=%d, n=%d)", m, n);
    if (m == 0 || n == 0) return 0;
    MX_REQUIRE(indptr && B && C, "mxd_spmm_csr_dense: null pointer");
    hipStream_t st = mx::as_stream(stream);
    if (dense_dtype == MX_F64)
        return mx::dispatch_spmm<double, 2>(m, n, indptr, indices, values, (const double *)B, ldb,
                                            (double *)C, ldc, colmajor_out, st);
    if (dense_dtype == MX_F32)
        return mx::dispatch_spmm<float, 4>(m, n, indptr, indices, values, (const float *)B, ldb,
                                           (float *)C, ldc, colmajor_out, st);
    return mx::set_error("mxd_spmm_csr_dense: unsupported dense dtype %d", dense_dtype);
}

// spmm_plan.hip — CSR x dense SpMM for gfx950 (MI355X), hand-written HIP.
//
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
#include "spmm_common.h"
#include <new>

namespace mx {

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
// indptr[r0 + 8] - indptr[r0], so the sizes (and the AUTO pad-ratio rule) come from indptr alone.  The sizing pass
// writes steps[oct] and, per tile of T octets (one workgroup), the sum of the tile's steps; the tile sums (at most
// PLAN_MAX_TILES of them) and nnz go back to the host in one pinned copy.  There is no scan: a fill workgroup adds up
// the tile sums in front of its tile and the steps in front of its octet inside the tile, and all tile sums for the
// step total.  Everything a kernel reads was written by an earlier kernel on the stream.
// Fill: one 512-thread workgroup per octet, one wavefront per bundle.  The wavefront reads its bundle's entries once
// (coalesced, 64 per load, PLAN_LD loads in flight) and classifies each 64-entry chunk once: the entry's panel, its
// rank among the chunk's entries of the same panel, and (lane q) the chunk's count of panel q.  The prefix over the
// panel counts gives the bundle's panel offsets, and every entry goes to (panel offset + entries of its panel in
// earlier chunks + rank), i.e. CSR order inside a panel.  Ranks come from a multisplit: NBITS = ceil(log2 P) ballots
// of the panel's bits give each lane the mask of its peers, so the cost does not grow with P; NBITS is a template
// parameter, the bit loops unroll exactly.  Octets of up to PLAN_STAGE_STEPS steps are assembled in LDS in their final
// slot order and written out with 16-byte stores; longer ones are scattered straight to global memory.
constexpr int PLAN_LD = 4;
constexpr int PLAN_STAGE_STEPS = 384;              // 384 x 64 slots x 12 B = 36 KiB of LDS: four workgroups per CU
constexpr int PLAN_PAD_NUM = 7, PLAN_PAD_DEN = 4;  // AUTO's pad rule: reject a plan of more than 1.75 x nnz + 65536 slots
constexpr int PLAN_MAX_TILES = 4096;               // tile sums per build: 16 KiB read back, 8 loads per fill thread
constexpr int PLAN_RB_HEAD = 16;                   // read-back block: [nnz : int64][go flag : int32][pad], then the tile sums

// octets per sizing tile: 32 (the 256 bundles of one sizing workgroup) until that would make more than PLAN_MAX_TILES
inline int plan_tile_octs(int noct) { return 32 * (int)ceil_div(noct > 0 ? noct : 1, 32 * PLAN_MAX_TILES); }

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

// steps[oct] = longest bundle of the octet rounded up to whole chunks; one thread per bundle, 8 per octet.  One
// workgroup per tile of tile_octs octets (a multiple of 32: whole passes of 256 bundles); tile_sums[tile] = the sum of
// its steps (unsigned: at most nnz + 31 per octet).
__global__ __launch_bounds__(256)
void plan_size_kernel(int m, int noct, int tile_octs, const int32_t *__restrict__ indptr, int32_t *__restrict__ steps,
                      unsigned *__restrict__ tile_sums, long long *__restrict__ nnz_out)
{
    __shared__ unsigned s_part[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) *nnz_out = indptr[m];   // rides back with the tile sums (one copy)
    unsigned sum = 0;
    for (int o = 0; o < tile_octs; o += 32) {
        const long long bl = ((long long)blockIdx.x * tile_octs + o) * 8 + threadIdx.x;    // bundle
        const bool live = bl < (long long)noct * 8;
        const int b = live ? (int)bl : 0;
        int len = 0;
        if (live) {
            const int r0 = (int)min((long long)b * PLAN_RB, (long long)m), r1 = (int)min((long long)b * PLAN_RB + PLAN_RB, (long long)m);
            len = indptr[r1] - indptr[r0];
        }
        len = max(len, __shfl_xor(len, 1, 8));
        len = max(len, __shfl_xor(len, 2, 8));
        len = max(len, __shfl_xor(len, 4, 8));
        if (live && (b & 7) == 0) {
            const int st = (len + 8 * PLAN_CHUNK - 1) & ~(8 * PLAN_CHUNK - 1);             // whole chunks of 4 batches of 8 steps
            steps[b >> 3] = st;
            sum += (unsigned)st;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// sum of v over the wavefront (wave-uniform): butterfly inside each row of 16 lanes by DPP (quad_perm [1,0,3,2] and
// [2,3,0,1], row_half_mirror, row_mirror), then the four rows' sums as scalars
__device__ __forceinline__ int wave_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

// lanes whose key agrees with `key` on the low NBITS bits, among the lanes in `valid` (bal[b] = ballot of key bit b)
template <int NBITS>
__device__ __forceinline__ unsigned long long multisplit_peers(int key, const unsigned long long (&bal)[6],
                                                                unsigned long long valid)
{
    unsigned long long peers = valid;
#pragma unroll
    for (int b = 0; b < NBITS; b++) peers &= ((key >> b) & 1) ? bal[b] : ~bal[b];
    return peers;
}

// Slot layout inside a batch of 8 steps: [bundle g][step u] — lane 8g+u of the sweep's reading wavefront holds bundle
// g's entry for step u, i.e. inside g's own lane group (intra-group DPP broadcast).  Step t of bundle g of an octet
// lands in slot (t & ~7) * 8 + g * 8 + (t & 7) of the octet.
// NBITS = ceil(log2 npanels), 0 for one panel.
template <int NBITS>
__global__ __launch_bounds__(512, 8)
void plan_fill_kernel(int m, int npanels, int panel_cols, const int32_t *__restrict__ indptr,
                      const int32_t *__restrict__ indices, const double *__restrict__ values,
                      const int32_t *__restrict__ steps, const unsigned *__restrict__ tile_sums, int ntiles, int tile_octs,
                      int32_t *__restrict__ pcol, double *__restrict__ pval,
                      int noct, int pad_col, int32_t *__restrict__ step_off,
                      const long long *__restrict__ nnz_dev, long long cap_slots, int pad_rule, int *__restrict__ go)
{
    __shared__ int32_t s_col[PLAN_STAGE_STEPS * 8];
    __shared__ double s_val[PLAN_STAGE_STEPS * 8];
    __shared__ int s_bpo[8][PLAN_MAXP];
    __shared__ long long s_tot[8];
    __shared__ int s_front[8];

    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int oct = blockIdx.x;

    // Where the octet starts and how long the whole plan is, from the sizing pass alone: this thread's share of the
    // tile sums (all of them: the step total; those in front of the octet's tile: its base) and of the steps in front
    // of the octet inside its tile.  These loads go out together with the row pointers; the entries are read once
    // the plan is accepted.
    const int tile = oct / tile_octs, oct0 = tile * tile_octs;
    int part_lo = 0, part_hi = 0, part_front = 0;                   // the total in 16-bit halves: 4096 of each fit an int
    for (int i = threadIdx.x; i < ntiles; i += 512) {
        const unsigned v = tile_sums[i];
        part_lo += (int)(v & 0xffffu);
        part_hi += (int)(v >> 16);
        part_front += i < tile ? (int)v : 0;
    }
    for (int i = oct0 + threadIdx.x; i < oct; i += 512) part_front += steps[i];
    const int steps_oct = steps[oct];
    const long long nnz = *nnz_dev;

    const int row0 = oct * PLAN_OCT_ROWS + g * PLAN_RB;
    int rp[PLAN_RB + 1];                                             // the bundle's row pointers (wave-uniform)
#pragma unroll
    for (int r = 0; r <= PLAN_RB; r++) rp[r] = uniform(indptr[min(row0 + r, m)]);
    const int s = rp[0], e = rp[PLAN_RB];
    const bool stage = steps_oct <= PLAN_STAGE_STEPS;                // workgroup-uniform
    const float inv_pc = 1.0f / (float)panel_cols;

    const int wave_lo = wave_sum(part_lo), wave_hi = wave_sum(part_hi), wave_front = wave_sum(part_front);
    if (lane == 0) { s_tot[g] = ((long long)wave_hi << 16) + wave_lo; s_front[g] = wave_front; }
    __syncthreads();
    long long total = 0;
    int base = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) { total += s_tot[w]; base += s_front[w]; }

    // a plan that does not fit (or that AUTO rejects) is not written at all, and the repack of B behind this kernel
    // is skipped with it
    const bool ok = plan_accept(total, nnz, cap_slots, pad_rule);
    if (blockIdx.x == 0 && threadIdx.x == 0) *go = ok ? 1 : 0;
    if (!ok) return;

    // The first PLAN_LD x 64 entries (all of a cfg2 bundle) stay in registers; longer bundles read the rest twice
    // (the second time from L2: the workgroup read it moments before).  A rejected plan does not read A at all.
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
        for (int b = 0; b < NBITS; b++) bal[b] = __ballot(pan >= 0 && ((pan >> b) & 1));
        return __ballot(pan >= 0);
    };
    // one chunk, classified: the entry's rank among the chunk's entries of its panel; lane q: the chunk's count of panel q
    auto classify = [&](int pan, int &rank, int &cnt) {
        unsigned long long bal[6];
        const unsigned long long valid = split(pan, bal);
        const unsigned long long peers = multisplit_peers<NBITS>(pan, bal, valid);
        rank = __builtin_amdgcn_mbcnt_hi((unsigned)(peers >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)peers, 0u));
        cnt = lane < npanels ? __popcll(multisplit_peers<NBITS>(lane, bal, valid)) : 0;
    };

    // classification of the register-resident chunks, once; kept in one register per chunk:
    // panel (signed byte, -1: no entry) | rank << 8 | count << 16
    int cls0[PLAN_LD];
    int mine = 0;                                                    // lane q: the bundle's entries in panel q
#pragma unroll
    for (int c = 0; c < PLAN_LD; c++) {
        cls0[c] = 0xff;
        if (s + 64 * c < e) {                                        // uniform
            const int pan = col0[c] >= 0 ? panel_of(col0[c], panel_cols, inv_pc, npanels) : -1;
            int rank, cnt;
            classify(pan, rank, cnt);
            cls0[c] = (pan & 0xff) | (rank << 8) | (cnt << 16);
            mine += cnt;
        }
    }
    // the part of a long bundle that does not fit in registers: counted here, read again for the placement
    for (int k0 = s + 64 * PLAN_LD; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        const int pan = k < e ? panel_of(indices[k], panel_cols, inv_pc, npanels) : -1;
        int rank, cnt;
        classify(pan, rank, cnt);
        mine += cnt;
    }
    // exclusive prefix over the panels (lanes 0..npanels-1): where panel q starts in the bundle's stream
    // (panels live in lanes 0..2^NBITS-1: NBITS steps; what the lanes above them hold is never used)
    int incl = mine;
#pragma unroll
    for (int off = 1; off < (1 << NBITS); off <<= 1) {
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
    auto local_row = [&](int k) {
        int lrow = 0;
#pragma unroll
        for (int r = 1; r < PLAN_RB; r++) lrow += k >= rp[r];
        return lrow;
    };

    // placement: every entry at its panel's next step + its rank among the chunk's entries of that panel
#pragma unroll
    for (int c = 0; c < PLAN_LD; c++) {
        if (s + 64 * c < e) {                                        // uniform
            const int pan = (int)(signed char)cls0[c], rank = (cls0[c] >> 8) & 0xff, cnt = cls0[c] >> 16;
            const int start = __shfl(nextstep, pan < 0 ? 0 : pan, 64);
            if (pan >= 0) put(start + rank, col0[c] | (local_row(s + 64 * c + lane) << PLAN_ROW_SHIFT), val0[c]);
            nextstep += cnt;
        }
    }
    for (int k0 = s + 64 * PLAN_LD; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        int col = -1;
        double av = 0.0;
        if (k < e) { col = indices[k]; av = values[k]; }
        const int pan = col >= 0 ? panel_of(col, panel_cols, inv_pc, npanels) : -1;
        int rank, cnt;
        classify(pan, rank, cnt);
        const int start = __shfl(nextstep, pan < 0 ? 0 : pan, 64);
        if (pan >= 0) put(start + rank, col | (local_row(k) << PLAN_ROW_SHIFT), av);
        nextstep += cnt;
    }
    // Padding up to the octet's length: a no-op entry — value 0, column `pad_col` (the all-zero extra row of the
    // packed B), row = the bundle's last entry's row so that it does not even trigger a row switch.  0 * 0 added to
    // an accumulator that is never -0.0 leaves it unchanged bit for bit.
    const int last_lrow = e > s ? local_row(e - 1) : 0;
    for (int t = (e - s) + lane; t < steps_oct; t += 64) put(t, pad_col | (last_lrow << PLAN_ROW_SHIFT), 0.0);

    __syncthreads();
    // panel boundaries of the octet for the sweep's panel meetings: mean start of the panel over the 8 bundles
    if (g == 0 && lane < npanels) {
        int sum = 0;
#pragma unroll
        for (int gg = 0; gg < 8; gg++) sum += s_bpo[gg][lane];
        step_off[(size_t)oct * npanels + lane] = base + (lane == 0 ? 0 : sum / 8);
        if (oct == noct - 1 && lane == 0) step_off[(size_t)noct * npanels] = (int32_t)total;
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
        const size_t dst = (size_t)total * 8 + threadIdx.x;
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

    // What a wavefront carries from one work item to its next one (item + nwg: octet n_oct), so that the next item
    // starts without a load it has to wait for behind its predecessor's stores of C:
    //   * n_row: the next octet's row of step_off (lane p = start of panel p), a vector load issued at the START of
    //     the current item: it is older than every B-line load of the item and returns with the first of them.
    //   * n_beg / n_end: the next octet's first step and end, scalars (the address is wave-uniform, so these are
    //     scalar loads).  A scalar load is waited for at the next barrier, whoever uses it, and the current item needs
    //     n_beg in front of its stream loop (the last read-ahead goes there).  So they are read one item EARLIER still:
    //     an item issues the loads for the item after next (f_oct, f_beg, f_end) behind its first barrier, and the
    //     next item takes them over as its n_beg / n_end.  Only a workgroup's first item waits for bounds.
    //   * (rc, rv): the next octet's first plan chunk, read by the stream loop's last read-ahead (see there);
    //     held_step is the step it was read from.  A chunk is a function of its step alone (the plan is read-only
    //     here), so an item may use the held chunk whenever held_step equals its first step, and loads the chunk itself
    //     in every other case: the first item, the item behind an empty stream, an item without a predecessor.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);       // the compiler cannot prove threadIdx.x >> 6 uniform
    // item = slab * ngens + gen moves on by nwg per item: one 64-bit divide in front of the first item, none between
    // the epilogue of one item and the first loads of the next
    const int gen_step = nwg % ngens, slab_step = nwg / ngens;
    int slab_c = (int)((lo + wg) / ngens), gen_c = (int)((lo + wg) % ngens);
    int n_oct = -1, n_row = 0, n_beg = 0, n_end = 0;
    int f_oct = -1, f_beg = 0, f_end = 0;
    int held_step = -1;
    int rc[PLAN_CHUNK];
    double rv[PLAN_CHUNK];
#pragma unroll
    for (int k = 0; k < PLAN_CHUNK; k++) { rc[k] = 0; rv[k] = 0.0; }
    //   * warm hand-over (WARM builds: column-major): the 8 B lines of the next item's first batch,
    //     requested from the held chunk in FRONT of the 16 (f32: 32) stores of C.  On gfx9 the stores count in vmcnt
    //     and retire in order with the loads, so a B line requested behind them waits for their acknowledgements;
    //     requested in front of them it waits for nothing but itself.  `warm` says that held_b is the item's batch 0,
    //     in flight; such an item enters its stream through a copy of the chunk body of its own (see there).  Only the
    //     lines are held (32 registers): the batch's (column, value) pairs are broadcast again from the held chunk
    //     when they are consumed.  The row-major instantiations have no register to hold anything across the epilogue
    //     (128 VGPRs as they are) and keep the cold start.
    constexpr bool WARM = COLMAJOR;
    real_t held_b[U][VEC];
    bool warm = false;

    for (int it = 0; it < niter; it++) {
        const long long item_raw = lo + wg + (long long)it * nwg;
        const bool have = item_raw < hi;
        const int slab = have ? slab_c : 0, gen = have ? gen_c : 0;
        const int oct = gen * PLAN_WAVES + wave_u;
        const bool oct_ok = have && oct < noct;

        // This item's bounds: carried by the previous item, or (first item, previous item without an octet) read
        // here and waited for inside the branch, so that the carried path meets no wait at all.
        int so_row = 0, sbeg = 0, send = 0;
        if (oct_ok) {
            if (n_oct != oct) {
                n_row = step_off[(size_t)oct * npanels + min(lane, npanels)];
                n_beg = step_off[(size_t)oct * npanels];
                n_end = step_off[(size_t)oct * npanels + npanels];
                asm volatile("" : "+v"(n_row));
            }
            so_row = n_row; sbeg = n_beg; send = n_end;
        }
        // The next item's bounds.  It exists iff item + nwg is inside the XCD group's range and its octet inside the
        // matrix; otherwise the load goes to octet 0 (always there) and is not used.  n_beg / n_end are what the
        // previous item read as f_beg / f_end, or (first item) are read here.
        int ngen = gen_c + gen_step;
        slab_c += slab_step + (ngen >= ngens ? 1 : 0);
        ngen -= ngen >= ngens ? ngens : 0;
        gen_c = ngen;
        {
            const int noct_raw = ngen * PLAN_WAVES + wave_u;
            const bool nvalid = item_raw + nwg < hi && noct_raw < noct;
            const size_t nrow0 = nvalid ? (size_t)noct_raw * npanels : 0;
            n_oct = nvalid ? noct_raw : -1;
            n_row = step_off[nrow0 + min(lane, npanels)];
            if (nvalid && f_oct != noct_raw) {
                f_beg = step_off[nrow0];
                f_end = step_off[nrow0 + npanels];
            }
            n_beg = f_beg; n_end = f_end;
        }
        // slab base is wave-uniform (scalar registers), the per-lane part is a 32-bit byte offset: one VALU op per
        // address.  A slab is K x 128 B < 4 GiB because K < 2^27... checked on the host (K * 128 < 2^32).
        const char *__restrict__ Bbase = reinterpret_cast<const char *>(Bp + (size_t)slab * slab_stride);
        const unsigned lane_off = (unsigned)(lg * VEC * sizeof(real_t));

        // A wavefront's accumulator rows are touched by that wavefront only (zeroing, folds, epilogue): no
        // workgroup-wide synchronisation around a generation, the wavefronts only meet at the panel boundaries.
        for (int i = lane; i < PLAN_OCT_ROWS * S; i += 64) my_oct[i] = 0;
        if (sync_mode > 0) __syncthreads();                          // locality only: start the first panel together
        // the bounds of the item after next, behind the barrier: nothing waits for them before the first panel meeting
        {
            int fgen = ngen + gen_step;
            fgen -= fgen >= ngens ? ngens : 0;
            const int foct_raw = fgen * PLAN_WAVES + wave_u;
            const bool fvalid = item_raw + 2LL * nwg < hi && foct_raw < noct;
            const size_t frow0 = fvalid ? (size_t)foct_raw * npanels : 0;
            f_oct = fvalid ? foct_raw : -1;
            f_beg = step_off[frow0];
            f_end = step_off[frow0 + npanels];
        }

        // One continuous, software-pipelined stream over the octet's entries of ALL panels (they are contiguous in
        // the plan).  Panel boundaries only matter for locality: when the stream crosses one, the 16 waves of the
        // CU's single workgroup meet at a __syncthreads: a bare s_barrier, nothing is loaded or waited for there, so
        // the B lines and the plan chunk in flight stay in flight (the boundaries come out of a register, see
        // so_row below).  Across the 32 CUs of the XCD group there is ONE global timing barrier per
        // generation (32 pollers per counter); in between the CUs run identical code on statistically identical
        // data and drift by a fraction of a panel.
        {
            if (sync_mode >= 2) xcd_timing_barrier(my_ctr, (unsigned)(it + 1) * (unsigned)nwg);
            // The octet's whole row of step_off is in a register (so_row, see the carry above): lane p holds the
            // start of panel p (npanels <= 64 lanes), the first step and the end of the last panel are scalars.
            // Every panel boundary the stream meets later is a v_readlane of that register: a load at the meeting
            // would have to be waited for with vmcnt(0), and vector loads return in order, so that wait would drain
            // the B lines and the plan chunk in flight.
            // Where the last read-ahead of this stream goes: the next item's first step, or (no next item) -1.  Taken
            // here, in front of the loop (n_beg was read an item ago), so that no wait for a scalar load is inside it.
            const int nfirst = n_oct >= 0 ? n_beg : -1;
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
            // per 32 steps.  The last read-ahead of an octet has nothing of this octet left to fetch: it reads the
            // first chunk of the wavefront's NEXT work item instead (a scalar select of the step, the same four loads),
            // which stays in (rc, rv) across the epilogue, so the next item starts its B-line loads without a plan
            // read (first touch of an HBM stream) to wait for.  Without a next item it runs one chunk past the octet,
            // as it always did, and is dropped.  Either way it reads slots [8 t, 8 t + 256) with t <= total steps
            // (t = this octet's end, or step_off[next octet * P], the sum of the steps in front of that octet):
            // inside the PLAN_TAIL_SLOTS = 512 slots of padding behind the last octet.
            // The next item's first batch of B lines is requested in front of the epilogue's stores where the hand-over
            // is warm (see `warm` above); in a cold one the turnover is last batch, epilogue, zeroing, first batch of
            // B lines, see DESIGN.md 4.1.
            int rn[PLAN_CHUNK];
            double rvn[PLAN_CHUNK];
            auto load_chunk = [&](int step, int (&c)[PLAN_CHUNK], double (&v)[PLAN_CHUNK]) {
                const long long e = (long long)step * 8 + lane;
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) { c[k] = pcol[e + 64 * k]; v[k] = pval[e + 64 * k]; }
            };
            // the batch in flight: this block's own, or (WARM builds) the one that lives across the epilogue
            int pc[U];
            double pv[U];
            real_t own_b[U][VEC];
            real_t (&b)[U][VEC] = *(WARM ? &held_b : &own_b);
#pragma unroll
            for (int u = 0; u < U; u++) {
                pc[u] = 0;
                pv[u] = 0.0;
            }
            if (!(WARM && warm)) {                                  // the no-op batch of a cold start
#pragma unroll
                for (int u = 0; u < U; u++)
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
            if (!(WARM && warm) && send > sbeg && held_step != sbeg) {
                load_chunk(sbeg, rc, rv);
                // the first chunk has to be there before anything can start; with it complete at loop entry the
                // compiler's vmcnt bookkeeping is exact on both edges of the loop.  (A held chunk is complete: it is
                // older than the B lines the previous stream's last batch waited for.)
#pragma unroll
                for (int k = 0; k < PLAN_CHUNK; k++) asm volatile("" : "+v"(rc[k]), "+v"(rv[k]));
            }
            // Consumption lags one batch behind the broadcast + B-line load: while batch t is consumed step by step,
            // the line of the same step of batch t+1 is requested into the registers the FMA just released, so 8
            // B-line loads per wavefront are in flight all the time.  The first pass consumes the no-op batch set up
            // above, the last batch is consumed after the loop.
            // One chunk of the stream: the read-ahead, then batches K0 .. PLAN_CHUNK - 1 of the chunk in (rc, rv); K0 = 0
            // everywhere but in the warm entry below.  A macro, not a lambda: each use has to be a copy of the code with
            // wait counts of its own, and as a lambda the body came out with other registers in every instantiation.
            // MX_PLAN_STEP: consume step UU of the batch in flight, request the same step of batch k of the chunk.
            // In the first batch of the warm entry (K0 = 1, k = 1) the step consumed is one of batch 0 of the held chunk,
            // of which only the B line was kept: its (column, value) pair is broadcast here.
            // The probe (MX_PROBE) closes an interval behind step 0, except behind the no-op batch of a cold start.
#define MX_PLAN_STEP(UU, K0)                                                                                          \
                    if (K0 != 0 && k == K0) plan_bcast<UU>(rc[0], rv[0], pc[UU], pv[UU]);                             \
                    consume(UU);                                                                                      \
                    plan_bcast<UU>(rc[k], rv[k], pc[UU], pv[UU]);                                                     \
                    vload<real_t, VEC>(b[UU], reinterpret_cast<const real_t *>(Bbase + b_offset(pc[UU])));            \
                    __builtin_amdgcn_sched_barrier(0);
#define MX_PLAN_CHUNK(K0)                                                                                             \
            {                                                                                                         \
                const int ahead = s + U * PLAN_CHUNK;                                                                 \
                const int ra = ahead >= send && nfirst >= 0 ? nfirst : ahead;                                         \
                load_chunk(ra, rn, rvn);                                                                              \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
                _Pragma("unroll")                                                                                     \
                for (int k = K0; k < PLAN_CHUNK; k++) {                                                               \
                    MX_PLAN_STEP(0, K0)                                                                               \
                    MX_PROBE(if (pr_kind && !(pr_kind == 3 && s == sbeg && k == 0)) {                                 \
                        const unsigned long long dt = (unsigned long long)(wall_clock64() - pr_t);                    \
                        _Pragma("unroll") for (int j = 0; j < 3; j++)                                                 \
                            if (pr_kind == j + 1) { pr_sum[j] += dt; pr_cnt[j]++; }                                   \
                        pr_kind = 0;                                                                                  \
                    })                                                                                                \
                    MX_PLAN_STEP(1, K0) MX_PLAN_STEP(2, K0) MX_PLAN_STEP(3, K0)                                       \
                    MX_PLAN_STEP(4, K0) MX_PLAN_STEP(5, K0) MX_PLAN_STEP(6, K0) MX_PLAN_STEP(7, K0)                   \
                    MX_PROBE(bool pr_met = false;)                                                                    \
                    if (sync_mode > 0) {                                                                              \
                        const int sn = s + U * k;                   /* steps consumed so far */                       \
                        while (p < npanels - 1 && sn >= next_b) {   /* the stream moved into the next panel */        \
                            p++;                                                                                      \
                            __syncthreads();                                                                          \
                            MX_PROBE(pr_met = true; if (pr_kind != 3) pr_t = wall_clock64();)                         \
                            next_b = p < npanels - 1 ? __builtin_amdgcn_readlane(so_row, p + 1) : send;               \
                        }                                                                                             \
                    }                                                                                                 \
                    MX_PROBE(if (pr_kind != 3) { pr_kind = pr_met ? 2 : 1; if (!pr_met) pr_t = wall_clock64(); })     \
                }                                                                                                     \
                _Pragma("unroll")                                                                                     \
                for (int k = 0; k < PLAN_CHUNK; k++) { rc[k] = rn[k]; rv[k] = rvn[k]; }                               \
                held_step = ra;                                                                                       \
            }
            int s = sbeg;                                            // sbeg, send are wave-uniform
            if constexpr (WARM) {
                if (warm) {
                    // Warm entry: the B lines of this stream's batch 0 were requested in front of the previous
                    // item's stores of C, so there is no no-op batch to consume: the first chunk starts at
                    // k = 1, which consumes batch 0 while it requests batch 1.  This copy of the chunk body is reached
                    // from the warm hand-over only, so its wait counts are those of that one path (the first consume
                    // waits for its own B line, not for the stores behind it); a boundary that k = 0 would have met
                    // is caught up by the meeting loop of k = 1.
                    MX_PLAN_CHUNK(1)
                    s += U * PLAN_CHUNK;
                }
            }
            for (; s < send; s += U * PLAN_CHUNK) MX_PLAN_CHUNK(0)
#undef MX_PLAN_CHUNK
#undef MX_PLAN_STEP
            MX_PROBE(if (send > sbeg) { pr_kind = 3; pr_t = wall_clock64(); })
#pragma unroll
            for (int u = 0; u < U; u++) consume(u);
            lds_fold<VEC>(my_rows + cur * S, acc);
            if (sync_mode > 0)
                for (; p < npanels - 1; p++) __syncthreads();           // every wave meets npanels-1 times per generation
        }

        // each wavefront writes the 64 x W tile of C it accumulated (streaming stores: C is not read again)
        // Warm hand-over: a full tile (so that the stores are straight-line code whose count the compiler knows
        // exactly), a next item with a stream, and its first chunk held.  All of it is wave-uniform.
        bool cold_tile = oct_ok;
        if constexpr (WARM) {
            warm = oct_ok && gen * PLAN_WG_ROWS + wave_u * PLAN_OCT_ROWS + PLAN_OCT_ROWS <= m && n - slab * W >= W &&
                   n_oct >= 0 && n_end > n_beg && held_step == n_beg;
            if (warm) {
                // slab_c has moved on: it is the next item's slab, which may be another one than this item's
                const char *__restrict__ Bnext = reinterpret_cast<const char *>(Bp + (size_t)slab_c * slab_stride);
#define MX_PLAN_WARM(UU)                                                                                              \
                vload<real_t, VEC>(held_b[UU], reinterpret_cast<const real_t *>(                                      \
                    Bnext + ((unsigned)group8_dpp_bcast<UU>(rc[0]) * (unsigned)(W * sizeof(real_t))) + lane_off));
                MX_PLAN_WARM(0) MX_PLAN_WARM(1) MX_PLAN_WARM(2) MX_PLAN_WARM(3)
                MX_PLAN_WARM(4) MX_PLAN_WARM(5) MX_PLAN_WARM(6) MX_PLAN_WARM(7)
#undef MX_PLAN_WARM
                __builtin_amdgcn_sched_barrier(0);
                // lane = row, one column per store, eight columns read from LDS at a time; the element offset moves on
                // in a vector register pair (W scalar offsets would not fit the scalar file)
                const real_t *src = my_oct + (size_t)lane * S;
                size_t off = (size_t)(slab * W) * ldc + (size_t)(gen * PLAN_WG_ROWS + wave * PLAN_OCT_ROWS + lane);
#pragma unroll
                for (int c0 = 0; c0 < W; c0 += 8) {
                    real_t t[8];
#pragma unroll
                    for (int c = 0; c < 8; c++) t[c] = src[c0 + c];
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        __builtin_nontemporal_store(t[c], C + off);
                        off += ldc;
                        asm volatile("" : "+v"(off));
                    }
                }
                cold_tile = false;
            }
        }
        if (cold_tile) {
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
    char *host = nullptr;                                           // PLAN_RB_HEAD bytes ([0] nnz : int64), then the tile sums
    hipEvent_t ev = nullptr;
};
constexpr size_t PLAN_RB_BYTES = PLAN_RB_HEAD + PLAN_MAX_TILES * sizeof(unsigned);
static PlanReadback *plan_readback()
{
    static thread_local PlanReadback rb;
    if (!rb.host) {
        if (hipHostMalloc((void **)&rb.host, PLAN_RB_BYTES, hipHostMallocDefault) != hipSuccess) { rb.host = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(rb.host); rb.host = nullptr; return nullptr; }
    }
    return &rb;
}

static int launch_fill(const mx_spmm_plan *pl, hipStream_t st)
{
    const int nbits = pl->npanels > 1 ? 32 - __builtin_clz((unsigned)(pl->npanels - 1)) : 0;
    return dispatch_int(int_list<0, 1, 2, 3, 4, 5, 6>{}, "spmm plan", "panel bits", nbits, [&](auto nb) {
        hipLaunchKernelGGL((plan_fill_kernel<nb()>), dim3((unsigned)pl->noct), dim3(512), 0, st, pl->m, pl->npanels,
                           pl->panel_cols, pl->indptr, pl->indices, pl->values, pl->steps, pl->tile_sums, pl->ntiles,
                           pl->tile_octs, pl->pcol, pl->pval, pl->noct, pl->K, pl->step_off, pl->nnz_dev, pl->fill_cap,
                           pl->pad_rule, pl->go);
        MX_LAUNCH_CHECK();
        return 0;
    });
}

// Building a plan is split in two so that the GPU never waits for the host.  plan_begin enqueues the sizing pass, the
// one read-back of [nnz, tile sums] and the fill, which decides on the device-side total whether the plan fits the
// current (grow-only) buffers; the caller may enqueue more work behind it (AUTO packs B).  plan_end waits for the
// read-back, adds the tile sums up to the step total, takes the same decision on the host and, when the buffers were
// too small (typically the first call), grows them and fills again (*refilled = true).
// pad_rule: AUTO's rejection of plans that would hold more than 1.75 x nnz slots (rows of very uneven length pad the
// 8-way interleave: an octet is as long as its longest bundle) — pl->ready then stays false and nothing is written.
int plan_begin(mx_spmm_plan *pl, int m, int K, const int32_t *indptr, const int32_t *indices, const double *values,
               int npanels, hipStream_t st, int pad_rule)
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
    pl->tile_octs = plan_tile_octs(pl->noct);
    pl->ntiles = (int)ceil_div(pl->noct, pl->tile_octs);
    if (grow(&pl->scratch, &pl->scratch_cap, steps_b + PLAN_RB_BYTES)) return 1;
    if (grow((void **)&pl->step_off, &pl->step_off_cap, (nop + 1) * 4)) return 1;
    int32_t *steps = (int32_t *)pl->scratch;
    char *rb_dev = (char *)steps + steps_b;                          // [nnz][go flag][tile sums]: read back in one copy
    pl->steps = steps;
    pl->nnz_dev = (long long *)rb_dev; pl->go = (int *)(rb_dev + 8);
    pl->tile_sums = (unsigned *)(rb_dev + PLAN_RB_HEAD);
    hipLaunchKernelGGL(plan_size_kernel, dim3((unsigned)pl->ntiles), dim3(256), 0, st, m, pl->noct, pl->tile_octs, indptr,
                       steps, (unsigned *)(rb_dev + PLAN_RB_HEAD), (long long *)rb_dev);
    MX_LAUNCH_CHECK();
    PlanReadback *rb = plan_readback();
    MX_REQUIRE(rb, "spmm plan: cannot allocate the pinned read-back buffer");
    MX_HIP(hipMemcpyAsync(rb->host, rb_dev, PLAN_RB_HEAD + (size_t)pl->ntiles * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    MX_HIP(hipEventRecord(rb->ev, st));
    pl->indptr = indptr; pl->indices = indices; pl->values = values;
    pl->pad_rule = pad_rule;
    pl->fill_cap = (long long)std::min(pl->pcol_cap / 4, pl->pval_cap / 8);
    if (launch_fill(pl, st)) return 1;
    pl->pending = true;
    return 0;
}

int plan_end(mx_spmm_plan *pl, hipStream_t st, bool *refilled)
{
    if (refilled) *refilled = false;
    if (!pl->pending) return 0;                                     // m == 0 (ready) or plan_begin failed
    pl->pending = false;
    PlanReadback *rb = plan_readback();
    MX_HIP(hipEventSynchronize(rb->ev));
    const long long nnz = *(const long long *)rb->host;           // hipHostMalloc'ed: aligned
    long long total = 0;
    const unsigned *sums = (const unsigned *)(rb->host + PLAN_RB_HEAD);
    for (int i = 0; i < pl->ntiles; i++) total += sums[i];
    pl->nnz = (int32_t)nnz;
    MX_REQUIRE(total >= 0 && total * 8 <= (long long)INT_MAX * 4LL, "spmm plan: too many steps (%lld)", total);
    MX_REQUIRE(total <= (long long)INT_MAX, "spmm plan: step offsets exceed int32");
    pl->total_steps = total;
    if (plan_accept(total, pl->nnz, pl->fill_cap, pl->pad_rule)) { pl->ready = true; return 0; }   // the fill wrote it
    if (plan_accept(total, pl->nnz, LLONG_MAX, pl->pad_rule) == false) return 0;                    // rejected by AUTO
    const size_t slots = (size_t)total * 8 + PLAN_TAIL_SLOTS;
    if (grow((void **)&pl->pcol, &pl->pcol_cap, slots * 4)) return 1;
    if (grow((void **)&pl->pval, &pl->pval_cap, slots * 8)) return 1;
    pl->fill_cap = (long long)std::min(pl->pcol_cap / 4, pl->pval_cap / 8);
    if (launch_fill(pl, st)) return 1;
    pl->ready = true;
    if (refilled) *refilled = true;
    return 0;
}

// slab-major copy of B with one extra all-zero row (index K) per slab: the plan's padding slots point at it
int plan_repack(int K, int n, const void *B, size_t ldb, int dense_dtype, hipStream_t st, void **Bp_out, const int *go)
{
    return dispatch_dense("spmm plan", dense_dtype, [&](auto t) {
        using real_t = typename decltype(t)::type;
        constexpr int W = SLAB_W<real_t>;
        const int nslabs = (int)ceil_div(n, W), Kp = K + 1;
        real_t *Bp = (real_t *)pack_workspace((size_t)nslabs * (size_t)Kp * W * sizeof(real_t));
        MX_REQUIRE(Bp, "spmm plan: cannot allocate the packed copy of B");
        if (launch_repack<real_t>(K, Kp, n, (const real_t *)B, ldb, Bp, go, st)) return 1;
        *Bp_out = Bp;
        return 0;
    });
}

int plan_run(const mx_spmm_plan *pl, int n, const void *B, size_t ldb, void *C, size_t ldc, int dense_dtype,
             int colmajor, int wg_per_cu, int sync_mode, hipStream_t st, const void *Bp)
{
    const char *what = "mxd_spmm_plan_run";
    return dispatch_dense(what, dense_dtype, [&](auto t) {
        using real_t = typename decltype(t)::type;
        constexpr int W = SLAB_W<real_t>;
        MX_REQUIRE(slab_ok<real_t>(n, (const real_t *)B, ldb, (const real_t *)C, ldc, colmajor),
                   "mxd_spmm_plan_run: operands do not meet the 16-byte alignment rules");
        const int m = pl->m, K = pl->K;
        const int nslabs = (int)ceil_div(n, W);
        if (!Bp) {                                                   // else the caller packed B (AUTO, behind the fill)
            void *packed = nullptr;
            if (plan_repack(K, n, B, ldb, dense_dtype, st, &packed)) return 1;
            Bp = packed;
        }
        if (wg_per_cu != 1 && wg_per_cu != 2 && wg_per_cu != 4) wg_per_cu = PLAN_DEFAULT_WG_PER_CU;
        const int waves = 16 / wg_per_cu;
        const int ngens = (int)ceil_div(m, PLAN_OCT_ROWS * waves);
        const unsigned grid = persistent_grid(wg_per_cu, (long long)nslabs * ngens);
        unsigned *sync = sync_workspace();
        if (!sync || pl->npanels <= 1) sync_mode = 0;
        if (sync_mode >= 2) MX_HIP(hipMemsetAsync(sync, 0, SYNC_BYTES, st));   // counters of the XCD timing barrier
        return dispatch_int(int_list<16, 8, 4>{}, what, "wavefronts per workgroup", waves, [&](auto wv) {
            return dispatch_int(int_list<0, 1>{}, what, "colmajor", colmajor ? 1 : 0, [&](auto cm) {
                kt_begin(st);
                hipLaunchKernelGGL((spmm_plan_kernel<real_t, cm() != 0, wv()>), dim3(grid), dim3(wv() * 64), 0, st, m, n,
                                   pl->npanels, pl->step_off, pl->pcol, pl->pval, (const real_t *)Bp, (size_t)(K + 1) * W,
                                   (real_t *)C, ldc, nslabs, ngens, pl->noct, K, sync, sync_mode);
                kt_end(st);
                MX_LAUNCH_CHECK();
                return 0;
            });
        });
    });
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

extern "C" int mxd_spmm_plan_run(const mx_spmm_plan *pl, int n, const void *B, size_t ldb, void *C, size_t ldc,
                                 int dense_dtype, int colmajor_out, int wg_per_cu, int sync_mode, void *stream)
{
    MX_REQUIRE(pl && n >= 0, "mxd_spmm_plan_run: bad arguments");
    MX_REQUIRE(pl->ready, "mxd_spmm_plan_run: the plan was sized but not built");
    if (pl->m == 0 || n == 0) return 0;
    MX_REQUIRE(B && C, "mxd_spmm_plan_run: null pointer");
    hipStream_t st = mx::as_stream(stream);
    if (sync_mode < 0) sync_mode = 1;       // panel meetings inside the CU's workgroup; 2 adds one XCD barrier per generation
    mx::note_spmm_kernel("spmm_plan_kernel");
    return mx::plan_run(pl, n, B, ldb, C, ldc, dense_dtype, colmajor_out, wg_per_cu, sync_mode, st);
}

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

// mx_compact_tile.h — the tile of a stable stream compaction, shared by compact.hip (keep rules on values / masks)
// and coona.hip (keep rule on the triplet's row and column): the tile geometry, the hoisted tile load, the tile's
// kept count and the in-tile ranks of the kept entries.  Device only.
//
// A tile is CP_TILE consecutive entries taken by one workgroup in CP_ROUNDS rounds of CP_BLOCK: lane t holds entries
// base + r * CP_BLOCK + t.  A wave ballot per round turns each lane's keep bit into a 64-bit mask; slot
// r * CP_WAVES + wave is the slot of entries [slot * 64, slot * 64 + 64) of the tile, so the slots are in storage
// order and entry q of the tile sits in slot q / 64 at bit q % 64.
#pragma once
#include "mx_common.h"

namespace mx {

constexpr int CP_BLOCK = 256;
constexpr int CP_WAVES = CP_BLOCK / MX_WAVE;
constexpr int CP_ROUNDS = 16;
constexpr int CP_TILE = CP_BLOCK * CP_ROUNDS;      // 4096 entries per tile
static_assert(CP_ROUNDS * CP_WAVES == MX_WAVE, "one lane of wave 0 per (round, wave) pair");

// a[r] = src[base + r * CP_BLOCK + threadIdx.x] for the tile's entries (0 past n)
template <typename T>
__device__ __forceinline__ void cp_load(T (&a)[CP_ROUNDS], const T *__restrict__ src, int64_t base, int64_t n)
{
    const T *s = src + base + threadIdx.x;
    if (base + CP_TILE <= n) {
#pragma unroll
        for (int r = 0; r < CP_ROUNDS; r++) a[r] = s[r * CP_BLOCK];
    } else {
#pragma unroll
        for (int r = 0; r < CP_ROUNDS; r++) a[r] = base + r * CP_BLOCK + threadIdx.x < n ? s[r * CP_BLOCK] : T{};
    }
}

// tile_counts[blockIdx.x] = the sum over the waves of `cnt`, each wave's own (wave-uniform) kept count
__device__ __forceinline__ void cp_store_tile_count(int cnt, int32_t *__restrict__ tile_counts)
{
    __shared__ int s_cnt[CP_WAVES];
    if (lane_id() == 0) s_cnt[threadIdx.x / MX_WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < CP_WAVES; w++) t += s_cnt[w];
        tile_counts[blockIdx.x] = t;
    }
}

// The tile's keep masks and what they give: off[slot] = kept entries of the tile before the slot, total = all of them.
struct CpTileRanks {
    unsigned long long mask[MX_WAVE];              // [round * CP_WAVES + wave]
    int off[MX_WAVE];
    int total;
};

// Publishes this wave's ballots bal[r] and scans the 64 slot counts in storage order; every thread of the workgroup
// calls it, and S is complete for all of them on return.
__device__ __forceinline__ void cp_rank_tile(CpTileRanks &S, const unsigned long long (&bal)[CP_ROUNDS])
{
    const int lane = lane_id(), wave = threadIdx.x / MX_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < CP_ROUNDS; r++) S.mask[r * CP_WAVES + wave] = bal[r];
    }
    __syncthreads();
    if (wave == 0) {
        const int c = __popcll(S.mask[lane]);
        int incl = c;
#pragma unroll
        for (int off = 1; off < MX_WAVE; off <<= 1) {
            const int o = __shfl_up(incl, off, MX_WAVE);
            if (lane >= off) incl += o;
        }
        S.off[lane] = incl - c;
        if (lane == MX_WAVE - 1) S.total = incl;
    }
    __syncthreads();
}

// in-tile rank of this lane's kept entry of round r
__device__ __forceinline__ int cp_rank_of(const CpTileRanks &S, int r, unsigned long long bal)
{
    return S.off[r * CP_WAVES + threadIdx.x / MX_WAVE] + __popcll(bal & ((1ull << lane_id()) - 1));
}

// kept entries of the tile before its entry q (0 <= q < CP_TILE)
__device__ __forceinline__ int cp_rank_before(const CpTileRanks &S, int q)
{
    const int slot = q / MX_WAVE;
    return S.off[slot] + __popcll(S.mask[slot] & ((1ull << (q % MX_WAVE)) - 1));
}

}  // namespace mx

// fs_body_loads.h — the device helpers the loads forms of the two bodies' passes share (kernels_bodies.hip k_bodies_loads,
// DESIGN.md §25; kernels_bodies3d.hip k3_bodies_loads, §26): the fixed-point rounding, the 64-bit wave sum and the fold of the
// shard table, over the number of words a body has (5 in 2D, 8 in 3D).  Device code only; the constants are fs_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "fs_device.h"
#include "fs_kernels.h"

namespace fsd {

// Q(x): the integer nearest to x * 2^20, ties to even; the product is exact for |x| < 2^14 and the result below 2^34.
__device__ __forceinline__ long long load_q(float x) { return (long long)rintf(x * (float)(1u << BODY_LOAD_SHIFT)); }

// v + (v of the lane SHR places below in the lane's row of 16, 0 where that leaves the row): one DPP move per half
template <int SHR>
__device__ __forceinline__ long long row_shr_add(long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u64)v, 0x110 + SHR, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((u64)v >> 32), 0x110 + SHR, 0xf, 0xf, true);
    return v + (long long)(((u64)(uint32_t)hi << 32) | (u64)(uint32_t)lo);
}

// The sum over the wave's 64 lanes, wave-uniform (all lanes active): four DPP steps leave each row's sum in its lane 15, the
// four row sums are read into scalar registers and added there.  No LDS traffic, unlike a __shfl_xor butterfly (measured first:
// 4 us slower with the paddle in the fluid, profiles/body_loads2d_cost.md).
__device__ __forceinline__ long long wave_sum(long long v) {
    v = row_shr_add<1>(v); v = row_shr_add<2>(v); v = row_shr_add<4>(v); v = row_shr_add<8>(v);
    const int lo = (int)(uint32_t)(u64)v, hi = (int)(uint32_t)((u64)v >> 32);
    u64 s = 0ull;
    for (int r = 15; r < 64; r += 16)
        s += ((u64)(uint32_t)__builtin_amdgcn_readlane(hi, r) << 32) | (u64)(uint32_t)__builtin_amdgcn_readlane(lo, r);
    return (long long)s;
}

// The fold's block k (one wave) owns word k = WORDS * kernel index + word of a shard table whose rows hold ROW words: lane r takes
// row r, zeroes what it found set for the next step, and lane 0 adds the wave's sum into the word of the body's slot.
template <uint32_t WORDS, uint32_t ROW>
__device__ __forceinline__ void body_loads_fold(const BodyLoadMap& M, u64* __restrict__ shards, u64* __restrict__ words) {
    static_assert(BODY_LOAD_SHARDS == 64u, "one wave holds a word's rows");
    const uint32_t k = blockIdx.x;                                        // < WORDS * M.count: the grid
    u64* const cell = shards + threadIdx.x * ROW + k;
    const u64 part = *cell;
    if (part != 0ull) *cell = 0ull;
    const u64 sum = (u64)wave_sum((long long)part);
    if (threadIdx.x == 0u && sum != 0ull) words[M.slot[k / WORDS] * WORDS + k % WORDS] += sum;
}

}  // namespace fsd

// fs_force_lists.h — the force pass's two lists of deferred waves: one definition of their layout for the kernels that
// write them (k_density: kernels_density.hip; the lean and quad force kernels), the kernel that reads them
// (k_force_general) and the allocation (engine.h).
//
// A wave the lean kernel k_force does not finish is handed to a later kernel by the 256-particle block it belongs to:
//   FS_LIST_PRE   the waves k_density names before the force launch (a row longer than 32 candidates, a tile that does not
//                 fit the LDS stage: dense clusters);
//   FS_LIST_LATE  the waves the lean kernel or k_force_quad gives up on itself (an operand outside the proven quotient
//                 ranges, a coincident pair in the quad kernel).
// Per list w:
//   defer_bits[force_defer_word(blk, w)]  bit k set: wave k of block blk is on list w (two words per block);
//   work_count[w]                         blocks on the list (zeroed by the reorder pass of the step);
//   worklist[force_list_base(n, w) + e]   block id of entry e < work_count[w]; a block is pushed once, by its first wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsd {

#define FS_LIST_PRE 0u
#define FS_LIST_LATE 1u

// First worklist entry of the late list for an array of n particles: behind the n / 256 (FS_BLOCK) entries the
// pre-registered list can hold, and 8 of slack.  (256: this header is also read by the host's engine.h, which does not see
// fs_neighbours.h; the units that push and read the lists assert FS_BLOCK == 256.)
__host__ __device__ __forceinline__ uint32_t force_late_base(uint32_t n) { return n / 256u + 8u; }
__host__ __device__ __forceinline__ uint32_t force_list_base(uint32_t n, uint32_t w) { return w ? force_late_base(n) : 0u; }
__host__ __device__ __forceinline__ uint32_t force_defer_word(uint32_t blk, uint32_t w) { return 2u * blk + w; }
// Wave `wave` of block `blk` joins list w; the block's first wave puts the block on the list.  Called by one lane.
__device__ __forceinline__ void force_list_push(uint32_t* __restrict__ defer_bits, uint32_t* __restrict__ worklist,
                                                uint32_t* __restrict__ work_count, uint32_t n, uint32_t blk, uint32_t wave, uint32_t w) {
    const uint32_t old = atomicOr(&defer_bits[force_defer_word(blk, w)], 1u << wave);
    if (old == 0u) worklist[force_list_base(n, w) + atomicAdd(&work_count[w], 1u)] = blk;
}
// Which work item a workgroup of a list-walking grid starts with (it then strides by the grid).  A list shorter than the
// grid would otherwise be worked off by the FIRST workgroups of the grid, neighbours in dispatch order, while most of the
// chip runs the workgroups that find nothing: grids of 40 k workgroups (sort_policy.h) deal consecutive items to the 8 XCDs
// and, inside an XCD, to workgroups five apart (1 M particles: force pass -1.5 us).  Other grids keep the plain order.
__device__ __forceinline__ uint32_t force_list_spread() {
    const uint32_t J = gridDim.x >> 3, j = blockIdx.x >> 3;
    const bool spread_ok = (gridDim.x & 7u) == 0u && J % 5u == 0u;
    return spread_ok ? (((j % 5u) * (J / 5u) + j / 5u) << 3) | (blockIdx.x & 7u) : blockIdx.x;
}
// Words of the worklist (both lists) and of defer_bits for `cap` slots.
static inline size_t force_worklist_words(size_t cap) { return 2 * (size_t)force_late_base((uint32_t)cap) + 16; }
static inline size_t force_defer_words(size_t cap) { return 2 * ((cap + 255) / 256 + 8); }

}  // namespace fsd

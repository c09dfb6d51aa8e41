// kernels_track.hip — opt-in particle tracking (build extension): a u32 id and up to FS_TRACK_MAX_CHANNELS
// f32 channels per particle that every step permutes exactly as it permutes the particle records.
//
// Both sort modes leave, in the low word of pairs[i], the slot that the particle now in slot i held before the step
// (k_reorder, kernels_reorder.hip; k_cs_fixreorder, kernels_csort.hip).  k_track_carry gathers through that word once per step:
//     id_out[i] = id_in[src],  attr_out[c][i] = attr_in[c][src]     (bit copies)
// It reads no simulation state and writes none, so the step computes the same bits with tracking on or off.
#include <hip/hip_runtime.h>

#include "fs_device.h"
#include "fs_kernels.h"

namespace fsd {

#define FS_TRACK_BLOCK 256

// C is a template argument: no form loops over a run-time count, and C = 0 moves 12 B per particle (4 B pair word, 4 B id in,
// 4 B id out).  The pair words and the stores are coalesced; the gathers are element-granular through a nearly sorted index
// (the input order is the previous step's cell order), so they are served by L2 lines their neighbours in the wave share.
// Channels move as 32-bit words: a bit copy, whatever the float they encode.
template <int C>
__global__ __launch_bounds__(FS_TRACK_BLOCK) void k_track_carry(uint32_t n, const uint32_t* __restrict__ pair_words,
                                                                const uint32_t* __restrict__ id_in, uint32_t* __restrict__ id_out,
                                                                const uint32_t* __restrict__ attr_in, uint32_t* __restrict__ attr_out,
                                                                uint32_t stride) {
    const uint32_t i = blockIdx.x * FS_TRACK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = pair_words[2u * i];     // little-endian: the low word of the 8-byte (key, source slot) pair
    if (src >= n) return;                        // never for i < n (padding sorts last); a corrupt pair must not read out of bounds
    uint32_t a[C > 0 ? C : 1];
    const uint32_t id = id_in[src];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = attr_in[(size_t)c * stride + src];    // all gathers in flight before the first store
    id_out[i] = id;
#pragma unroll
    for (int c = 0; c < C; ++c) attr_out[(size_t)c * stride + i] = a[c];
}

__global__ __launch_bounds__(FS_TRACK_BLOCK) void k_track_iota(uint32_t n, uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * FS_TRACK_BLOCK + threadIdx.x;
    if (i < n) id[i] = i;
}

void launch_track_carry(hipStream_t st, uint32_t n, int channels, const u64* pairs, const uint32_t* id_in, uint32_t* id_out,
                        const float* attr_in, float* attr_out, uint32_t stride) {
    if (n == 0) return;
    const dim3 grid((n + FS_TRACK_BLOCK - 1) / FS_TRACK_BLOCK), block(FS_TRACK_BLOCK);
    const uint32_t* pw = (const uint32_t*)pairs;
    const uint32_t* ai = (const uint32_t*)attr_in;
    uint32_t* ao = (uint32_t*)attr_out;
    switch (channels) {
        case 0: hipLaunchKernelGGL(k_track_carry<0>, grid, block, 0, st, n, pw, id_in, id_out, ai, ao, stride); break;
        case 1: hipLaunchKernelGGL(k_track_carry<1>, grid, block, 0, st, n, pw, id_in, id_out, ai, ao, stride); break;
        case 2: hipLaunchKernelGGL(k_track_carry<2>, grid, block, 0, st, n, pw, id_in, id_out, ai, ao, stride); break;
        case 3: hipLaunchKernelGGL(k_track_carry<3>, grid, block, 0, st, n, pw, id_in, id_out, ai, ao, stride); break;
        default: hipLaunchKernelGGL(k_track_carry<4>, grid, block, 0, st, n, pw, id_in, id_out, ai, ao, stride); break;
    }
}

void launch_track_iota(hipStream_t st, uint32_t n, uint32_t* id) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_track_iota, dim3((n + FS_TRACK_BLOCK - 1) / FS_TRACK_BLOCK), dim3(FS_TRACK_BLOCK), 0, st, n, id);
}

}  // namespace fsd

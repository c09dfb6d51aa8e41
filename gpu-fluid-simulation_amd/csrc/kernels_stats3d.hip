// kernels_stats3d.hip — fluid diagnostics of the 3D handle (include/fluidsim.h "3D fluid diagnostics"): k3_stats,
// one streaming pass over pos, vel and pred (.w: the density) as launch3_export reads them.  Chunks of STATS_CHUNK = 512 particles
// as in kernels_stats.hip; a record is three 16-byte loads, so lane t of a chunk takes the records t and 256 + t (contiguous over
// the wave) and, independently — a channel is summed over all slots, whatever the record — the channel values 2t and 2t + 1 in
// one 8-byte load.  The fold is kernels_stats.hip's.
#include <hip/hip_runtime.h>

#include "fs_3d.h"
#include "fs_stats.h"

namespace fsd {

template <int C>
__global__ __launch_bounds__(STATS_THREADS) void k3_stats(Stats3Input I, u64* __restrict__ slab) {
    StatsAcc<3> A;
    A.init();
    const uint32_t full = I.n / STATS_CHUNK;
    const bool wide = (I.attr_stride & 1u) == 0u;                    // every channel row starts on 8 bytes
    for (uint32_t chunk = blockIdx.x; chunk < full; chunk += gridDim.x) {
        const uint32_t base = chunk * STATS_CHUNK;                   // base + 511 < n
        const uint32_t i0 = base + threadIdx.x, i1 = i0 + STATS_THREADS;
        const float4 p0 = I.pos[i0], p1 = I.pos[i1], v0 = I.vel[i0], v1 = I.vel[i1], q0 = I.pred[i0], q1 = I.pred[i1];
        float a0[C ? C : 1], a1[C ? C : 1];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* row = I.attr + (size_t)c * I.attr_stride + base;
            if (wide) {
                const float2 a = ((const float2*)row)[threadIdx.x];  // base is even
                a0[c] = a.x; a1[c] = a.y;
            } else {
                a0[c] = row[threadIdx.x]; a1[c] = row[threadIdx.x + STATS_THREADS];
            }
        }
        const float pa[3] = {p0.x, p0.y, p0.z}, va[3] = {v0.x, v0.y, v0.z}, pb[3] = {p1.x, p1.y, p1.z}, vb[3] = {v1.x, v1.y, v1.z};
        stats_record<3>(A, pa, va, q0.w);
        stats_record<3>(A, pb, vb, q1.w);
#pragma unroll
        for (int c = 0; c < C; ++c) { stats_attr<3>(A, c, a0[c]); stats_attr<3>(A, c, a1[c]); }
    }
    if (I.n % STATS_CHUNK != 0u && full % gridDim.x == blockIdx.x) {  // the ragged chunk, in the turn of the block it falls to
        for (uint32_t i = full * STATS_CHUNK + threadIdx.x; i < I.n; i += STATS_THREADS) {
            const float4 p = I.pos[i], v = I.vel[i];
            const float pa[3] = {p.x, p.y, p.z}, va[3] = {v.x, v.y, v.z};
            stats_record<3>(A, pa, va, I.pred[i].w);
#pragma unroll
            for (int c = 0; c < C; ++c) stats_attr<3>(A, c, I.attr[(size_t)c * I.attr_stride + i]);
        }
    }
    stats_block_store<3>(A, slab + (size_t)blockIdx.x * stats_words(3));
}

// ------------------------------------------------------------------------------------ launcher (fs_3d.h)
void launch3_stats(hipStream_t st, const Stats3Input& I, unsigned long long* slab, void* out) {
    const uint32_t blocks = stats_blocks(I.n);
    const dim3 g(blocks), b(STATS_THREADS);
    switch (I.channels) {
    case 0: hipLaunchKernelGGL(k3_stats<0>, g, b, 0, st, I, slab); break;
    case 1: hipLaunchKernelGGL(k3_stats<1>, g, b, 0, st, I, slab); break;
    case 2: hipLaunchKernelGGL(k3_stats<2>, g, b, 0, st, I, slab); break;
    case 3: hipLaunchKernelGGL(k3_stats<3>, g, b, 0, st, I, slab); break;
    default: hipLaunchKernelGGL(k3_stats<4>, g, b, 0, st, I, slab); break;
    }
    launch_stats_fold(st, 3, slab, blocks, I.n, I.tick, I.channels, out);
}

}  // namespace fsd

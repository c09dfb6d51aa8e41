// kernels_stats.hip — fluid diagnostics of the 2D handle (include/fluidsim.h "fluid diagnostics"): k_stats, one
// streaming pass over the arrays a download would export, and k_stats_fold for both handles.  Nothing here is part of a step.
// A block takes chunks of STATS_CHUNK = 512 consecutive particles, chunk = blockIdx.x, + gridDim.x, ...; lane t of a chunk takes
// the particles 2t and 2t + 1, so that every load of a full chunk is 16 bytes (8 for `rho` and a channel row) and a wave's loads
// are contiguous.  The one ragged chunk at the end goes element by element, with bounds.
#include <hip/hip_runtime.h>

#include "fs_stats.h"

namespace fsd {

template <int C>
__global__ __launch_bounds__(STATS_THREADS) void k_stats(StatsInput I, u64* __restrict__ slab) {
    StatsAcc<2> A;
    A.init();
    const uint32_t full = I.n / STATS_CHUNK;
    const float4* __restrict__ pos2 = (const float4*)I.pos;
    const float4* __restrict__ vel2 = (const float4*)I.vel;
    const bool wide = (I.attr_stride & 1u) == 0u;                    // every channel row starts on 8 bytes
    for (uint32_t chunk = blockIdx.x; chunk < full; chunk += gridDim.x) {
        const uint32_t j = chunk * STATS_THREADS + threadIdx.x;      // the pair: particles 2j, 2j + 1 < full * 512 <= n
        const float4 p = pos2[j], v = vel2[j];
        float r0, r1;
        if (I.rho2) {
            const float4 r = ((const float4*)I.rho2)[j];
            r0 = r.x; r1 = r.z;
        } else {
            const float2 r = ((const float2*)I.rho)[j];
            r0 = r.x; r1 = r.y;
        }
        float a0[C ? C : 1], a1[C ? C : 1];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* row = I.attr + (size_t)c * I.attr_stride;
            if (wide) {
                const float2 a = ((const float2*)row)[j];
                a0[c] = a.x; a1[c] = a.y;
            } else {
                a0[c] = row[2u * j]; a1[c] = row[2u * j + 1u];
            }
        }
        const float pa[2] = {p.x, p.y}, va[2] = {v.x, v.y}, pb[2] = {p.z, p.w}, vb[2] = {v.z, v.w};
        stats_record<2>(A, pa, va, r0);
        stats_record<2>(A, pb, vb, r1);
#pragma unroll
        for (int c = 0; c < C; ++c) { stats_attr<2>(A, c, a0[c]); stats_attr<2>(A, c, a1[c]); }
    }
    if (I.n % STATS_CHUNK != 0u && full % gridDim.x == blockIdx.x) {  // the ragged chunk, in the turn of the block it falls to
        for (uint32_t i = full * STATS_CHUNK + threadIdx.x; i < I.n; i += STATS_THREADS) {
            const float2 p = I.pos[i], v = I.vel[i];
            const float pa[2] = {p.x, p.y}, va[2] = {v.x, v.y};
            stats_record<2>(A, pa, va, I.rho2 ? I.rho2[i].x : I.rho[i]);
#pragma unroll
            for (int c = 0; c < C; ++c) stats_attr<2>(A, c, I.attr[(size_t)c * I.attr_stride + i]);
        }
    }
    stats_block_store<2>(A, slab + (size_t)blockIdx.x * stats_words(2));
}

template <int D>
__global__ __launch_bounds__(64) void k_stats_fold(const u64* __restrict__ slab, uint32_t rows, uint32_t n, uint32_t tick,
                                                   uint32_t channels, unsigned char* __restrict__ out) {
    stats_fold<D>(slab, rows, n, tick, channels, out);
}

// ------------------------------------------------------------------------------------ launchers (fs_kernels.h)
void launch_stats_fold(hipStream_t st, int dims, const unsigned long long* slab, uint32_t rows, uint32_t n, uint32_t tick,
                       int channels, void* out) {
    if (dims == 2)
        hipLaunchKernelGGL(k_stats_fold<2>, dim3(stats_words(2)), dim3(64), 0, st, slab, rows, n, tick, (uint32_t)channels, (unsigned char*)out);
    else
        hipLaunchKernelGGL(k_stats_fold<3>, dim3(stats_words(3)), dim3(64), 0, st, slab, rows, n, tick, (uint32_t)channels, (unsigned char*)out);
}

void launch_stats(hipStream_t st, const StatsInput& I, unsigned long long* slab, void* out) {
    const uint32_t blocks = stats_blocks(I.n);
    const dim3 g(blocks), b(STATS_THREADS);
    switch (I.channels) {
    case 0: hipLaunchKernelGGL(k_stats<0>, g, b, 0, st, I, slab); break;
    case 1: hipLaunchKernelGGL(k_stats<1>, g, b, 0, st, I, slab); break;
    case 2: hipLaunchKernelGGL(k_stats<2>, g, b, 0, st, I, slab); break;
    case 3: hipLaunchKernelGGL(k_stats<3>, g, b, 0, st, I, slab); break;
    default: hipLaunchKernelGGL(k_stats<4>, g, b, 0, st, I, slab); break;
    }
    launch_stats_fold(st, 2, slab, blocks, I.n, I.tick, I.channels, out);
}

}  // namespace fsd

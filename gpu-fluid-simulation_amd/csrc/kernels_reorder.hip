// kernels_reorder.hip — the payload gather after the sort, the dense cell-start table, the AoS <-> SoA boundary.
// Device state is SoA (float2 pos / vel / pred, f32 density): coalesced 8-byte
// per-lane streams instead of the reference's 32-byte AoS records.
//   (predict_next_position + create_spatial_lookup, compute.wgsl:8-42, are fused into the first
//    kernel of the sort: kernels_sort_tile.inc k_bitonic_local<INIT, KEYGEN> / kernels_csort.hip k_cs_hist)
//   k_reorder       = payload gather after the (key,index) sort + compute_start_indices
//                     (compute.wgsl:45-56) + dense cell-start table
#include "fs_kernels.h"
#include "fs_neighbours.h"

namespace fsd {

// --------------------------------------------------- dense cell-start table fill
// cs[c] = index of the first sorted particle whose key is >= c (c in [0, ncell]).
// Short gaps are written by the boundary lane; long gaps go to a worklist.
__global__ __launch_bounds__(FS_BLOCK) void k_fill_gaps(uint32_t* __restrict__ cs, const GapEntry* __restrict__ work,
                                                        const uint32_t* __restrict__ counter, uint32_t work_cap) {
    uint32_t count = *counter;
    if (count > work_cap) count = work_cap;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const GapEntry g = work[e];
        for (uint32_t c = g.begin + threadIdx.x; c < g.end; c += FS_BLOCK) cs[c] = g.value;
    }
}

// -------------------------------------------------------------------- reorder
// Gathers the payload into cell order (the reference swaps whole 32-byte records
// inside the sort, sort.wgsl:44-50; sorting (key,index) pairs and gathering once
// gives the identical arrangement because the network only looks at keys).
template <bool FILL>
__global__ __launch_bounds__(FS_BLOCK) void k_reorder(StepParams P, const u64* __restrict__ pairs,
                                                      const float2* __restrict__ pos_in,
                                                      const float2* __restrict__ vel_in, float2* __restrict__ pos_s,
                                                      float2* __restrict__ vel_s, float2* __restrict__ pred_s,
                                                      uint32_t* __restrict__ key_s, uint32_t* __restrict__ cs,
                                                      uint32_t* __restrict__ start_ref, GapEntry* __restrict__ work,
                                                      uint32_t* __restrict__ counter, uint32_t work_cap,
                                                      unsigned long long* __restrict__ safe, uint32_t* __restrict__ force_defer,
                                                      uint32_t* __restrict__ force_work_count) {
    const uint32_t i = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (threadIdx.x == 0) {                      // the force pass's worklists of this step (same block size and count)
        force_defer[2u * blockIdx.x] = 0u;       // [2 blk] pre-registered by k_density, [2 blk + 1] found late by k_force
        force_defer[2u * blockIdx.x + 1u] = 0u;
        if (blockIdx.x == 0) { force_work_count[0] = 0u; force_work_count[1] = 0u; }
    }
    if (i >= P.n) return;
    const u64 pr = pairs[i];
    const uint32_t key = (uint32_t)(pr >> 32);
    const uint32_t src = (uint32_t)pr;
    const float2 p = pos_in[src];
    const float2 v = vel_in[src];
    if (pos_s) pos_s[i] = p;                  // uniform; nullptr: the force pass reads pos_in[src] itself (StepParams::pos_by_src)
    vel_s[i] = v;
    const float2 pd = predict_pos(P, p, v);   // same expression as the key generation in the sort -> same bits
    pred_s[i] = pd;
    if (key_s) key_s[i] = key;                // uniform; single-domain handles read the key back from `pairs` instead
    {   // fs_device.h "safe operand" classification (finished by k_density): one 64-bit word per wave
        const unsigned long long sb = __builtin_amdgcn_ballot_w64(kin_safe(pd, v));   // lanes that returned above: 0
        if ((threadIdx.x & 63u) == 0u) safe[i >> 6] = sb;
    }

    const uint32_t kc = key < P.ncell ? key : P.ncell;   // clamp for table writes only
    if (i == 0) {
        if (!P.ref_quirks && key < P.ncell) start_ref[key] = 0;   // compute.wgsl:50 skips index 0
        if (FILL) fill_cells(cs, 0u, kc + 1u, 0u, work, counter, work_cap);
    } else {
        const uint32_t prev = (uint32_t)(pairs[i - 1] >> 32);
        if (key != prev) {
            if (key < P.ncell) start_ref[key] = i;                // compute.wgsl:53-55
            const uint32_t pc = prev < P.ncell ? prev : P.ncell;
            if (FILL) fill_cells(cs, pc + 1u, kc + 1u, i, work, counter, work_cap);
        }
    }
    if (FILL && i == P.n - 1) fill_cells(cs, kc + 1u, P.ncell + 1u, P.n, work, counter, work_cap);
}

// --------------------------------------------------------------- AoS <-> SoA

__global__ __launch_bounds__(FS_BLOCK) void k_export_aos(uint32_t n, const float2* __restrict__ pos,
                                                         const float2* __restrict__ pred,
                                                         const float2* __restrict__ vel,
                                                         const float* __restrict__ rho,
                                                         const uint32_t* __restrict__ key,
                                                         const u64* __restrict__ pairs,
                                                         const float2* __restrict__ rho2,
                                                         AosParticle* __restrict__ out) {
    const uint32_t i = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i >= n) return;
    AosParticle a;
    a.position = pos[i]; a.predicted = pred[i]; a.velocity = vel[i]; a.density = rho2 ? rho2[i].x : rho[i];
    a.grid = pairs ? (uint32_t)(pairs[i] >> 32) : key[i];     // after a step the sorted (key, source) pairs hold the keys
    out[i] = a;
}

__global__ __launch_bounds__(FS_BLOCK) void k_import_aos(uint32_t n, const AosParticle* __restrict__ in,
                                                         float2* __restrict__ pos, float2* __restrict__ pred,
                                                         float2* __restrict__ vel, float* __restrict__ rho,
                                                         uint32_t* __restrict__ key) {
    const uint32_t i = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const AosParticle a = in[i];
    pos[i] = a.position; pred[i] = a.predicted; vel[i] = a.velocity; rho[i] = a.density; key[i] = a.grid;
}

// The launchers unpack StepArrays in the kernel's parameter order.
void launch_reorder(hipStream_t st, const StepParams& P, const StepArrays& A, uint32_t work_cap, bool cs_ready) {
    if (cs_ready) {   // counting sort already produced the dense table
        hipLaunchKernelGGL(k_reorder<false>, dim3(nblk(P.n)), dim3(FS_BLOCK), 0, st, P, A.pairs, A.pos, A.vel, A.pos_s,
                           A.vel_s, A.pred, A.key_s, A.cs, A.start_ref, (GapEntry*)A.work, A.counter, work_cap, A.safe, A.fdefer, A.fcount);
        return;
    }
    hipLaunchKernelGGL(k_reorder<true>, dim3(nblk(P.n)), dim3(FS_BLOCK), 0, st, P, A.pairs, A.pos, A.vel, A.pos_s, A.vel_s,
                       A.pred, A.key_s, A.cs, A.start_ref, (GapEntry*)A.work, A.counter, work_cap, A.safe, A.fdefer, A.fcount);
    hipLaunchKernelGGL(k_fill_gaps, dim3(1024), dim3(FS_BLOCK), 0, st, A.cs, (const GapEntry*)A.work, A.counter, work_cap);
}

void launch_export_aos(hipStream_t st, uint32_t n, const float2* pos, const float2* pred, const float2* vel,
                       const float* rho, const uint32_t* key, void* out, const u64* pairs, const float2* rho2) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_export_aos, dim3(nblk(n)), dim3(FS_BLOCK), 0, st, n, pos, pred, vel, rho, key, pairs, rho2,
                       (AosParticle*)out);
}

__global__ __launch_bounds__(FS_BLOCK) void k_keys_from_pairs(uint32_t n, const u64* __restrict__ pairs, uint32_t* __restrict__ key,
                                                              const float2* __restrict__ rho2, float* __restrict__ rho) {
    const uint32_t i = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (pairs) key[i] = (uint32_t)(pairs[i] >> 32);
    if (rho2) rho[i] = rho2[i].x;
}
void launch_keys_from_pairs(hipStream_t st, uint32_t n, const u64* pairs, uint32_t* key, const float2* rho2, float* rho) {
    if (n) hipLaunchKernelGGL(k_keys_from_pairs, dim3(nblk(n)), dim3(FS_BLOCK), 0, st, n, pairs, key, rho2, rho);
}

void launch_import_aos(hipStream_t st, uint32_t n, const void* in, float2* pos, float2* pred, float2* vel, float* rho,
                       uint32_t* key) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_import_aos, dim3(nblk(n)), dim3(FS_BLOCK), 0, st, n, (const AosParticle*)in, pos, pred, vel,
                       rho, key);
}

size_t gap_entry_size() { return sizeof(GapEntry); }

void launch_fill_gaps(hipStream_t st, uint32_t* cs, const void* work, const uint32_t* counter, uint32_t work_cap) {
    hipLaunchKernelGGL(k_fill_gaps, dim3(1024), dim3(FS_BLOCK), 0, st, cs, (const GapEntry*)work, counter, work_cap);
}

}  // namespace fsd

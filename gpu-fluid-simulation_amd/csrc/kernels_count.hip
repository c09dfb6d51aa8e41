// kernels_count.hip — the 2D device passes of a particle count that changes at run time (build extension, DESIGN.md §22;
// include/fluidsim.h "2D particle count"): the nozzle that appends generated records, the box test of a removal and the
// scatter of its stable compaction.  No reference counterpart (the reference's count is fixed).
//
// The shape is that of kernels_count3d.hip — 256-lane workgroups, stream-ordered launches, no atomics, nothing waits on
// another workgroup — and the passes without a dimension in them are that file's: the offsets workgroup over the
// per-workgroup survivor sums, the count of a caller's flags, and tracking's share of an emission.  Both files' flags passes
// leave the same `sums`, so either feeds the one offsets pass.
//   k_emit_nozzle      one lane per record: slots [count, count + M) of pos, pred, vel, rho, key (the host offsets the arrays)
//   k_remove_box       one lane per slot: the inclusive box test -> the kill flag, and per-workgroup survivor sums
//   k_remove_scatter   the flags again, a workgroup scan -> the survivor's slot; out of place, into arrays the pass does not read
#include <hip/hip_runtime.h>

#include "fs_kernels.h"
#include "fs_scan.h"

namespace fsd {

#define BC 256                     // workgroup of every pass: four waves (the block of kernels_count3d.hip's flags pass)

// position.c = (origin.c + sa * u.c) + sb * v.c, f32 without contraction (the build's -ffp-contract=off)
__global__ __launch_bounds__(BC) void k_emit_nozzle(Nozzle2 Z, uint32_t m, float2* __restrict__ pos, float2* __restrict__ pred,
                                                    float2* __restrict__ vel, float* __restrict__ rho, uint32_t* __restrict__ key) {
    const uint32_t q = blockIdx.x * BC + threadIdx.x;
    if (q >= m) return;
    const uint32_t a = q % Z.nu, b = q / Z.nu;
    const float sa = ((float)a + 0.5f) - 0.5f * (float)Z.nu;
    const float sb = ((float)b + 0.5f) - 0.5f * (float)Z.nv;
    const float x = (Z.origin.x + sa * Z.u.x) + sb * Z.v.x;
    const float y = (Z.origin.y + sa * Z.u.y) + sb * Z.v.y;
    pos[q] = make_float2(x, y);
    pred[q] = make_float2(x, y);
    vel[q] = Z.velocity;
    rho[q] = 0.0f;
    key[q] = 0u;
}

// flags[i] = lo.a <= position.a <= hi.a on both axes (a NaN coordinate fails every comparison: kept), stored for the scatter.
// sums[workgroup] = survivors among its slots.
__global__ __launch_bounds__(BC) void k_remove_box(uint32_t n, const float2* __restrict__ pos, float2 lo, float2 hi,
                                                   uint8_t* __restrict__ flags, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[BC / 64];
    const uint32_t i = blockIdx.x * BC + threadIdx.x;
    uint32_t keep = 0u;
    if (i < n) {
        const float2 p = pos[i];
        const bool kill = lo.x <= p.x && p.x <= hi.x && lo.y <= p.y && p.y <= hi.y;
        flags[i] = kill ? 1u : 0u;
        keep = kill ? 0u : 1u;
    }
    uint32_t total;
    (void)block_scan3<BC / 64>(keep, s_wave, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// Survivor i goes to slot sums[workgroup] + its rank among the workgroup's survivors (< the survivors' total <= n).  Bit copies.
__global__ __launch_bounds__(BC) void k_remove_scatter(uint32_t n, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums,
                                                       Compact2 C) {
    __shared__ uint32_t s_wave[BC / 64];
    const uint32_t i = blockIdx.x * BC + threadIdx.x;
    const uint32_t keep = (i < n && flags[i] == 0u) ? 1u : 0u;
    uint32_t total;
    const uint32_t excl = block_scan3<BC / 64>(keep, s_wave, &total);
    if (!keep) return;
    const uint32_t d = sums[blockIdx.x] + excl;
    C.pos_out[d] = C.pos[i];
    C.vel_out[d] = C.vel[i];
    C.pred_out[d] = C.pred[i];
    C.rho_out[d] = C.rho[i];           // (as words: a NaN's payload survives)
    C.key_out[d] = C.key[i];
    if (C.ids) {
        C.ids_out[d] = C.ids[i];
        for (int c = 0; c < C.channels; ++c) C.attr_out[(size_t)c * C.stride + d] = C.attr[(size_t)c * C.stride + i];
    }
}

// ------------------------------------------------------------------------------------ launchers (fs_kernels.h)
void launch_emit_nozzle(hipStream_t st, const Nozzle2& Z, float2* pos, float2* pred, float2* vel, float* rho, uint32_t* key) {
    const uint32_t m = Z.nu * Z.nv;                                 // <= 2^28: the host's check
    hipLaunchKernelGGL(k_emit_nozzle, dim3((m + BC - 1u) / BC), dim3(BC), 0, st, Z, m, pos, pred, vel, rho, key);
}

void launch_remove_box(hipStream_t st, uint32_t n, const float2* pos, float2 lo, float2 hi, uint8_t* flags, uint32_t* sums) {
    const uint32_t nwg = remove_workgroups(n);
    hipLaunchKernelGGL(k_remove_box, dim3(nwg), dim3(BC), 0, st, n, pos, lo, hi, flags, sums);
    launch_remove_offsets(st, nwg, sums);
}

void launch_remove_scatter(hipStream_t st, uint32_t n, const uint8_t* flags, const uint32_t* sums, const Compact2& C) {
    hipLaunchKernelGGL(k_remove_scatter, dim3(remove_workgroups(n)), dim3(BC), 0, st, n, flags, sums, C);
}

}  // namespace fsd

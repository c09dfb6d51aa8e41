// kernels_count.hip — the device passes of a particle count that changes at run time, for both handles (build extension,
// DESIGN.md §21 and §22; include/fluidsim.h "3D particle count", "2D particle count"; the launchers' list: fs_count.h): the
// nozzles that append generated records, and the stable compaction of a removal.  No reference counterpart (the reference is
// 2D only and its count is fixed).
//
// Emission writes slots [count, count + M) of the state arrays and, with tracking on, their ids and channels; the host passes
// the arrays already offset by `count`.
//
// Removal, in the shape of kernels_mesh3d.hip — 256-lane workgroups, stream-ordered launches, nothing waits on another
// workgroup, no atomics: every survivor's new slot is a prefix sum of the keep flags in slot order, so the compaction is stable.
//   a flags pass   one lane per slot: the kill flag (the inclusive box test, or the caller's flags) and per-workgroup survivor sums
//   the offsets    ONE workgroup over the <= 2^20 sums: sums -> exclusive offsets, the survivors' total behind them
//   a scatter      the flags again, a workgroup scan -> the survivor's slot; out of place, into arrays the pass does not read
// In place would be a race between workgroups (a survivor's new slot belongs to a lower workgroup that may not have read it yet).
// Every flags pass leaves the same `sums`, so each feeds the one offsets pass.
#include <hip/hip_runtime.h>

#include "fs_3d.h"
#include "fs_scan.h"

namespace fsd {

#define BC 256                     // workgroup of every pass but the offsets: four waves
#define BC_SCAN 1024               // the offsets' single workgroup

// ------------------------------------------------------------------------------------ the dimension-free passes
// Three kernels that touch no position serve both handles.  They carry the 3D prefix because the 3D handle had the feature
// first, and a kernel's name is what the device-code comparison of two trees (tools/isa_compare.py) matches by: they keep it.
// k3_remove_flags<false> is the flags pass over a caller's flags; its position and box arguments are not read.

// ids[q] = first + q (wrapping) and +0.0f in every channel, for the m slots emitted; channel c at attr + c * stride
__global__ __launch_bounds__(BC) void k3_emit_track(uint32_t m, uint32_t first, uint32_t* __restrict__ ids, int channels,
                                                    float* __restrict__ attr, uint32_t stride) {
    const uint32_t q = blockIdx.x * BC + threadIdx.x;
    if (q >= m) return;
    ids[q] = first + q;
    for (int c = 0; c < channels; ++c) attr[(size_t)c * stride + q] = 0.0f;
}

// BOX (the 3D handle's): flags[i] = lo.a <= position.a <= hi.a on every axis (a NaN coordinate fails every comparison: kept),
// stored for the scatter; else the caller's flags are read.  sums[workgroup] = survivors among its slots.
template <bool BOX>
__global__ __launch_bounds__(BC) void k3_remove_flags(uint32_t n, const float4* __restrict__ pos, float3 lo, float3 hi,
                                                      uint8_t* __restrict__ flags, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[BC / 64];
    const uint32_t i = blockIdx.x * BC + threadIdx.x;
    uint32_t keep = 0u;
    if (i < n) {
        if (BOX) {
            const float4 p = pos[i];
            const bool kill = lo.x <= p.x && p.x <= hi.x && lo.y <= p.y && p.y <= hi.y && lo.z <= p.z && p.z <= hi.z;
            flags[i] = kill ? 1u : 0u;
            keep = kill ? 0u : 1u;
        } else {
            keep = flags[i] == 0u ? 1u : 0u;
        }
    }
    uint32_t total;
    (void)block_scan3<BC / 64>(keep, s_wave, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// One workgroup: thread t owns the sums [t * chunk, (t + 1) * chunk).  In place: sums -> exclusive offsets; sums[nwg] = survivors.
__global__ __launch_bounds__(BC_SCAN) void k3_remove_offsets(uint32_t nwg, uint32_t chunk, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[BC_SCAN / 64];
    const uint32_t lo = threadIdx.x * chunk < nwg ? threadIdx.x * chunk : nwg;
    const uint32_t hi = lo + chunk < nwg ? lo + chunk : nwg;
    uint32_t v = 0u;
    for (uint32_t b = lo; b < hi; ++b) v += sums[b];
    uint32_t total;
    uint32_t e = block_scan3<BC_SCAN / 64>(v, s_wave, &total);
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t s = sums[b];
        sums[b] = e;
        e += s;
    }
    if (threadIdx.x == 0u) sums[nwg] = total;
}

uint32_t remove_workgroups(uint32_t n) { return (n + BC - 1u) / BC; }

void launch_remove_offsets(hipStream_t st, uint32_t nwg, uint32_t* sums) {
    hipLaunchKernelGGL(k3_remove_offsets, dim3(1), dim3(BC_SCAN), 0, st, nwg, (nwg + BC_SCAN - 1u) / BC_SCAN, sums);
}

void launch_remove_count_flags(hipStream_t st, uint32_t n, const uint8_t* flags, uint32_t* sums) {
    const uint32_t nwg = remove_workgroups(n);
    hipLaunchKernelGGL(k3_remove_flags<false>, dim3(nwg), dim3(BC), 0, st, n, (const float4*)nullptr, float3{}, float3{},
                       const_cast<uint8_t*>(flags), sums);          // (BOX == false only reads them)
    launch_remove_offsets(st, nwg, sums);
}

void launch_emit_track(hipStream_t st, uint32_t m, uint32_t first_id, uint32_t* ids, int channels, float* attr, uint32_t stride) {
    hipLaunchKernelGGL(k3_emit_track, dim3((m + BC - 1u) / BC), dim3(BC), 0, st, m, first_id, ids, channels, attr, stride);
}

// ------------------------------------------------------------------------------------ the 2D passes
// position.c = (origin.c + sa * u.c) + sb * v.c, f32 without contraction (the build's -ffp-contract=off); slots of pos, pred,
// vel, rho, key
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

// ------------------------------------------------------------------------------------ the 3D passes
// as k_emit_nozzle; slots of pos, pred, vel, key
__global__ __launch_bounds__(BC) void k3_emit_nozzle(Nozzle3 Z, uint32_t m, float4* __restrict__ pos, float4* __restrict__ pred,
                                                     float4* __restrict__ vel, uint32_t* __restrict__ key) {
    const uint32_t q = blockIdx.x * BC + threadIdx.x;
    if (q >= m) return;
    const uint32_t a = q % Z.nu, b = q / Z.nu;
    const float sa = ((float)a + 0.5f) - 0.5f * (float)Z.nu;
    const float sb = ((float)b + 0.5f) - 0.5f * (float)Z.nv;
    const float x = (Z.origin.x + sa * Z.u.x) + sb * Z.v.x;
    const float y = (Z.origin.y + sa * Z.u.y) + sb * Z.v.y;
    const float z = (Z.origin.z + sa * Z.u.z) + sb * Z.v.z;
    pos[q] = make_float4(x, y, z, 0.0f);
    pred[q] = make_float4(x, y, z, 0.0f);                           // .w: density +0
    vel[q] = make_float4(Z.velocity.x, Z.velocity.y, Z.velocity.z, 0.0f);
    key[q] = 0u;
}

// as k_remove_scatter
__global__ __launch_bounds__(BC) void k3_remove_scatter(uint32_t n, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums,
                                                        Compact3 C) {
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
    C.key_out[d] = C.key[i];
    if (C.ids) {
        C.ids_out[d] = C.ids[i];
        for (int c = 0; c < C.channels; ++c) C.attr_out[(size_t)c * C.stride + d] = C.attr[(size_t)c * C.stride + i];
    }
}

void launch3_emit_nozzle(hipStream_t st, const Nozzle3& Z, uint32_t first_slot, const Arrays3& A) {
    const uint32_t m = Z.nu * Z.nv;                                 // <= 2^28: the host's check
    hipLaunchKernelGGL(k3_emit_nozzle, dim3((m + BC - 1u) / BC), dim3(BC), 0, st, Z, m, A.pos + first_slot, A.pred + first_slot,
                       A.vel + first_slot, A.key + first_slot);
}

void launch3_remove_box(hipStream_t st, uint32_t n, const float4* pos, float3 lo, float3 hi, uint8_t* flags, uint32_t* sums) {
    const uint32_t nwg = remove_workgroups(n);
    hipLaunchKernelGGL(k3_remove_flags<true>, dim3(nwg), dim3(BC), 0, st, n, pos, lo, hi, flags, sums);
    launch_remove_offsets(st, nwg, sums);
}

void launch3_remove_scatter(hipStream_t st, uint32_t n, const uint8_t* flags, const uint32_t* sums, const Compact3& C) {
    hipLaunchKernelGGL(k3_remove_scatter, dim3(remove_workgroups(n)), dim3(BC), 0, st, n, flags, sums, C);
}

}  // namespace fsd

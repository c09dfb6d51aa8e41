// fs_count.h — the device interface of a particle count that changes at run time (kernels_count.hip; DESIGN.md §21 for the 3D
// handle, §22 for the 2D one): what a kernel takes by value, and the launchers.  Device pointers; host side only.  Both launcher
// lists include it (fs_kernels.h, fs_3d.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsd {

struct Arrays3;                            // fs_3d.h

// ---- the passes without a dimension in them: what both handles call
uint32_t remove_workgroups(uint32_t n);    // `sums` holds one word per workgroup of a flags pass and one more, the survivors' total
// sums[w] = survivors (flags[i] == 0) among workgroup w's 256 slots of the caller's `flags`, then launch_remove_offsets
void launch_remove_count_flags(hipStream_t st, uint32_t n, const uint8_t* flags, uint32_t* sums);
// one workgroup: sums[w] -> survivors below workgroup w's slots, sums[nwg] = all
void launch_remove_offsets(hipStream_t st, uint32_t nwg, uint32_t* sums);
// Tracking's share of an emission of m records: ids[q] = first_id + q (wrapping), +0.0f in each channel (c at attr + c * stride);
// ids and attr point at the first emitted slot.
void launch_emit_track(hipStream_t st, uint32_t m, uint32_t first_id, uint32_t* ids, int channels, float* attr, uint32_t stride);

// ---- the 2D passes.  The nozzle of fs_emit_nozzle, by value: record q of nu * nv goes to element q of the five arrays, which
// the caller passes offset by the live count.
struct Nozzle2 {
    float2 origin, u, v, velocity;
    uint32_t nu, nv;
};
void launch_emit_nozzle(hipStream_t st, const Nozzle2& Z, float2* pos, float2* pred, float2* vel, float* rho, uint32_t* key);
// The removal's compaction: what the scatter reads and the arrays, none of them among those, it writes.  The densities move as
// words.  ids null: no tracking.
struct Compact2 {
    const float2 *pos, *vel, *pred;
    const uint32_t *rho, *key;
    float2 *pos_out, *vel_out, *pred_out;
    uint32_t *rho_out, *key_out;
    const uint32_t* ids;
    uint32_t* ids_out;
    const float* attr;
    float* attr_out;
    int channels;
    uint32_t stride;
};
// flags[i] = the inclusive box test of pos[i] (n bytes), the per-workgroup survivor sums, then launch_remove_offsets
void launch_remove_box(hipStream_t st, uint32_t n, const float2* pos, float2 lo, float2 hi, uint8_t* flags, uint32_t* sums);
void launch_remove_scatter(hipStream_t st, uint32_t n, const uint8_t* flags, const uint32_t* sums, const Compact2& C);

// ---- the 3D passes.  The nozzle of fs3_emit_nozzle, by value: record q of nu * nv goes to slot first_slot + q of pos, pred, vel
// and key.
struct Nozzle3 {
    float3 origin, u, v, velocity;
    uint32_t nu, nv;
};
void launch3_emit_nozzle(hipStream_t st, const Nozzle3& Z, uint32_t first_slot, const Arrays3& A);
// As Compact2; the density rides in pred.w.
struct Compact3 {
    const float4 *pos, *vel, *pred;
    const uint32_t* key;
    float4 *pos_out, *vel_out, *pred_out;
    uint32_t* key_out;
    const uint32_t* ids;
    uint32_t* ids_out;
    const float* attr;
    float* attr_out;
    int channels;
    uint32_t stride;
};
// as launch_remove_box
void launch3_remove_box(hipStream_t st, uint32_t n, const float4* pos, float3 lo, float3 hi, uint8_t* flags, uint32_t* sums);
void launch3_remove_scatter(hipStream_t st, uint32_t n, const uint8_t* flags, const uint32_t* sums, const Compact3& C);

}  // namespace fsd

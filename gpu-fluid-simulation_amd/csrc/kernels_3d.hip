// kernels_3d.hip — kernels of the 3D extension of the step (27-cell neighbour path) and their launchers (fs_3d.h).  NOT in the
// reference (2D only); build-defined per SURVEY.md Appendix B.3, normative statement oracle/sph_oracle3d.cpp.
// Same pass chain as 2D: predict+key -> bitonic (key,index) sort -> reorder + dense cell starts -> density -> force+integrate.
// SoA with 16-byte lanes: pos4 / vel4 / pred4 (xyz, pred.w carries the density for the force pass): a neighbour is two 16-B loads.
// Here: predict + key, reorder, import / export.  The passes that walk neighbours: kernels_density3d.hip (density, surface
// tension) and kernels_force3d.hip (force + integrate), over the sweep of fs_sweep3.h.
#include <hip/hip_runtime.h>

#include "../../include/fluidsim.h"
#include "fs_sweep3.h"     // B3F: blocks3()

static_assert(sizeof(fs3_particle) == 48, "fs3_particle is 48 bytes");

namespace fsd {

#define B3 256

__global__ __launch_bounds__(B3) void k3_predict_key(Params3 P, const float4* __restrict__ pos,
                                                     const float4* __restrict__ vel, u64* __restrict__ pairs,
                                                     uint32_t* __restrict__ gap_counter) {
    const uint32_t i = blockIdx.x * B3 + threadIdx.x;
    if (i == 0) *gap_counter = 0;
    if (i >= P.n) return;
    pairs[i] = ((u64)cell_key3(P, predict3(P, pos[i], vel[i])) << 32) | (u64)i;
}

__global__ __launch_bounds__(B3) void k3_reorder(Params3 P, const u64* __restrict__ pairs,
                                                 const float4* __restrict__ pos_in, const float4* __restrict__ vel_in,
                                                 float4* __restrict__ pos_s, float4* __restrict__ vel_s,
                                                 float4* __restrict__ pred, uint32_t* __restrict__ key_s,
                                                 uint32_t* __restrict__ cs, GapEntry* __restrict__ work,
                                                 uint32_t* __restrict__ counter, uint32_t work_cap) {
    const uint32_t i = blockIdx.x * B3 + threadIdx.x;
    if (i >= P.n) return;
    const u64 pr = pairs[i];
    const uint32_t key = (uint32_t)(pr >> 32), src = (uint32_t)pr;
    const float4 p = pos_in[src], v = vel_in[src];
    const float4 pd = predict3(P, p, v);
    // "safe operand" classification, kinematic part (fs_device.h): coordinates and velocity components 0 or >= 2^-53,
    // |v| <= 2^59 — carried as the sign of vel_s.w (the lane is free: a velocity has three components); k3_density
    // finishes it with the density / pressure bounds and leaves +-RN(1/rho) there for the force pass
    const bool ksafe = lo_safe(pd.x) && lo_safe(pd.y) && lo_safe(pd.z) && lo_safe(v.x) && lo_safe(v.y) && lo_safe(v.z) &&
                       fabsf(v.x) <= 0x1p59f && fabsf(v.y) <= 0x1p59f && fabsf(v.z) <= 0x1p59f;
    float4 vs = v;
    vs.w = ksafe ? 1.0f : -1.0f;
    // no sorted copy of the positions: k3_force takes its own particle's position from the previous state through the pair's
    // source index and writes the new state into the spare buffer (16 B / particle less in this HBM-bound pass)
    vel_s[i] = vs; pred[i] = pd; key_s[i] = key;
    const uint32_t kc = key < P.ncell ? key : P.ncell;
    if (i == 0) {
        fill_cells(cs, 0u, kc + 1u, 0u, work, counter, work_cap);
    } else {
        const uint32_t prev = (uint32_t)(pairs[i - 1] >> 32);
        if (key != prev) fill_cells(cs, (prev < P.ncell ? prev : P.ncell) + 1u, kc + 1u, i, work, counter, work_cap);
    }
    if (i == P.n - 1) fill_cells(cs, kc + 1u, P.ncell + 1u, P.n, work, counter, work_cap);
}

__global__ __launch_bounds__(B3) void k3_export(uint32_t n, const float4* __restrict__ pos, const float4* __restrict__ pred,
                                                const float4* __restrict__ vel, const uint32_t* __restrict__ key,
                                                fs3_particle* __restrict__ out) {
    const uint32_t i = blockIdx.x * B3 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pos[i], q = pred[i], v = vel[i];
    fs3_particle a;
    a.position = fs_vec3{p.x, p.y, p.z};
    a.predicted_position = fs_vec3{q.x, q.y, q.z};
    a.velocity = fs_vec3{v.x, v.y, v.z};
    a.density = q.w; a.grid = key[i]; a.pad = 0;
    out[i] = a;
}
__global__ __launch_bounds__(B3) void k3_import(uint32_t n, const fs3_particle* __restrict__ in, float4* __restrict__ pos,
                                                float4* __restrict__ pred, float4* __restrict__ vel,
                                                uint32_t* __restrict__ key) {
    const uint32_t i = blockIdx.x * B3 + threadIdx.x;
    if (i >= n) return;
    const fs3_particle a = in[i];
    pos[i] = make_float4(a.position.x, a.position.y, a.position.z, 0.0f);
    pred[i] = make_float4(a.predicted_position.x, a.predicted_position.y, a.predicted_position.z, a.density);
    vel[i] = make_float4(a.velocity.x, a.velocity.y, a.velocity.z, 0.0f);
    key[i] = a.grid;
}

// ------------------------------------------------------------------------------------ launchers (fs_3d.h)
uint32_t blocks3(uint32_t n) { return (n + B3F - 1) / B3F; }

void launch3_predict_key(hipStream_t st, const Params3& P, const Arrays3& A) {
    hipLaunchKernelGGL(k3_predict_key, dim3((P.n + B3 - 1) / B3), dim3(B3), 0, st, P, A.pos, A.vel, A.pairs, A.counter);
}

void launch3_reorder(hipStream_t st, const Params3& P, const Arrays3& A) {
    hipLaunchKernelGGL(k3_reorder, dim3((P.n + B3 - 1) / B3), dim3(B3), 0, st, P, A.pairs, A.pos, A.vel, A.pos_out, A.vel_s, A.pred,
                       A.key, A.cs, (GapEntry*)A.work, A.counter, A.work_cap);
    launch_fill_gaps(st, A.cs, A.work, A.counter, A.work_cap);
}

void launch3_import(hipStream_t st, uint32_t n, const Arrays3& A) {
    hipLaunchKernelGGL(k3_import, dim3((n + B3 - 1) / B3), dim3(B3), 0, st, n, (const fs3_particle*)A.aos, A.pos, A.pred, A.vel, A.key);
}

void launch3_export(hipStream_t st, uint32_t n, const Arrays3& A) {
    hipLaunchKernelGGL(k3_export, dim3((n + B3 - 1) / B3), dim3(B3), 0, st, n, A.pos, A.pred, A.vel, A.key, (fs3_particle*)A.aos);
}

}  // namespace fsd

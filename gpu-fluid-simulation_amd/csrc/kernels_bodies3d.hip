// kernels_bodies3d.hip — the opt-in moving bodies of the 3D step (build extension): the operators B_0 .. B_7 of
// include/fluidsim.h "3D moving bodies" on the position and velocity the force pass just stored, one streaming pass behind it.
// A pass of its own and no further flag on force3_body (kernels_force3d.hip): that kernel's instantiations sit at a pinned 128
// VGPRs with a spill-free tail, and a handle without bodies must launch what it launched before.
// One lane per particle.  The bodies come by value (fs_3d.h Bodies3, about 1 KB of kernel arguments): everything per body is
// wave-uniform and stays in SGPRs.  A lane reads its 16-byte position; it reads its velocity only once a body hits it and stores
// both only then, so a particle no body touches costs 16 bytes.  The early-out is the statement's own box test — nothing
// coarser: a bounding sphere can reject a corner particle by rounding.  No LDS, no atomics, nothing waits on another workgroup;
// every voxel index is clamped, so no position reads outside a field.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "fs_3d.h"
#include "fs_device.h"

namespace fsd {

#define B3B 256

__device__ __forceinline__ uint32_t body_voxel3(float q, float hb, float extent, uint32_t w) {
    const uint32_t i = f32_to_u32_sat(__fdiv_rn(q + hb, extent) * (float)w);
    return i < w - 1u ? i : w - 1u;
}

__global__ __launch_bounds__(B3B) void k3_bodies(Bodies3 B, uint32_t n, float bx, float by, float bz, float damping,
                                                 float4* __restrict__ pos, float4* __restrict__ vel) {
    const uint32_t i = blockIdx.x * B3B + threadIdx.x;
    if (i >= n) return;
    float4 p = pos[i], v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool hit = false;
    for (uint32_t b = 0; b < B.count; ++b) {
        const Body3& K = B.body[b];
        const float dx = p.x - K.cx, dy = p.y - K.cy, dz = p.z - K.cz;
        const float qx = (K.r[0] * dx + K.r[3] * dy) + K.r[6] * dz;       // R^T d: the body frame
        const float qy = (K.r[1] * dx + K.r[4] * dy) + K.r[7] * dz;
        const float qz = (K.r[2] * dx + K.r[5] * dy) + K.r[8] * dz;
        if (!(fabsf(qx) <= K.hx && fabsf(qy) <= K.hy && fabsf(qz) <= K.hz)) continue;      // NaN: outside; on a face: inside
        const uint32_t ix = body_voxel3(qx, K.hx, K.ex, K.w), iy = body_voxel3(qy, K.hy, K.ey, K.h), iz = body_voxel3(qz, K.hz, K.ez, K.d);
        const float4 g = K.field[(size_t)((iz * K.h + iy) * K.w + ix)];
        if (!(g.x != 0.0f || g.y != 0.0f || g.z != 0.0f)) continue;
        const float len = sqrt_rn((g.x * g.x + g.y * g.y) + g.z * g.z);
        if (!(len > 0.0f)) continue;                                      // a vector whose squares all underflow is free space
        if (!hit) { v = vel[i]; hit = true; }
        const float fx = (K.r[0] * g.x + K.r[1] * g.y) + K.r[2] * g.z;    // R g: back to the world
        const float fy = (K.r[3] * g.x + K.r[4] * g.y) + K.r[5] * g.z;
        const float fz = (K.r[6] * g.x + K.r[7] * g.y) + K.r[8] * g.z;
        const float nx = __fdiv_rn(fx, len), ny = __fdiv_rn(fy, len), nz = __fdiv_rn(fz, len);
        p.x = p.x + fx; p.y = p.y + fy; p.z = p.z + fz;
        const float sx = p.x - K.cx, sy = p.y - K.cy, sz = p.z - K.cz;    // the pushed position
        const float usx = K.ux + (K.wy * sz - K.wz * sy);                 // the body surface's velocity there
        const float usy = K.uy + (K.wz * sx - K.wx * sz);
        const float usz = K.uz + (K.wx * sy - K.wy * sx);
        const float rx = v.x - usx, ry = v.y - usy, rz = v.z - usz;
        const float rn = (rx * nx + ry * ny) + rz * nz;
        const float k = (1.0f - damping) * rn;
        v.x = usx + (rx - k * nx); v.y = usy + (ry - k * ny); v.z = usz + (rz - k * nz);
        if (fabsf(p.x) > bx) { p.x = bx * sign_f32(p.x); v.x *= -1.0f * damping; }
        if (fabsf(p.y) > by) { p.y = by * sign_f32(p.y); v.y *= -1.0f * damping; }
        if (fabsf(p.z) > bz) { p.z = bz * sign_f32(p.z); v.z *= -1.0f * damping; }
    }
    if (hit) {
        pos[i] = p;
        vel[i] = v;
    }
}

void launch3_bodies(hipStream_t st, const Params3& P, const Arrays3& A, const Bodies3& B, hipEvent_t done) {
    const dim3 grid((P.n + B3B - 1u) / B3B), block(B3B);
    hipExtLaunchKernelGGL(k3_bodies, grid, block, 0, st, nullptr, done, 0, B, P.n, P.bx, P.by, P.bz, P.damping, A.pos_out, A.vel);
}

}  // namespace fsd

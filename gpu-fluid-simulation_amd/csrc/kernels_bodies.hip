// kernels_bodies.hip — the opt-in moving bodies of the 2D step (build extension): the operators B_0 .. B_7 of
// include/fluidsim.h "2D moving bodies" on the position and velocity the force pass just stored, one streaming pass behind it.
// A pass of its own and no further flag on k_force (kernels_force.hip): that kernel's instantiations and register budget stay
// what they are, and a handle without bodies must launch what it launched before.
// The bodies come by value (fs_kernels.h Bodies2, about 0.6 KB of kernel arguments): everything per body is wave-uniform and
// stays in SGPRs.  A lane takes two neighbouring particles: their positions come through one 16-byte load and the same
// per-particle code runs on each (measured against one particle per lane: 23.2 against 28.5 us at 16 M with one body,
// profiles/bodies2d_cost.md).  A particle's velocity is read only once a body hits it and both are stored only then, so a
// particle no body touches costs 8 bytes.  The early-out is the statement's own box test — nothing coarser: a bounding circle
// can reject a corner particle by rounding.  AOS: a renderer hand-off is registered and the force pass wrote the 32-byte records
// itself, so a hit also stores position (record + 0) and velocity (record + 16); the records of untouched particles are neither
// read nor written.  No LDS, no atomics, nothing waits on another workgroup; every pixel index is clamped, so no position reads
// outside a field.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "fs_device.h"
#include "fs_kernels.h"

namespace fsd {

#define B2B 256

__device__ __forceinline__ uint32_t body_pixel(float q, float hb, float extent, uint32_t w) {
    const uint32_t i = f32_to_u32_sat(__fdiv_rn(q + hb, extent) * (float)w);
    return i < w - 1u ? i : w - 1u;
}

// Every body's operator on particle i, whose position p the caller has loaded; i < n.
template <bool AOS>
__device__ __forceinline__ void bodies_apply(const Bodies2& B, uint32_t i, float2 p, float bx, float by, float damping,
                                             float2* __restrict__ pos, float2* __restrict__ vel, float2* __restrict__ aos) {
    float2 v = make_float2(0.0f, 0.0f);
    bool hit = false;
    for (uint32_t b = 0; b < B.count; ++b) {
        const Body2& K = B.body[b];
        const float dx = p.x - K.cx, dy = p.y - K.cy;
        const float qx = K.r00 * dx + K.r10 * dy;                         // R^T d: the body frame
        const float qy = K.r01 * dx + K.r11 * dy;
        if (!(fabsf(qx) <= K.hx && fabsf(qy) <= K.hy)) continue;          // NaN: outside; on an edge: inside
        const uint32_t ix = body_pixel(qx, K.hx, K.ex, K.w), iy = body_pixel(qy, K.hy, K.ey, K.h);
        const float2 g = K.field[(size_t)(iy * K.w + ix)];
        if (!(g.x != 0.0f || g.y != 0.0f)) continue;
        const float len = sqrt_rn(g.x * g.x + g.y * g.y);
        if (!(len > 0.0f)) continue;                                      // a vector whose squares underflow is free space
        if (!hit) { v = vel[i]; hit = true; }
        const float fx = K.r00 * g.x + K.r01 * g.y;                       // R g: back to the world
        const float fy = K.r10 * g.x + K.r11 * g.y;
        const float nx = __fdiv_rn(fx, len), ny = __fdiv_rn(fy, len);
        p.x = p.x + fx; p.y = p.y + fy;
        const float sx = p.x - K.cx, sy = p.y - K.cy;                     // the pushed position
        const float usx = K.ux - K.wz * sy;                               // the body surface's velocity there
        const float usy = K.uy + K.wz * sx;
        const float rx = v.x - usx, ry = v.y - usy;
        const float rn = rx * nx + ry * ny;
        const float k = (1.0f - damping) * rn;
        v.x = usx + (rx - k * nx); v.y = usy + (ry - k * ny);
        if (fabsf(p.x) > bx) { p.x = bx * sign_f32(p.x); v.x *= -1.0f * damping; }
        if (fabsf(p.y) > by) { p.y = by * sign_f32(p.y); v.y *= -1.0f * damping; }
    }
    if (hit) {
        pos[i] = p;
        vel[i] = v;
        if (AOS) {                                                        // ParticleInstance: four float2 — position, predicted, velocity, {density, grid}
            aos[4u * (size_t)i] = p;
            aos[4u * (size_t)i + 2u] = v;
        }
    }
}

template <bool AOS>
__global__ __launch_bounds__(B2B) void k_bodies(Bodies2 B, uint32_t n, float bx, float by, float damping,
                                                float2* __restrict__ pos, float2* __restrict__ vel, float2* __restrict__ aos) {
    const uint32_t t = blockIdx.x * B2B + threadIdx.x;
    const uint32_t i = 2u * t;                                            // (n <= 2^28: no overflow)
    if (i >= n) return;
    if (i + 1u < n) {
        const float4 pp = reinterpret_cast<const float4*>(pos)[t];        // pos is the base of an allocation: 16-byte aligned
        bodies_apply<AOS>(B, i, make_float2(pp.x, pp.y), bx, by, damping, pos, vel, aos);
        bodies_apply<AOS>(B, i + 1u, make_float2(pp.z, pp.w), bx, by, damping, pos, vel, aos);
    } else {                                                              // an odd count's last particle
        bodies_apply<AOS>(B, i, pos[i], bx, by, damping, pos, vel, aos);
    }
}

void launch_bodies(hipStream_t st, const StepParams& P, const StepArrays& A, const Bodies2& B, void* aos, hipEvent_t done) {
    const dim3 grid(nblk((P.n + 1u) / 2u)), block(B2B);
    float2* const rec = (float2*)aos;
    hipExtLaunchKernelGGL(aos ? k_bodies<true> : k_bodies<false>, grid, block, 0, st, nullptr, done, 0, B, P.n, P.bs_x, P.bs_y,
                          P.damping, A.pos_out, A.vel_out, rec);
}

}  // namespace fsd

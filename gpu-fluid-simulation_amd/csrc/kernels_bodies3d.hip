// kernels_bodies3d.hip — the opt-in moving bodies of the 3D step (build extension): the operators B_0 .. B_7 of
// include/fluidsim.h "3D moving bodies" on the position and velocity the force pass just stored, one streaming pass behind it.
// A pass of its own and no further flag on force3_body (kernels_force3d.hip): that kernel's instantiations sit at a pinned 128
// VGPRs with a spill-free tail, and a handle without bodies must launch what it launched before.
// One lane per particle.  The bodies come by value (fs_3d.h Bodies3, about 1 KB of kernel arguments): everything per body is
// wave-uniform and stays in SGPRs.  A lane reads its 16-byte position; it reads its velocity only once a body hits it and stores
// both only then, so a particle no body touches costs 16 bytes.  The early-out is the statement's own box test — nothing
// coarser: a bounding sphere can reject a corner particle by rounding.  No LDS, no atomics, nothing waits on another workgroup;
// every voxel index is clamped, so no position reads outside a field.
// The second form, k3_bodies_loads, is launched instead only while the handle's loads are on (include/fluidsim.h "3D body loads",
// DESIGN.md §26): the same operators, and per body the fixed-point sums of what its hits took from the fluid — eight 64-bit words.
// It carries its own copy of the operator, as the 2D loads form does (§25: sharing the function moved instructions of the plain
// kernels, which must stay what they are; profiles/body_loads3d_resource_usage.txt).  Every lane reaches the barrier, so there is
// no early return; a lane past n loads nothing, stores nothing and contributes nothing.  Per body and wave one wave-uniform
// ballot of "this lane hit"; only behind it the six Q values, six DPP wave sums (fs_body_loads.h), two ballot pop-counts and the
// wave's eight words into its own LDS row.  One barrier, then threads 0 .. 8*count-1 add the four rows and, where the sum is not
// zero, issue ONE non-returning 64-bit atomic add into row blockIdx % 64 of the 64 x 64-word shard table.  k3_body_loads_fold, one
// wave per word, adds the rows into the handle's words by slot and zeroes them; it carries the step's completion event.  Integer
// sums only: any order gives the same words.  Nothing waits on another workgroup.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "fs_3d.h"
#include "fs_body_loads.h"
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

// ---- the loads form --------------------------------------------------------------------------------------------------------
// What a hit leaves in registers for the loads: the velocity on entry to the body's operator, the velocity the operator computed
// before its wall re-clamp, and the pushed position relative to the centre.
struct Body3Hit {
    float v0x, v0y, v0z, v1x, v1y, v1z, sx, sy, sz;
};

// The operator of ONE body on one particle — k3_bodies' loop body, line for line — with position p and velocity v in registers
// across the bodies (v is read from vel[i] when the first body hits: `loaded`).  True: K hit, and h holds its quantities.
__device__ __forceinline__ bool body3_apply(const Body3& K, uint32_t i, float4& p, float4& v, bool& loaded, float bx, float by,
                                            float bz, float damping, const float4* __restrict__ vel, Body3Hit& h) {
    const float dx = p.x - K.cx, dy = p.y - K.cy, dz = p.z - K.cz;
    const float qx = (K.r[0] * dx + K.r[3] * dy) + K.r[6] * dz;
    const float qy = (K.r[1] * dx + K.r[4] * dy) + K.r[7] * dz;
    const float qz = (K.r[2] * dx + K.r[5] * dy) + K.r[8] * dz;
    if (!(fabsf(qx) <= K.hx && fabsf(qy) <= K.hy && fabsf(qz) <= K.hz)) return false;
    const uint32_t ix = body_voxel3(qx, K.hx, K.ex, K.w), iy = body_voxel3(qy, K.hy, K.ey, K.h), iz = body_voxel3(qz, K.hz, K.ez, K.d);
    const float4 g = K.field[(size_t)((iz * K.h + iy) * K.w + ix)];
    if (!(g.x != 0.0f || g.y != 0.0f || g.z != 0.0f)) return false;
    const float len = sqrt_rn((g.x * g.x + g.y * g.y) + g.z * g.z);
    if (!(len > 0.0f)) return false;
    if (!loaded) { v = vel[i]; loaded = true; }
    const float fx = (K.r[0] * g.x + K.r[1] * g.y) + K.r[2] * g.z;
    const float fy = (K.r[3] * g.x + K.r[4] * g.y) + K.r[5] * g.z;
    const float fz = (K.r[6] * g.x + K.r[7] * g.y) + K.r[8] * g.z;
    const float nx = __fdiv_rn(fx, len), ny = __fdiv_rn(fy, len), nz = __fdiv_rn(fz, len);
    p.x = p.x + fx; p.y = p.y + fy; p.z = p.z + fz;
    const float sx = p.x - K.cx, sy = p.y - K.cy, sz = p.z - K.cz;
    const float usx = K.ux + (K.wy * sz - K.wz * sy);
    const float usy = K.uy + (K.wz * sx - K.wx * sz);
    const float usz = K.uz + (K.wx * sy - K.wy * sx);
    const float rx = v.x - usx, ry = v.y - usy, rz = v.z - usz;
    const float rn = (rx * nx + ry * ny) + rz * nz;
    const float k = (1.0f - damping) * rn;
    h.v0x = v.x; h.v0y = v.y; h.v0z = v.z; h.sx = sx; h.sy = sy; h.sz = sz;
    v.x = usx + (rx - k * nx); v.y = usy + (ry - k * ny); v.z = usz + (rz - k * nz);
    h.v1x = v.x; h.v1y = v.y; h.v1z = v.z;                                // before the wall: what it does is not the body's load
    if (fabsf(p.x) > bx) { p.x = bx * sign_f32(p.x); v.x *= -1.0f * damping; }
    if (fabsf(p.y) > by) { p.y = by * sign_f32(p.y); v.y *= -1.0f * damping; }
    if (fabsf(p.z) > bz) { p.z = bz * sign_f32(p.z); v.z *= -1.0f * damping; }
    return true;
}

__device__ __forceinline__ bool load3_in_range(float x) { return fabsf(x) < 16384.0f; }                // NaN: false

// One hit's j and t into q[0 .. 6); false: one of the six is out of range or NaN, the hit is dropped and q stays zero.
__device__ __forceinline__ bool load3_q(const Body3Hit& h, long long (&q)[6]) {
    const float jx = h.v0x - h.v1x, jy = h.v0y - h.v1y, jz = h.v0z - h.v1z;
    const float tx = h.sy * jz - h.sz * jy;                               // (no contraction: two products, one subtraction)
    const float ty = h.sz * jx - h.sx * jz;
    const float tz = h.sx * jy - h.sy * jx;
    if (!(load3_in_range(jx) && load3_in_range(jy) && load3_in_range(jz) && load3_in_range(tx) && load3_in_range(ty) &&
          load3_in_range(tz)))
        return false;
    q[0] = load_q(jx); q[1] = load_q(jy); q[2] = load_q(jz); q[3] = load_q(tx); q[4] = load_q(ty); q[5] = load_q(tz);
    return true;
}

__global__ __launch_bounds__(B3B) void k3_bodies_loads(Bodies3 B, uint32_t n, float bx, float by, float bz, float damping,
                                                       float4* __restrict__ pos, float4* __restrict__ vel, u64* __restrict__ shards) {
    static_assert(BODY3_LOAD_ROW == 64u, "a wave zeroes and owns one LDS row; one shard row is one wave wide");
    __shared__ u64 part[B3B / 64][BODY3_LOAD_ROW];                        // per wave: [kernel index][word]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    part[wave][lane] = 0ull;                                              // (the wave's own row: its later writes follow in order)
    const uint32_t i = blockIdx.x * B3B + threadIdx.x;
    const bool in = i < n;                                                // no early return: every lane reaches the barrier
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = p;
    if (in) p = pos[i];
    bool loaded = false;
    for (uint32_t b = 0; b < B.count; ++b) {
        Body3Hit h;
        const bool hit = in && body3_apply(B.body[b], i, p, v, loaded, bx, by, bz, damping, vel, h);
        const wave_mask m = wm(hit);
        if (m == 0ull) continue;                                          // wave-uniform, one ballot: most waves hit nothing
        long long q[6] = {0, 0, 0, 0, 0, 0};
        const bool drop = hit && !load3_q(h, q);
        const u64 hits = (u64)__popcll(m), dropped = (u64)__popcll(wm(drop));
        for (int c = 0; c < 6; ++c) q[c] = wave_sum(q[c]);
        if (lane < BODY3_LOAD_WORDS)
            part[wave][b * BODY3_LOAD_WORDS + lane] = lane == 0u ? (u64)q[0] : lane == 1u ? (u64)q[1] : lane == 2u ? (u64)q[2]
                                                    : lane == 3u ? (u64)q[3] : lane == 4u ? (u64)q[4] : lane == 5u ? (u64)q[5]
                                                    : lane == 6u ? hits : dropped;
    }
    if (loaded) {
        pos[i] = p;
        vel[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < B.count * BODY3_LOAD_WORDS) {
        u64 s = 0ull;
        for (uint32_t w = 0; w < B3B / 64; ++w) s += part[w][threadIdx.x];
        if (s != 0ull)                                                    // result unused: a non-returning atomic
            (void)__hip_atomic_fetch_add(&shards[(blockIdx.x % BODY_LOAD_SHARDS) * BODY3_LOAD_ROW + threadIdx.x], s, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Block k (one wave) owns word k = 8 * kernel index + word: lane r takes row r of the shard table and zeroes it for the next step.
__global__ __launch_bounds__(BODY_LOAD_SHARDS) void k3_body_loads_fold(BodyLoadMap M, u64* __restrict__ shards, u64* __restrict__ words) {
    body_loads_fold<BODY3_LOAD_WORDS, BODY3_LOAD_ROW>(M, shards, words);
}

void launch3_bodies_loads(hipStream_t st, const Params3& P, const Arrays3& A, const Bodies3& B, const BodyLoadMap& M, u64* shards,
                          u64* words, hipEvent_t done) {
    const dim3 grid((P.n + B3B - 1u) / B3B), block(B3B);
    hipLaunchKernelGGL(k3_bodies_loads, grid, block, 0, st, B, P.n, P.bx, P.by, P.bz, P.damping, A.pos_out, A.vel, shards);
    hipExtLaunchKernelGGL(k3_body_loads_fold, dim3(M.count * BODY3_LOAD_WORDS), dim3(BODY_LOAD_SHARDS), 0, st, nullptr, done, 0, M,
                          shards, words);
}

void launch3_bodies(hipStream_t st, const Params3& P, const Arrays3& A, const Bodies3& B, hipEvent_t done) {
    const dim3 grid((P.n + B3B - 1u) / B3B), block(B3B);
    hipExtLaunchKernelGGL(k3_bodies, grid, block, 0, st, nullptr, done, 0, B, P.n, P.bx, P.by, P.bz, P.damping, A.pos_out, A.vel);
}

}  // namespace fsd

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
// The second form, k_bodies_loads<AOS>, is launched instead only while the handle's loads are on (include/fluidsim.h "2D body
// loads"): the same operators, and per body the fixed-point sums of what its hits took from the fluid.  It walks
// body by body over the lane's two particles, so that a body's hits of a whole wave are in registers together; it carries its own
// copy of the operator, because sharing one function with the plain form moved four instructions of k_bodies<false> and
// k_bodies<true>, which must stay what they are (profiles/body_loads2d_resource_usage.txt).  Reduction: 64-bit integers, so any
// order gives the same words — under a wave-uniform "any lane hit" ballot a DPP row reduction with four scalar reads, the wave's
// five words into its own LDS row, one barrier, then threads 0 .. 5*count-1 add the four rows and, where the sum is not zero, issue ONE non-returning 64-bit
// atomic add into row blockIdx % BODY_LOAD_SHARDS of the shard table.  k_body_loads_fold, one wave per word, then adds the rows
// into the handle's words by slot and zeroes them; it carries the step's completion event.  Nothing waits on another workgroup.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "fs_body_loads.h"
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

// ---- the loads form --------------------------------------------------------------------------------------------------------
// What a hit leaves in registers for the loads: the velocity on entry to the body's operator, the velocity the operator computed
// before its wall re-clamp, and the pushed position relative to the centre.
struct BodyHit {
    float v0x, v0y, v1x, v1y, sx, sy;
};

// The operator of ONE body on one particle — bodies_apply's loop body, line for line — with position p and velocity v in
// registers across the bodies (v is read from vel[i] when the first body hits: `loaded`).  True: K hit, and h holds its quantities.
__device__ __forceinline__ bool body_apply(const Body2& K, uint32_t i, float2& p, float2& v, bool& loaded, float bx, float by,
                                           float damping, const float2* __restrict__ vel, BodyHit& h) {
    const float dx = p.x - K.cx, dy = p.y - K.cy;
    const float qx = K.r00 * dx + K.r10 * dy;
    const float qy = K.r01 * dx + K.r11 * dy;
    if (!(fabsf(qx) <= K.hx && fabsf(qy) <= K.hy)) return false;
    const uint32_t ix = body_pixel(qx, K.hx, K.ex, K.w), iy = body_pixel(qy, K.hy, K.ey, K.h);
    const float2 g = K.field[(size_t)(iy * K.w + ix)];
    if (!(g.x != 0.0f || g.y != 0.0f)) return false;
    const float len = sqrt_rn(g.x * g.x + g.y * g.y);
    if (!(len > 0.0f)) return false;
    if (!loaded) { v = vel[i]; loaded = true; }
    const float fx = K.r00 * g.x + K.r01 * g.y;
    const float fy = K.r10 * g.x + K.r11 * g.y;
    const float nx = __fdiv_rn(fx, len), ny = __fdiv_rn(fy, len);
    p.x = p.x + fx; p.y = p.y + fy;
    const float sx = p.x - K.cx, sy = p.y - K.cy;
    const float usx = K.ux - K.wz * sy;
    const float usy = K.uy + K.wz * sx;
    const float rx = v.x - usx, ry = v.y - usy;
    const float rn = rx * nx + ry * ny;
    const float k = (1.0f - damping) * rn;
    h.v0x = v.x; h.v0y = v.y; h.sx = sx; h.sy = sy;
    v.x = usx + (rx - k * nx); v.y = usy + (ry - k * ny);
    h.v1x = v.x; h.v1y = v.y;                                             // before the wall: what it does is not the body's load
    if (fabsf(p.x) > bx) { p.x = bx * sign_f32(p.x); v.x *= -1.0f * damping; }
    if (fabsf(p.y) > by) { p.y = by * sign_f32(p.y); v.y *= -1.0f * damping; }
    return true;
}

// One hit's j and tz into the lane's three sums; false: out of range or NaN, the hit is dropped and adds nothing.
__device__ __forceinline__ bool load_add(const BodyHit& h, long long& ax, long long& ay, long long& at) {
    const float jx = h.v0x - h.v1x, jy = h.v0y - h.v1y;
    const float t0 = h.sx * jy;
    const float t1 = h.sy * jx;
    const float tz = t0 - t1;
    if (!(fabsf(jx) < 16384.0f && fabsf(jy) < 16384.0f && fabsf(tz) < 16384.0f)) return false;      // NaN: dropped
    ax += load_q(jx); ay += load_q(jy); at += load_q(tz);
    return true;
}

template <bool AOS>
__device__ __forceinline__ void bodies_store(uint32_t i, float2 p, float2 v, float2* __restrict__ pos, float2* __restrict__ vel,
                                             float2* __restrict__ aos) {
    pos[i] = p;
    vel[i] = v;
    if (AOS) {
        aos[4u * (size_t)i] = p;
        aos[4u * (size_t)i + 2u] = v;
    }
}

template <bool AOS>
__global__ __launch_bounds__(B2B) void k_bodies_loads(Bodies2 B, uint32_t n, float bx, float by, float damping,
                                                      float2* __restrict__ pos, float2* __restrict__ vel, float2* __restrict__ aos,
                                                      u64* __restrict__ shards) {
    __shared__ u64 part[B2B / 64][BODY_LOAD_ROW];                         // per wave: [kernel index][word]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane < BODY_LOAD_ROW) part[wave][lane] = 0ull;                    // (the wave's own row: its later writes follow in order)
    const uint32_t t = blockIdx.x * B2B + threadIdx.x;
    const uint32_t i = 2u * t;                                            // (n <= 2^28: no overflow)
    const bool in0 = i < n, in1 = i + 1u < n;                             // no early return: every lane reaches the barrier
    float2 p0 = make_float2(0.0f, 0.0f), p1 = p0, v0 = p0, v1 = p0;
    if (in1) {
        const float4 pp = reinterpret_cast<const float4*>(pos)[t];
        p0 = make_float2(pp.x, pp.y); p1 = make_float2(pp.z, pp.w);
    } else if (in0) {                                                     // an odd count's last particle
        p0 = pos[i];
    }
    bool ld0 = false, ld1 = false;
    for (uint32_t b = 0; b < B.count; ++b) {
        const Body2& K = B.body[b];
        BodyHit h0, h1;
        const bool hit0 = in0 && body_apply(K, i, p0, v0, ld0, bx, by, damping, vel, h0);
        const bool hit1 = in1 && body_apply(K, i + 1u, p1, v1, ld1, bx, by, damping, vel, h1);
        if (wm(hit0 | hit1) == 0ull) continue;                            // wave-uniform, one ballot: most waves hit nothing
        const wave_mask m0 = wm(hit0), m1 = wm(hit1);
        long long ax = 0, ay = 0, at = 0;
        const bool dr0 = hit0 && !load_add(h0, ax, ay, at);
        const bool dr1 = hit1 && !load_add(h1, ax, ay, at);
        const u64 hits = (u64)(__popcll(m0) + __popcll(m1)), dropped = (u64)(__popcll(wm(dr0)) + __popcll(wm(dr1)));
        ax = wave_sum(ax); ay = wave_sum(ay); at = wave_sum(at);
        if (lane < BODY_LOAD_WORDS)
            part[wave][b * BODY_LOAD_WORDS + lane] = lane == 0u ? (u64)ax : lane == 1u ? (u64)ay : lane == 2u ? (u64)at : lane == 3u ? hits : dropped;
    }
    if (ld0) bodies_store<AOS>(i, p0, v0, pos, vel, aos);
    if (ld1) bodies_store<AOS>(i + 1u, p1, v1, pos, vel, aos);
    __syncthreads();
    if (threadIdx.x < B.count * BODY_LOAD_WORDS) {
        u64 s = 0ull;
        for (uint32_t w = 0; w < B2B / 64; ++w) s += part[w][threadIdx.x];
        if (s != 0ull)                                                    // result unused: a non-returning atomic
            (void)__hip_atomic_fetch_add(&shards[(blockIdx.x % BODY_LOAD_SHARDS) * BODY_LOAD_ROW + threadIdx.x], s, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Block k (one wave) owns word k = 5 * kernel index + word: lane r takes row r of the shard table and zeroes it for the next step
// (fs_body_loads.h, shared with the 3D pass).
__global__ __launch_bounds__(BODY_LOAD_SHARDS) void k_body_loads_fold(BodyLoadMap M, u64* __restrict__ shards, u64* __restrict__ words) {
    body_loads_fold<BODY_LOAD_WORDS, BODY_LOAD_ROW>(M, shards, words);
}

void launch_bodies_loads(hipStream_t st, const StepParams& P, const StepArrays& A, const Bodies2& B, void* aos, const BodyLoadMap& M,
                         u64* shards, u64* words, hipEvent_t done) {
    const dim3 grid(nblk((P.n + 1u) / 2u)), block(B2B);
    float2* const rec = (float2*)aos;
    hipLaunchKernelGGL(aos ? k_bodies_loads<true> : k_bodies_loads<false>, grid, block, 0, st, B, P.n, P.bs_x, P.bs_y, P.damping,
                       A.pos_out, A.vel_out, rec, shards);
    hipExtLaunchKernelGGL(k_body_loads_fold, dim3(M.count * BODY_LOAD_WORDS), dim3(BODY_LOAD_SHARDS), 0, st, nullptr, done, 0, M,
                          shards, words);
}

void launch_bodies(hipStream_t st, const StepParams& P, const StepArrays& A, const Bodies2& B, void* aos, hipEvent_t done) {
    const dim3 grid(nblk((P.n + 1u) / 2u)), block(B2B);
    float2* const rec = (float2*)aos;
    hipExtLaunchKernelGGL(aos ? k_bodies<true> : k_bodies<false>, grid, block, 0, st, nullptr, done, 0, B, P.n, P.bs_x, P.bs_y,
                          P.damping, A.pos_out, A.vel_out, rec);
}

}  // namespace fsd

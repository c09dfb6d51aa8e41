// kernels_force3d.hip — the force + integrate pass of the 3D step and its launcher (fs_3d.h): the pair terms (exact, shared
// reciprocals, tolerance mode), the three-deep pipelined walk of the pass masks, the three sweeps of a staged plane
// (fs_sweep3.h has the driver, the stage and the masks), the opt-in collider tail and the surface-tension
// force in the sum.  pred.w carries the density, vel_s.w +-RN(1/rho) from the density pass.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "fs_sweep3.h"

namespace fsd {
struct Acc3 { float px, py, pz, vx, vy, vz; uint32_t seed; };
struct Terms3 { float px, py, pz, vx, vy, vz; };

__device__ __forceinline__ Terms3 terms3(const Params3& P, float4 me, float4 mv, float pressure, float4 q, float4 nv,
                                         uint32_t& seed) {
    const float h = P.h;
    const float ox = q.x - me.x, oy = q.y - me.y, oz = q.z - me.z;
    const float r2 = ox * ox + oy * oy + oz * oz;
    const float dst = sqrt_rn(r2);
    float dx, dy, dz;
    if (dst == 0.0f) {
        const float rx = rand_f32(&seed), ry = rand_f32(&seed), rz = rand_f32(&seed);
        const float len = sqrt_rn(rx * rx + ry * ry + rz * rz);
        dx = __fdiv_rn(rx, len); dy = __fdiv_rn(ry, len); dz = __fdiv_rn(rz, len);
    } else {
        dx = __fdiv_rn(ox, dst); dy = __fdiv_rn(oy, dst); dz = __fdiv_rn(oz, dst);
    }
    const float nrho = q.w;
    const float npress = P.pressure_k * (nrho - P.rest_density);
    const float kern = (dst <= h) ? (-(h - dst)) * P.spiky : 0.0f;
    const float shared = (pressure + npress) * 0.5f;
    float kv = 0.0f;
    if (dst <= h) {
        if (dst == 0.0f) {
            kv = P.visc_k;
        } else {
            float a, b;
            if (dst < 9.5367431640625e-07f) {            // 2^-20: outside the proven range, true division
                a = __fdiv_rn(-(dst * dst * dst), P.div_2h3.c);
                b = __fdiv_rn(dst * dst, P.div_h2.c);
            } else {
                a = div_const(P.div_2h3, -(dst * dst * dst));
                b = div_const(P.div_h2, dst * dst);
            }
            kv = P.visc_k * (a + b + (__fdiv_rn(h, 2.0f * dst)) - 1.0f);
        }
    }
    Terms3 T;
    T.px = __fdiv_rn(dx * kern * shared, nrho);
    T.py = __fdiv_rn(dy * kern * shared, nrho);
    T.pz = __fdiv_rn(dz * kern * shared, nrho);
    T.vx = __fdiv_rn(nv.x - mv.x, nrho) * kv;
    T.vy = __fdiv_rn(nv.y - mv.y, nrho) * kv;
    T.vz = __fdiv_rn(nv.z - mv.z, nrho) * kv;
    return T;
}

// The same terms with one reciprocal per denominator (dst, neighbour density) and div_by_rcp() for
// the ten quotients — bit-identical to terms3() for every lane whose bit stays set in `good`
// (fs_device.h: the proven ranges).  No PRNG / tiny-distance path: those lanes clear their bit and
// the caller re-evaluates the pair with terms3() for the whole wave.
__device__ __forceinline__ wave_mask num_lo_ok3(float a) { return wm(fabsf(a) >= 0x1p-76f) | wm(a == 0.0f); }   // NaN: 0
__device__ __forceinline__ Terms3 terms3_shared(const Params3& P, float4 me, float4 mv, float pressure, float4 q,
                                                float4 nv, wave_mask& good) {
    const float h = P.h;
    const float ox = q.x - me.x, oy = q.y - me.y, oz = q.z - me.z;
    const float r2 = ox * ox + oy * oy + oz * oz;
    const float nrho = q.w;                                            // >= 0.1 (k3_density)
    const float yrho = nv.w;                                           // +-RN(1/nrho): the sign is the neighbour's classification
    good = wm(r2 >= FS_SQRT_LO) & wm(yrho > 0.0f);
    const float dst = sqrt_rn_fast(r2);                                // r2 <= h*h: the scan admitted it
    const float ydst = rcp_rn_fast(dst);
    const float dx = div_by_rcp(ox, dst, ydst), dy = div_by_rcp(oy, dst, ydst), dz = div_by_rcp(oz, dst, ydst);
    const float npress = P.pressure_k * (nrho - P.rest_density);
    const bool inside = dst <= h;
    const float kern = inside ? (-(h - dst)) * P.spiky : 0.0f;
    const float shared = (pressure + npress) * 0.5f;
    const float apx = dx * kern * shared, apy = dy * kern * shared, apz = dz * kern * shared;
    const float dvx = nv.x - mv.x, dvy = nv.y - mv.y, dvz = nv.z - mv.z;
    // both particles safe => every numerator is 0 or in [2^-76, 2^60] except the lower bound of the three pressure
    // numerators (a product of three factors can be tiny without any factor being unusual)
    good &= num_lo_ok3(apx) & num_lo_ok3(apy) & num_lo_ok3(apz);
    const float a = div_const_fast(-(dst * dst * dst), P.div_2h3.c, P.div_2h3.y);   // share_div implies both proofs
    const float b = div_const_fast(dst * dst, P.div_h2.c, P.div_h2.y);
    const float hq = div_by_rcp(h, 2.0f * dst, 0.5f * ydst);
    const float kv = inside ? P.visc_k * (a + b + hq - 1.0f) : 0.0f;
    Terms3 T;
    T.px = div_by_rcp(apx, nrho, yrho); T.py = div_by_rcp(apy, nrho, yrho); T.pz = div_by_rcp(apz, nrho, yrho);
    T.vx = div_by_rcp(dvx, nrho, yrho) * kv; T.vy = div_by_rcp(dvy, nrho, yrho) * kv; T.vz = div_by_rcp(dvz, nrho, yrho) * kv;
    return T;
}

__device__ __forceinline__ void acc3_add(Acc3& A, const Terms3& T) {
    A.px += T.px; A.py += T.py; A.pz += T.pz; A.vx += T.vx; A.vy += T.vy; A.vz += T.vz;
}

__device__ __forceinline__ Terms3 pair3(const Params3& P, float4 me, float4 mv, float pressure, float4 q, float4 nv,
                                        Acc3& A) {
    wave_mask good = 0;
    Terms3 T;
    if (P.share_div) { T = terms3_shared(P, me, mv, pressure, q, nv, good); good &= wm(mv.w > 0.0f); }   // + the lane's own classification
    if (good != wm(true)) T = terms3(P, me, mv, pressure, q, nv, A.seed);      // rare, wave-uniform
    return T;
}

// ---- tolerance mode (fs3_create_ex math_mode = FS_MATH_TOLERANCE): the pressure and viscosity terms of one in-radius
// neighbour merged algebraically, as fs_force_pair.h force_accum_tol does in 2D: one v_rsq_f32, fused multiply-adds,
// 1/rho_j from the density pass (vel_s.w), ~32 issue slots per pair instead of ~95.  Coincident particles keep the
// oracle's xorshift direction.
struct Tol3 { float cP, c3, c2, hh, kp0; };
__device__ __forceinline__ Tol3 tol3_consts(const Params3& P) {
    Tol3 C;
    const float h = P.h;
    C.cP = -0.5f * P.spiky;
    C.c3 = -1.0f / (2.0f * h * h * h);
    C.c2 = 1.0f / (h * h);
    C.hh = 0.5f * h;
    C.kp0 = -P.pressure_k * P.rest_density;           // pressure_j = fma(k, rho_j, kp0)
    return C;
}
__device__ __forceinline__ void accum3_tol(const Params3& P, const Tol3& C, float4 me, float4 mv, float pressure, float4 q,
                                           float4 nv, Acc3& A) {
    const float ox = q.x - me.x, oy = q.y - me.y, oz = q.z - me.z;
    const float r2 = __builtin_fmaf(ox, ox, __builtin_fmaf(oy, oy, oz * oz));
    float dx = ox, dy = oy, dz = oz, inv, dst;
    if (r2 == 0.0f) {                                                   // rare: the PRNG direction
        const float rx = rand_f32(&A.seed), ry = rand_f32(&A.seed), rz = rand_f32(&A.seed);
        const float il = __builtin_amdgcn_rsqf(__builtin_fmaf(rx, rx, __builtin_fmaf(ry, ry, rz * rz)));
        dx = rx * il; dy = ry * il; dz = rz * il;
        dst = 0.0f; inv = 1.0f;
    } else {
        inv = __builtin_amdgcn_rsqf(r2);
        dst = r2 * inv;
    }
    const float yrho = fabsf(nv.w);                                     // 1 / rho_j
    const float pj = __builtin_fmaf(P.pressure_k, q.w, C.kp0);
    const float w = fmaxf(P.h - dst, 0.0f);
    const float coefP = (w * C.cP) * (pressure + pj) * yrho * inv;
    float u = __builtin_fmaf(C.c3, dst, C.c2);
    u = __builtin_fmaf(u, r2, -1.0f);
    u = r2 == 0.0f ? 1.0f : __builtin_fmaf(C.hh, inv, u);
    const float kvv = u * (P.visc_k * yrho);
    A.px = __builtin_fmaf(dx, coefP, A.px); A.py = __builtin_fmaf(dy, coefP, A.py); A.pz = __builtin_fmaf(dz, coefP, A.pz);
    A.vx = __builtin_fmaf(nv.x - mv.x, kvv, A.vx); A.vy = __builtin_fmaf(nv.y - mv.y, kvv, A.vy); A.vz = __builtin_fmaf(nv.z - mv.z, kvv, A.vz);
}
template <int MODE>
__device__ __forceinline__ void pair3_accum(const Params3& P, const Tol3& C, float4 me, float4 mv, float pressure, float4 q,
                                            float4 nv, Acc3& A) {
    if (MODE == 2) accum3_tol(P, C, me, mv, pressure, q, nv, A);
    else acc3_add(A, pair3(P, me, mv, pressure, q, nv, A));
}

// The walk shared by the 64-bit and the 128-bit mask sweeps: three mask words with the LDS index of their first candidate,
// consumed in order.
template <int MODE>
__device__ __forceinline__ void walk3(const Params3& P, const Tol3& C, const u64m* m, const uint32_t* la, float4 me, float4 mv,
                                      float pressure, const float4* s_flat, Acc3& A) {
    // The three masks are walked as a shift register: `cur` is the mask being consumed with its LDS base, (n1, n2) wait
    // behind it.  Empty masks are squeezed out first, so "cur == 0 -> pull n1" is all a refill ever needs and the
    // per-neighbour bit extraction touches ONE 64-bit mask and ONE base.  Row order 0, 1, 2 is kept.
    u64m cur = m[0], n1 = m[1], n2 = m[2];
    uint32_t lac = la[0] << 4, la_1 = la[1] << 4, la_2 = la[2] << 4;   // in bytes
    if (n1 == 0ull) { n1 = n2; la_1 = la_2; n2 = 0ull; }
    if (cur == 0ull) { cur = n1; lac = la_1; n1 = n2; la_1 = la_2; n2 = 0ull; }
    // Software-pipelined (as in the 2D kernel): the LDS read and the velocity gather of later neighbours are issued
    // before the terms of neighbour k are evaluated — two neighbours ahead (k+1 and k+2: three slots refilled in turn, the
    // loop unrolled by three so no value is moved).  At 4 waves per SIMD the kernel has the registers for it (the one-deep
    // form: profiles/r03_rejected.md).
#define FS3_FETCH(have, qn, vn)                                                                                      \
    do {                                                                                                             \
        have = cur != 0ull;                                                                                          \
        if (have) {                                                                                                  \
            const uint32_t t = (uint32_t)__builtin_clzll(cur);                                                       \
            cur ^= 0x8000000000000000ull >> t;                                                                       \
            qn = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_flat) + (lac + (t << 4)));         \
            vn = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_flat) + (lac + (t << 4)) + TILE3_VEL_OFF); \
            if (cur == 0ull) { cur = n1; lac = la_1; n1 = n2; la_1 = la_2; n2 = 0ull; }                              \
        }                                                                                                            \
    } while (0)
    float4 qA = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vA = qA, qB = qA, vB = qA, qC = qA, vC = qA;
    bool hA = false, hB = false, hC = false;
    FS3_FETCH(hA, qA, vA);
    FS3_FETCH(hB, qB, vB);
    FS3_FETCH(hC, qC, vC);
    for (;;) {       // a slot is refilled right after its neighbour's terms: two bodies later it is consumed
        if (!__any(hA)) break;
        { const bool cv = hA; const float4 q0 = qA, v0 = vA; if (cv) pair3_accum<MODE>(P, C, me, mv, pressure, q0, v0, A); }
        FS3_FETCH(hA, qA, vA);
        if (!__any(hB)) break;
        { const bool cv = hB; const float4 q0 = qB, v0 = vB; if (cv) pair3_accum<MODE>(P, C, me, mv, pressure, q0, v0, A); }
        FS3_FETCH(hB, qB, vB);
        if (!__any(hC)) break;
        { const bool cv = hC; const float4 q0 = qC, v0 = vC; if (cv) pair3_accum<MODE>(P, C, me, mv, pressure, q0, v0, A); }
        FS3_FETCH(hC, qC, vC);
    }
#undef FS3_FETCH
}

// Mask sweep of one staged z-plane (see fs_force_sweep.h force_sweep_masks): every lane walks the set bits of its three
// 64-bit pass masks, row 0, 1, 2, ascending — the oracle's visiting order.  The masks come from k3_density (Params3::handoff,
// `masks` != nullptr) or from a scan of the staged plane (fs_sweep3.h masks3_plane).  In the middle plane the lane's own
// particle sits in row 1 and is skipped (k != i).
template <int MODE>
__device__ __forceinline__ void sweep3_masks(const Params3& P, const Tol3& C, const RowRanges& R, const uint32_t* blo, int plane,
                                             uint32_t ii, float4 me, float4 mv, float pressure, const float4* s_flat,
                                             const u64m* __restrict__ masks, Acc3& A) {
    u64m m[3];
    uint32_t la[3];
    masks3_plane(P, masks, plane, ii, R, blo, me, s_flat, m, la);
    if (plane == 1 && ii - R.lo[1] < R.hi[1] - R.lo[1]) m[1] &= ~(0x8000000000000000ull >> (ii - R.lo[1]));   // k != i
    walk3<MODE>(P, C, m, la, me, mv, pressure, s_flat, A);
}

// Rows of up to 128 candidates (plane_class() == 2): two words per row, walked as (r0.hi, r0.lo, r1.hi) then (r1.lo, r2.hi,
// r2.lo) — the same visiting order.
template <int MODE>
__device__ __forceinline__ void sweep3_masks128(const Params3& P, const Tol3& C, const RowRanges& R, const uint32_t* blo, int plane,
                                                uint32_t ii, float4 me, float4 mv, float pressure, const float4* s_flat,
                                                const u64m* __restrict__ masks, Acc3& A) {
    u64m mh[3], ml[3];
    uint32_t la[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        la[r] = row_la(R, blo, r);
        masks3_row128(P, masks, plane, r, ii, s_flat + la[r], R.hi[r] - R.lo[r], me, &mh[r], &ml[r]);
    }
    if (plane == 1 && ii - R.lo[1] < R.hi[1] - R.lo[1]) {                  // k != i
        const uint32_t d = ii - R.lo[1];
        if (d < 64u) mh[1] &= ~(0x8000000000000000ull >> d);
        else ml[1] &= ~(0x8000000000000000ull >> (d - 64u));
    }
    {
        const u64m m[3] = {mh[0], ml[0], mh[1]};
        const uint32_t l[3] = {la[0], la[0] + 64u, la[1]};
        walk3<MODE>(P, C, m, l, me, mv, pressure, s_flat, A);
    }
    {
        const u64m m[3] = {ml[1], mh[2], ml[2]};
        const uint32_t l[3] = {la[1] + 64u, la[2], la[2] + 64u};
        walk3<MODE>(P, C, m, l, me, mv, pressure, s_flat, A);
    }
}

// General sweep of three rows (one z-plane) for waves that hold a row longer than 64 candidates, or whose
// plane does not fit the LDS tile: the same machinery one 32-candidate chunk of one row at a time (see
// fs_force_sweep.h force_sweep_chunks) — wave-uniform scan into a 32-bit mask, pipelined walk.  Rows and
// chunks in order = the oracle's visiting order.  STAGED: candidates from the LDS tile, else from global
// memory (pred is allocated with FS_PRED_SLACK elements of slack for the read-ahead).
#define FS3_CHUNK_BATCH 4    // 32-candidate chunks scanned per walk
template <bool STAGED, int MODE>
__device__ __forceinline__ void sweep3_chunks(const Params3& P, const Tol3& C, const RowRanges& R, const uint32_t* blo, bool self_plane,
                                              uint32_t ii, float4 me, float4 mv, float pressure,
                                              const float4* __restrict__ pred, const float4* __restrict__ vel_s,
                                              const float4* s_flat, Acc3& A) {
    const float lim = P.h2;
    uint32_t lo0 = R.lo[0], lo1 = R.lo[1], lo2 = R.lo[2], hi0 = R.hi[0], hi1 = R.hi[1], hi2 = R.hi[2];
    uint32_t b00 = blo[0], b01 = blo[1], b02 = blo[2];
    asm volatile("" : "+v"(lo0), "+v"(lo1), "+v"(lo2), "+v"(hi0), "+v"(hi1), "+v"(hi2), "+v"(b00), "+v"(b01), "+v"(b02));
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
        const uint32_t lo = r == 0 ? lo0 : r == 1 ? lo1 : lo2;
        const uint32_t hi = r == 0 ? hi0 : r == 1 ? hi1 : hi2;
        const uint32_t b0 = r == 0 ? b00 : r == 1 ? b01 : b02;
        const uint32_t len = hi - lo;
        // FS3_CHUNK_BATCH chunks of 32 candidates are scanned before the walk starts and their masks are walked as one shift
        // register (fs_force_sweep.h force_sweep_chunks: a lane then waits for the wave's slowest lane once per 128
        // candidates instead of once per 32); the chunks of a batch are consecutive in the row, a refill advances the bases
#pragma unroll 1
        for (uint32_t c0 = 0; __any(c0 < len); c0 += 32u * FS3_CHUNK_BATCH) {   // c0 is wave-uniform
            uint32_t mq[FS3_CHUNK_BATCH];
            const uint32_t g0 = c0 < len ? lo + c0 : 0u;                 // global index of the batch's first candidate
            const uint32_t boff0 = (STAGED ? (c0 < len ? (uint32_t)r * TILE3_ROW + (g0 - b0) : 0u) : g0) << 4;
            const char* src = STAGED ? reinterpret_cast<const char*>(s_flat) : reinterpret_cast<const char*>(pred);
#define FS3_CAND(off, k) (*reinterpret_cast<const float4*>(src + ((off) + ((k) << 4))))
#pragma unroll
            for (int q = 0; q < FS3_CHUNK_BATCH; ++q) {
                const uint32_t cq = c0 + 32u * (uint32_t)q;
                const uint32_t clen = cq < len ? (len - cq < 32u ? len - cq : 32u) : 0u;
                const uint32_t boff = clen ? boff0 + 512u * (uint32_t)q : 0u;
                uint32_t mask = 0, t = 0;
                for (; __any(t < clen); t += 4u) {
                    const float4 q0 = FS3_CAND(boff, t), q1 = FS3_CAND(boff, t + 1u), q2 = FS3_CAND(boff, t + 2u), q3 = FS3_CAND(boff, t + 3u);
                    const float4 qq[4] = {q0, q1, q2, q3};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float ox = qq[u].x - me.x, oy = qq[u].y - me.y, oz = qq[u].z - me.z;
                        shift_in_not_greater(mask, ox * ox + oy * oy + oz * oz, lim);
                    }
                }
                mask = t ? mask << (32u - t) : 0u;
                mask &= clen ? 0xFFFFFFFFu << (32u - clen) : 0u;
                const uint32_t g = g0 + 32u * (uint32_t)q;
                if (r == 1 && self_plane && clen && ii - g < clen) mask &= ~(0x80000000u >> (ii - g));   // k != i
                mq[q] = mask;
            }
            static_assert(FS3_CHUNK_BATCH == 4, "the walk's shift register holds four chunk masks");
            uint32_t cur = mq[0], n1 = mq[1], n2 = mq[2], n3 = mq[3];
            uint32_t boff = boff0, goff = g0 << 4;
            float4 qn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vn = qn;
            bool have = false, pending = false;
#define FS3_FETCH_NEXT1()                                                                                            \
    do {                                                                                                             \
        if (cur == 0u) { cur = n1; n1 = n2; n2 = n3; n3 = 0u; boff += 512u; goff += 512u; }   /* next chunk of the batch */ \
        have = cur != 0u;                                                                                            \
        pending = (cur | n1 | n2 | n3) != 0u;            /* an empty chunk in the middle costs this lane one idle trip */ \
        if (have) {                                                                                                  \
            const uint32_t tt = (uint32_t)__builtin_clz(cur);                                                        \
            cur ^= 0x80000000u >> tt;                                                                                \
            qn = FS3_CAND(boff, tt);                                                                                 \
            if (STAGED) vn = *reinterpret_cast<const float4*>(src + (boff + (tt << 4)) + TILE3_VEL_OFF);                 \
            else vn = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(vel_s) + (goff + (tt << 4)));   \
        }                                                                                                            \
    } while (0)
            FS3_FETCH_NEXT1();
            while (__any(pending)) {
                const bool cur_valid = have;
                const float4 q0 = qn, v0 = vn;
                FS3_FETCH_NEXT1();
                if (cur_valid) pair3_accum<MODE>(P, C, me, mv, pressure, q0, v0, A);
            }
#undef FS3_FETCH_NEXT1
#undef FS3_CAND
        }
    }
}

// The opt-in static collider (include/fluidsim.h "3D colliders"): the operator C on the position and velocity the
// step is about to store — the 3D form of move_particle's force-texture push (compute.wgsl:127-140), after the wall clamp and
// followed by the wall clamp again.  One aligned 16-byte load per particle; every index is clamped, so no p reads out of bounds
// (NaN -> voxel 0).
__device__ __forceinline__ uint32_t voxel3(float p, float b, float size, uint32_t w) {
    const uint32_t i = f32_to_u32_sat(__fdiv_rn(p + b, size) * (float)w);
    return i < w - 1u ? i : w - 1u;
}
__device__ __forceinline__ void collide3(const Params3& P, const Collide3& K, float4& p, float4& v) {
    const uint32_t ix = voxel3(p.x, P.bx, K.sx, K.w), iy = voxel3(p.y, P.by, K.sy, K.h), iz = voxel3(p.z, P.bz, K.sz, K.d);
    const float4 f = K.field[(size_t)((iz * K.h + iy) * K.w + ix)];
    if (!(f.x != 0.0f || f.y != 0.0f || f.z != 0.0f)) return;
    const float len = sqrt_rn((f.x * f.x + f.y * f.y) + f.z * f.z);
    if (!(len > 0.0f)) return;                          // a vector whose squares all underflow is free space
    const float nx = __fdiv_rn(f.x, len), ny = __fdiv_rn(f.y, len), nz = __fdiv_rn(f.z, len);
    p.x = p.x + f.x; p.y = p.y + f.y; p.z = p.z + f.z;
    const float vn = (v.x * nx + v.y * ny) + v.z * nz;
    const float k = (1.0f - P.damping) * vn;
    v.x = v.x - k * nx; v.y = v.y - k * ny; v.z = v.z - k * nz;
    if (fabsf(p.x) > P.bx) { p.x = P.bx * sign_f32(p.x); v.x *= -1.0f * P.damping; }
    if (fabsf(p.y) > P.by) { p.y = P.by * sign_f32(p.y); v.y *= -1.0f * P.damping; }
    if (fabsf(p.z) > P.bz) { p.z = P.bz * sign_f32(p.z); v.z *= -1.0f * P.damping; }
}

// Per plane of the sweep (fs_sweep3.h sweep3_planes) the workgroup's three row ranges are staged into LDS and swept with register
// pass-masks (sweep3_masks, sweep3_masks128); waves that hold a range longer than 128, and planes whose rows do not fit the tile,
// take the chunked sweep.  COLLIDE: collide3() before the stores.  ST: the surface-tension force of k3_surface_tension joins the
// force sum (one aligned 16-byte load after the sweep).
template <int MODE, bool COLLIDE, bool ST>
__device__ __forceinline__ void force3_body(const Params3& P, const float4* __restrict__ pos_s, const float4* __restrict__ vel_s,
                                            const float4* __restrict__ pred, const uint32_t* __restrict__ cs,
                                            float4* __restrict__ pos_out, float4* __restrict__ vel_out, const u64m* __restrict__ masks,
                                            const uint32_t* __restrict__ key_s, const u64* __restrict__ srcs, float4* s_buf,
                                            uint32_t* s_red, const Collide3& K, const float4* __restrict__ st) {
    Lane3 L;
    if (!sweep3_lane(P, pred, &L)) return;
    const uint32_t i = L.i, ii = L.ii;
    const float4 me = L.me, mv = vel_s[ii];
    const float mrho = me.w;
    const float pressure = P.pressure_k * (mrho - P.rest_density);
    const Tol3 C = tol3_consts(P);                      // dead code unless MODE == 2
    Acc3 A;
    A.px = A.py = A.pz = A.vx = A.vy = A.vz = 0.0f; A.seed = ii * 12u + P.frame * 69u;
    sweep3_planes(P, cs, key_s, L, s_red, [&](int plane, const RowRanges& R, const uint32_t* blo, const uint32_t* bhi, bool fit, int pclass)
                                       __attribute__((always_inline)) {
        if (fit) stage3_rows<true>(blo, bhi, pred, vel_s, s_buf);
        if (pclass == 1) sweep3_masks<MODE>(P, C, R, blo, plane, ii, me, mv, pressure, s_buf, masks, A);
        else if (pclass == 2) sweep3_masks128<MODE>(P, C, R, blo, plane, ii, me, mv, pressure, s_buf, masks, A);
        else if (fit) sweep3_chunks<true, MODE>(P, C, R, blo, plane == 1, ii, me, mv, pressure, pred, vel_s, s_buf, A);
        else sweep3_chunks<false, MODE>(P, C, R, blo, plane == 1, ii, me, mv, pressure, pred, vel_s, s_buf, A);
    });
    if (!L.live) return;
    float4 v = mv, p = pos_s[(uint32_t)srcs[i]];        // pos_s: the PREVIOUS state, source order (see k3_reorder)
    float ax = A.px + A.vx * P.visc_coeff, ay = A.py + A.vy * P.visc_coeff, az = A.pz + A.vz * P.visc_coeff;
    if (ST) { const float4 f = st[i]; ax = ax + f.x; ay = ay + f.y; az = az + f.z; }
    v.x += __fdiv_rn(ax, mrho) * P.dt; v.y += __fdiv_rn(ay, mrho) * P.dt; v.z += __fdiv_rn(az, mrho) * P.dt;
    v.x += P.gx * P.dt; v.y += P.gy * P.dt; v.z += P.gz * P.dt;
    if (!(v.x == v.x && v.y == v.y && v.z == v.z)) { v.x = 0.0f; v.y = 0.0f; v.z = 0.0f; }
    const float s2 = v.x * v.x + v.y * v.y + v.z * v.z;
    if (s2 > 249000.0f) {                           // below that the root is < 500 whatever the rounding: no clamp (kernels_force.hip)
        const float speed = sqrt_rn(s2);
        if (speed > 500.0f) {
            v.x = __fdiv_rn(v.x, speed) * 500.0f; v.y = __fdiv_rn(v.y, speed) * 500.0f; v.z = __fdiv_rn(v.z, speed) * 500.0f;
        }
    }
    p.x += v.x * P.dt; p.y += v.y * P.dt; p.z += v.z * P.dt;
    if (fabsf(p.x) > P.bx) { p.x = P.bx * sign_f32(p.x); v.x *= -1.0f * P.damping; }
    if (fabsf(p.y) > P.by) { p.y = P.by * sign_f32(p.y); v.y *= -1.0f * P.damping; }
    if (fabsf(p.z) > P.bz) { p.z = P.bz * sign_f32(p.z); v.z *= -1.0f * P.damping; }
    if (COLLIDE) collide3(P, K, p, v);
    p.w = 0.0f; v.w = 0.0f;
    pos_out[i] = p;
    vel_out[i] = v;
}
// 4 waves per SIMD is what the LDS of the staged plane allows: take their registers.
template <int MODE>
__global__ __launch_bounds__(B3F) __attribute__((amdgpu_waves_per_eu(4, 4))) void k3_force(
    Params3 P, const float4* __restrict__ pos_s, const float4* __restrict__ vel_s, const float4* __restrict__ pred,
    const uint32_t* __restrict__ cs, float4* __restrict__ pos_out, float4* __restrict__ vel_out, const u64m* __restrict__ masks,
    const uint32_t* __restrict__ key_s, const u64* __restrict__ srcs) {
    __shared__ float4 s_buf[TILE3_FORCE_LDS];     // the staged plane: positions, then velocities
    __shared__ uint32_t s_red[24];
    force3_body<MODE, false, false>(P, pos_s, vel_s, pred, cs, pos_out, vel_out, masks, key_s, srcs, s_buf, s_red, Collide3{}, nullptr);
}
// The same kernel with the collider operator in its tail: the only instantiations that take a Collide3.  At the tail the
// accumulators are dead, so the register budget of four waves per SIMD holds (DESIGN.md §18 has the figures).
template <int MODE>
__global__ __launch_bounds__(B3F) __attribute__((amdgpu_waves_per_eu(4, 4))) void k3_force_collide(
    Params3 P, const float4* __restrict__ pos_s, const float4* __restrict__ vel_s, const float4* __restrict__ pred,
    const uint32_t* __restrict__ cs, float4* __restrict__ pos_out, float4* __restrict__ vel_out, const u64m* __restrict__ masks,
    const uint32_t* __restrict__ key_s, const u64* __restrict__ srcs, Collide3 K) {
    __shared__ float4 s_buf[TILE3_FORCE_LDS];
    __shared__ uint32_t s_red[24];
    force3_body<MODE, true, false>(P, pos_s, vel_s, pred, cs, pos_out, vel_out, masks, key_s, srcs, s_buf, s_red, K, nullptr);
}

// The same kernel with the surface-tension force in the force sum, with and without the collider tail: the only instantiations
// that take `st`.  Its load comes after the sweep, where the accumulators are about to die (DESIGN.md §19 has the figures).
template <int MODE, bool COLLIDE>
__global__ __launch_bounds__(B3F) __attribute__((amdgpu_waves_per_eu(4, 4))) void k3_force_st(
    Params3 P, const float4* __restrict__ pos_s, const float4* __restrict__ vel_s, const float4* __restrict__ pred,
    const uint32_t* __restrict__ cs, float4* __restrict__ pos_out, float4* __restrict__ vel_out, const u64m* __restrict__ masks,
    const uint32_t* __restrict__ key_s, const u64* __restrict__ srcs, Collide3 K, const float4* __restrict__ st) {
    __shared__ float4 s_buf[TILE3_FORCE_LDS];
    __shared__ uint32_t s_red[24];
    force3_body<MODE, COLLIDE, true>(P, pos_s, vel_s, pred, cs, pos_out, vel_out, masks, key_s, srcs, s_buf, s_red, K, st);
}

// ------------------------------------------------------------------------------------ launchers (fs_3d.h)
// positions ping-pong: read the previous state (A.pos, source order) through the pairs, write the new one into A.pos_out
void launch3_force(hipStream_t st, const Params3& P, const Arrays3& A, bool tol, hipEvent_t done, const Collide3* K, const float4* stf) {
    const dim3 grid(xcd_grid3(blocks3(P.n), P.xcd_chunk_log2)), block(B3F);
    const Collide3 K0 = K ? *K : Collide3{};
    const auto go = [&](auto kernel, auto... extra) {       // the arguments every instantiation takes, then its own
        hipExtLaunchKernelGGL(kernel, grid, block, 0, st, nullptr, done, 0, P, A.pos, A.vel_s, A.pred, A.cs, A.pos_out, A.vel, A.masks,
                              A.key, A.pairs, extra...);
    };
    if (stf && K) tol ? go(k3_force_st<2, true>, K0, stf) : go(k3_force_st<0, true>, K0, stf);
    else if (stf) tol ? go(k3_force_st<2, false>, K0, stf) : go(k3_force_st<0, false>, K0, stf);
    else if (K) tol ? go(k3_force_collide<2>, K0) : go(k3_force_collide<0>, K0);
    else tol ? go(k3_force<2>) : go(k3_force<0>);
}

}  // namespace fsd

// fs_force_pair.h — what ONE in-radius neighbour costs the 2D force pass: the pressure and viscosity terms of a pair in the
// three math modes, and the sums they go into.
//   force_terms<false>   strict (FS_MATH_IEEE): IEEE division and square root, bit for bit the oracle's;
//   force_terms_shared   strict, one true division per denominator (bit-identical inside the proven operand ranges, `good`);
//   force_terms<true>    FS_MATH_WGSL_ULP: native reciprocal and square root;
//   force_accum_tol      FS_MATH_TOLERANCE: the two terms merged algebraically.
// Which of them a pair gets is decided by the sweeps (fs_force_sweep.h) and by k_force_quad (kernels_force_quad.inc).
#pragma once
#include "fs_device.h"

namespace fsd {

struct ForceAcc { float fpx, fpy, fvx, fvy; uint32_t seed; };
struct ForceTerms { float px, py, vx, vy; };

// One in-radius neighbour: pressure (compute.wgsl:207-223) and viscosity (:283-288) terms.
// `seed` only advances on the coincident-particle path (dst == 0, compute.wgsl:211-212).
// FAST (fs_options.math_mode = FS_MATH_WGSL_ULP): `/` becomes n * v_rcp_f32(d) (<= ~1.5 ulp) and sqrt
// the native v_sqrt_f32 (1 ulp) — inside WGSL's own accuracy contract for the reference shaders (f32
// division 2.5 ULP, sqrt via inverseSqrt 2 ULP), but no longer bit-identical to the IEEE oracle.
template <bool FAST> __device__ __forceinline__ float fs_div(float n, float d) {
    return FAST ? n * __builtin_amdgcn_rcpf(d) : __fdiv_rn(n, d);
}
template <bool FAST> __device__ __forceinline__ float fs_sqrt(float x) {
    return FAST ? __builtin_amdgcn_sqrtf(x) : sqrt_rn(x);
}

template <bool FAST>
__device__ __forceinline__ ForceTerms force_terms(const StepParams& P, const float2 me, const float2 mv,
                                                  float pressure, const float2 q, const float2 nv, float nrho,
                                                  uint32_t& seed) {
    const float h = P.h;
    const float ox = q.x - me.x, oyv = q.y - me.y;
    const float r2 = ox * ox + oyv * oyv;
    const float dst = fs_sqrt<FAST>(r2);                                // compute.wgsl:207,283
    float dx, dy;
    if (dst == 0.0f) {                                                  // :211-212
        const float rx = rand_f32(&seed);
        const float ry = rand_f32(&seed);
        const float len = fs_sqrt<FAST>(rx * rx + ry * ry);
        dx = fs_div<FAST>(rx, len);
        dy = fs_div<FAST>(ry, len);
    } else {
        dx = fs_div<FAST>(ox, dst);
        dy = fs_div<FAST>(oyv, dst);
    }
    const float npress = P.pressure_k * (nrho - P.rest_density);
    const float kern = (dst <= h) ? (-(h - dst)) * P.spiky : 0.0f;      // funcs.wgsl:101-109
    const float shared = (pressure + npress) * 0.5f;
    ForceTerms T;
    T.px = fs_div<FAST>(dx * kern * shared, nrho);                         // compute.wgsl:223
    T.py = fs_div<FAST>(dy * kern * shared, nrho);
    float kv = 0.0f;                                                    // funcs.wgsl:112-123
    if (dst <= h) {
        if (dst == 0.0f) {
            kv = P.visc_k;
        } else {
            // the two constant denominators go through div_const (bit-identical to `/`, proven per
            // constant at create time); 2.0f*h*h*h and h*h are exactly P.div_2h3.c / P.div_h2.c
            // (proven for FS_CONSTDIV_MIN <= |x| <= c; dst >= 2^-20 puts dst^2 and dst^3 inside, and
            //  dst <= h keeps them <= h^2 and h^3 = c/2)
            const bool tiny = dst < 9.5367431640625e-07f;                                   // 2^-20: rare, true division
            float a, b;
            if (FAST) {
                a = fs_div<true>(-(dst * dst * dst), 2.0f * h * h * h);
                b = fs_div<true>(dst * dst, h * h);
            } else if (tiny) {
                a = __fdiv_rn(-(dst * dst * dst), P.div_2h3.c);
                b = __fdiv_rn(dst * dst, P.div_h2.c);
            } else {
                a = div_const(P.div_2h3, -(dst * dst * dst));
                b = div_const(P.div_h2, dst * dst);
            }
            kv = P.visc_k * (a + b + (fs_div<FAST>(h, 2.0f * dst)) - 1.0f);
        }
    }
    T.vx = fs_div<FAST>(nv.x - mv.x, nrho) * kv;                           // compute.wgsl:288
    T.vy = fs_div<FAST>(nv.y - mv.y, nrho) * kv;
    return T;
}

// ---- tolerance mode (MODE 2, fs_options.math_mode = FS_MATH_TOLERANCE) ------------------------------------------
// The pressure and viscosity terms of one in-radius neighbour merged algebraically (compute.wgsl:207-223, :283-288,
// funcs.wgsl:101-123): one v_rsq_f32, fused multiply-adds, pressure_j and 1/rho_j precomputed per particle by
// k_density<true> — 24 issue slots per pair instead of ~85.  Within rtol 1e-5 / atol 1e-4*h of the IEEE oracle per
// step (tests/test_parity_gpu.py::test_tolerance_mode_*); cell keys and start_indices stay bit-exact (they come
// from the sort and the reorder pass, which this mode does not touch).  Coincident particles (r == 0) keep the
// reference's xorshift direction.
struct TolConsts { float cP, c3, c2, hh; };
__device__ __forceinline__ TolConsts tol_consts(const StepParams& P) {
    TolConsts C;
    const float h = P.h;
    C.cP = -0.5f * P.spiky;                       // kern * 0.5 = -(h - dst) * spiky * 0.5
    C.c3 = -1.0f / (2.0f * h * h * h);
    C.c2 = 1.0f / (h * h);
    C.hh = 0.5f * h;
    return C;
}
__device__ __forceinline__ void force_accum_tol(const StepParams& P, const TolConsts& C, const float2 me, const float2 mv,
                                                float pressure, const float2 q, const float2 nv,
                                                const float2 nd /* {pressure_j, 1/rho_j} */, ForceAcc& A) {
    const float ox = q.x - me.x, oy = q.y - me.y;
    const float r2 = __builtin_fmaf(ox, ox, oy * oy);
    float dirx = ox, diry = oy, inv, dst;
    if (r2 == 0.0f) {                                                   // compute.wgsl:211-212 (rare)
        const float rx = rand_f32(&A.seed), ry = rand_f32(&A.seed);
        const float il = __builtin_amdgcn_rsqf(__builtin_fmaf(rx, rx, ry * ry));
        dirx = rx * il; diry = ry * il;
        dst = 0.0f; inv = 1.0f;                                         // dir is already normalised
    } else {
        inv = __builtin_amdgcn_rsqf(r2);
        dst = r2 * inv;
    }
    const float w = fmaxf(P.h - dst, 0.0f);                             // dst <= h for every admitted candidate
    const float coefP = (w * C.cP) * (pressure + nd.x) * nd.y * inv;
    float u = __builtin_fmaf(C.c3, dst, C.c2);
    u = __builtin_fmaf(u, r2, -1.0f);
    u = r2 == 0.0f ? 1.0f : __builtin_fmaf(C.hh, inv, u);               // funcs.wgsl:116: r == 0 -> the bare constant
    const float kvv = u * (P.visc_k * nd.y);
    A.fpx = __builtin_fmaf(dirx, coefP, A.fpx);
    A.fpy = __builtin_fmaf(diry, coefP, A.fpy);
    A.fvx = __builtin_fmaf(nv.x - mv.x, kvv, A.fvx);
    A.fvy = __builtin_fmaf(nv.y - mv.y, kvv, A.fvy);
}

// The same terms with ONE true division per denominator (1/dst, 1/nrho) and div_by_rcp() for the
// seven quotients — bit-identical to force_terms<false> whenever `good` comes back all-ones (operands
// inside the proven range, fs_device.h).  Straight-line: no PRNG path, no tiny-distance path;
// those (and any out-of-range operand) clear the lane's bit in `good`, and the caller re-evaluates
// the pair with the exact body for the whole wave when any active lane's bit is missing.
// Guards per pair: r2 >= 2^-40 (excludes r2 == 0 = the PRNG path, NaN and div_const's tiny range; r2 <= h*h
// because the scan admitted it, and the host only enables this path for h <= 2^19: the proven sqrt range), the
// neighbour's "safe operand" sign (fs_device.h; the lane's own is folded in by the caller), and the lower bound
// of the two pressure numerators.
__device__ __forceinline__ wave_mask num_lo_ok(float a) { return wm(fabsf(a) >= 0x1p-76f) | wm(a == 0.0f); }   // NaN: 0 (fs_device.h: why 2^-76)
__device__ __forceinline__ ForceTerms force_terms_shared(const StepParams& P, const float2 me, const float2 mv,
                                                         float pressure, const float2 q, const float2 nv,
                                                         const float2 nd /* {density, +-RN(1/density)} */, wave_mask& good) {
    const float h = P.h;
    const float nrho = nd.x, yrho = nd.y;
    const float ox = q.x - me.x, oyv = q.y - me.y;
    const float r2 = ox * ox + oyv * oyv;
    good = wm(r2 >= FS_SQRT_LO) & wm(yrho > 0.0f);
    const float dst = sqrt_rn_fast(r2);                                 // in [2^-20, ~h]
    const float ydst = rcp_rn_fast(dst);
    const float dx = div_by_rcp(ox, dst, ydst);
    const float dy = div_by_rcp(oyv, dst, ydst);
    const float npress = P.pressure_k * (nrho - P.rest_density);
    // no `dst <= h` test here (the exact body keeps the reference's): it cannot fail for a pair this path is answerable for.
    // Every caller admits a pair by !(r2 > sqr_radius), `good` sends r2 < 2^-40 and NaN to the exact body, and share_div implies
    // sqr_radius == RN(h * h) (engine.hip): sqrt is monotone and RN(sqrt(RN(h * h))) <= h for every f32 h of [2^-19, 2^19]
    // (tests/test_force_identities.py enumerates them), so dst == RN(sqrt(r2)) <= h.
    const float kern = (-(h - dst)) * P.spiky;
    const float shared = (pressure + npress) * 0.5f;
    const float apx = dx * kern * shared, apy = dy * kern * shared;
    const float dvx = nv.x - mv.x, dvy = nv.y - mv.y;
    good &= num_lo_ok(apx) & num_lo_ok(apy);
    ForceTerms T;
    T.px = div_by_rcp(apx, nrho, yrho);
    T.py = div_by_rcp(apy, nrho, yrho);
    // share_div implies both constant-division proofs succeeded (engine.hip)
    const float a = div_const_fast(-(dst * dst * dst), P.div_2h3.c, P.div_2h3.y);
    const float b = div_const_fast(dst * dst, P.div_h2.c, P.div_h2.y);
    // h / (2 dst) as (h/2) / dst: q0, the residual and the final fma are those of div_by_rcp(h, 2 dst, RN(1/dst)/2) halved, all
    // exactly (h in [2^-19, 2^19], dst in [2^-20, h]: nothing underflows), and h/2 comes in a scalar register (StepParams::half_h) — three instructions per pair
    const float hq = div_by_rcp(P.half_h, dst, ydst);
    const float kv = P.visc_k * (a + b + hq - 1.0f);
    T.vx = div_by_rcp(dvx, nrho, yrho) * kv;
    T.vy = div_by_rcp(dvy, nrho, yrho) * kv;
    return T;
}

}  // namespace fsd

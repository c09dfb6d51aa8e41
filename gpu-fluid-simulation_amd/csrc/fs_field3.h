// fs_field3.h — the field of the 3D fluid at one point, for the kernels that evaluate it where THEY choose (kernels_render3d.hip:
// along a ray; kernels_mesh3d.hip: at lattice nodes and mesh vertices): the density-only walk and the full-sample walk of the
// "3D field sampling" statement (include/fluidsim.h), one lane per point, every sum in the statement's order.
//
// k3_sample (kernels_sample3d.hip) keeps its own copy of the walk: its instruction stream is pinned (tools/isa_compare.py), and
// the walks here differ in what they carry (density3_at: the ranges are hoisted, the body is the density term alone).
#pragma once
#include "fs_3d.h"

namespace fsd {

// The valid columns of cx-1 .. cx+1: consecutive, also when cx wrapped to 0 (k3_sample).
__device__ __forceinline__ void columns3(const Params3& P, uint32_t cx, uint32_t* xlo, uint32_t* xn) {
    *xlo = 0u; *xn = 0u;
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        const uint32_t X = cx + (uint32_t)ox;
        if (X < P.gw) { if (*xn == 0u) *xlo = X; *xn += 1u; }
    }
}

// sum m W at (x, y, z): the `density` of the sampling statement, nothing else of its record.
__device__ __forceinline__ float density3_at(const Params3& P, float x, float y, float z, const float4* __restrict__ pred,
                                             const uint32_t* __restrict__ cs) {
    uint32_t cx, cy, cz, xlo, xn;
    cell_xyz3(P, make_float4(x, y, z, 0.0f), &cx, &cy, &cz);
    columns3(P, cx, &xlo, &xn);
    uint32_t lo[9], hi[9], total = 0u;
#pragma unroll
    for (int r = 0; r < 9; ++r) {                                   // row r: oz = r / 3 - 1, oy = r % 3 - 1
        const uint32_t Z = cz + (uint32_t)(r / 3 - 1), Y = cy + (uint32_t)(r % 3 - 1);
        lo[r] = 0u; hi[r] = 0u;
        if (Z < P.gd && Y < P.gh && xn != 0u) {
            const uint32_t id_lo = (Z * P.gh + Y) * P.gw + xlo;     // < ncell; id_lo + xn <= ncell: cs has ncell + 1 entries
            lo[r] = cs[id_lo];
            hi[r] = cs[id_lo + xn];
            if (hi[r] > P.n) hi[r] = P.n;
            if (hi[r] > lo[r]) total += hi[r] - lo[r];
        }
    }
    float density = 0.0f;
    if (total == 0u) return density;                                // no particle in the 27 cells: exactly +0
    const float h2 = P.h2, c6 = P.poly6, m = P.mass;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        for (uint32_t k = lo[r]; k < hi[r]; ++k) {
            const float4 p = pred[k];
            const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
            const float r2 = dx * dx + dy * dy + dz * dz;
            if (r2 > h2) continue;
            const float e = h2 - r2;
            density += m * (((c6 * e) * e) * e);
        }
    }
    return density;
}

struct FullSample3 { float density, weight, vx, vy, vz, gx, gy, gz; };

// The full record of the sampling statement at (x, y, z), k3_sample's loop and expression order.
__device__ __forceinline__ FullSample3 sample3_at(const Params3& P, float x, float y, float z, const float4* __restrict__ pred,
                                                  const float4* __restrict__ vel, const uint32_t* __restrict__ cs) {
    uint32_t cx, cy, cz, xlo, xn;
    cell_xyz3(P, make_float4(x, y, z, 0.0f), &cx, &cy, &cz);
    columns3(P, cx, &xlo, &xn);
    const float h2 = P.h2, c6 = P.poly6, cg = 6.0f * P.poly6, m = P.mass;
    FullSample3 S = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int oz = -1; oz <= 1; ++oz) {
        const uint32_t Z = cz + (uint32_t)oz;
        if (Z >= P.gd || xn == 0u) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            const uint32_t Y = cy + (uint32_t)oy;
            if (Y >= P.gh) continue;
            const uint32_t id_lo = (Z * P.gh + Y) * P.gw + xlo;
            const uint32_t lo = cs[id_lo];
            uint32_t hi = cs[id_lo + xn];
            if (hi > P.n) hi = P.n;
            for (uint32_t k = lo; k < hi; ++k) {
                const float4 p = pred[k];
                const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (r2 > h2) continue;
                const float e = h2 - r2;
                const float W = ((c6 * e) * e) * e;
                S.density += m * W;
                const float g = m * ((cg * e) * e);
                S.gx += g * dx; S.gy += g * dy; S.gz += g * dz;
                const float t = __fdiv_rn(m, p.w) * W;
                const float4 v = vel[k];
                S.weight += t;
                S.vx += t * v.x; S.vy += t * v.y; S.vz += t * v.z;
            }
        }
    }
    return S;
}

}  // namespace fsd

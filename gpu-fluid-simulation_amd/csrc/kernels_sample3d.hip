// kernels_sample3d.hip — 3D field sampling (build extension): density, density gradient and velocity of the 3D
// fluid at arbitrary points, from the cell-sorted state the last step left on the device (pred with the density in .w, vel,
// cs).  The 3D form of kernels_sample.hip; no reference counterpart (the reference is 2D only).
//
// Statement (include/fluidsim.h "3D field sampling"), f32 without contraction, for a query point x:
//   (cx, cy, cz) = cell coordinates of x (true division by h: a query is not bounded like a clamped particle position)
//   for oz in -1..1, oy in -1..1, ox in -1..1:  X = cx + ox, ... (wrapping u32), skipped when X >= grid_w, Y >= grid_h or Z >= grid_d
//     for the particles k of cell (X, Y, Z), ascending:
//       d = q_k - x, r2 = d.d;  skipped when r2 > h2;  e = h2 - r2;  W = ((C6 e) e) e
//       density += m W;  g = m ((Cg e) e);  gradient += g d;  t = (m / rho_k) W;  weight += t;  velocity += t v_k;  neighbours += 1
// The valid cells of one (Z, Y) sweep row are consecutive ids and the slots are in id order, so a row is ONE contiguous slot
// range [cs[id_lo], cs[id_lo + count]) of the dense cell-start table, walked ascending: exactly the order above.  A skipped
// candidate adds nothing — a branch, not an added zero: the velocity and gradient terms can be -0.
//
// One lane per query keeps that order for free; nothing is staged.  The wave tiles a grid is taken in: fs_sample3.h.
#include "fs_sample3.h"

namespace fsd {

struct Sample3Rec {                // fs3_sample (include/fluidsim.h), 40 bytes
    float density, weight, vx, vy, vz, gx, gy, gz;
    uint32_t neighbours, cell;
};
static_assert(sizeof(Sample3Rec) == 40, "fs3_sample is 40 bytes");

// GRID: the points are the voxel centres of a view (fs_sample_grid's expression per axis) instead of loaded.
template <bool GRID>
__global__ __launch_bounds__(B3S) void k3_sample(Params3 P, uint32_t nq, const float* __restrict__ points, float3 wmin,
                                                      float3 wmax, uint32_t width, uint32_t height, uint32_t depth,
                                                      Sample3Tile T, const float4* __restrict__ pred,
                                                      const float4* __restrict__ vel, const uint32_t* __restrict__ cs,
                                                      Sample3Rec* __restrict__ out) {
    size_t q;
    float x, y, z;
    if (GRID) {
        if (!sample3_tile_voxel(T, wmin, wmax, width, height, depth, &q, &x, &y, &z)) return;
    } else {
        q = (size_t)blockIdx.x * B3S + threadIdx.x;
        if (q >= nq) return;
        x = points[3 * q]; y = points[3 * q + 1]; z = points[3 * q + 2];
    }
    uint32_t cx, cy, cz;
    cell_xyz3(P, make_float4(x, y, z, 0.0f), &cx, &cy, &cz);       // the true division: no create-time proof covers a query
    // the valid columns of cx-1 .. cx+1: consecutive, also when cx wrapped to 0
    uint32_t xlo = 0u, xn = 0u;
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        const uint32_t X = cx + (uint32_t)ox;
        if (X < P.gw) { if (xn == 0u) xlo = X; ++xn; }
    }
    const float h2 = P.h2, c6 = P.poly6, cg = 6.0f * P.poly6, m = P.mass;
    float density = 0.0f, weight = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    uint32_t nb = 0u;
    for (int oz = -1; oz <= 1; ++oz) {
        const uint32_t Z = cz + (uint32_t)oz;
        if (Z >= P.gd || xn == 0u) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            const uint32_t Y = cy + (uint32_t)oy;
            if (Y >= P.gh) continue;
            const uint32_t id_lo = (Z * P.gh + Y) * P.gw + xlo;    // < ncell; id_lo + xn <= ncell: cs has ncell + 1 entries
            const uint32_t lo = cs[id_lo];
            uint32_t hi = cs[id_lo + xn];
            if (hi > P.n) hi = P.n;
            for (uint32_t k = lo; k < hi; ++k) {
                const float4 p = pred[k];                          // position and density: one 16-byte load
                const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (r2 > h2) continue;
                const float e = h2 - r2;
                const float W = ((c6 * e) * e) * e;
                density += m * W;
                const float g = m * ((cg * e) * e);
                gx += g * dx; gy += g * dy; gz += g * dz;
                // the division: vel_s.w holds +-RN(1 / rho), which is m / rho for m == 1 only, behind a second 16-byte load
                const float t = __fdiv_rn(m, p.w) * W;
                const float4 v = vel[k];
                weight += t;
                vx += t * v.x; vy += t * v.y; vz += t * v.z;
                nb += 1u;
            }
        }
    }
    Sample3Rec r;
    r.density = density; r.weight = weight; r.vx = vx; r.vy = vy; r.vz = vz; r.gx = gx; r.gy = gy; r.gz = gz;
    r.neighbours = nb; r.cell = (cz * P.gh + cy) * P.gw + cx;
    out[q] = r;
}

void launch3_sample(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3Query& Q) {
    if (Q.n == 0u) return;
    if (Q.points) {
        hipLaunchKernelGGL(k3_sample<false>, dim3((Q.n + B3S - 1u) / B3S), dim3(B3S), 0, st, P, Q.n, Q.points, Q.wmin,
                           Q.wmax, Q.width, Q.height, Q.depth, Sample3Tile{}, A.pred, A.vel, A.cs, (Sample3Rec*)Q.out);
    } else {
        const Sample3Tile T = sample3_tile(Q.width, Q.height, Q.depth);
        hipLaunchKernelGGL(k3_sample<true>, dim3(sample3_tile_blocks(T, Q.depth)), dim3(B3S), 0, st, P, Q.n, Q.points, Q.wmin, Q.wmax,
                           Q.width, Q.height, Q.depth, T, A.pred, A.vel, A.cs, (Sample3Rec*)Q.out);
    }
}

}  // namespace fsd

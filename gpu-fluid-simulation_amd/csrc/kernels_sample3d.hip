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
// One lane per query keeps that order for free; nothing is staged.  As in 2D the ORDER of the queries decides the speed: lanes
// of a wave that fall into the same or adjacent cells walk the same cache lines and leave the loops together.  A grid is
// therefore taken in wave tiles that are compact in every axis that has extent (launch3_sample picks them).
#include "fs_3d.h"

namespace fsd {

struct Sample3Rec {                // fs3_sample (include/fluidsim.h), 40 bytes
    float density, weight, vx, vy, vz, gx, gy, gz;
    uint32_t neighbours, cell;
};
static_assert(sizeof(Sample3Rec) == 40, "fs3_sample is 40 bytes");

#define B3S 256                    // workgroup: four waves, one query per lane

// The 256 threads of a workgroup over a GRID tile: the low bits of the lane (then of the wave) number go to x, the next to y,
// the rest to z.  lane = log2 extents of a wave's tile (they sum to 6), wave = those of the 2 x 2 (x 1) waves of a workgroup.
struct Sample3Tile {
    uint32_t lx, ly, wx, wy;       // log2: lane bits in x, in y (z: the rest); wave bits in x, in y (z: the rest)
    uint32_t tx, ty, tz;           // log2 extents of the workgroup's tile
    uint32_t nbx, nby;             // workgroup tiles along x, along y
};

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
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const uint32_t bi = blockIdx.x % T.nbx, bj = (blockIdx.x / T.nbx) % T.nby, bk = blockIdx.x / (T.nbx * T.nby);
        const uint32_t i = (bi << T.tx) + ((wave & ((1u << T.wx) - 1u)) << T.lx) + (lane & ((1u << T.lx) - 1u));
        const uint32_t j = (bj << T.ty) + (((wave >> T.wx) & ((1u << T.wy) - 1u)) << T.ly) + ((lane >> T.lx) & ((1u << T.ly) - 1u));
        const uint32_t k = (bk << T.tz) + ((wave >> (T.wx + T.wy)) << (6u - T.lx - T.ly)) + (lane >> (T.lx + T.ly));
        if (i >= width || j >= height || k >= depth) return;        // edge tiles are masked
        q = ((size_t)k * height + j) * width + i;
        x = wmin.x + __fdiv_rn((float)i + 0.5f, (float)width) * (wmax.x - wmin.x);
        y = wmin.y + __fdiv_rn((float)j + 0.5f, (float)height) * (wmax.y - wmin.y);
        z = wmin.z + __fdiv_rn((float)k + 0.5f, (float)depth) * (wmax.z - wmin.z);
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

// The wave tile of a view: six lane bits dealt round-robin (x, y, z) to the axes that have extent — 4 x 4 x 4 voxels for a
// volume, 8 x 8 for a slice, 64 in a row for a line —, then the two wave bits of the workgroup the same way (8 x 8 x 4,
// 16 x 16, 256).
static Sample3Tile sample3_tile(uint32_t width, uint32_t height, uint32_t depth) {
    const bool has[3] = {width > 1u, height > 1u || (width <= 1u && depth <= 1u), depth > 1u};
    uint32_t lane[3] = {0, 0, 0}, wave[3] = {0, 0, 0};
    int a = 0;
    for (int bit = 0; bit < 8; ++bit) {
        while (!has[a]) a = (a + 1) % 3;
        (bit < 6 ? lane : wave)[a] += 1u;
        a = (a + 1) % 3;
    }
    Sample3Tile T;
    T.lx = lane[0]; T.ly = lane[1]; T.wx = wave[0]; T.wy = wave[1];
    T.tx = lane[0] + wave[0]; T.ty = lane[1] + wave[1]; T.tz = lane[2] + wave[2];
    T.nbx = (width + (1u << T.tx) - 1u) >> T.tx;
    T.nby = (height + (1u << T.ty) - 1u) >> T.ty;
    return T;
}

void launch3_sample(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3Query& Q) {
    if (Q.n == 0u) return;
    if (Q.points) {
        hipLaunchKernelGGL(k3_sample<false>, dim3((Q.n + B3S - 1u) / B3S), dim3(B3S), 0, st, P, Q.n, Q.points, Q.wmin,
                           Q.wmax, Q.width, Q.height, Q.depth, Sample3Tile{}, A.pred, A.vel, A.cs, (Sample3Rec*)Q.out);
    } else {
        const Sample3Tile T = sample3_tile(Q.width, Q.height, Q.depth);
        const uint32_t nbz = (Q.depth + (1u << T.tz) - 1u) >> T.tz;
        hipLaunchKernelGGL(k3_sample<true>, dim3(T.nbx * T.nby * nbz), dim3(B3S), 0, st, P, Q.n, Q.points, Q.wmin, Q.wmax,
                           Q.width, Q.height, Q.depth, T, A.pred, A.vel, A.cs, (Sample3Rec*)Q.out);
    }
}

}  // namespace fsd

// kernels_sample.hip — field sampling (build extension): density, velocity and tracking channels of the 2D fluid
// at arbitrary points, from the cell-sorted state the last step left on the device.  NOT in the reference; the quantity is its
// calculate_density_at_point (funcs.wgsl:157-203) evaluated at a point that need not be a particle, plus the SPH interpolants
// sum_j (m / rho_j) W_j f_j of the velocity and of the channels.
//
// Statement (include/fluidsim.h "field sampling"), f32 without contraction, for a query point x:
//   (cx, cy) = cell coordinates of x (true division by h: a query is not bounded like a clamped particle position)
//   for oy in -1..1, ox in -1..1:  X = cx + ox, Y = cy + oy (wrapping u32), skipped when X >= grid_w or Y >= grid_h
//     for the particles k of cell (X, Y), ascending, from the reference start index (the stale-start quirk included):
//       d = q_k - x, r2 = d.d;  skipped when r2 > h2;  e = h2 - r2;  W = ((Cv e) e) e
//       density += m W;  t = (m / rho_k) W;  weight += t;  velocity += t v_k;  a_c += t attr_c[k];  neighbours += 1
// The valid cells of one sweep row are consecutive ids and the slots are in id order, so a row is ONE contiguous slot range
// [cs[id_lo], cs[id_hi]) of the dense cell-start table, walked ascending: exactly the order above (fs_neighbours.h
// "neighbour ranges").  A skipped candidate adds nothing — a branch, not an added zero: the velocity and channel terms can be -0.
//
// One lane per query keeps that order for free.  Nothing is staged: scattered points share no candidates.  What decides the
// speed is the ORDER of the queries.  Lanes of a wave that fall into the same or adjacent cells (a grid — taken in 16 x 16
// pixel tiles here —, points sorted by cell, the particles' own positions in slot order) walk the same few cache lines and
// leave the loop together; randomly ordered points make every lane gather from its own lines and every wave wait for its
// longest row.  The caller chooses the order; nothing is sorted behind its back.
#include "fs_kernels.h"
#include "fs_neighbours.h"

namespace fsd {

struct SampleRec {                 // fs_sample (include/fluidsim.h), 24 bytes
    float density, weight, vx, vy;
    uint32_t neighbours, cell;
};
static_assert(sizeof(SampleRec) == 24, "fs_sample is 24 bytes");

#define FS_SAMPLE_TILE 16u         // GRID: a workgroup takes a 16 x 16 pixel tile (a wave: 16 x 4)

// C: channels (0..4).  GRID: the points are the pixel centres of a view (fs_render_density's expression) instead of loaded.
// RCP: rho2[k].y holds +-RN(1 / rho_k) and m == 1.0f, so m / rho_k is |rho2[k].y| — the same bits as the division.
// Otherwise rho != nullptr (tolerance mode, or an uploaded state): the densities are rho[k], else rho2[k].x.
template <int C, bool GRID, bool RCP>
__global__ __launch_bounds__(FS_BLOCK) void k_sample(StepParams P, uint32_t nq, const float2* __restrict__ points, float2 wmin,
                                                     float2 wmax, uint32_t width, uint32_t height,
                                                     const float2* __restrict__ pred, const float2* __restrict__ vel,
                                                     const float2* __restrict__ rho2, const float* __restrict__ rho,
                                                     const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                                     const u64* __restrict__ pairs, const float* __restrict__ attr,
                                                     uint32_t attr_stride, SampleRec* __restrict__ out,
                                                     float* __restrict__ attr_out) {
    size_t q;
    float2 x;
    if (GRID) {
        const uint32_t tiles_x = (width + FS_SAMPLE_TILE - 1u) / FS_SAMPLE_TILE;
        const uint32_t i = (blockIdx.x % tiles_x) * FS_SAMPLE_TILE + (threadIdx.x % FS_SAMPLE_TILE);
        const uint32_t j = (blockIdx.x / tiles_x) * FS_SAMPLE_TILE + (threadIdx.x / FS_SAMPLE_TILE);
        if (i >= width || j >= height) return;
        q = (size_t)j * width + i;
        x.x = wmin.x + __fdiv_rn((float)i + 0.5f, (float)width) * (wmax.x - wmin.x);
        x.y = wmin.y + __fdiv_rn((float)j + 0.5f, (float)height) * (wmax.y - wmin.y);
    } else {
        q = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
        if (q >= nq) return;
        x = points[q];
    }
    const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    uint32_t cx, cy;
    xy_local(P, x, &cx, &cy);          // P.div_h.ok == 0 (launch_sample): the true division
    // not row_range (fs_neighbours.h), on purpose: reference-layout ids, only a row's valid columns (a query may lie outside), hi <= n
    // the valid columns of cx-1 .. cx+1: consecutive, also when cx wrapped to 0
    uint32_t xlo = 0u, xn = 0u;
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        const uint32_t X = cx + (uint32_t)ox;
        if (X < P.grid_w) { if (xn == 0u) xlo = X; ++xn; }
    }
    const float h2 = P.h * P.h, cv = P.poly6_norm, m = P.mass;
    float density = 0.0f, weight = 0.0f, vx = 0.0f, vy = 0.0f;
    float a[C > 0 ? C : 1];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = 0.0f;
    uint32_t nb = 0u;
    for (int oy = -1; oy <= 1; ++oy) {
        const uint32_t Y = cy + (uint32_t)oy;
        if (Y >= P.grid_h || xn == 0u) continue;
        const uint32_t id_lo = Y * P.grid_w + xlo;         // < ncell; id_lo + xn <= ncell: cs has ncell + 1 entries
        uint32_t lo = cs[id_lo], hi = cs[id_lo + xn];
        if (lo == 0u) lo = lo_fix;
        if (hi > P.n) hi = P.n;
        for (uint32_t k = lo; k < hi; ++k) {
            const float2 p = pred[k];
            const float dx = p.x - x.x, dy = p.y - x.y;
            const float r2 = dx * dx + dy * dy;
            if (r2 > h2) continue;
            const float e = h2 - r2;
            const float W = ((cv * e) * e) * e;
            density += m * W;
            const float t = (RCP ? fabsf(rho2[k].y) : __fdiv_rn(m, rho ? rho[k] : rho2[k].x)) * W;
            const float2 v = vel[k];
            weight += t;
            vx += t * v.x;
            vy += t * v.y;
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] += t * attr[(size_t)c * attr_stride + k];
            nb += 1u;
        }
    }
    SampleRec r;
    r.density = density; r.weight = weight; r.vx = vx; r.vy = vy;
    r.neighbours = nb; r.cell = cy * P.grid_w + cx;
    out[q] = r;
#pragma unroll
    for (int c = 0; c < C; ++c) attr_out[(size_t)c * nq + q] = a[c];
}

template <int C, bool GRID>
static void launch_sample_c(hipStream_t st, const StepParams& P, const SampleQuery& Q, const SampleState& S, bool rcp) {
    const uint32_t tile = FS_SAMPLE_TILE;
    const uint32_t grid = GRID ? ((Q.width + tile - 1u) / tile) * ((Q.height + tile - 1u) / tile) : (Q.n + FS_BLOCK - 1u) / FS_BLOCK;
    if (rcp)
        hipLaunchKernelGGL((k_sample<C, GRID, true>), dim3(grid), dim3(FS_BLOCK), 0, st, P, Q.n, Q.points, Q.wmin, Q.wmax, Q.width,
                           Q.height, S.pred, S.vel, S.rho2, S.rho, S.cs, S.start_ref, S.pairs, S.attr, S.attr_stride,
                           (SampleRec*)Q.out, Q.attr_out);
    else
        hipLaunchKernelGGL((k_sample<C, GRID, false>), dim3(grid), dim3(FS_BLOCK), 0, st, P, Q.n, Q.points, Q.wmin, Q.wmax, Q.width,
                           Q.height, S.pred, S.vel, S.rho2, S.rho, S.cs, S.start_ref, S.pairs, S.attr, S.attr_stride,
                           (SampleRec*)Q.out, Q.attr_out);
}

void launch_sample(hipStream_t st, const StepParams& P_in, const SampleQuery& Q, const SampleState& S) {
    if (Q.n == 0u) return;
    StepParams P = P_in;
    P.div_h.ok = 0;                    // the 3-instruction quotient is proven for clamped positions only
    const bool rcp = S.rho == nullptr && P.mass == 1.0f;
    const bool grid = Q.points == nullptr;
#define FS_SAMPLE_CASE(C)                                               \
    case C:                                                             \
        if (grid) launch_sample_c<C, true>(st, P, Q, S, rcp);           \
        else launch_sample_c<C, false>(st, P, Q, S, rcp);               \
        break
    switch (S.channels) {
        FS_SAMPLE_CASE(0); FS_SAMPLE_CASE(1); FS_SAMPLE_CASE(2); FS_SAMPLE_CASE(3); FS_SAMPLE_CASE(4);
    }
#undef FS_SAMPLE_CASE
}

}  // namespace fsd

// kernels_sample_attr3d.hip — the tracking channels in 3D field sampling (build extension): the SPH interpolant
// sum_k (m / rho_k) W_k attr[c][k] of the C channels an fs_sim3 carries (kernels_track.hip) at arbitrary points, from the same
// cell-sorted state k3_sample walks (kernels_sample3d.hip).  A kernel of its own: k3_sample keeps its instruction stream, and a
// caller who wants no channels pays nothing for them.
//
// Statement (include/fluidsim.h "3D channel sampling"): the cells, their order, the skip rules, the r2 > h2 branch, W and
// t = (m / rho_k) W of "3D field sampling"; for an in-radius candidate  weight += t;  a_c += t * attr[c][k]  for c < C.  The sums
// start at +0.0f, a skipped candidate is a branch, the results are un-normalised.  Hence, bit for bit: `weight` is fs3_sample's,
// a channel that holds 1.0f everywhere sums to `weight`, and one that holds a velocity component sums to fs3_sample's velocity.
//
// One lane per query keeps the statement's order for free.  Per candidate one 16-byte load (position and density); the C channel
// words are gathered for in-radius candidates only, all of them issued before the first add.  `vel` is never touched.  A grid is
// taken in k3_sample<true>'s wave tiles (fs_sample3.h).
#include "fs_sample3.h"

namespace fsd {

// attr: channel c at attr + c * stride, slot order.  attr_out: channel c at attr_out + c * nq.  weight_out: may be null.
template <int C, bool GRID>
__global__ __launch_bounds__(B3S) void k3_sample_attr(Params3 P, uint32_t nq, const float* __restrict__ points, float3 wmin,
                                                      float3 wmax, uint32_t width, uint32_t height, uint32_t depth, Sample3Tile T,
                                                      const float4* __restrict__ pred, const uint32_t* __restrict__ cs,
                                                      const float* __restrict__ attr, uint32_t stride,
                                                      float* __restrict__ weight_out, float* __restrict__ attr_out) {
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
    const float h2 = P.h2, c6 = P.poly6, m = P.mass;
    float weight = 0.0f;
    float sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.0f;
    for (int oz = -1; oz <= 1; ++oz) {
        const uint32_t Z = cz + (uint32_t)oz;
        if (Z >= P.gd || xn == 0u) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            const uint32_t Y = cy + (uint32_t)oy;
            if (Y >= P.gh) continue;
            const uint32_t id_lo = (Z * P.gh + Y) * P.gw + xlo;    // < ncell; id_lo + xn <= ncell: cs has ncell + 1 entries
            const uint32_t lo = cs[id_lo];
            uint32_t hi = cs[id_lo + xn];
            if (hi > P.n) hi = P.n;                                // k < n <= stride below
            for (uint32_t k = lo; k < hi; ++k) {
                const float4 p = pred[k];                          // position and density: one 16-byte load
                const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (r2 > h2) continue;
                float a[C];
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] = attr[(size_t)c * stride + k];   // all gathers in flight before the first add
                const float e = h2 - r2;
                const float W = ((c6 * e) * e) * e;
                const float t = __fdiv_rn(m, p.w) * W;
                weight += t;
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += t * a[c];
            }
        }
    }
    if (weight_out) weight_out[q] = weight;
#pragma unroll
    for (int c = 0; c < C; ++c) attr_out[(size_t)c * nq + q] = sum[c];
}

template <int C>
static void launch3_sample_attr_c(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3AttrQuery& Q) {
    if (Q.points) {
        hipLaunchKernelGGL((k3_sample_attr<C, false>), dim3((Q.n + B3S - 1u) / B3S), dim3(B3S), 0, st, P, Q.n, Q.points, Q.wmin,
                           Q.wmax, Q.width, Q.height, Q.depth, Sample3Tile{}, A.pred, A.cs, Q.attr, Q.attr_stride, Q.weight_out,
                           Q.attr_out);
    } else {
        const Sample3Tile T = sample3_tile(Q.width, Q.height, Q.depth);
        hipLaunchKernelGGL((k3_sample_attr<C, true>), dim3(sample3_tile_blocks(T, Q.depth)), dim3(B3S), 0, st, P, Q.n, Q.points,
                           Q.wmin, Q.wmax, Q.width, Q.height, Q.depth, T, A.pred, A.cs, Q.attr, Q.attr_stride, Q.weight_out,
                           Q.attr_out);
    }
}

void launch3_sample_attr(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3AttrQuery& Q) {
    if (Q.n == 0u) return;
    switch (Q.channels) {
        case 1: launch3_sample_attr_c<1>(st, P, A, Q); break;
        case 2: launch3_sample_attr_c<2>(st, P, A, Q); break;
        case 3: launch3_sample_attr_c<3>(st, P, A, Q); break;
        default: launch3_sample_attr_c<4>(st, P, A, Q); break;
    }
}

}  // namespace fsd

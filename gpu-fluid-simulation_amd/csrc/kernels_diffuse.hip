// kernels_diffuse.hip — opt-in diffusion and buoyancy of the tracking channels (build extension), between the
// density pass (and the surface-tension pass, when on) and the force pass.
//   k_diffuse<D, MASS1> = D diffusing channels over the density pass's neighbour walk; its tail also forms the buoyancy force
//   k_buoyancy          = the buoyancy force alone (no diffusing channel): no walk
//
// Normative statement: include/fluidsim.h "channel diffusion and buoyancy".  Per sorted slot i, over the candidates the density
// pass visits (same rows, same order, the particle itself and the stale-start quirk included), all f32 without contraction:
//   o = q_j - q_i, r2 = o.o;  skip if r2 > h2;  d = h2 - r2;  w = m / rho_j;  wk = w * ((Cg d) d)
//   acc_c += wk * (A_c[j] - A_c[i])                       for each diffusing channel c
// then u_i = 1 / rho_i and A_c'[i] = A_c[i] + (g_c acc_c) u_i with g_c = (2 kappa_c) delta from the host.  Jacobi: every A_c[j] is
// read from `attr_in` and every A_c' goes to the same row of `attr_out`, the spare tracking set; a channel that does not diffuse
// is neither read nor written.  The walk is the driver's (fs_neighbours.h walk_lane / walk_bounds / walk_rows, as k_density and
// k_surface_tension use it) with DiffuseTerms: three rows staged in LDS where the block's ranges fit, the unstaged global sweep where they
// do not; w_j is formed once per staged candidate (with MASS1 it is the density pass's |rho2.y| = RN(1/rho_j)) and sits next to q_j and
// the D channel values in LDS: (12 + 4 D) x 3 x NB_TILE bytes.
// Buoyancy (channel b, may be one of the diffusing ones or not): a = A_b[i] before the pass,
//   s = beta (A0 - a);  fb = (st_i +) ((rho_i s) g.x, (rho_i s) g.y)
// which the force launch takes as the `st` operand of its ST instantiations.
#include <stdlib.h>

#include "fs_kernels.h"
#include "fs_neighbours.h"

namespace fsd {

// By value: the compact list of the diffusing channels of this launch and the buoyancy channel's constants.
struct DiffuseConsts {
    float h2, cg;
    uint32_t ch[4];                 // channel index of each of the D accumulators, ascending
    float g[4];                     // (2 kappa_c) delta of each
    int32_t buoy;                   // the buoyancy channel, or -1: this launch writes no fb
    float beta, a0, gx, gy;
};

template <int D> struct DfAcc { float v[D]; };
template <int D> struct DfCandidate { float2 q; float d; DfAcc<D> a; };   // staged of a candidate: position, weight operand, channels

template <int D>
__device__ __forceinline__ void df_term(float h2, float cg, float2 me, const DfAcc<D>& mine, float2 q, float w, const DfAcc<D>& a,
                                        DfAcc<D>& acc) {
    const float ox = q.x - me.x, oy = q.y - me.y;
    const float r2 = ox * ox + oy * oy;
    const bool in = !(r2 > h2);                     // a NaN candidate is not skipped (the statement's test, as written)
    const float d = h2 - r2;
    const float wk = w * ((cg * d) * d);
    // a select, not a product with zero: a skipped candidate's A may be a NaN.  An accumulator that starts at +0.0f is never
    // -0.0f, so adding +0.0f for a skipped candidate IS skipping it
#pragma unroll
    for (int c = 0; c < D; ++c) acc.v[c] += in ? wk * (a.v[c] - mine.v[c]) : 0.0f;
}

// The buoyancy force of slot i (the tail of k_diffuse, the whole of k_buoyancy).
__device__ __forceinline__ float2 buoyancy_force(const DiffuseConsts& C, float a, float rho_i, const float2* __restrict__ st_in, uint32_t i) {
    const float s = C.beta * (C.a0 - a);
    const float rs = rho_i * s;
    const float bx = rs * C.gx, by = rs * C.gy;
    if (st_in) {
        const float2 f = st_in[i];
        return make_float2(f.x + bx, f.y + by);
    }
    return make_float2(bx, by);
}

// The diffusion terms as walk_rows takes them (fs_neighbours.h).  `rows` (the D diffusing rows of attr_in), `mine` and `acc` are locals
// of the kernel (as members they cost up to 10 SGPRs), which loads `mine` between the two halves of walk_lane.
template <int D, bool MASS1> struct DiffuseTerms {
    const StepParams& P; const DiffuseConsts& C;
    const float2 *__restrict__ pred, *__restrict__ rho2;
    const float* __restrict__ rho_arr;
    float2 (*s_q)[NB_TILE]; float (*s_w)[NB_TILE]; float (*s_a)[3][NB_TILE];
    float2 me;
    const float* const* rows; const DfAcc<D>& mine; DfAcc<D>& acc;
    __device__ __forceinline__ DfCandidate<D> fetch(uint32_t k) const {
        DfCandidate<D> c;
        c.q = pred[k]; c.d = walk_weight_operand<MASS1>(rho2, rho_arr, k);
#pragma unroll
        for (int e = 0; e < D; ++e) c.a.v[e] = rows[e][k];
        return c;
    }
    __device__ __forceinline__ void put(int r, uint32_t j, const DfCandidate<D>& c) {
        s_q[r][j] = c.q; s_w[r][j] = walk_weight_of<MASS1>(P, c.d);
#pragma unroll
        for (int e = 0; e < D; ++e) s_a[e][r][j] = c.a.v[e];
    }
    __device__ __forceinline__ DfAcc<D> staged_a(int r, uint32_t k) const {
        DfAcc<D> a;
#pragma unroll
        for (int e = 0; e < D; ++e) a.v[e] = s_a[e][r][k];
        return a;
    }
    __device__ __forceinline__ void row(int r, uint32_t k, uint32_t hi) {
        // read once, in front of the loops: read inside them, every trip's LDS reads wait for a kernel-argument load (profiles/walk2d_ab.txt)
        const float h2 = C.h2, cg = C.cg;
        for (; k + 2u <= hi; k += 2u) {          // two candidates per trip: independent LDS reads, adds in index order
            const float2 q0 = s_q[r][k], q1 = s_q[r][k + 1u]; const float w0 = s_w[r][k], w1 = s_w[r][k + 1u];
            const DfAcc<D> a0 = staged_a(r, k), a1 = staged_a(r, k + 1u);
            df_term<D>(h2, cg, me, mine, q0, w0, a0, acc);
            df_term<D>(h2, cg, me, mine, q1, w1, a1, acc);
        }
        if (k < hi) df_term<D>(h2, cg, me, mine, s_q[r][k], s_w[r][k], staged_a(r, k), acc);
    }
    __device__ __forceinline__ void one(uint32_t k) { const DfCandidate<D> c = fetch(k); df_term<D>(C.h2, C.cg, me, mine, c.q, walk_weight_of<MASS1>(P, c.d), c.a, acc); }
};

template <int D, bool MASS1>
__global__ __launch_bounds__(FS_BLOCK) void k_diffuse(StepParams P, DiffuseConsts C, const float2* __restrict__ pred,
                                                      const float2* __restrict__ rho2, const float* __restrict__ rho_arr,
                                                      const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                                      const u64* __restrict__ pairs, const float* __restrict__ attr_in,
                                                      float* __restrict__ attr_out, uint32_t stride, const float2* __restrict__ st_in,
                                                      float2* __restrict__ fb_out) {
    __shared__ float2 s_q[3][NB_TILE];
    __shared__ float s_w[3][NB_TILE];
    __shared__ float s_a[D][3][NB_TILE];
    __shared__ uint32_t s_red[24];
    uint32_t blk;
    if (!xcd_block(P, (P.n + FS_BLOCK - 1) / FS_BLOCK, &blk)) return;   // uniform
    WalkLane L = walk_lane_particle(blk, P.n, pred);
    const float* rows[D];
    DfAcc<D> mine, acc;
#pragma unroll
    for (int c = 0; c < D; ++c) {       // the particle's own channel values: in flight with its position
        rows[c] = attr_in + (size_t)C.ch[c] * stride;
        mine.v[c] = rows[c][L.ii];
        acc.v[c] = 0.0f;
    }
    walk_lane_rows(P, cs, start_ref, pairs, L);
    DiffuseTerms<D, MASS1> T{P, C, pred, rho2, rho_arr, s_q, s_w, s_a, L.me, rows, mine, acc};
    uint32_t blo[3], bhi[3];
    const bool fit = walk_bounds<true>(P, blk, L.R, s_red, blo, bhi, NB_TILE);
    walk_rows<0>(L.R, blo, bhi, fit, T);
    if (!L.live) return;
    const uint32_t i = L.i;
    const float rho_i = rho_arr ? rho_arr[i] : rho2[i].x;
    const float u = __fdiv_rn(1.0f, rho_i);
#pragma unroll
    for (int c = 0; c < D; ++c) attr_out[(size_t)C.ch[c] * stride + i] = mine.v[c] + (C.g[c] * acc.v[c]) * u;
    if (C.buoy >= 0)            // uniform
        fb_out[i] = buoyancy_force(C, attr_in[(size_t)C.buoy * stride + i], rho_i, st_in, i);
}

__global__ __launch_bounds__(FS_BLOCK) void k_buoyancy(uint32_t n, DiffuseConsts C, const float2* __restrict__ rho2,
                                                       const float* __restrict__ rho_arr, const float* __restrict__ attr_in,
                                                       uint32_t stride, const float2* __restrict__ st_in, float2* __restrict__ fb_out) {
    const uint32_t i = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float rho_i = rho_arr ? rho_arr[i] : rho2[i].x;
    fb_out[i] = buoyancy_force(C, attr_in[(size_t)C.buoy * stride + i], rho_i, st_in, i);
}

namespace {
template <int D>
void launch_diffuse_d(hipStream_t st, const StepParams& P, const StepArrays& A, const DiffuseConsts& C, const float* attr_in, float* attr_out,
                      uint32_t stride, const float2* st_in, float2* fb_out) {
    const uint32_t grid = xcd_grid(nblk(P.n), P.xcd_chunk_log2);
    if (P.mass == 1.0f && !A.rho)
        hipLaunchKernelGGL((k_diffuse<D, true>), dim3(grid), dim3(FS_BLOCK), 0, st, P, C, A.pred, A.rho2, A.rho, A.cs, A.start_ref, A.pairs,
                           attr_in, attr_out, stride, st_in, fb_out);
    else
        hipLaunchKernelGGL((k_diffuse<D, false>), dim3(grid), dim3(FS_BLOCK), 0, st, P, C, A.pred, A.rho2, A.rho, A.cs, A.start_ref, A.pairs,
                           attr_in, attr_out, stride, st_in, fb_out);
}

// channels [first, first + d) of the plan as one launch; with_buoyancy: this launch's tail also writes fb
void launch_diffuse_part(hipStream_t st, const StepParams& P, const StepArrays& A, const DiffusePlan& D, int first, int d, bool with_buoyancy,
                         float cg, const float* attr_in, float* attr_out, uint32_t stride, const float2* st_in, float2* fb_out) {
    DiffuseConsts C{};
    C.h2 = P.sqr_radius;
    C.cg = cg;
    for (int k = 0; k < d; ++k) { C.ch[k] = (uint32_t)D.channel[first + k]; C.g[k] = D.g[first + k]; }
    C.buoy = with_buoyancy ? D.buoyancy_channel : -1;
    C.beta = D.beta; C.a0 = D.reference; C.gx = D.gravity_x; C.gy = D.gravity_y;
    switch (d) {
        case 1: launch_diffuse_d<1>(st, P, A, C, attr_in, attr_out, stride, st_in, fb_out); break;
        case 2: launch_diffuse_d<2>(st, P, A, C, attr_in, attr_out, stride, st_in, fb_out); break;
        case 3: launch_diffuse_d<3>(st, P, A, C, attr_in, attr_out, stride, st_in, fb_out); break;
        default: launch_diffuse_d<4>(st, P, A, C, attr_in, attr_out, stride, st_in, fb_out); break;
    }
}
}  // namespace

void launch_diffuse(hipStream_t st, const StepParams& P, const StepArrays& A, const DiffusePlan& D, float cg, const float* attr_in,
                    float* attr_out, uint32_t stride, const float2* st_in, float2* fb_out) {
    if (P.n == 0) return;
    // Four diffusing channels go as two launches of two (channels are independent under Jacobi semantics: the same bits; measured
    // 0.021 ms per step faster at 16 M than one launch of four).  A/B: FS_DIFFUSE_SPLIT=0 is the one launch.
    static const bool split4 = [] { const char* e = getenv("FS_DIFFUSE_SPLIT"); return e ? atoi(e) != 0 : true; }();
    const bool buoy = D.buoyancy_channel >= 0;
    if (D.count == 0) {
        if (!buoy) return;
        DiffuseConsts C{};
        C.buoy = D.buoyancy_channel;
        C.beta = D.beta; C.a0 = D.reference; C.gx = D.gravity_x; C.gy = D.gravity_y;
        hipLaunchKernelGGL(k_buoyancy, dim3(nblk(P.n)), dim3(FS_BLOCK), 0, st, P.n, C, A.rho2, A.rho, attr_in, stride, st_in, fb_out);
        return;
    }
    if (D.count == 4 && split4) {
        launch_diffuse_part(st, P, A, D, 0, 2, buoy, cg, attr_in, attr_out, stride, st_in, fb_out);
        launch_diffuse_part(st, P, A, D, 2, 2, false, cg, attr_in, attr_out, stride, st_in, fb_out);
        return;
    }
    launch_diffuse_part(st, P, A, D, 0, D.count, buoy, cg, attr_in, attr_out, stride, st_in, fb_out);
}

}  // namespace fsd

// kernels_density.hip — the density pass and what walks the same neighbour rows right after it.
//   k_density         = calculate_density (compute.wgsl:59-74, funcs.wgsl:157-203)
//   k_surface_tension = the opt-in colour-field force, between the density and the force pass
// Both are their terms (DensityTerms, TensionTerms) plus the walk of fs_neighbours.h: walk_lane, walk_bounds, walk_rows.
#include <stdlib.h>

#include "fs_force_lists.h"
#include "fs_kernels.h"
#include "fs_neighbours.h"

namespace fsd {

static_assert(FS_BLOCK == 256, "fs_force_lists.h lays the lists out for blocks of 256 particles");

// -------------------------------------------------------------------- density
__device__ __forceinline__ float density_cube_tol(float h2, float2 me, float2 q, float acc) {
    const float dx = q.x - me.x, dy = q.y - me.y;
    const float t = fmaxf(h2 - __builtin_fmaf(dx, dx, dy * dy), 0.0f);      // NaN candidate: contributes nothing
    return __builtin_fmaf(t * t, t, acc);
}

// MASS1: the tick's particle_mass is exactly 1.0f (the reference's default, src/renderer.rs:374-388): `mass * kern` IS kern then
// (x * 1.0f == x for every f32), and the multiplication — one of the ~14 instructions per candidate — is left out.
template <bool MASS1 = false>
__device__ __forceinline__ float density_term(const StepParams& P, float h2, float2 me, float2 q) {
    const float dx = q.x - me.x, dy = q.y - me.y;
    const float r2 = dx * dx + dy * dy;
    float kern = 0.0f;
    if (!(r2 > h2)) {
        const float diff = h2 - r2;
        kern = P.poly6_norm * diff * diff * diff;       // funcs.wgsl:77
    }
    return MASS1 ? kern : P.mass * kern * 1.0f;         // funcs.wgsl:192
}

// The density terms as walk_rows takes them (fs_neighbours.h).  A staged candidate is its position.
template <bool TOL, bool MASS1> struct DensityTerms {
    const StepParams& P;
    const float2* __restrict__ pred;
    float2 (*s_pred)[NB_TILE];
    float h2, rho; float2 me;
    __device__ __forceinline__ float2 fetch(uint32_t k) const { return pred[k]; }
    __device__ __forceinline__ void put(int r, uint32_t j, float2 q) { s_pred[r][j] = q; }
    __device__ __forceinline__ void add(float2 q) { rho = TOL ? density_cube_tol(h2, me, q, rho) : rho + density_term<MASS1>(P, h2, me, q); }
    // four candidates per trip (independent LDS reads and kernel evaluations give the wave ILP), adds in index order; then a scalar tail
    __device__ __forceinline__ void row(int r, uint32_t k, uint32_t hi) {
        // the trips' only bookkeeping is one LDS pointer and its compare with the end of the lane's whole fours (k <= hi: walk_rows)
        const float2* sp = s_pred[r] + k;
        const float2* const end4 = sp + ((hi - k) & ~3u);
        const float2* const end = s_pred[r] + hi;
        for (; sp != end4; sp += 4) {
            const float2 q0 = sp[0], q1 = sp[1], q2 = sp[2], q3 = sp[3];
            if (TOL) { add(q0); add(q1); add(q2); add(q3); continue; }
            const float t0 = density_term<MASS1>(P, h2, me, q0), t1 = density_term<MASS1>(P, h2, me, q1);
            const float t2 = density_term<MASS1>(P, h2, me, q2), t3 = density_term<MASS1>(P, h2, me, q3);
            rho += t0; rho += t1; rho += t2; rho += t3;
        }
        for (; sp != end; ++sp) add(*sp);
    }
    __device__ __forceinline__ void one(uint32_t k) { add(pred[k]); }
};

// TOL (fs_options.math_mode = FS_MATH_TOLERANCE): r2 by one fma, max(h2 - r2, 0) instead of the compare/select, the
// constant factor mass * 4/(pi h^8) applied once to the sum; stores {pressure_i, 1/rho_i} for the merged force terms.
template <bool TOL, bool MASS1>
__device__ __forceinline__ void density_block(const StepParams& P, uint32_t blk, uint32_t n, const float2* __restrict__ pred,
                                              const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                              const u64* __restrict__ pairs, const unsigned long long* __restrict__ safe,
                                              float* __restrict__ rho_out, float2* __restrict__ rho2_out,
                                              uint32_t* __restrict__ force_defer, uint32_t* __restrict__ force_work,
                                              uint32_t* __restrict__ force_count, float2 (*s_pred)[NB_TILE], uint32_t* s_red) {
    const WalkLane L = walk_lane(P, blk, n, pred, cs, start_ref, pairs);
    const RowRanges& R = L.R;
    uint32_t blo[3], bhi[3];
    const bool fit = walk_bounds<false>(P, blk, R, s_red, blo, bhi, NB_TILE);
    // the force pass reads these instead of reducing the same ranges again
    if (P.block_bounds && threadIdx.x == 0) store_block_bounds(P, blk, blo, bhi);
    {   // The force pass sweeps the same row ranges: a wave it could not finish on its lean path — a row longer than
        // 32 candidates, or a block whose rows do not fit ITS LDS stage — is named here already, so that the general
        // workgroups of the force launch can start on it at once, beside the lean ones (k_force).
        const bool unfit = bhi[0] - blo[0] > NBF_TILE || bhi[1] - blo[1] > NBF_TILE || bhi[2] - blo[2] > NBF_TILE;
        const bool long_row = R.hi[0] - R.lo[0] > 32u || R.hi[1] - R.lo[1] > 32u || R.hi[2] - R.lo[2] > 32u;
        if ((unfit || __any(long_row)) && __builtin_amdgcn_ballot_w64(L.live) != 0 && (threadIdx.x & 63u) == 0u) {
            force_list_push(force_defer, force_work, force_count, P.n, blk, threadIdx.x >> 6, FS_LIST_PRE);
        }
    }
    DensityTerms<TOL, MASS1> T{P, pred, s_pred, P.h * P.h /* funcs.wgsl:73 */, 0.0f, L.me};
    walk_rows<FS_PRIO_DENSITY>(R, blo, bhi, fit, T);    // lowers the priority k_density raised (k_density_edge never did)
    if (!L.live) return;
    const uint32_t i = L.i;
    float rho = T.rho;
    if (TOL) {
        rho = rho * (P.mass * P.poly6_norm);                    // sum of (h2 - r2)^3 -> density
        rho = fmaxf(fmaxf(rho, 1.19209290e-07f), 0.1f);
        rho_out[i] = rho;
        rho2_out[i] = make_float2(P.pressure_k * (rho - P.rest_density),
                                  (P.share_div && rho <= FS_RCP_HI) ? rcp_rn_fast(rho) : __fdiv_rn(1.0f, rho));   // same bits (proven range)
        return;
    }
    rho = fmaxf(rho, 1.19209290e-07f);                          // funcs.wgsl:202
    rho = fmaxf(rho, 0.1f);                                     // compute.wgsl:70
    if (rho_out) rho_out[i] = rho;                              // uniform; single-domain handles read it back from rho2.x
    // {rho, +-RN(1/rho)}: the force pass divides by neighbours' densities; the sign carries the particle's
    // "safe operand" classification (fs_device.h) — negative sends every pair it takes part in to true divisions
    const float press = P.pressure_k * (rho - P.rest_density);  // the expression the force pass evaluates
    const bool ok = ((safe[i >> 6] >> (i & 63u)) & 1ull) != 0ull && rho <= FS_RCP_HI && fabsf(press) <= FS_PRESSURE_HI;
    // rho >= 0.1; the lean reciprocal is proven correctly rounded on [2^-20, 2^20] (share_div implies that proof)
    const float y = (P.share_div && rho <= FS_RCP_HI) ? rcp_rn_fast(rho) : __fdiv_rn(1.0f, rho);
    rho2_out[i] = make_float2(rho, ok ? y : -y);
}

#define FS_DENSITY_ARGS                                                                                                   \
    StepParams P, const float2* __restrict__ pred, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref, \
        const u64* __restrict__ pairs, const unsigned long long* __restrict__ safe, float* __restrict__ rho_out,         \
        float2* __restrict__ rho2_out, uint32_t* __restrict__ force_defer, uint32_t* __restrict__ force_work,            \
        uint32_t* __restrict__ force_count
template <bool TOL, bool MASS1>
__global__ __launch_bounds__(FS_BLOCK) void k_density(FS_DENSITY_ARGS) {
    __shared__ float2 s_pred[3][NB_TILE];
    __shared__ uint32_t s_red[24];
    const uint32_t n = P.n_live ? *P.n_live : P.n;
    uint32_t blk;
    if (!xcd_block(P, (n + FS_BLOCK - 1) / FS_BLOCK, &blk)) return;   // uniform: no live particle in this block
    wave_prio_raise<FS_PRIO_DENSITY>();          // for the prologue's round trips; density_block lowers it in front of its sweep
    density_block<TOL, MASS1>(P, blk, n, pred, cs, start_ref, pairs, safe, rho_out, rho2_out, force_defer, force_work, force_count, s_pred, s_red);
}
// Edge-first slab step, column-major ids (fs_device.h EdgeBlocks): the density of the columns the edge columns' force launch
// reads — the edge columns and one more towards the interior — ahead of the full launch, on the exchange stream.  (The full
// launch writes the same values again.)
template <bool TOL, bool MASS1>
__global__ __launch_bounds__(FS_BLOCK) void k_density_edge(FS_DENSITY_ARGS) {
    __shared__ float2 s_pred[3][NB_TILE];
    __shared__ uint32_t s_red[24];
    const uint32_t n = *P.n_live;
    const EdgeBlocks E = edge_blocks(P, cs, n, 1u);
    for (uint32_t t = blockIdx.x; t < edge_block_count(E); t += gridDim.x) {
        density_block<TOL, MASS1>(P, edge_block_at(E, t), n, pred, cs, start_ref, pairs, safe, rho_out, rho2_out, force_defer, force_work,
                           force_count, s_pred, s_red);
        __syncthreads();                             // the LDS stage is reused
    }
}

// ---------------------------------------------------------- surface tension (build extension, NOT in the reference)
// Continuum surface force (Mueller, Charypar & Gross 2003, §4.4) with the density pass's 2D poly6 kernel
// W = 4/(pi h^8) (h^2 - r^2)^3, normative statement in DESIGN.md §11.  Per sorted slot i, over the candidates the density pass
// visits (same rows, same order, the particle itself and the stale-start quirk included), all f32 without contraction:
//   o = q_j - q_i, r2 = o.o;  skip if r2 > h2;  d = h2 - r2;  w = m / rho_j
//   n += w * (((Cg d) d) o)                      Cg = 24/(pi h^8): n = sum m/rho_j grad W(q_i - q_j)
//   L += w * ((Cl d) (3 r2 - h2))                Cl = 48/(pi h^8): the 2D Laplacian -48/(pi h^8)(h^2-r^2)(h^2-3r^2)
// then |n| = sqrt(n.n) (IEEE) and st = |n| > tau && |n| > 0 ? ((-sigma L) / |n|) n : 0.  The reference's own
// calculate_surface_tension (compute.wgsl:303-498) is dead code and its gradient vanishes identically.
// w_j is formed once per staged candidate (with MASS1 it is the density pass's |rho2.y| = RN(1/rho_j)), next to q_j in LDS.
// One pass after k_density, before the force pass; it reads rho2 / rho and the cell tables and writes st[] only.
struct StConsts { float h2, cg, cl, sigma, tau; };

__device__ __forceinline__ void st_term(const StConsts& C, float2 me, float2 q, float w, float& nx, float& ny, float& L) {
    const float ox = q.x - me.x, oy = q.y - me.y;
    const float r2 = ox * ox + oy * oy;
    const bool in = !(r2 > C.h2);                   // a NaN candidate is not skipped (the statement's test, as written)
    const float d = C.h2 - r2;
    const float k = (C.cg * d) * d;
    const float lk = (C.cl * d) * ((3.0f * r2) - C.h2);
    // an accumulator that starts at +0.0f is never -0.0f, so adding +0.0f for a skipped candidate IS skipping it
    nx += in ? w * (k * ox) : 0.0f;
    ny += in ? w * (k * oy) : 0.0f;
    L += in ? w * lk : 0.0f;
}

struct StCandidate { float2 q; float d; };          // what k_surface_tension stages of a candidate: position, weight operand
// The tension terms as walk_rows takes them (fs_neighbours.h).
template <bool MASS1> struct TensionTerms {
    const StepParams& P; const StConsts& C;
    const float2 *__restrict__ pred, *__restrict__ rho2;
    const float* __restrict__ rho_arr;
    float2 (*s_q)[NB_TILE]; float (*s_w)[NB_TILE];
    float2 me; float nx, ny, L;
    __device__ __forceinline__ StCandidate fetch(uint32_t k) const { return StCandidate{pred[k], walk_weight_operand<MASS1>(rho2, rho_arr, k)}; }
    __device__ __forceinline__ void put(int r, uint32_t j, const StCandidate& c) { s_q[r][j] = c.q; s_w[r][j] = walk_weight_of<MASS1>(P, c.d); }
    __device__ __forceinline__ void row(int r, uint32_t k, uint32_t hi) {
        for (; k + 2u <= hi; k += 2u) {          // two candidates per trip: independent LDS reads, adds in index order
            const float2 q0 = s_q[r][k], q1 = s_q[r][k + 1u]; const float w0 = s_w[r][k], w1 = s_w[r][k + 1u];
            st_term(C, me, q0, w0, nx, ny, L);
            st_term(C, me, q1, w1, nx, ny, L);
        }
        if (k < hi) st_term(C, me, s_q[r][k], s_w[r][k], nx, ny, L);
    }
    __device__ __forceinline__ void one(uint32_t k) { const StCandidate c = fetch(k); st_term(C, me, c.q, walk_weight_of<MASS1>(P, c.d), nx, ny, L); }
};

template <bool MASS1>
__global__ __launch_bounds__(FS_BLOCK) void k_surface_tension(StepParams P, StConsts C, const float2* __restrict__ pred,
                                                              const float2* __restrict__ rho2, const float* __restrict__ rho_arr,
                                                              const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                                              const u64* __restrict__ pairs, float2* __restrict__ st_out) {
    __shared__ float2 s_q[3][NB_TILE];
    __shared__ float s_w[3][NB_TILE];
    __shared__ uint32_t s_red[24];
    uint32_t blk;
    if (!xcd_block(P, (P.n + FS_BLOCK - 1) / FS_BLOCK, &blk)) return;   // uniform
    const WalkLane L = walk_lane(P, blk, P.n, pred, cs, start_ref, pairs);
    uint32_t blo[3], bhi[3];
    const bool fit = walk_bounds<true>(P, blk, L.R, s_red, blo, bhi, NB_TILE);
    TensionTerms<MASS1> T{P, C, pred, rho2, rho_arr, s_q, s_w, L.me, 0.0f, 0.0f, 0.0f};
    walk_rows<0>(L.R, blo, bhi, fit, T);
    if (!L.live) return;
    const float nx = T.nx, ny = T.ny;
    const float nl = sqrt_rn(nx * nx + ny * ny);
    float2 f = make_float2(0.0f, 0.0f);
    if (nl > C.tau && nl > 0.0f) {
        const float sc = __fdiv_rn(-C.sigma * T.L, nl);
        f = make_float2(sc * nx, sc * ny);
    }
    st_out[L.i] = f;
}

void launch_density(hipStream_t st, const StepParams& P, const StepArrays& A, uint32_t edge_grid) {
    static const bool no_mass1 = getenv("FS_NO_MASS1") != nullptr;          // A/B: always the general form
    const bool tol = P.fast_math == 2, mass1 = P.mass == 1.0f && !tol && !no_mass1;     // (the tolerance form applies the constant factor once anyway)
#define FS_LAUNCH_DENSITY(K, G)                                                                                        \
    do {                                                                                                               \
        if (tol) hipLaunchKernelGGL((K<true, false>), dim3(G), dim3(FS_BLOCK), 0, st, P, A.pred, A.cs, A.start_ref, A.pairs, A.safe, A.rho, A.rho2, A.fdefer, A.fwork, A.fcount); \
        else if (mass1) hipLaunchKernelGGL((K<false, true>), dim3(G), dim3(FS_BLOCK), 0, st, P, A.pred, A.cs, A.start_ref, A.pairs, A.safe, A.rho, A.rho2, A.fdefer, A.fwork, A.fcount); \
        else hipLaunchKernelGGL((K<false, false>), dim3(G), dim3(FS_BLOCK), 0, st, P, A.pred, A.cs, A.start_ref, A.pairs, A.safe, A.rho, A.rho2, A.fdefer, A.fwork, A.fcount); \
    } while (0)
    if (edge_grid) {   // edge-first slab step: the edge columns' blocks only (k_density_edge)
        FS_LAUNCH_DENSITY(k_density_edge, edge_grid);
        return;
    }
    const uint32_t nb = nblk(P.n), grid = xcd_grid(nb, P.xcd_chunk_log2);
    FS_LAUNCH_DENSITY(k_density, grid);
#undef FS_LAUNCH_DENSITY
}

void launch_surface_tension(hipStream_t st, const StepParams& P, const StepArrays& A, float sigma, float tau, float cg, float2* st_out) {
    if (P.n == 0) return;
    StConsts C;
    C.h2 = P.sqr_radius;
    C.cg = cg;
    C.cl = 2.0f * cg;                                 // 48/(pi h^8): x2 is exact
    C.sigma = sigma;
    C.tau = tau;
    const uint32_t grid = xcd_grid(nblk(P.n), P.xcd_chunk_log2);
    if (P.mass == 1.0f && !A.rho)
        hipLaunchKernelGGL(k_surface_tension<true>, dim3(grid), dim3(FS_BLOCK), 0, st, P, C, A.pred, A.rho2, A.rho, A.cs, A.start_ref, A.pairs, st_out);
    else
        hipLaunchKernelGGL(k_surface_tension<false>, dim3(grid), dim3(FS_BLOCK), 0, st, P, C, A.pred, A.rho2, A.rho, A.cs, A.start_ref, A.pairs, st_out);
}

}  // namespace fsd

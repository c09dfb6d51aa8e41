// kernels_density.hip — the density pass and what walks the same neighbour rows right after it.
//   k_density         = calculate_density (compute.wgsl:59-74, funcs.wgsl:157-203)
//   k_surface_tension = the opt-in colour-field force, between the density and the force pass
//   k_render_density  = the density-splat image (fluid_shader.wgsl:27-102)
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

// TOL (fs_options.math_mode = FS_MATH_TOLERANCE): r2 by one fma, max(h2 - r2, 0) instead of the compare/select, the
// constant factor mass * 4/(pi h^8) applied once to the sum; stores {pressure_i, 1/rho_i} for the merged force terms.
template <bool TOL, bool MASS1>
__device__ __forceinline__ void density_block(const StepParams& P, uint32_t blk, uint32_t n, const float2* __restrict__ pred,
                                              const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                              const u64* __restrict__ pairs, const unsigned long long* __restrict__ safe,
                                              float* __restrict__ rho_out, float2* __restrict__ rho2_out,
                                              uint32_t* __restrict__ force_defer, uint32_t* __restrict__ force_work,
                                              uint32_t* __restrict__ force_count, float2 (*s_pred)[NB_TILE], uint32_t* s_red) {
    const uint32_t i = blk * FS_BLOCK + threadIdx.x;
    const bool live = i < n;
    const float2 me = pred[live ? i : n - 1];      // issued first: the quirk's two dependent scalar loads run beside it
    const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    uint32_t cx, cy;                // (u, v) of the cell-id layout: (x, y) unless the handle is a transposed slab rank
    int32_t cg;
    uv_local(P, me, &cx, &cy, &cg);
    const float h2 = P.h * P.h;     // funcs.wgsl:73
    const RowRanges R = lane_row_ranges(P, cs, lo_fix, cx, cy, live);
    uint32_t blo[3], bhi[3];
    const bool fit = block_tile_bounds(R, s_red, blo, bhi, NB_TILE);
    // the force pass reads these instead of reducing the same ranges again
    if (P.block_bounds && threadIdx.x == 0) store_block_bounds(P, blk, blo, bhi);
    {   // The force pass sweeps the same row ranges: a wave it could not finish on its lean path — a row longer than
        // 32 candidates, or a block whose rows do not fit ITS LDS stage — is named here already, so that the general
        // workgroups of the force launch can start on it at once, beside the lean ones (k_force).
        const bool unfit = bhi[0] - blo[0] > NBF_TILE || bhi[1] - blo[1] > NBF_TILE || bhi[2] - blo[2] > NBF_TILE;
        const bool long_row = R.hi[0] - R.lo[0] > 32u || R.hi[1] - R.lo[1] > 32u || R.hi[2] - R.lo[2] > 32u;
        if ((unfit || __any(long_row)) && __builtin_amdgcn_ballot_w64(live) != 0 && (threadIdx.x & 63u) == 0u) {
            force_list_push(force_defer, force_work, force_count, P.n, blk, threadIdx.x >> 6, FS_LIST_PRE);
        }
    }
    float rho = 0.0f;
    if (fit) {
        StagedRows<float2> S;       // all loads of the three rows, then the LDS writes (fs_neighbours.h)
        stage_rows_load(S, blo, bhi, [&](uint32_t k) { return pred[k]; });
        stage_rows_store(S, blo, bhi, [&](int r, uint32_t j, float2 q) { s_pred[r][j] = q; });
        __syncthreads();
        wave_prio_lower<FS_PRIO_DENSITY>();     // the load phase is over (k_density raised it; k_density_edge never did)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            // four candidates per trip (independent LDS reads and kernel evaluations give the wave
            // ILP), adds in index order; then a scalar tail
            const float2* sp = s_pred[r] - 0;
            const bool any = R.lo[r] < R.hi[r];
            const uint32_t hi = any ? R.hi[r] - blo[r] : 0u;
            uint32_t k = any ? R.lo[r] - blo[r] : 0u;
            if (TOL) {
                for (; k + 4u <= hi; k += 4u) {
                    const float2 q0 = sp[k], q1 = sp[k + 1u], q2 = sp[k + 2u], q3 = sp[k + 3u];
                    rho = density_cube_tol(h2, me, q0, rho); rho = density_cube_tol(h2, me, q1, rho);
                    rho = density_cube_tol(h2, me, q2, rho); rho = density_cube_tol(h2, me, q3, rho);
                }
                for (; k < hi; ++k) rho = density_cube_tol(h2, me, sp[k], rho);
                continue;
            }
            for (; k + 4u <= hi; k += 4u) {
                const float t0 = density_term<MASS1>(P, h2, me, sp[k]);
                const float t1 = density_term<MASS1>(P, h2, me, sp[k + 1u]);
                const float t2 = density_term<MASS1>(P, h2, me, sp[k + 2u]);
                const float t3 = density_term<MASS1>(P, h2, me, sp[k + 3u]);
                rho += t0; rho += t1; rho += t2; rho += t3;
            }
            for (; k < hi; ++k) rho += density_term<MASS1>(P, h2, me, sp[k]);
        }
    } else {
        wave_prio_lower<FS_PRIO_DENSITY>();
#pragma unroll
        for (int r = 0; r < 3; ++r)
            for (uint32_t k = R.lo[r]; k < R.hi[r]; ++k) {
                if (TOL) rho = density_cube_tol(h2, me, pred[k], rho);
                else rho += density_term<MASS1>(P, h2, me, pred[k]);
            }
    }
    if (!live) return;
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

// The weight in two halves, so that the staging can load every candidate's operand before it forms the first weight:
// st_weight_operand is the one word read per candidate, st_weight_of the weight from it.
template <bool MASS1>
__device__ __forceinline__ float st_weight_operand(const float2* __restrict__ rho2, const float* __restrict__ rho_arr, uint32_t j) {
    if (MASS1) return rho2[j].y;                    // +-RN(1/rho_j): the sign is the density pass's safe bit
    return rho_arr ? rho_arr[j] : rho2[j].x;        // rho_j.  rho_arr: tolerance mode (rho2 = {pressure, 1/rho})
}
template <bool MASS1>
__device__ __forceinline__ float st_weight_of(const StepParams& P, float d) {
    if (MASS1) return fabsf(d);                     // RN(1/rho_j) == RN(1.0f / rho_j)
    return __fdiv_rn(P.mass, d);
}
template <bool MASS1>
__device__ __forceinline__ float st_weight(const StepParams& P, const float2* __restrict__ rho2, const float* __restrict__ rho_arr,
                                           uint32_t j) {
    return st_weight_of<MASS1>(P, st_weight_operand<MASS1>(rho2, rho_arr, j));
}
struct StCandidate { float2 q; float d; };          // what k_surface_tension stages of a candidate: position, weight operand

template <bool MASS1>
__global__ __launch_bounds__(FS_BLOCK) void k_surface_tension(StepParams P, StConsts C, const float2* __restrict__ pred,
                                                              const float2* __restrict__ rho2, const float* __restrict__ rho_arr,
                                                              const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                                              const u64* __restrict__ pairs, float2* __restrict__ st_out) {
    __shared__ float2 s_q[3][NB_TILE];
    __shared__ float s_w[3][NB_TILE];
    __shared__ uint32_t s_red[24];
    const uint32_t n = P.n;
    uint32_t blk;
    if (!xcd_block(P, (n + FS_BLOCK - 1) / FS_BLOCK, &blk)) return;   // uniform
    const uint32_t i = blk * FS_BLOCK + threadIdx.x;
    const bool live = i < n;
    const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    const float2 me = pred[live ? i : n - 1];
    uint32_t cx, cy;
    int32_t cg;
    uv_local(P, me, &cx, &cy, &cg);
    const RowRanges R = lane_row_ranges(P, cs, lo_fix, cx, cy, live);
    uint32_t blo[3], bhi[3];
    bool fit;
    if (P.block_bounds) {       // this step's density pass reduced the same ranges over the same 256 particles
        fit = recorded_tile_bounds(P, blk, blo, bhi, NB_TILE);
    } else {
        fit = block_tile_bounds(R, s_red, blo, bhi, NB_TILE);
    }
    float nx = 0.0f, ny = 0.0f, L = 0.0f;
    if (fit) {
        StagedRows<StCandidate> S;  // all loads of the three rows, then the weights and the LDS writes (fs_neighbours.h)
        stage_rows_load(S, blo, bhi, [&](uint32_t k) { return StCandidate{pred[k], st_weight_operand<MASS1>(rho2, rho_arr, k)}; });
        stage_rows_store(S, blo, bhi, [&](int r, uint32_t j, const StCandidate& c) {
            s_q[r][j] = c.q;
            s_w[r][j] = st_weight_of<MASS1>(P, c.d);
        });
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const bool any = R.lo[r] < R.hi[r];
            const uint32_t hi = any ? R.hi[r] - blo[r] : 0u;
            uint32_t k = any ? R.lo[r] - blo[r] : 0u;
            for (; k + 2u <= hi; k += 2u) {          // two candidates per trip: independent LDS reads, adds in index order
                const float2 q0 = s_q[r][k], q1 = s_q[r][k + 1u];
                const float w0 = s_w[r][k], w1 = s_w[r][k + 1u];
                st_term(C, me, q0, w0, nx, ny, L);
                st_term(C, me, q1, w1, nx, ny, L);
            }
            if (k < hi) st_term(C, me, s_q[r][k], s_w[r][k], nx, ny, L);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            for (uint32_t k = R.lo[r]; k < R.hi[r]; ++k) st_term(C, me, pred[k], st_weight<MASS1>(P, rho2, rho_arr, k), nx, ny, L);
    }
    if (!live) return;
    const float nl = sqrt_rn(nx * nx + ny * ny);
    float2 f = make_float2(0.0f, 0.0f);
    if (nl > C.tau && nl > 0.0f) {
        const float sc = __fdiv_rn(-C.sigma * L, nl);
        f = make_float2(sc * nx, sc * ny);
    }
    st_out[i] = f;
}

// ------------------------------------------------------- density-splat image (fluid_shader.wgsl:27-102)
__device__ __forceinline__ float smoothstep_f(float a, float b, float x) {
    float t = __fdiv_rn(x - a, b - a);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

__global__ __launch_bounds__(FS_BLOCK) void k_render_density(StepParams P, float2 wmin, float2 wmax, uint32_t width,
                                                             uint32_t height, const float2* __restrict__ pred,
                                                             const float2* __restrict__ vel,
                                                             const uint32_t* __restrict__ cs,
                                                             const uint32_t* __restrict__ start_ref,
                                                             const u64* __restrict__ pairs, float4* __restrict__ out) {
    const uint32_t pix = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (pix >= width * height) return;
    const uint32_t i = pix % width, j = pix / width;
    float2 pt;
    pt.x = wmin.x + __fdiv_rn((float)i + 0.5f, (float)width) * (wmax.x - wmin.x);
    pt.y = wmin.y + __fdiv_rn((float)j + 0.5f, (float)height) * (wmax.y - wmin.y);
    const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    uint32_t cx, cy;
    xy_local(P, pt, &cx, &cy);         // P.div_h.ok == 0 (launch_render_density): the true division
    float density = 0.0f, vfac = 0.0f;
    const float denom = P.sqr_radius / 2.0f;                            // fluid_shader.wgsl:66
    // not row_range (fs_neighbours.h), on purpose: five columns clamped to the grid, reference-layout ids; the stale-start rule is shared.
    // The columns cx - 2 .. cx + 2 that lie in the grid (X = (u32)(cx + ox) < grid_w), in unsigned arithmetic throughout: whatever
    // (cx, cy) a coordinate gives, xlo < xhi <= grid_w and y < grid_h, so every cs[] index is <= ncell.
    const uint32_t xlo = cx < 2u ? 0u : cx - 2u;
    const bool no_column = xlo >= P.grid_w;                             // (so cx < grid_w + 2: cx + 3 below does not wrap)
    const uint32_t xhi = no_column ? xlo : (cx + 3u < P.grid_w ? cx + 3u : P.grid_w);
    for (int oy = -2; oy < 3; ++oy) {                                   // :39-40 (5x5 cells)
        const uint32_t y = cy + (uint32_t)oy;
        if (y >= P.grid_h || no_column) continue;
        uint32_t a = cs[y * P.grid_w + xlo];
        const uint32_t b = cs[y * P.grid_w + xhi];
        if (a == 0u) a = lo_fix;
        for (uint32_t k = a; k < b; ++k) {
            const float2 q = pred[k];
            const float2 v = vel[k];
            const float ox = q.x - pt.x, oyv = q.y - pt.y;
            const float r2 = ox * ox + oyv * oyv;
            const float contrib = expf(__fdiv_rn(-r2, denom));
            density += contrib;
            vfac += contrib * sqrt_rn(v.x * v.x + v.y * v.y);           // :68
        }
    }
    vfac = vfac * 0.01f;                                                // :79-83
    vfac = __fdiv_rn(logf(1.0f + 5.0f * vfac), logf(1.0f + 5.0f));
    vfac = fminf(fmaxf(vfac, 0.0f), 1.0f);
    const float interior = smoothstep_f(0.5f, 1.5f, density);           // :86
    float edge = smoothstep_f(0.7f, 1.0f, density) - smoothstep_f(1.0f, 1.5f, density);
    edge = edge * (1.0f + vfac * 2.0f);                                 // :89-90
    const float br = (0.0f * (1.0f - vfac) + 1.0f * vfac) * interior;   // mix(blue, red, vfac) * interior, :93
    const float bg = (0.5f * (1.0f - vfac) + 0.0f * vfac) * interior;
    const float bb = (1.0f * (1.0f - vfac) + 0.0f * vfac) * interior;
    out[pix] = make_float4(br + edge, bg + edge, bb + edge, fminf(fmaxf(interior, 0.0f), 1.0f));
}

void launch_render_density(hipStream_t st, const StepParams& P_in, float2 wmin, float2 wmax, uint32_t width,
                           uint32_t height, const float2* pred, const float2* vel, const uint32_t* cs,
                           const uint32_t* start_ref, const u64* pairs, float4* out) {
    StepParams P = P_in;
    P.div_h.ok = 0;                    // the 3-instruction quotient is proven for clamped positions only; a view may leave the domain
    const uint32_t npix = width * height;
    hipLaunchKernelGGL(k_render_density, dim3((npix + FS_BLOCK - 1) / FS_BLOCK), dim3(FS_BLOCK), 0, st, P, wmin, wmax,
                       width, height, pred, vel, cs, start_ref, pairs, out);
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

// kernels_force.hip — the force pass of the SPH step.
//   k_force         = move_particle + both force sweeps fused (compute.wgsl:79-299)
// This file: the integrator (integrate_store), one workgroup's 256 particles (force_block), the lean kernel k_force, its
// slab form k_force_edge, the general kernel k_force_general and the pass's host schedule launch_force.  What a pair costs
// is in fs_force_pair.h, the two sweeps in fs_force_sweep.h, the deferred-wave lists in fs_force_lists.h, and k_force_quad
// in kernels_force_quad.inc (compiled as part of this unit, see there).
#include <hip/hip_ext.h>

#include <type_traits>

#include "fs_force_lists.h"
#include "fs_force_sweep.h"
#include "fs_kernels.h"

namespace fsd {

static_assert(FS_BLOCK == 256, "fs_force_lists.h lays the lists out for blocks of 256 particles");

// Integration of one particle from its accumulated force sums (compute.wgsl:93-153, :298) and the stores of its new state.
// ST (compile-time, single-domain handles with fs_set_surface_tension on): the surface-tension force k_surface_tension wrote for
// this sorted slot is added to the force sum, `ax = (fp.x + fv.x) + st.x`; nothing else changes.
template <int MODE, bool AOS, bool ST = false>
__device__ __forceinline__ void integrate_store(const StepParams& P, uint32_t i, const float2 me, const float2 mv, const float2 mrec,
                                                float mrho, const float2 p_own, const ForceAcc& A, uint32_t cx, uint32_t cy,
                                                const float2* __restrict__ tex, float2* __restrict__ pos_out,
                                                float2* __restrict__ vel_out, AosParticle* __restrict__ aos_out,
                                                const float* __restrict__ rho_arr, const float2* __restrict__ st_in) {
    const float fvx = A.fvx * P.visc_coeff;                             // compute.wgsl:298
    const float fvy = A.fvy * P.visc_coeff;

    // integrate (compute.wgsl:93-153)
    float2 v = mv;
    float2 p = p_own;
    float ax = A.fpx + fvx, ay = A.fpy + fvy;
    if (ST) {
        const float2 fs = st_in[i];
        ax = ax + fs.x;
        ay = ay + fs.y;
    }
    if (MODE == 2) {
        v.x = __builtin_fmaf(ax * mrec.y, P.dt, v.x);
        v.y = __builtin_fmaf(ay * mrec.y, P.dt, v.y);
    } else {
        v.x += __fdiv_rn(ax, mrho) * P.dt;
        v.y += __fdiv_rn(ay, mrho) * P.dt;
    }
    v.x += P.gx * P.dt;
    v.y += P.gy * P.dt;
    if (P.mouse_state != 0) {
        const float dx = P.mouse_x - me.x, dy = P.mouse_y - me.y;
        const float dist = sqrt_rn(dx * dx + dy * dy);
        if (dist <= P.mouse_radius) {
            const float dirx = __fdiv_rn(__fdiv_rn(dx, dist), dist);
            const float diry = __fdiv_rn(__fdiv_rn(dy, dist), dist);
            const float ratio = __fdiv_rn(dist, P.mouse_radius);
            v.x += dirx * P.mouse_power * (float)P.mouse_state * ratio;
            v.y += diry * P.mouse_power * (float)P.mouse_state * ratio;
        }
    }
    if (!(v.x == v.x && v.y == v.y)) { v.x = 0.0f; v.y = 0.0f; }
    if (MODE == 2) {
        const float s2 = __builtin_fmaf(v.x, v.x, v.y * v.y);
        if (s2 > 250000.0f) { const float k = 500.0f * __builtin_amdgcn_rsqf(s2); v.x *= k; v.y *= k; }
    } else {
        // compute.wgsl:118-122.  The square root (an IEEE sequence of ~15 instructions) is only needed near the clamp:
        // for s2 <= 249 000 it is at most 498.999 < 500 whatever the rounding, so nothing can change; NaN was reset
        // above and an infinite s2 takes the branch.
        const float s2 = v.x * v.x + v.y * v.y;
        if (s2 > 249000.0f) {
            const float speed = sqrt_rn(s2);
            if (speed > 500.0f) {
                v.x = __fdiv_rn(v.x, speed) * 500.0f;
                v.y = __fdiv_rn(v.y, speed) * 500.0f;
            }
        }
    }
    p.x += v.x * P.dt;
    p.y += v.y * P.dt;

    float2 force = make_float2(0.0f, 0.0f);
    if (!P.tex_zero) {   // uniform; an all-zero field (the default, and the benchmark's) changes nothing below
        const float uvx = (__fdiv_rn(me.x, P.bounds_x) * 1.0f) + 0.5f;      // compute.wgsl:127
        const float uvy = (__fdiv_rn(me.y, P.bounds_y) * 1.0f) + 0.5f;
        const uint32_t px = f32_to_u32_sat(uvx * P.tex_w);
        const uint32_t py = f32_to_u32_sat(uvy * P.tex_h);
        const uint32_t tix = py * P.tex_w_u + px;
        if (tix < P.tex_len) force = tex[tix];
    }
    if (force.x != 0.0f || force.y != 0.0f) {                           // compute.wgsl:131-140
        const float p2wx = __fdiv_rn(P.bounds_x * 2.0f, P.tex_w);
        const float p2wy = __fdiv_rn(P.bounds_y * 2.0f, P.tex_h);
        const float fwx = force.x * p2wx, fwy = force.y * p2wy;
        const float len = sqrt_rn(force.x * force.x + force.y * force.y);
        const float nx = __fdiv_rn(force.x, len), ny = __fdiv_rn(force.y, len);
        p.x += fwx;
        p.y += fwy;
        const float vn = v.x * nx + v.y * ny;
        v.x -= (1.0f - P.damping) * vn * nx;
        v.y -= (1.0f - P.damping) * vn * ny;
    }
    if (fabsf(p.x) > P.bs_x) { p.x = P.bs_x * sign_f32(p.x); v.x *= -1.0f * P.damping; }
    if (fabsf(p.y) > P.bs_y) { p.y = P.bs_y * sign_f32(p.y); v.y *= -1.0f * P.damping; }
    pos_out[i] = p;
    vel_out[i] = v;
    if (AOS) {       // compile-time (even unused, the store costs the plain kernel 5 %): a renderer hand-off is registered (fs_export_handle) — the 32-byte ParticleInstance the
                     // reference's fragment shader binds (src/simulation.rs:552-559) is written here, no export pass
        AosParticle a;
        a.position = p; a.predicted = me; a.velocity = v; a.density = MODE == 2 ? rho_arr[i] : mrho;
        a.grid = cy * P.grid_u + cx;      // == the sorted key: same expression as cell_of_point(pred) (single-domain handles only)
        aos_out[i] = a;
    }
}

// amdgpu_waves_per_eu(8, 8) on the lean kernels (FS_FORCE_WAVES).  Measured in round 2, when one kernel still held
// both sweeps: uncapped, the allocator took 83 VGPRs (5 waves/SIMD) and the common path lost 9 %; capped at 64 it spilled in
// the rarely taken branches instead (0.77 vs 0.86 ms in the bench window, 2.67 vs 2.82 ms in the dense regime).  Today the
// cap costs k_force nothing and k_force_edge<0> 3 - 4 spilled VGPRs (profiles/force_split_resource_usage.txt).
#ifndef FS_FORCE_WAVES
#define FS_FORCE_WAVES 8
#endif
// The load half of k_force's stage (fs_neighbours.h); the kernels that keep the staging loop hold no rows in flight.
struct NoStagedRows {};
__device__ __forceinline__ void force_stage_load(StagedRows<float2>& S, const uint32_t* blo, const uint32_t* bhi,
                                                 const float2* __restrict__ pred) {
    stage_rows_load(S, blo, bhi, [&](uint32_t k) { return pred[k]; });
}
// One workgroup's 256 particles.  GENERAL = false is the lean main path: mask sweep with the shared-reciprocal terms
// only.  A wave it cannot finish that way — its tile does not fit the LDS stage, one of its sweep rows is longer than
// 32 candidates (dense clusters), or an operand fell outside the proven quotient ranges — is handed to the general
// kernel through a device worklist (`defer_bits[blk]` bit w, the block id pushed once) and writes nothing.
// GENERAL = true is the complete body (chunked sweeps, true-division fallback) for the waves named in `wave_bits`.
// The split keeps the rare paths out of the common kernel's register allocation.  When it was made (round 2) a
// timing-only build without them needed 39 VGPRs instead of 64 + 35 spilled, force 0.72 -> 0.665 ms at 16M
// (profiles/r02_d_rejected.md).  Today: k_force 56 - 58 VGPRs by mode and AOS with its staged rows in flight, no spills
// (profiles/prologue_resource_usage.txt).
// The two lists — waves named by k_density before the launch ("pre"), waves the lean path gives up on itself ("late") —
// are laid out in fs_force_lists.h.
template <int MODE, bool AOS, bool GENERAL, bool ST, bool EARLY>
__device__ __forceinline__ void force_block(const StepParams& P, uint32_t blk, uint32_t n, uint32_t wave_bits,
                                            const float2* __restrict__ pos_s, const float2* __restrict__ vel_s,
                                            const float2* __restrict__ pred, const float2* __restrict__ rho2,
                                            const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                            const u64* __restrict__ pairs, const float2* __restrict__ tex,
                                            float2* __restrict__ pos_out, float2* __restrict__ vel_out,
                                            AosParticle* __restrict__ aos_out, const float* __restrict__ rho_arr,
                                            uint32_t* __restrict__ defer_bits, uint32_t* __restrict__ worklist,
                                            uint32_t* __restrict__ work_count, const float2* __restrict__ st_in,
                                            float2 (*s_pred)[NBF_ROW], uint32_t* s_red) {
    const uint32_t tid = threadIdx.x;
    const uint32_t i = blk * FS_BLOCK + tid;
    bool live = i < n;
    if (GENERAL) live = live && ((wave_bits >> (tid >> 6)) & 1u);   // only the waves handed over to the general path
    // lean path: a wave k_density pre-registered is being finished by a general workgroup of this same launch
    const bool pre = !GENERAL && ((wave_bits >> (tid >> 6)) & 1u);
    if (pre) live = false;
    const uint32_t ii = i < n ? i : n - 1;           // dead lanes shadow the last particle, store nothing
    // EARLY (k_force): the prologue's global loads in three round trips.  With the density pass's record of the block-wide ranges
    // (every single-domain step) nothing the lane computes decides what is staged: the staging loads go out first, the lane's own
    // record right behind them, then the source position and the six cell-table entries; the LDS writes come last.
    // k_force_edge and k_force_general have no registers for the rows in flight (profiles/prologue_resource_usage.txt): they
    // stage where they did, with the loop.
    uint32_t blo[3], bhi[3];
    bool staged = false;
    std::conditional_t<EARLY, StagedRows<float2>, NoStagedRows> S;     // the rows in flight: k_force only
    const bool ahead = EARLY && P.block_bounds != nullptr;     // uniform
    if constexpr (EARLY) {
        if (ahead) {
            staged = recorded_tile_bounds(P, blk, blo, bhi, NBF_TILE);
            if (staged) force_stage_load(S, blo, bhi, pred);
        }
    }
    const float2 me = pred[ii];
    const float2 mv = vel_s[ii];
    const float2 mrec = rho2[ii];                   // {rho, +-1/rho}; MODE 2: {pressure, 1/rho}
    // own position at the start of the step: the sorted copy, or (pos_by_src) the previous state through the pair's source index
    const float2 p_own = pos_s[P.pos_by_src ? (uint32_t)pairs[ii] : ii];
    const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    const float mrho = MODE == 2 ? 0.0f : mrec.x;
    const bool me_ok = mrec.y > 0.0f;               // this particle's "safe operand" classification (fs_device.h)
    const float pressure = MODE == 2 ? mrec.x : P.pressure_k * (mrho - P.rest_density);      // funcs.wgsl:152-154
    ForceAcc A;
    A.fpx = A.fpy = A.fvx = A.fvy = 0.0f;
    A.seed = ii * 12u + P.frame_time * 69u;                             // compute.wgsl:161
    uint32_t cx, cy;                // (u, v) of the cell-id layout: (x, y) unless the handle is a transposed slab rank
    int32_t cg;
    uv_local(P, me, &cx, &cy, &cg);
    if (P.n_live) {   // slab mode: ghosts (outside the owned columns) are not advanced, and an overlapped step splits the owned
                      // columns between two launches (fs_device.h slab_advances)
        if (!slab_advances(P, cg)) live = false;
    }
    const RowRanges R = lane_row_ranges(P, cs, lo_fix, cx, cy, live);
    if (!ahead) {
        // the density pass of this step reduced the same ranges over the same 256 particles (a slab launch that advances only
        // some columns zeroes the other lanes' ranges: the stored bounds are then a superset — more is staged, nothing is missed)
        if (P.block_bounds) staged = recorded_tile_bounds(P, blk, blo, bhi, NBF_TILE);
        else staged = block_tile_bounds(R, s_red, blo, bhi, NBF_TILE);
        if constexpr (EARLY) {
            if (staged) force_stage_load(S, blo, bhi, pred);
        }
    }
    bool defer = !staged;                            // lean path only; wave-uniform from here on
    if (staged) {
        if constexpr (EARLY) {
            stage_rows_store(S, blo, bhi, [&](int r, uint32_t j, float2 q) { s_pred[r][j] = q; });
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
                for (uint32_t j = tid; j < bhi[r] - blo[r]; j += FS_BLOCK) s_pred[r][j] = pred[blo[r] + j];
        }
        __syncthreads();
        if constexpr (EARLY) wave_prio_lower<FS_PRIO_FORCE>();      // k_force raised it for the prologue's round trips
        const bool long_row = R.hi[0] - R.lo[0] > 32u || R.hi[1] - R.lo[1] > 32u || R.hi[2] - R.lo[2] > 32u;
        if (!__any(long_row))
            defer = force_sweep_masks<MODE, GENERAL>(P, R, blo, ii, me, mv, pressure, vel_s, rho2, &s_pred[0][0], me_ok, A);
        else if (GENERAL)
            force_sweep_chunks<true, MODE>(P, R, blo, ii, me, mv, pressure, pred, vel_s, rho2, &s_pred[0][0], me_ok, A);
        else
            defer = true;
    } else if (GENERAL) {
        force_sweep_chunks<false, MODE>(P, R, blo, ii, me, mv, pressure, pred, vel_s, rho2, &s_pred[0][0], me_ok, A);
    } else if constexpr (EARLY) {
        wave_prio_lower<FS_PRIO_FORCE>();            // not staged: the lean wave defers below
    }
    defer = __any(defer);
    if (!GENERAL && defer) {                         // wave-uniform: hand this wave over (late list), write nothing
        if (__builtin_amdgcn_ballot_w64(live) != 0 && (tid & 63u) == 0u) {
            force_list_push(defer_bits, worklist, work_count, P.n, blk, tid >> 6, FS_LIST_LATE);
        }
        return;
    }
    if (!live) return;
    integrate_store<MODE, AOS, ST>(P, i, me, mv, mrec, mrho, p_own, A, cx, cy, tex, pos_out, vel_out, aos_out, rho_arr, st_in);
}

// Slab ranks with column-major cell ids (StepParams::transposed): a block's 256 consecutive sorted particles span the cell
// columns [column of its first key, column of its last key].  A launch that advances only the edge columns (or only the interior,
// fs_device.h slab_advances) leaves every block whose span misses its columns after two scalar loads.
__device__ __forceinline__ bool block_may_advance(const StepParams& P, const u64* __restrict__ pairs, uint32_t blk, uint32_t n) {
    if (!P.n_live || !P.transposed) return true;
    const uint32_t i0 = blk * FS_BLOCK;
    const uint32_t i1 = (i0 + FS_BLOCK < n ? i0 + FS_BLOCK : n) - 1u;
    const int32_t cf = (int32_t)((uint32_t)(pairs[i0] >> 32) / P.grid_u) + P.col_origin;
    const int32_t cl = (int32_t)((uint32_t)(pairs[i1] >> 32) / P.grid_u) + P.col_origin;
    if (P.adv_outside)
        return (cf < (int32_t)P.adv_lo && cl >= (int32_t)P.own_lo) || (cl >= (int32_t)P.adv_hi && cf < (int32_t)P.own_hi);
    return cl >= (int32_t)P.adv_lo && cf < (int32_t)P.adv_hi;
}

#define FS_FORCE_ARGS                                                                                                  \
    StepParams P, const float2* __restrict__ pos_s, const float2* __restrict__ vel_s, const float2* __restrict__ pred,  \
        const float2* __restrict__ rho2, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,       \
        const u64* __restrict__ pairs, const float2* __restrict__ tex, float2* __restrict__ pos_out,                   \
        float2* __restrict__ vel_out, AosParticle* __restrict__ aos_out, const float* __restrict__ rho_arr,            \
        uint32_t* __restrict__ defer_bits, uint32_t* __restrict__ worklist, uint32_t* __restrict__ work_count
// (the ST instantiations' input, the per-slot surface-tension force, is each kernel's LAST argument: the other arguments keep
// their kernarg offsets)

// Lean main kernel: every block once — mask sweep + shared reciprocals only, skipping the waves k_density
// pre-registered.  (Folding the general workgroups into this launch was tried: the kernel then carries the general
// body's spills and scratch set-up and the strict lean path ran 1.7x slower; two kernels on two streams instead.)
template <int MODE, bool AOS, bool ST>
__global__ __launch_bounds__(FS_BLOCK) __attribute__((amdgpu_waves_per_eu(FS_FORCE_WAVES, FS_FORCE_WAVES))) void k_force(FS_FORCE_ARGS, uint32_t which, const float2* __restrict__ st_in) {
    __shared__ float2 s_pred[3][NBF_ROW];
    __shared__ uint32_t s_red[24];
    const uint32_t n = P.n_live ? *P.n_live : P.n;
    uint32_t blk;
    if (!xcd_block(P, (n + FS_BLOCK - 1) / FS_BLOCK, &blk)) return;   // uniform: no live particle in this block
    if (!block_may_advance(P, pairs, blk, n)) return;                 // uniform: none of its columns belongs to this launch
    wave_prio_raise<FS_PRIO_FORCE>();            // for the prologue's round trips; force_block lowers it in front of the sweep
    force_block<MODE, AOS, false, ST, true>(P, blk, n, defer_bits[force_defer_word(blk, FS_LIST_PRE)], pos_s, vel_s, pred, rho2, cs, start_ref, pairs, tex,
                                      pos_out, vel_out, aos_out, rho_arr, defer_bits, worklist, work_count, st_in, s_pred, s_red);
}

// Edge-first slab step, column-major ids: the lean kernel over the blocks that hold the edge columns only (fs_device.h
// EdgeBlocks), a small fixed grid walking them.
template <int MODE, bool AOS, bool ST>
__global__ __launch_bounds__(FS_BLOCK) __attribute__((amdgpu_waves_per_eu(FS_FORCE_WAVES, FS_FORCE_WAVES))) void k_force_edge(FS_FORCE_ARGS, uint32_t which, const float2* __restrict__ st_in) {
    static_assert(!ST, "surface tension: single-domain handles only");
    __shared__ float2 s_pred[3][NBF_ROW];
    __shared__ uint32_t s_red[24];
    const uint32_t n = *P.n_live;
    const EdgeBlocks E = edge_blocks(P, cs, n, 0u);
    for (uint32_t t = blockIdx.x; t < edge_block_count(E); t += gridDim.x) {
        const uint32_t blk = edge_block_at(E, t);
        if (block_may_advance(P, pairs, blk, n))         // uniform (the ghost columns' blocks at the very ends)
            force_block<MODE, AOS, false, false, false>(P, blk, n, defer_bits[force_defer_word(blk, FS_LIST_PRE)], pos_s, vel_s, pred, rho2, cs, start_ref, pairs, tex,
                                                 pos_out, vel_out, aos_out, rho_arr, defer_bits, worklist, work_count, st_in, s_pred, s_red);
        __syncthreads();                                 // the LDS stage is reused
    }
}

// General kernel: a fixed grid walks one of the two worklists with the complete body.
//   which = 0: the waves k_density pre-registered (long rows / unstaged tiles: dense clusters) — launched on the
//              simulation's second stream so that it runs BESIDE the lean kernel: a general workgroup's latency (a wave
//              alone with 100+ neighbours per particle) hides under the lean work;
//   which = 1: the waves the lean kernel gave up on itself (an operand outside the proven quotient ranges) — after
//              both, on the main stream; usually empty.
// amdgpu_waves_per_eu(5, 5): 91 - 96 VGPRs and no scratch, but for 2 spilled VGPRs in the strict AOS forms
// (profiles/force_split_resource_usage.txt) — at 8 waves (64 VGPRs, 52 spilled, when measured) even an EMPTY launch
// cost ~17 us for the scratch set-up of its 1024 workgroups (bench window force 0.707 -> 0.690 ms).
#ifndef FS_GENERAL_WAVES
#define FS_GENERAL_WAVES 5
#endif
template <int MODE, bool AOS, bool ST>
__global__ __launch_bounds__(FS_BLOCK) __attribute__((amdgpu_waves_per_eu(FS_GENERAL_WAVES, FS_GENERAL_WAVES))) void k_force_general(FS_FORCE_ARGS, uint32_t which, uint32_t* __restrict__ hint, const float2* __restrict__ st_in) {
    __shared__ float2 s_pred[3][NBF_ROW];
    __shared__ uint32_t s_red[24];
    const uint32_t n = P.n_live ? *P.n_live : P.n;
    // how much work the lists held: the host sizes the next steps' grid of this kernel from it (a few steps late,
    // through pinned memory; an idle launch costs what its workgroups cost to come and go)
    if (hint && blockIdx.x == 0 && threadIdx.x == 0) *hint = which == 2u ? work_count[FS_LIST_PRE] + work_count[FS_LIST_LATE] : work_count[which];
    // Which entry a workgroup starts with: a list shorter than the grid (a small scene, the first dense clusters) is spread over
    // the chip (fs_force_lists.h); longer lists keep the plain order (consecutive entries are neighbouring blocks: they share
    // their candidates in one XCD's L2).
    const uint32_t e_spread = force_list_spread();
    // which = 0 / 1: one list; which = 2: the pre-registered list, then the late one (the usual single follow-up launch)
    for (uint32_t w = (which == 2u ? 0u : which); w <= (which == 2u ? 1u : which); ++w) {
        const uint32_t count = work_count[w];        // written earlier in the stream (k_density / the lean kernel)
        const uint32_t* list = worklist + force_list_base(P.n, w);
        for (uint32_t e = count < gridDim.x ? e_spread : blockIdx.x; e < count; e += gridDim.x) {
            const uint32_t blk = list[e];
            if (!block_may_advance(P, pairs, blk, n)) continue;          // uniform
            const uint32_t bits = defer_bits[force_defer_word(blk, w)];
            force_block<MODE, AOS, true, ST, false>(P, blk, n, bits, pos_s, vel_s, pred, rho2, cs, start_ref, pairs,
                                             tex, pos_out, vel_out, aos_out, rho_arr, defer_bits, worklist, work_count, st_in, s_pred,
                                             s_red);
            __syncthreads();                         // the LDS stage is reused by the next entry
        }
    }
}

#include "kernels_force_quad.inc"

// ---- the host schedule ----------------------------------------------------------------------------------------------
// The values of the kernels' common parameter list (FS_FORCE_ARGS), in its order and with exactly its types:
// hipExtLaunchKernelGGL takes the kernel's parameter types from the arguments it is given.
struct ForceArgs {
    StepParams P;
    const float2 *pos_s, *vel_s, *pred, *rho2;
    const uint32_t *cs, *start_ref;
    const u64* pairs;
    const float2* tex;
    float2 *pos_out, *vel_out;
    AosParticle* aos_out;
    const float* rho_arr;
    uint32_t *defer_bits, *worklist, *work_count;
};
// One launch: the common list, then the kernel's own arguments; `stop_ev` completes with the kernel.
template <typename K, typename... Own>
static void launch_force_kernel(K kernel, uint32_t grid, hipStream_t s, hipEvent_t stop_ev, const ForceArgs& a, Own... own) {
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(FS_BLOCK), 0, s, nullptr, stop_ev, 0, a.P, a.pos_s, a.vel_s, a.pred, a.rho2, a.cs,
                          a.start_ref, a.pairs, a.tex, a.pos_out, a.vel_out, a.aos_out, a.rho_arr, a.defer_bits, a.worklist,
                          a.work_count, own...);
}

// Which instantiation a launch takes, one place per kernel: the math mode (StepParams::fast_math), AOS (a renderer hand-off is
// registered) and ST (the surface-tension input is there: single-domain handles only, so never k_force_edge).
typedef void (*GeneralKernel)(FS_FORCE_ARGS, uint32_t, uint32_t*, const float2*);
typedef void (*LeanKernel)(FS_FORCE_ARGS, uint32_t, const float2*);
typedef void (*QuadKernel)(FS_FORCE_ARGS, uint32_t*, const float2*);

template <int MODE, bool ST> static GeneralKernel general_kernel(bool aos) { return aos ? k_force_general<MODE, true, ST> : k_force_general<MODE, false, ST>; }
template <bool ST> static GeneralKernel general_kernel(int mode, bool aos) {
    if (mode == 2) return general_kernel<2, ST>(aos);
    else if (mode == 1) return general_kernel<1, ST>(aos);
    else return general_kernel<0, ST>(aos);
}
static GeneralKernel general_kernel(int mode, bool aos, bool st) { return st ? general_kernel<true>(mode, aos) : general_kernel<false>(mode, aos); }

template <int MODE> static LeanKernel edge_kernel(bool aos) { return aos ? k_force_edge<MODE, true, false> : k_force_edge<MODE, false, false>; }
static LeanKernel edge_kernel(int mode, bool aos) {
    if (mode == 2) return edge_kernel<2>(aos);
    else if (mode == 1) return edge_kernel<1>(aos);
    else return edge_kernel<0>(aos);
}

template <int MODE, bool ST> static LeanKernel lean_kernel(bool aos) { return aos ? k_force<MODE, true, ST> : k_force<MODE, false, ST>; }
template <bool ST> static LeanKernel lean_kernel(int mode, bool aos) {
    if (mode == 2) return lean_kernel<2, ST>(aos);
    else if (mode == 1) return lean_kernel<1, ST>(aos);
    else return lean_kernel<0, ST>(aos);
}
static LeanKernel lean_kernel(int mode, bool aos, bool st) { return st ? lean_kernel<true>(mode, aos) : lean_kernel<false>(mode, aos); }

// (no tolerance-mode form: launch_force never gives that mode to the quad kernel)
template <int MODE, bool ST> static QuadKernel quad_kernel(bool aos) { return aos ? k_force_quad<MODE, true, ST> : k_force_quad<MODE, false, ST>; }
template <bool ST> static QuadKernel quad_kernel(int mode, bool aos) { return mode == 1 ? quad_kernel<1, ST>(aos) : quad_kernel<0, ST>(aos); }
static QuadKernel quad_kernel(int mode, bool aos, bool st) { return st ? quad_kernel<true>(mode, aos) : quad_kernel<false>(mode, aos); }

#ifndef FS_GENERAL_GRID
#define FS_GENERAL_GRID 4080u   // 16M, steps 150-250: force 1.175 (1024) -> 1.126 (2048) -> 1.117 ms (4096); steps 10-110 unchanged
#endif
void launch_force(hipStream_t st, const StepParams& P, const StepArrays& A, const ForceLaunch& L) {
    const ForceArgs a = {P, A.pos_s, A.vel_s, A.pred, A.rho2, A.cs, A.start_ref, A.pairs, A.tex, A.pos_out, A.vel_out,
                         (AosParticle*)L.aos_out, A.rho, A.fdefer, A.fwork, A.fcount};
    const int mode = P.fast_math;
    const bool aos = L.aos_out != nullptr, surf = L.st_in != nullptr;
    const GeneralKernel general = general_kernel(mode, aos, surf);
    uint32_t* const no_hint = nullptr;
    const uint32_t nb = nblk(P.n), grid = xcd_grid(nb, P.xcd_chunk_log2);
    uint32_t gg = L.general_grid ? L.general_grid : FS_GENERAL_GRID;      // the host's choice (sort_policy.h), else the full grid
    if (gg > nb) gg = nb;
    // (L.done goes to the pass's last launch only)
    if (L.side) {   // fork: the pre-registered waves on the second stream, beside the lean kernel
        (void)hipEventRecord(L.ev_fork, st);
        (void)hipStreamWaitEvent(L.side, L.ev_fork, 0);
        launch_force_kernel(general, gg, L.side, nullptr, a, FS_LIST_PRE, no_hint, L.st_in);
        (void)hipEventRecord(L.ev_join, L.side);
    }
    if (L.edge_grid) launch_force_kernel(edge_kernel(mode, aos), L.edge_grid, st, nullptr, a, 0u, L.st_in);      // edge-first slab step: the edge columns' blocks only
    else launch_force_kernel(lean_kernel(mode, aos, surf), grid, st, nullptr, a, 0u, L.st_in);
    if (L.side) {
        (void)hipStreamWaitEvent(st, L.ev_join, 0);
        launch_force_kernel(general, (nb < 256u ? nb : 256u), st, L.done, a, FS_LIST_LATE, no_hint, L.st_in);
    } else if (L.quad_entries != 0u && mode != 2 && (mode == 1 || P.share_div)) {
        // a short pre-registered list (the host's view of it, a few steps old): four lanes per particle (k_force_quad), then the
        // late list — what the lean kernel and the quad kernel gave up on — in the general kernel
        uint32_t qg = 8u * L.quad_entries;               // 4 work items per entry, twice that for a list that has grown since
        qg = qg < 80u ? 80u : qg > 4080u ? 4080u : (qg + 39u) / 40u * 40u;       // a multiple of 40 (the kernel's item mapping)
        launch_force_kernel(quad_kernel(mode, aos, surf), qg, st, nullptr, a, L.general_hint, L.st_in);
        launch_force_kernel(general, 240u, st, L.done, a, FS_LIST_LATE, no_hint, L.st_in);
    } else {
        launch_force_kernel(general, gg, st, L.done, a, 2u, L.general_hint, L.st_in);      // both lists in one follow-up launch
    }
}
}  // namespace fsd

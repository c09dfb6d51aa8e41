// kernels_strip.hip — the strips step of a slab handle (engine_slab.hip slab_interior / step_strips).  Ghosts
// stay OUT of the main sorted array.  While the two halo messages are in flight the rank sorts its carried-over particles and
// runs density + force for the INTERIOR columns [adv_lo, adv_hi); what the received records can influence — the owned columns
// within `Z` of a slab edge — is computed afterwards on a small second array, the STRIP: every particle of the main array
// whose cell column lies in a strip window (the two ghost columns, the boundary columns, and two columns of interior context),
// plus the received records.  The strip uses the main array's own window and cell keys, is counting-sorted like it, and goes
// through the SAME k_density / k_force (StepParams::adv_outside); k_strip_writeback puts the results back: boundary particles
// to their index in the main arrays, migrants to the slot past the main ones that mirrors their position in the message
// (k_slab_pack carries them over in the next step).
//
//   k_strip_rows      (1 workgroup) per grid row and window: the main array's index range -> exclusive offsets; totals
//   k_strip_gather    one wave per (row, window): copies {pos, vel} of the range into the strip's slots, histogram + ticket
//   k_strip_unpack    the received records behind them; classification (ghost / migrant), protocol checks
//   k_strip_writeback results -> main arrays
#include "fs_device.h"
#include "fs_kernels.h"
#include "fs_scan.h"
#include "fs_slab.h"

namespace fsd {

struct StripWin { uint32_t lo0, hi0, lo1, hi1; };      // LOCAL columns [lo0, hi0) and [lo1, hi1); an empty window has lo == hi
#define STRIP_NONE 0xFFFFFFFFu

#define SR_BLOCK 1024
__global__ __launch_bounds__(SR_BLOCK) void k_strip_rows(uint32_t grid_w, uint32_t grid_h, StripWin W, uint32_t R2,
                                                         const uint32_t* __restrict__ cs, uint32_t* __restrict__ rowbase,
                                                         uint32_t* __restrict__ strip_counters) {
    __shared__ uint32_t s_wave[SR_BLOCK / 64];
    __shared__ uint32_t s_carry;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0u;
    __syncthreads();
    const uint32_t entries = 2u * grid_h;
    for (uint32_t e0 = 0; e0 < entries; e0 += SR_BLOCK) {
        const uint32_t e = e0 + threadIdx.x;
        uint32_t c = 0;
        if (e < entries) {
            const uint32_t y = e >> 1, lo = (e & 1u) ? W.lo1 : W.lo0, hi = (e & 1u) ? W.hi1 : W.hi0;
            if (lo < hi) c = cs[y * grid_w + hi] - cs[y * grid_w + lo];
        }
        const uint32_t inc = wave_inclusive_scan(c);
        if (lane == 63u) s_wave[w] = inc;
        __syncthreads();
        uint32_t off = s_carry, tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < SR_BLOCK / 64; ++k) { const uint32_t t = s_wave[k]; if (k < w) off += t; tot += t; }
        if (e < entries) rowbase[e] = off + inc - c;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        strip_counters[1] = s_carry;                 // slots filled from the main array
        strip_counters[2] = s_carry + R2;            // slots in use once the received records sit behind them
    }
}

__global__ __launch_bounds__(SL_BLOCK) void k_strip_gather(uint32_t grid_w, uint32_t grid_h, uint32_t ncell, StripWin W,
                                                           uint32_t strip_cap, const uint32_t* __restrict__ cs,
                                                           const uint32_t* __restrict__ rowbase, const u64* __restrict__ pairs,
                                                           const float2* __restrict__ pos_s, const float2* __restrict__ vel_s,
                                                           float2* __restrict__ sp_pos, float2* __restrict__ sp_vel,
                                                           u64* __restrict__ kt, uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ back, unsigned long long* __restrict__ safe,
                                                           uint32_t* __restrict__ counters) {
    {   // the strip's safe-operand words (k_cs_fixreorder clears the unsafe bits)
        const uint32_t words = (strip_cap + 63u) / 64u;
        for (uint32_t t = blockIdx.x * SL_BLOCK + threadIdx.x; t < words; t += gridDim.x * SL_BLOCK) safe[t] = ~0ull;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * (SL_BLOCK / 64) + (threadIdx.x >> 6);       // wave-uniform
    if (e >= 2u * grid_h) return;
    const uint32_t y = e >> 1, lo = (e & 1u) ? W.lo1 : W.lo0, hi = (e & 1u) ? W.hi1 : W.hi0;
    if (lo >= hi) return;
    const uint32_t a = cs[y * grid_w + lo], c = cs[y * grid_w + hi] - a, base = rowbase[e];
    for (uint32_t k0 = 0; k0 < c; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool active = k < c && base + k < strip_cap;
        if (k < c && !active) atomicAdd(&counters[3], 1u);           // strip capacity exceeded (never: it equals the main array's)
        uint32_t key = 0;
        if (active) key = (uint32_t)(pairs[a + k] >> 32);
        const uint32_t ticket = cell_ticket(hist, key, ncell, active);
        if (active) {
            const uint32_t slot = base + k;
            kt[slot] = ((u64)key << 32) | (u64)ticket;
            sp_pos[slot] = pos_s[a + k];
            sp_vel[slot] = vel_s[a + k];
            back[slot] = a + k;                      // the main arrays' sorted index: where the force pass writes
        }
    }
}

// Received records -> strip slots [n_sm + j]; `P` is the MAIN array's StepParams (same window, same keys).
__global__ __launch_bounds__(SL_BLOCK) void k_strip_unpack(StepParams P, uint32_t main_slots, uint32_t R, uint32_t strip_cap,
                                                           const SlabHeader* __restrict__ hdr_left,
                                                           const float4* __restrict__ rec_left,
                                                           const SlabHeader* __restrict__ hdr_right,
                                                           const float4* __restrict__ rec_right,
                                                           float2* __restrict__ sp_pos, float2* __restrict__ sp_vel,
                                                           u64* __restrict__ kt, uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ back,
                                                           const uint32_t* __restrict__ strip_counters,
                                                           uint32_t* __restrict__ counters) {
    const uint32_t j = blockIdx.x * SL_BLOCK + threadIdx.x;
    const ReceivedRecord r(j, R, hdr_left, rec_left, hdr_right, rec_right, counters);
    const uint32_t slot = strip_counters[1] + j;
    const bool room = slot < strip_cap;
    uint32_t key = FS_DEAD_KEY, dst = STRIP_NONE;
    if (r.has()) {
        if (!room) {
            atomicAdd(&counters[3], 1u);
        } else {
            uint32_t cxg;
            key = r.read(P, &sp_pos[slot], &sp_vel[slot], counters, &cxg);
            // a migrant that lands within 2 columns of the interior (or in it) was not seen by the interior launch, which ran
            // while this message was in flight: the boundary zone was too narrow for its speed (fs_slab_set_boundary_cols)
            if (key != FS_DEAD_KEY && P.adv_lo < P.adv_hi) {
                if (!r.right && cxg + 2u >= P.adv_lo) atomicAdd(&counters[4], 1u);
                if (r.right && cxg < P.adv_hi + 2u) atomicAdd(&counters[4], 1u);
            }
            if (key != FS_DEAD_KEY && cxg >= P.own_lo && cxg < P.own_hi) dst = main_slots + j;   // a migrant: mine from now on
        }
    }
    const bool active = key != FS_DEAD_KEY;
    const uint32_t ticket = cell_ticket(hist, key, P.ncell, active);
    if (r.in_range && room) {
        kt[slot] = ((u64)key << 32) | (u64)(active ? ticket : 0u);
        back[slot] = dst;
    }
}

// Results of the strip's force pass -> the main arrays.  `P` = the strip's StepParams (adv_outside = 1).
__global__ __launch_bounds__(SL_BLOCK) void k_strip_writeback(StepParams P, uint32_t main_slots, const u64* __restrict__ sp_pairs,
                                                              const uint32_t* __restrict__ back,
                                                              const float2* __restrict__ sp_pos_out,
                                                              const float2* __restrict__ sp_vel_out,
                                                              const float2* __restrict__ sp_pred, const float* __restrict__ sp_rho,
                                                              float2* __restrict__ pos, float2* __restrict__ vel,
                                                              float2* __restrict__ pred, float* __restrict__ rho,
                                                              uint32_t* __restrict__ key, unsigned char* __restrict__ owned,
                                                              uint32_t* __restrict__ counters) {
    const uint32_t i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= *P.n_live) return;
    const u64 pr = sp_pairs[i];
    const uint32_t k = (uint32_t)(pr >> 32), dst = back[(uint32_t)pr];
    if (dst == STRIP_NONE || k == FS_DEAD_KEY) return;     // a ghost record
    if (!slab_advances(P, global_col(P, k))) {
        // interior context (advanced by the interior launch) — or a migrant that landed beyond the boundary zone: nobody
        // advanced it, it is lost (k_strip_unpack has counted it in far_halo already)
        if (dst >= main_slots) atomicAdd(&counters[2], 1u);
        return;
    }
    pos[dst] = sp_pos_out[i];
    vel[dst] = sp_vel_out[i];
    rho[dst] = sp_rho[i];
    if (dst >= main_slots) {                               // a migrant: the rest of its record, and it is carried over from now on
        pred[dst] = sp_pred[i];
        key[dst] = k;
        owned[dst] = 1;
    }
}

// ------------------------------------------------------------------ launchers
void launch_strip_gather(hipStream_t st, const StepParams& P, const SlabArrays& A, const StripArrays& T, const OverlapPlan& plan, uint32_t R) {
    const StripWin W{plan.win[0], plan.win[1], plan.win[2], plan.win[3]};
    hipLaunchKernelGGL(k_strip_rows, dim3(1), dim3(SR_BLOCK), 0, st, P.grid_w, P.grid_h, W, 2u * R, A.cs, T.rowbase, T.counters);
    const uint32_t waves = 2u * P.grid_h, per_block = SL_BLOCK / 64;
    hipLaunchKernelGGL(k_strip_gather, dim3((waves + per_block - 1) / per_block), dim3(SL_BLOCK), 0, st, P.grid_w, P.grid_h, P.ncell,
                       W, T.cap, A.cs, T.rowbase, A.pairs, A.pos_s, A.vel_s, T.pos, T.vel, T.kt, T.hist, T.back, T.safe, A.counters);
}

void launch_strip_unpack(hipStream_t st, const StepParams& P, const SlabArrays& A, const StripArrays& T, const SlabMessages& M) {
    const SlabHeader* hl = (const SlabHeader*)M.left;
    const SlabHeader* hr = (const SlabHeader*)M.right;
    hipLaunchKernelGGL(k_strip_unpack, dim3(sl_blocks(2 * M.R)), dim3(SL_BLOCK), 0, st, P, A.main_slots, M.R, T.cap, hl,
                       records(hl), hr, records(hr), T.pos, T.vel, T.kt, T.hist, T.back, T.counters, A.counters);
}

void launch_strip_writeback(hipStream_t st, const StepParams& P_strip, const SlabArrays& A, const StripArrays& T) {
    hipLaunchKernelGGL(k_strip_writeback, dim3(sl_blocks(T.cap)), dim3(SL_BLOCK), 0, st, P_strip, A.main_slots, T.pairs, T.back, T.pos_out,
                       T.vel_out, T.pred, T.rho, A.pos_out, A.vel_out, A.pred, A.rho, A.key_s, A.owned, A.counters);
}

}  // namespace fsd

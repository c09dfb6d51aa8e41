// kernels_sort_tile.inc — compiled only as part of kernels_sort.hip (see its last lines); include it nowhere else.
// The kernels of the bitonic sort that work inside 4096-pair tiles (fs_sort_tile.h), and their
// launch functions for the schedule (kernels_sort.hip):
//   * k_bitonic_local<INIT,KEYGEN>, k_bitonic_local32<KEYGEN>: predict + key fused into the tile load, then stages 0..11;
//   * k_bitonic_local<TAIL>:  the last 12 steps of a later stage;
//   * k_bitonic_stage12:      stage 12 (mirror step between two tiles + both tails) in one kernel.
#include <string.h>

#include "fs_3d.h"
#include "fs_device.h"
#include "fs_kernels.h"
#include "fs_sort.h"
#include "fs_sort_tile.h"

namespace fsd {

// `dirty[tile]` != 0 when a strided pass of the current stage swapped an element of the tile.
// A clean tile is still sorted (it was left sorted by the previous stage's tail / the init
// pass), so every compare of its tail is lower-index <= higher-index: a no-op.  Skipping it
// is therefore exact, not an approximation.
// KEYGEN (2D engine): the init pass also IS predict_next_position + create_spatial_lookup
// (compute.wgsl:8-42): it reads pos/vel and builds the (key, index) pairs on the fly instead of
// reading them — one launch and one write+read of the pair array less per step.
// KEYGEN: 0 = the pairs exist, 1 = 2D (StepParams, float2 pos / vel), 2 = 3D (KeyGen3 in the first words of the
// StepParams argument, float4 pos / vel: fs_3d.h predict3 / cell_key3, as in k3_predict_key).
__device__ __forceinline__ u64 keygen3(const KeyGen3& K, const float4* __restrict__ pos, const float4* __restrict__ vel, uint32_t i) {
    return ((u64)cell_key3(K, predict3(K, pos[i], vel[i])) << 32) | (u64)i;
}
template <bool INIT, int KEYGEN, int GB>
__global__ __launch_bounds__(LT<GB>::THREADS) void k_bitonic_local(u64* __restrict__ pairs, uint32_t n,
                                                                   uint32_t num_stages, uint32_t* __restrict__ dirty,
                                                                   StepParams P, const float2* __restrict__ pos,
                                                                   const float2* __restrict__ vel,
                                                                   uint32_t* __restrict__ gap_counter,
                                                                   const uint32_t* __restrict__ gate = nullptr,
                                                                   uint32_t gate_lo = 0, uint32_t gate_hi = 0) {
    constexpr int E = LT<GB>::E;
    __shared__ u64 s[LT<GB>::LDS];
    const uint32_t base = blockIdx.x * SORT_T;
    const uint32_t t = threadIdx.x;
    if (!INIT) {
        wave_prio_raise<FS_PRIO_SORT>();               // the tails: for the tile's loads (a wave that returns needs no lowering)
        if (gate_closed(gate, gate_lo, gate_hi)) return;   // uniform: this launch belongs to the other late-stage plan
        if (dirty[blockIdx.x] == 0) return;            // uniform: whole tile provably unchanged
    }
    u64 x[E];
    if (INIT) {
        // gate_lo == 2 with no gate (launch_bitonic_sort): this launch only serves the tiles the packed kernel
        // (k_bitonic_local32) could not take — their flag is FS_TILE_WIDE; anything else returns at once
        if (gate_lo == FS_TILE_WIDE && dirty[blockIdx.x] != FS_TILE_WIDE) return;
        if (KEYGEN != 0 && blockIdx.x == 0 && t == 0) *gap_counter = 0;      // consumed by k_reorder later in the stream
        // coalesced load, straight into LDS, then the group-0 view
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
            u64 v = ~0ull;
            if (base + j < n) {
                if (KEYGEN == 1) {
                    const uint32_t i = base + j;
                    v = ((u64)cell_of_point(P, predict_pos(P, pos[i], vel[i])) << 32) | (u64)i;
                } else if (KEYGEN == 2) {
                    v = keygen3(*reinterpret_cast<const KeyGen3*>(&P), reinterpret_cast<const float4*>(pos),
                                reinterpret_cast<const float4*>(vel), base + j);
                } else {
                    v = pairs[base + j];
                }
            }
            s[lt_pad<GB>(j)] = v;
        }
        __syncthreads();
        lt_read<GB, 0, GB - 1, false>(s, x, t);
        {   // A tile whose keys are already in order passes through the network unchanged: every compare-exchange of
            // an ascending network tests key[lower index] > key[higher index], which never holds (strict compare, so
            // equal keys stay put as well).  While the fluid still moves as a lattice whole steps change no key at
            // all, and then this kernel is key generation, one check and a store (steps 2-7, 9-11, 13-19 of the
            // 16M dam break: 190 -> ~55 us).
            int ok = 1;
#pragma unroll
            for (int r = 0; r + 1 < E; ++r) ok &= (uint32_t)(x[r] >> 32) <= (uint32_t)(x[r + 1] >> 32);
            if (t + 1u < (uint32_t)LT<GB>::THREADS) ok &= (uint32_t)(x[E - 1] >> 32) <= (uint32_t)(s[lt_pad<GB>((t + 1u) << GB)] >> 32);
            if (__syncthreads_and(ok)) {
                lt_store<GB>(pairs, s, x, base, t, n, true);   // the tile is still in LDS at its natural positions
                if (t == 0) dirty[blockIdx.x] = 0;
                return;
            }
        }
        lt_stage<GB, 0>(s, x, t);
        if (num_stages > 1) lt_stage<GB, 1>(s, x, t);
        if (num_stages > 2) lt_stage<GB, 2>(s, x, t);
        if (num_stages > 3) lt_stage<GB, 3>(s, x, t);
        if (num_stages > 4) lt_stage<GB, 4>(s, x, t);
        if (num_stages > 5) lt_stage<GB, 5>(s, x, t);
        if (num_stages > 6) lt_stage<GB, 6>(s, x, t);
        if (num_stages > 7) lt_stage<GB, 7>(s, x, t);
        if (num_stages > 8) lt_stage<GB, 8>(s, x, t);
        if (num_stages > 9) lt_stage<GB, 9>(s, x, t);
        if (num_stages > 10) lt_stage<GB, 10>(s, x, t);
        if (num_stages > 11) lt_stage<GB, 11>(s, x, t);
    } else {
        lt_tail<GB, FS_PRIO_SORT>(pairs, n, base, s, x, t);      // (lowers the priority behind its loads)
    }
    lt_store<GB>(pairs, s, x, base, t, n);
    if (t == 0) dirty[blockIdx.x] = 0;                 // sorted again
}

// ---- the first kernel in PACKED form --------------------------------------------------------------------------------
// Stages 0..11 of a tile only ever compare keys and move (key, index) pairs INSIDE the tile, and the index is
// base + position: one 32-bit word (key - tile_min) << 12 | position carries the same information whenever the keys of
// the tile span less than 2^20 — always, for a state that was in cell order one step ago (a tile of 4096 particles covers
// ~1000 cells plus at most a few row ends; an uploaded, shuffled state does not, see FS_TILE_WIDE).  Half the LDS per
// tile (17.4 KB: 8 tiles per CU instead of 4 — the round-2 kernel sat at 3 waves per SIMD with its load, network and
// store phases adding up instead of overlapping), half the registers, half the LDS traffic, and a compare-exchange of
// 4 instructions instead of 5 (lt_cx).  The pairs are rebuilt at the store.  Same network, same strict compare on
// keys only: the arrangement — ties included — is bit for bit the 64-bit kernel's (tests/test_sort_gpu.py).
// Tiles whose keys span 2^20 or more are left untouched and flagged FS_TILE_WIDE in `dirty`; the 64-bit kernel follows
// in the stream and takes exactly those (an idle launch otherwise).
#ifndef FS_SORT32_WAVES
#define FS_SORT32_WAVES 0      // > 0: pin the register budget to that many waves per SIMD (A/B: tools/ab_variant.py)
#endif
#if FS_SORT32_WAVES > 0
#define FS_SORT32_ATTR __attribute__((amdgpu_waves_per_eu(FS_SORT32_WAVES, FS_SORT32_WAVES)))
#else
#define FS_SORT32_ATTR
#endif
template <int KEYGEN, int GB>
__global__ __launch_bounds__(LT<GB>::THREADS) FS_SORT32_ATTR void k_bitonic_local32(u64* __restrict__ pairs, uint32_t n,
                                                                     uint32_t num_stages, uint32_t* __restrict__ dirty,
                                                                     StepParams P, const float2* __restrict__ pos,
                                                                     const float2* __restrict__ vel,
                                                                     uint32_t* __restrict__ gap_counter, uint32_t wide_word) {
    constexpr int E = LT<GB>::E;
    __shared__ uint32_t s[LT<GB>::LDS];
    __shared__ uint32_t s_mm[2 * (LT<GB>::THREADS / 64)];
    const uint32_t base = blockIdx.x * SORT_T;
    const uint32_t t = threadIdx.x;
    wave_prio_raise<FS_PRIO_SORT>();                                     // for the position / velocity loads and the key arithmetic
    if (KEYGEN != 0 && blockIdx.x == 0 && t == 0) *gap_counter = 0;      // consumed by k_reorder later in the stream
    uint32_t key[E];
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int r = 0; r < E; ++r) {                                        // coalesced: position j = r << TOPB | t
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        uint32_t k = 0xFFFFFFFFu;                                        // padding sorts last (as ~0ull does in the 64-bit form)
        if (base + j < n) {
            if (KEYGEN == 1) k = cell_of_point(P, predict_pos(P, pos[base + j], vel[base + j]));
            else if (KEYGEN == 2) k = (uint32_t)(keygen3(*reinterpret_cast<const KeyGen3*>(&P), reinterpret_cast<const float4*>(pos),
                                                         reinterpret_cast<const float4*>(vel), base + j) >> 32);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        key[r] = k;
    }
    wave_prio_lower<FS_PRIO_SORT>();                                     // the loads are out and the keys formed
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((t & 63u) == 0) { s_mm[2 * (t >> 6)] = kmin; s_mm[2 * (t >> 6) + 1] = kmax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LT<GB>::THREADS / 64; ++w) {
        const uint32_t a = s_mm[2 * w], b = s_mm[2 * w + 1];
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    static_assert(KEYGEN == 1 || KEYGEN == 2, "the packed form builds the pairs itself: index = base + position");
    if (kmax - kmin >= (1u << 20) - 1u) {                                // uniform; 0xFFFFF is reserved for the padding
        if (t == 0) { dirty[blockIdx.x] = FS_TILE_WIDE; atomicAdd(&dirty[wide_word], 1u); }   // (counted: fs_sort_plan_info.wide_tiles)
        return;
    }
    uint32_t x[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        const uint32_t rel = key[r] == 0xFFFFFFFFu ? 0xFFFFFu : key[r] - kmin;
        s[lt_pad<GB>(j)] = (rel << 12) | j;
    }
    __syncthreads();
    lt_read<GB, 0, GB - 1, false>(s, x, t);
    bool sorted_already;
    {   // a tile whose keys are already in order passes through the network unchanged (see k_bitonic_local)
        int ok = 1;
#pragma unroll
        for (int r = 0; r + 1 < E; ++r) ok &= (x[r] >> 12) <= (x[r + 1] >> 12);
        if (t + 1u < (uint32_t)LT<GB>::THREADS) ok &= (x[E - 1] >> 12) <= (s[lt_pad<GB>((t + 1u) << GB)] >> 12);
        sorted_already = __syncthreads_and(ok) != 0;
    }
    if (!sorted_already) {
        lt_stage<GB, 0>(s, x, t);
        if (num_stages > 1) lt_stage<GB, 1>(s, x, t);
        if (num_stages > 2) lt_stage<GB, 2>(s, x, t);
        if (num_stages > 3) lt_stage<GB, 3>(s, x, t);
        if (num_stages > 4) lt_stage<GB, 4>(s, x, t);
        if (num_stages > 5) lt_stage<GB, 5>(s, x, t);
        if (num_stages > 6) lt_stage<GB, 6>(s, x, t);
        if (num_stages > 7) lt_stage<GB, 7>(s, x, t);
        if (num_stages > 8) lt_stage<GB, 8>(s, x, t);
        if (num_stages > 9) lt_stage<GB, 9>(s, x, t);
        if (num_stages > 10) lt_stage<GB, 10>(s, x, t);
        if (num_stages > 11) lt_stage<GB, 11>(s, x, t);
        lt_write<GB, 0, GB - 1, false>(s, x, t);           // back to LDS at the natural positions
    }
    __syncthreads();
    lt_read<GB, LT<GB>::TOPB, GB - 1, false>(s, x, t);     // the coalesced layout: 512 contiguous bytes per wave store
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        if (base + j < n) {
            pairs[base + j] = ((u64)(kmin + (x[r] >> 12)) << 32) | (u64)(base + (x[r] & 0xFFFu));
        }
    }
    if (t == 0) dirty[blockIdx.x] = 0;
}

// Stage 12 in ONE kernel: its only global step is the mirror step between the two tiles of an 8192-block, so a
// workgroup takes both tiles: A in the top layout, B read back to front (thread t holds B[4095 - (r << TOPB | t)],
// still a coalesced load) — the mirror partners then sit in the same register slot of the same thread.  After the
// compare-exchanges A's tail runs from the registers; B's registers, renamed r -> E-1 - r, ARE the top layout of thread
// THREADS-1 - t, so its tail only writes its first LDS round with that thread id.  Saves the strided pass (one read +
// write of the pair array) and a launch.  Certificate: last(A) <= first(B) (both tiles are sorted on entry) => no
// compare of the stage can swap; otherwise the pair (last(A), first(B)) itself swaps and both tails are needed.
template <int GB>
__global__ __launch_bounds__(LT<GB>::THREADS) void k_bitonic_stage12(u64* __restrict__ pairs, uint32_t n) {
    constexpr int E = LT<GB>::E;
    __shared__ u64 s[LT<GB>::LDS];
    const uint32_t t = threadIdx.x;
    const uint32_t base_a = blockIdx.x * (2u * SORT_T), base_b = base_a + SORT_T;
    wave_prio_raise<FS_PRIO_SORT>();                   // for the two tiles' loads
    if (base_b >= n) return;                           // B holds sentinels only: nothing can swap
    {
        const uint32_t last_a = (uint32_t)(pairs[base_b - 1u] >> 32), first_b = (uint32_t)(pairs[base_b] >> 32);
        if (last_a <= first_b) return;                 // uniform
    }
    u64 xa[E], xb[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        xa[r] = pairs[base_a + j];                     // base_b < n: A is complete
        const uint32_t pb = base_b + (SORT_T - 1u - j);
        xb[r] = pb < n ? pairs[pb] : ~0ull;
    }
    wave_prio_lower<FS_PRIO_SORT>();
#pragma unroll
    for (int r = 0; r < E; ++r) lt_cx(xa[r], xb[r]);               // A[j] vs B[4095 - j]: the stage's mirror step
    lt_tail_regs<GB>(s, xa, t, t);
    lt_store<GB>(pairs, s, xa, base_a, t, n);
    u64 xn[E];
#pragma unroll
    for (int r = 0; r < E; ++r) xn[r] = xb[E - 1 - r];             // natural order of thread THREADS-1 - t
    __syncthreads();                                   // A's last LDS reads are done
    lt_tail_regs<GB>(s, xn, (uint32_t)LT<GB>::THREADS - 1u - t, t);
    lt_store<GB>(pairs, s, xn, base_b, t, n);
}

// ---- launch functions ------------------------------------------------------------------------------------------------
void launch_sort_tails(hipStream_t st, u64* pairs, uint32_t n, uint32_t* dirty, int gb, const uint32_t* gate, uint32_t glo,
                       uint32_t ghi) {
    // num_stages, P, pos, vel and gap_counter are unused by the <false, ...> form: they stay in the one parameter list the
    // template has, whose layout the first kernel was measured with.
    StepParams P0;
    memset(&P0, 0, sizeof P0);
    const dim3 grid((n + SORT_T - 1) / SORT_T);
    if (gb == 3)
        hipLaunchKernelGGL((k_bitonic_local<false, 0, 3>), grid, dim3(LT<3>::THREADS), 0, st, pairs, n, 0u, dirty, P0,
                           (const float2*)nullptr, (const float2*)nullptr, (uint32_t*)nullptr, gate, glo, ghi);
    else
        hipLaunchKernelGGL((k_bitonic_local<false, 0, 4>), grid, dim3(LT<4>::THREADS), 0, st, pairs, n, 0u, dirty, P0,
                           (const float2*)nullptr, (const float2*)nullptr, (uint32_t*)nullptr, gate, glo, ghi);
}

template <int KEYGEN, int GB>
static int first_kernel(hipStream_t st, u64* pairs, uint32_t n, uint32_t init_stages, uint32_t* dirty, const StepParams& P,
                        const float2* pos, const float2* vel, uint32_t* gap_counter, bool packed) {
    const dim3 grid((n + SORT_T - 1) / SORT_T), block(LT<GB>::THREADS);
    if constexpr (KEYGEN != 0) {
        if (packed) {
            hipLaunchKernelGGL((k_bitonic_local32<KEYGEN, GB>), grid, block, 0, st, pairs, n, init_stages, dirty, P, pos, vel,
                               gap_counter, sort_plan_word(n) + SORT_PW_WIDE_TILES);
            // gate_lo == FS_TILE_WIDE with no gate: only the tiles the packed kernel flagged.  The parameter is overloaded
            // because a parameter of its own would change the kernel's argument list, which stays as measured.
            hipLaunchKernelGGL((k_bitonic_local<true, KEYGEN, GB>), grid, block, 0, st, pairs, n, init_stages, dirty, P, pos,
                               vel, gap_counter, (const uint32_t*)nullptr, FS_TILE_WIDE, 0u);
            return 2;
        }
    }
    hipLaunchKernelGGL((k_bitonic_local<true, KEYGEN, GB>), grid, block, 0, st, pairs, n, init_stages, dirty, P, pos, vel,
                       gap_counter, (const uint32_t*)nullptr, 0u, 0u);
    return 1;
}
template <int KEYGEN>
static int first_kernel_gb(int gb, hipStream_t st, u64* pairs, uint32_t n, uint32_t init_stages, uint32_t* dirty,
                        const StepParams& P, const float2* pos, const float2* vel, uint32_t* gap_counter, bool packed) {
    return gb == 3 ? first_kernel<KEYGEN, 3>(st, pairs, n, init_stages, dirty, P, pos, vel, gap_counter, packed)
                   : first_kernel<KEYGEN, 4>(st, pairs, n, init_stages, dirty, P, pos, vel, gap_counter, packed);
}

int launch_sort_first(hipStream_t st, u64* pairs, uint32_t n, uint32_t init_stages, uint32_t* dirty, const SortKeys* keys,
                      int gb, bool packed) {
    if (keys && keys->keygen == 1)
        return first_kernel_gb<1>(gb, st, pairs, n, init_stages, dirty, keys->P, keys->pos, keys->vel, keys->gap_counter, packed);
    if (keys)
        return first_kernel_gb<2>(gb, st, pairs, n, init_stages, dirty, keys->P, keys->pos, keys->vel, keys->gap_counter, packed);
    StepParams P0;                                      // the pairs exist: no packed form, it builds them itself
    memset(&P0, 0, sizeof P0);
    return first_kernel_gb<0>(gb, st, pairs, n, init_stages, dirty, P0, nullptr, nullptr, nullptr, false);
}

void launch_sort_stage12(hipStream_t st, u64* pairs, uint32_t n, int gb) {
    const dim3 grid(((n + SORT_T - 1) / SORT_T + 1u) / 2u);
    if (gb == 3) hipLaunchKernelGGL((k_bitonic_stage12<3>), grid, dim3(LT<3>::THREADS), 0, st, pairs, n);
    else hipLaunchKernelGGL((k_bitonic_stage12<4>), grid, dim3(LT<4>::THREADS), 0, st, pairs, n);
}

}  // namespace fsd

// fs_sort_tile.h — the bitonic network inside one 4096-pair tile, in registers and LDS: LT and the lt_* primitives of the
// tile kernels (kernels_sort_tile.inc) and of the stand-by kernel's tails (kernels_sort_global.inc k_late_fallback).
// Device code: the kernels' register counts depend on how it is written (one recursive helper in place of the unrolled
// stage lists cost k_bitonic_local32<1,4> six VGPRs), so it changes only with the instruction streams compared.
#pragma once
#include "fs_device.h"
#include "fs_sort.h"

namespace fsd {

// Register-blocked: 2^(12-GB) threads x E = 2^GB elements.  The 12 index bits of a tile are split in groups of GB;
// a thread holds the E elements that differ in ONE group, so GB consecutive steps run in VGPRs, and the tile is
// re-distributed through LDS between groups (instead of one LDS round trip per step).  Layout of group g (in-thread
// bits [g GB, (g+1) GB), B = g GB):   idx = (t >> B) << (B + GB) | r << B | t & (2^B - 1)
// — the top group is also the coalesced global layout (idx = r << (12-GB) | t), group 0 holds E contiguous elements.
//   GB = 4: 256 threads x 16 elements, three groups — for sorts of more than 512 tiles;
//   GB = 3: 512 threads x  8 elements, four groups: twice the waves per tile (the tile's LDS footprint bounds the
//           occupancy: four tiles per CU) for a third more LDS round trips.  Measured at 16M: first kernel 179 -> 190 us,
//           tails equal, stage 12 42 -> 38 us, sort 0.435 -> 0.445 ms.  Few tiles cannot fill the chip (1M particles: 256
//           tiles on 256 CUs) and there the shorter per-thread chains win: sort_gb().
// LDS addresses are padded (lt_pad) so that the 8-byte accesses of all layouts are bank-conflict free, or 2-way at
// worst (64 x 4-B banks; GB = 3: chosen by enumeration over the layouts and their mirrored reads).
// The mirror step of stage s is done as in k_bitonic_strided: rows with bit s set are read
// from idx ^ (2^s - 1), after which it is a plain distance-2^s step and the remaining steps
// of that round compare in reversed order on those rows.
template <int GB> struct LT {
    static constexpr int E = 1 << GB;                     // elements per thread
    static constexpr int THREADS = (int)SORT_T >> GB;
    static constexpr int TOPB = SORT_LOG_T - GB;          // bit position of the top group
    static constexpr int NG = SORT_LOG_T / GB;            // groups
    static constexpr int LDS = GB == 4 ? (int)SORT_T + ((int)SORT_T >> 4) : 4384;
};

template <int GB>
__device__ __forceinline__ uint32_t lt_pad(uint32_t idx) {
    if (GB == 4) return idx + (idx >> 4);
    return idx + ((idx >> 5) << 1) + (idx >> 7);          // max 4380
}

template <int GB, int B>
__device__ __forceinline__ uint32_t lt_idx(uint32_t r, uint32_t t) {
    return ((t >> B) << (B + GB)) | (r << B) | (t & ((1u << B) - 1u));
}

__device__ __forceinline__ void lt_cx(u64& lo, u64& hi) {     // lo = physically lower element
    if ((uint32_t)(lo >> 32) > (uint32_t)(hi >> 32)) { const u64 t = lo; lo = hi; hi = t; }
}
// Packed form of the first kernel (k_bitonic_local32): one 32-bit word per element, (key - tile_min) << 12 | position in
// the tile.  key(a) > key(b)  <=>  a > (b | 0xFFF): with equal keys a <= key << 12 | 0xFFF, with key(a) > key(b)
// a >= (key(b) + 1) << 12.  Equal keys never swap, exactly as in the 64-bit form: 4 VALU instead of 5, half the LDS.
__device__ __forceinline__ void lt_cx(uint32_t& lo, uint32_t& hi) {
    if (lo > (hi | 0xFFFu)) { const uint32_t t = lo; lo = hi; hi = t; }
}

// Steps on in-thread bits TOP..0 of a group.  FLIP: the step on bit TOP is a stage's mirror step.
template <int GB, int TOP, bool FLIP, class T>
__device__ __forceinline__ void lt_round(T (&x)[1 << GB]) {
#pragma unroll
    for (int b = TOP; b >= 0; --b) {
#pragma unroll
        for (int r = 0; r < (1 << GB); ++r) {
            if (r & (1 << b)) continue;
            const int r1 = r | (1 << b);
            if (FLIP && b < TOP && ((r >> TOP) & 1)) lt_cx(x[r1], x[r]);   // reversed rows (see header)
            else lt_cx(x[r], x[r1]);
        }
    }
}

template <int GB, int B, int TOP, bool FLIP, class T>
__device__ __forceinline__ void lt_read(const T* s, T (&x)[1 << GB], uint32_t t) {
#pragma unroll
    for (int r = 0; r < (1 << GB); ++r) {
        uint32_t idx = lt_idx<GB, B>((uint32_t)r, t);
        if (FLIP && ((r >> TOP) & 1)) idx ^= (1u << (B + TOP)) - 1u;
        x[r] = s[lt_pad<GB>(idx)];
    }
}

template <int GB, int B, int TOP, bool FLIP, class T>
__device__ __forceinline__ void lt_write(T* s, const T (&x)[1 << GB], uint32_t t) {
#pragma unroll
    for (int r = 0; r < (1 << GB); ++r) {
        uint32_t idx = lt_idx<GB, B>((uint32_t)r, t);
        if (FLIP && ((r >> TOP) & 1)) idx ^= (1u << (B + TOP)) - 1u;
        s[lt_pad<GB>(idx)] = x[r];
    }
}

// A re-distribution that involves group G exchanges data between the 2^(G GB) threads that share t >> (G GB).  Up to 64
// of them that is one wave: a wave's LDS instructions execute in program order, so no workgroup barrier is needed
// there — only a compiler-level fence.
__device__ __forceinline__ void lt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int GB, int G>
__device__ __forceinline__ void lt_sync() {
    if (G * GB > 6) __syncthreads();
    else lt_wave_sync();
}

// From group G (just written to LDS in its layout) down to group 0: the remaining plain steps of a stage or tail.
template <int GB, int G, class T>
__device__ __forceinline__ void lt_descend(T* s, T (&x)[1 << GB], uint32_t t) {
    if constexpr (G > 0) {
        lt_sync<GB, G>();
        lt_read<GB, (G - 1) * GB, GB - 1, false>(s, x, t);
        lt_round<GB, GB - 1, false>(x);
        if constexpr (G - 1 > 0) {
            lt_write<GB, (G - 1) * GB, GB - 1, false>(s, x, t);
            lt_descend<GB, G - 1>(s, x, t);
        }
    }
}

// Stage S (0..11) of the network inside a tile; on entry and exit the tile is in the group-0 layout, in registers.
template <int GB, int S, class T>
__device__ __forceinline__ void lt_stage(T* s, T (&x)[1 << GB], uint32_t t) {
    constexpr int G = S / GB, TOP = S % GB;
    if constexpr (G == 0) {
#pragma unroll
        for (int r = 0; r < (1 << GB); ++r) {
            if (r & (1 << S)) continue;
            lt_cx(x[r], x[r ^ ((2 << S) - 1)]);          // mirror inside the 2^(S+1) block
        }
        if constexpr (S > 0) lt_round<GB, (S > 0 ? S - 1 : 0), false>(x);
    } else {
        lt_write<GB, 0, GB - 1, false>(s, x, t);
        lt_sync<GB, G>();                 // group 0 -> group G (mirrored reads stay inside the 2^(S+1) block: same threads)
        lt_read<GB, G * GB, TOP, true>(s, x, t);
        lt_round<GB, TOP, true>(x);
        lt_write<GB, G * GB, TOP, true>(s, x, t);
        lt_descend<GB, G>(s, x, t);
    }
}

// The tile leaves the network in the group-0 layout (E contiguous elements per thread): stored from there, a wave's
// store instruction touches 64 different lines, 16 bytes each.  One more trip through LDS puts it into the top
// layout, whose stores are 512 contiguous bytes per wave instruction.  (A thread's group-0 positions are its own: no
// barrier before the write; the top-layout reads cross waves: one barrier after it.)
template <int GB>
__device__ __forceinline__ void lt_store(u64* __restrict__ pairs, u64* s, u64 (&x)[1 << GB], uint32_t base, uint32_t t,
                                         uint32_t n, bool in_lds = false) {
    if (!in_lds) lt_write<GB, 0, GB - 1, false>(s, x, t);
    __syncthreads();
    lt_read<GB, LT<GB>::TOPB, GB - 1, false>(s, x, t);
#pragma unroll
    for (int r = 0; r < (1 << GB); ++r) {
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        if (base + j < n) pairs[base + j] = x[r];
    }
}

// The twelve plain steps of a tail on a tile already in registers (top layout as held by thread `t1`: the caller may
// hold the tile mirrored, see k_bitonic_stage12), ending in the group-0 layout of the real thread.
template <int GB>
__device__ __forceinline__ void lt_tail_regs(u64* s, u64 (&x)[1 << GB], uint32_t t1, uint32_t t) {
    lt_round<GB, GB - 1, false>(x);
    lt_write<GB, LT<GB>::TOPB, GB - 1, false>(s, x, t1);
    lt_descend<GB, LT<GB>::NG - 1>(s, x, t);
}

// tail of a stage >= 12: plain steps on bits 11..0 of one tile; the top layout IS the coalesced global layout
// PRIO: the priority level the calling kernel raised its waves to for these loads (fs_device.h wave_prio_raise), dropped
// again in front of the network steps; 0 (the stand-by kernel): nothing.
template <int GB, int PRIO = 0>
__device__ __forceinline__ void lt_tail(const u64* __restrict__ pairs, uint32_t n, uint32_t base, u64* s, u64 (&x)[1 << GB],
                                        uint32_t t) {
#pragma unroll
    for (int r = 0; r < (1 << GB); ++r) {
        const uint32_t j = ((uint32_t)r << LT<GB>::TOPB) | t;
        x[r] = (base + j < n) ? pairs[base + j] : ~0ull;
    }
    wave_prio_lower<PRIO>();
    lt_tail_regs<GB>(s, x, t, t);
}

}  // namespace fsd

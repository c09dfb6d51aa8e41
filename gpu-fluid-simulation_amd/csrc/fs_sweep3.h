// fs_sweep3.h — the 27-cell sweep of the 3D passes that walk neighbours (kernels_density3d.hip: density and surface tension,
// kernels_force3d.hip: force + integrate), the 3D counterpart of fs_neighbours.h: the block mapping, the nine row ranges from
// a particle's key, the plane-by-plane driver (sweep3_lane + sweep3_planes), the staged plane, its pass masks and their
// hand-over from the density pass.  A pass is its term code plus a call to the driver.
#pragma once
#include "fs_3d.h"

namespace fsd {

// Workgroup -> block of particles for the density / force kernels, XCD-aware as in 2D (fs_device.h xcd_block): the
// hardware deals consecutive workgroup ids round-robin to the 8 XCDs, and a block's nine sweep rows are the rows of the
// blocks 3 (next cell row) and ~310 (next z-plane) away — dealt block by block, EVERY XCD's L2 fetches every row.  Chunks
// of 2^c consecutive blocks per XCD keep the y-neighbour rows in one L2.  Grid: xcd_grid3() blocks.
__device__ __forceinline__ bool xcd_block3(const Params3& P, uint32_t nblocks, uint32_t* logical) {
    const uint32_t c = P.xcd_chunk_log2;
    const uint32_t slot = blockIdx.x >> 3, xcd = blockIdx.x & 7u;
    const uint32_t chunk = ((slot >> c) << 3) | xcd;
    const uint32_t lb = (chunk << c) | (slot & ((1u << c) - 1u));
    *logical = lb;
    return lb < nblocks;
}
static inline uint32_t xcd_grid3(uint32_t nb, uint32_t c) {
    const uint32_t chunks = (nb + (1u << c) - 1u) >> c;
    return (((chunks + 7u) >> 3) << 3) << c;
}

// Sweep row j in 0..8, (oz, oy) = (j/3 - 1, j%3 - 1), from the particle's KEY: cells (cx-1 .. cx+1, cy+oy, cz+oz) are the ids
// key + (oz gh + oy) gw - 1 .. + 2, so the density and force passes need no cell coordinates (three IEEE divisions per
// particle) — only the stored key.  Cell index 0 of every row / plane is padding and always empty (coordinates are
// floor(..) + 1 >= 1), so a row that wraps into the next row or plane reads an empty range exactly where the row is outside
// the grid, and ids past the table are cut off here.  false: no candidates.
__device__ __forceinline__ bool row3_key(const Params3& P, const uint32_t* __restrict__ cs, uint32_t key, int j,
                                         uint32_t* lo, uint32_t* hi) {
    const int32_t off = ((j / 3 - 1) * (int32_t)P.gh + (j % 3 - 1)) * (int32_t)P.gw - 1;      // scalar
    const uint32_t id_lo = key + (uint32_t)off;                       // wraps for a row below the grid: >= ncell
    if (id_lo >= P.ncell) return false;
    const uint32_t id_hi = id_lo + 3u > P.ncell ? P.ncell : id_lo + 3u;
    *lo = cs[id_lo];
    *hi = cs[id_hi];
    return *lo < *hi;
}

// All 18 cell-start look-ups of a particle's nine sweep rows up front: independent loads, one latency.  Empty row: lo = hi = 0.
__device__ __forceinline__ void rows3_lookup(const Params3& P, const uint32_t* __restrict__ cs, uint32_t key, bool live,
                                             uint32_t* lo9, uint32_t* hi9) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        lo9[j] = 0; hi9[j] = 0;
        if (live && !row3_key(P, cs, key, j, &lo9[j], &hi9[j])) { lo9[j] = 0; hi9[j] = 0; }
    }
}

#define B3F 256              // workgroup of the density / force kernels (one wave per workgroup is slower: profiles/r03_rejected.md)
#define W3F (B3F / 64)
#define TILE3 400            // staged candidates per sweep row; one z-plane (3 rows) is staged at a time.  8 M, steps 10-110, strict / tolerance step: 352: 3.30 / 2.70, 384: 3.21 / 2.60, 400: 3.18 / 2.56, 408: 3.18 / 2.56 ms (408 is the most four workgroups per CU have room for)
#define TILE3_ROW TILE3      // rows 0 and 1 over-read into the next row's stage (masked off), only the last row needs the slack
#define TILE3_PAD 72u        // the wave-uniform scan reads up to the wave's longest row (<= 64) + 3 past a lane's own range
#define TILE3_LDS (3 * TILE3_ROW + TILE3_PAD)
// k3_force stages the neighbours' VELOCITY records {vx, vy, vz, +-1/rho} behind the positions, same row pitch: the walk's
// second fetch is then an LDS read at a constant offset from the first instead of a 16-byte gather per neighbour (with the
// masks handed over the kernel was bound by exactly those gathers: waves parked 65 - 79 %, profiles/r03_counters_3d*.md).
// 19.6 + 18.4 KB per workgroup: four workgroups (16 waves) per CU.
#define TILE3_VEL_OFF (TILE3_LDS * 16u)          // bytes from a staged position to the same candidate's velocity
#define TILE3_FORCE_LDS (TILE3_LDS + 3 * TILE3_ROW)
typedef unsigned long long u64m;

// One z-plane of the sweep that fits the tile, staged for the workgroup: the three rows [blo, bhi) into s_flat with coalesced
// loads — positions, and with VEL the velocity records TILE3_LDS entries behind them — and a barrier.
template <bool VEL>
__device__ __forceinline__ void stage3_rows(const uint32_t* blo, const uint32_t* bhi, const float4* pred, const float4* vel_s,
                                            float4* s_flat) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        for (uint32_t j = threadIdx.x; j < bhi[r] - blo[r]; j += B3F) {
            s_flat[r * TILE3_ROW + j] = pred[blo[r] + j];
            if (VEL) s_flat[TILE3_LDS + r * TILE3_ROW + j] = vel_s[blo[r] + j];
        }
    __syncthreads();
}

// ---- pass masks of one staged z-plane -----------------------------------------------------------------------
// A 3D row of three cells holds ~24 candidates at rest (8 particles per cell) and passes 32 as soon as the column
// compresses, so the pass masks are 64 bits, filled as two 32-bit shift registers: v_cmp + one v_addc_co per candidate shift
// `!(r2 > h^2)` in (fs_device.h shift_in_not_greater; fs_force_sweep.h force_sweep_masks is the 2D form).  Candidate t of a row ends up at bit 63 - t.
// Valid for waves whose three rows hold <= 64 candidates each; the rows are read from the LDS stage `s_flat`
// (TILE3_ROW entries per row).  Both the density and the force pass need exactly these masks: k3_density computes
// them, walks them for its own sum and (Params3::handoff) stores them — 72 B per particle — so that k3_force does not
// scan the 216 candidates a second time (~2 600 of its ~9 900 VALU instructions per wave).
// Where a lane's row r starts in the staged plane, and the bits of a pass mask that are the lane's own `len` candidates
// (candidate k at bit 63 - k; rows of up to 128: candidates 0 .. 63 in the hi word, 64 .. 127 in the lo word).
__device__ __forceinline__ uint32_t row_la(const RowRanges& R, const uint32_t* blo, int r) {
    const uint32_t len = R.hi[r] - R.lo[r];
    return (uint32_t)r * TILE3_ROW + (len ? R.lo[r] - blo[r] : 0u);
}
__device__ __forceinline__ u64m keep64(uint32_t len) { return len ? ~0ull << (64u - len) : 0ull; }            // len <= 64
__device__ __forceinline__ u64m keep128_hi(uint32_t len) { return len >= 64u ? ~0ull : keep64(len); }
__device__ __forceinline__ u64m keep128_lo(uint32_t len) { return len > 64u ? ~0ull << (128u - len) : 0ull; }   // len <= 128
// Candidates t, t + 1, .. of the staged row `base` shifted into the 32-bit register `w`, four at a time, until t reaches
// `limit` or no lane of the wave has candidates left (t is wave-uniform: scalar branches).  Reads up to 3 entries past the
// wave's longest row.
__device__ __forceinline__ void scan3_word(uint32_t& w, uint32_t& t, uint32_t limit, const float4* base, uint32_t len, float4 me,
                                           float lim) {
    for (; t < limit && __any(t < len); t += 4u) {
        const float4 q0 = base[t], q1 = base[t + 1u], q2 = base[t + 2u], q3 = base[t + 3u];
        const float4 qq[4] = {q0, q1, q2, q3};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float ox = qq[u].x - me.x, oy = qq[u].y - me.y, oz = qq[u].z - me.z;
            shift_in_not_greater(w, ox * ox + oy * oy + oz * oz, lim);
        }
    }
}
__device__ __forceinline__ void scan3_plane(const Params3& P, const RowRanges& R, const uint32_t* blo, float4 me,
                                            const float4* s_flat, u64m m[3], uint32_t la[3]) {
    const float lim = P.h2;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t len = R.hi[r] - R.lo[r];                           // <= 64 (caller)
        la[r] = row_la(R, blo, r);
        const float4* base = s_flat + la[r];
        uint32_t mlo = 0, mhi = 0, t = 0;
        // Two 32-bit shift registers, one v_addc_co per candidate (the 64-bit form needs two): candidates 0 .. 31 go
        // through `mhi`, the rest through `mlo` (len <= 64: the second limit never binds)
        scan3_word(mhi, t, 32u, base, len, me, lim);
        const uint32_t ta = t;                                            // <= 32: candidates that went through mhi
        scan3_word(mlo, t, 64u, base, len, me, lim);
        {   // candidate k sits at bit 63 - k: left-align each half, keep the lane's own len candidates
            const uint32_t hi32 = ta ? mhi << (32u - ta) : 0u;
            const uint32_t lo32 = t > ta ? mlo << (32u - (t - ta)) : 0u;
            u64m mask = ((u64m)hi32 << 32) | lo32;
            mask &= keep64(len);
            m[r] = mask;
        }
    }
}
// Rows of 65 .. 128 candidates (the compressing column: 5 % of the waves at step 60, 12 - 14 % from step 80 on,
// tools/rows3d_stats.py): the same hand-off with TWO 64-bit words per row — candidates 0 .. 63 in `hi` (stored in
// masks[0 .. 9n)), 64 .. 127 in `lo` (masks[9n .. 18n)).  plane_class(): 1 = every row of the wave <= 64, 2 = every row <= 128,
// 0 = the chunked sweep.  The producer and the consumers of the masks must agree: the one call is the driver's (sweep3_planes).
__device__ __forceinline__ int plane_class(const RowRanges& R, bool fit) {
    const uint32_t l0 = R.hi[0] - R.lo[0], l1 = R.hi[1] - R.lo[1], l2 = R.hi[2] - R.lo[2];
    const uint32_t mx = l0 > l1 ? (l0 > l2 ? l0 : l2) : (l1 > l2 ? l1 : l2);
    if (!fit) return 0;
    if (!__any(mx > 64u)) return 1;
    return !__any(mx > 128u) ? 2 : 0;
}
// One row of up to 128 candidates into four 32-bit shift registers (t is wave-uniform: the switches are scalar branches).
__device__ __forceinline__ void scan3_row128(const Params3& P, const float4* base, uint32_t len, float4 me, u64m* hi, u64m* lo) {
    const float lim = P.h2;
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u, t = 0u;
    scan3_word(w0, t, 32u, base, len, me, lim); const uint32_t t0 = t;
    scan3_word(w1, t, 64u, base, len, me, lim); const uint32_t t1 = t;
    scan3_word(w2, t, 96u, base, len, me, lim); const uint32_t t2 = t;
    scan3_word(w3, t, 128u, base, len, me, lim);
    // candidate c of the row sits at bit 31 - (c & 31) of word c / 32: left-align each word by the candidates it took
    const uint32_t a0 = t0 ? w0 << (32u - t0) : 0u, a1 = t1 > t0 ? w1 << (32u - (t1 - t0)) : 0u;
    const uint32_t a2 = t2 > t1 ? w2 << (32u - (t2 - t1)) : 0u, a3 = t > t2 ? w3 << (32u - (t - t2)) : 0u;
    u64m h = ((u64m)a0 << 32) | a1, l = ((u64m)a2 << 32) | a3;
    h &= keep128_hi(len);
    l &= keep128_lo(len);
    *hi = h; *lo = l;
}

// ---- the pass masks k3_density hands over (Params3::handoff) ------------------------------------------------------------
// Word w (0: candidates 0 .. 63, 1: 64 .. 127) of row r of plane `plane` of particle i in the 18 x n array.  k3_density stores
// through it, the two fetches below read through it: nothing else knows the layout.
__device__ __forceinline__ size_t mask3_slot(const Params3& P, int w, int plane, int r, uint32_t i) {
    return (size_t)(w * 9 + plane * 3 + r) * P.n + i;
}
// plane_class() == 1: the plane's three masks and the LDS index of each row's first candidate — handed over (`masks` non-null:
// three coalesced 8-byte loads, cut to the lane's own candidates; lanes past the end: len 0) or from a scan of the staged plane.
__device__ __forceinline__ void masks3_plane(const Params3& P, const u64m* __restrict__ masks, int plane, uint32_t ii,
                                             const RowRanges& R, const uint32_t* blo, float4 me, const float4* s_flat, u64m m[3],
                                             uint32_t la[3]) {
    if (!masks) return scan3_plane(P, R, blo, me, s_flat, m, la);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        la[r] = row_la(R, blo, r);
        m[r] = masks[mask3_slot(P, 0, plane, r, ii)] & keep64(R.hi[r] - R.lo[r]);
    }
}
// plane_class() == 2: the two words of row r, whose `len` candidates start at `base` — handed over or scanned.
__device__ __forceinline__ void masks3_row128(const Params3& P, const u64m* __restrict__ masks, int plane, int r, uint32_t ii,
                                              const float4* base, uint32_t len, float4 me, u64m* hi, u64m* lo) {
    if (!masks) return scan3_row128(P, base, len, me, hi, lo);
    *hi = masks[mask3_slot(P, 0, plane, r, ii)] & keep128_hi(len);
    *lo = masks[mask3_slot(P, 1, plane, r, ii)] & keep128_lo(len);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------
// The lane's particle: sorted slot i of the workgroup's block (lanes past the end work on the last particle, ii, and store
// nothing) and its {position, density} record.  false: the whole block is past the end (uniform).
struct Lane3 { uint32_t i, ii; bool live; float4 me; };
__device__ __forceinline__ bool sweep3_lane(const Params3& P, const float4* __restrict__ pred, Lane3* L) {
    uint32_t blk;
    if (!xcd_block3(P, (P.n + B3F - 1) / B3F, &blk)) return false;
    L->i = blk * B3F + threadIdx.x; L->live = L->i < P.n; L->ii = L->live ? L->i : P.n - 1;
    L->me = pred[L->ii];
    return true;
}
// The 27-cell sweep, plane by plane (z outer): the lane's three row ranges, the workgroup's bounds of each row [blo, bhi), whether
// they fit the tile and the wave's plane class go to the force-inlined body(plane, R, blo, bhi, fit, pclass); one barrier ends the
// plane (the next one reuses the pass's stage and s_red[24]).  The nine looked-up ranges are locals of THIS function, indexed here:
// handed to a helper by pointer they end up in scratch (96 B per kernel, k3_density 72 -> 54 VGPRs, k3_force 128 -> 107 / 109).
template <class Body>
__device__ __forceinline__ void sweep3_planes(const Params3& P, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ key_s,
                                              const Lane3& L, uint32_t* s_red, Body&& body) {
    uint32_t lo9[9], hi9[9];
    rows3_lookup(P, cs, key_s[L.ii], L.live, lo9, hi9);
#pragma unroll 1
    for (int plane = 0; plane < 3; ++plane) {
        RowRanges R;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            R.lo[r] = plane == 0 ? lo9[r] : plane == 1 ? lo9[3 + r] : lo9[6 + r];
            R.hi[r] = plane == 0 ? hi9[r] : plane == 1 ? hi9[3 + r] : hi9[6 + r];
        }
        uint32_t blo[3], bhi[3];
        const bool fit = block_tile_bounds<W3F>(R, s_red, blo, bhi, TILE3);
        body(plane, R, blo, bhi, fit, plane_class(R, fit));
        __syncthreads();
    }
}

}  // namespace fsd

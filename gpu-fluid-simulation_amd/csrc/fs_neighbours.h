// fs_neighbours.h — the neighbour walk of the 2D passes: the row ranges of the 3x3 sweep in the dense cell-start table, the stale-start
// quirk, the block-wide candidate tiles and their staging (the force pass stages for itself: kernels_force.hip), and the driver of the
// passes that add per-candidate terms: walk_lane, walk_bounds, walk_rows.  RowRanges / block_tile_bounds (shared with 3D): fs_device.h.
#pragma once
#include "fs_device.h"

namespace fsd {

#define FS_BLOCK 256

// ------------------------------------------------------------ neighbour ranges
// Cells (cx-1..cx+1, y) are consecutive ids, and particles are in id order, so a
// row of the 3x3 sweep is ONE contiguous index range [cs[id_lo], cs[id_lo+3]).
// Visiting it ascending is exactly the reference order (offset_x inner, index
// ascending: funcs.wgsl:161-199).
//
// Quirk: the cell of sorted index 0 never gets its start written
// (compute.wgsl:50), so the reference walks it from a stale start v.  Its
// particles are [0,cnt); the walk sees [min(v,cnt), cnt).  Any row range that
// begins at index 0 begins with that cell, so `lo == 0 -> lo = lo_fix`.
__device__ __forceinline__ uint32_t quirk_lo_fix(const StepParams& P, const u64* __restrict__ pairs,
                                                 const uint32_t* __restrict__ cs,
                                                 const uint32_t* __restrict__ start_ref) {
    if (!P.ref_quirks) return 0u;
    const uint32_t cmin = (uint32_t)(pairs[0] >> 32);
    if (cmin >= P.ncell) return 0u;
    const uint32_t v = start_ref[cmin];
    const uint32_t cnt = cs[cmin + 1];
    return v < cnt ? v : cnt;
}

// (row_range and lane_row_ranges are __host__ too: tests/row_ranges_checker.hip sweeps them against each other on the CPU.)
// (cx, y) are the cell's (u, v) of the handle's id layout (fs_device.h StepParams::transposed; the reference layout: u = x, v = y).
__host__ __device__ __forceinline__ bool row_range(const StepParams& P, const uint32_t* __restrict__ cs, uint32_t cx,
                                          uint32_t y, uint32_t lo_fix, uint32_t* lo, uint32_t* hi) {
    if (y >= P.grid_v) return false;             // id >= ncell: OOB start_indices read -> nothing
    const uint32_t id_lo = y * P.grid_u + cx - 1u;
    if (id_lo >= P.ncell) return false;
    uint32_t id_hi = id_lo + 3u;
    if (id_hi > P.ncell) id_hi = P.ncell;
    uint32_t a = cs[id_lo];
    const uint32_t b = cs[id_hi];
    if (a == 0u) a = lo_fix;
    *lo = a;
    *hi = b;
    return a < b;
}

// The lane's three row ranges: rows cy - 1, cy, cy + 1 of the sweep around its cell (cx, cy).  A dead lane, a row outside the grid
// and an empty row all come back as lo == hi.  Same integers as three row_range() calls, without their branches: a row that
// row_range() refuses (dead lane, y >= grid_v, id_lo >= ncell — the wrapped cy - 1 and cx - 1 included) reads entry 0 instead, which
// is always there (cs has ncell + 1 entries), so the six loads depend on nothing but the cell and are all in flight together —
// one round trip to the cell table per lane instead of three.  The selects come after the loads.
__host__ __device__ __forceinline__ RowRanges lane_row_ranges(const StepParams& P, const uint32_t* cs, uint32_t lo_fix, uint32_t cx,
                                                     uint32_t cy, bool live) {
    RowRanges R;
    bool ok[3];
    uint32_t a[3], b[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t y = cy + (uint32_t)(r - 1);
        const uint32_t id_lo = y * P.grid_u + cx - 1u;
        ok[r] = live && y < P.grid_v && id_lo < P.ncell;
        uint32_t id_hi = id_lo + 3u;
        if (id_hi > P.ncell) id_hi = P.ncell;
        a[r] = cs[ok[r] ? id_lo : 0u];
        b[r] = cs[ok[r] ? id_hi : 0u];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        uint32_t lo = a[r] == 0u ? lo_fix : a[r];
        uint32_t hi = b[r];
        if (!ok[r]) { lo = 0u; hi = 0u; }
        R.lo[r] = lo;
        R.hi[r] = hi < lo ? lo : hi;
    }
    return R;
}

// ------------------------------------------------------------ block neighbour tiles
// A workgroup owns 256 consecutive sorted particles (a strip of cells in one grid row), so
// the candidates of ALL its lanes for sweep row r form one short contiguous index range
// [blo_r, bhi_r).  The three ranges are staged into LDS with coalesced loads once and the
// per-lane loops then read LDS instead of issuing one gather per candidate.  Strips that
// straddle a grid-row end (or very sparse ones) exceed the tile and take the global path.
#define NB_TILE 640          // staged candidates per sweep row
#ifndef NBF_TILE
#define NBF_TILE 544         // ... of the force pass (k_force).  384 (round 2) left the blocks of the fluid's free surface — half-empty
                             // cells: 256 particles span 128 cells and their full neighbour row holds 516 - 526 — to the general
                             // kernel's unstaged sweep: 32 blocks per step at 16 M even on the lattice, a ~15 us tail behind the
                             // lean kernel in every step (force 0.603 -> 0.595 ms at 16 M; more at 1 M and per slab rank)
#endif

// Staging the three block-wide ranges, in two halves: every global load of the three rows goes to registers first
// (stage_rows_load), the LDS writes follow (stage_rows_store), so a thread's loads are all in flight at once instead of one
// load - wait - write round trip per 256 candidates of a row.  A tile is at most FS_STAGE_TRIPS x 256 entries, so the trips are
// unrolled: 3 rows x 3 trips of T in registers between the halves, most of them predicated off (a row holds 260 - 300
// candidates in the fluid's bulk).  `fetch(k)` reads what is staged of candidate k, `put(r, j, v)` writes it to slot j of row r.
#define FS_STAGE_TRIPS 3
static_assert(NB_TILE <= FS_STAGE_TRIPS * FS_BLOCK && NBF_TILE <= FS_STAGE_TRIPS * FS_BLOCK,
              "stage_rows_load / stage_rows_store cover a tile in FS_STAGE_TRIPS trips of the workgroup");
template <typename T> struct StagedRows { T v[3][FS_STAGE_TRIPS]; };

template <typename T, typename Fetch>
__device__ __forceinline__ void stage_rows_load(StagedRows<T>& S, const uint32_t* blo, const uint32_t* bhi, Fetch fetch) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int t = 0; t < FS_STAGE_TRIPS; ++t) {
            const uint32_t j = threadIdx.x + (uint32_t)t * FS_BLOCK;
            if (j < bhi[r] - blo[r]) S.v[r][t] = fetch(blo[r] + j);
        }
}
template <typename T, typename Put>
__device__ __forceinline__ void stage_rows_store(const StagedRows<T>& S, const uint32_t* blo, const uint32_t* bhi, Put put) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int t = 0; t < FS_STAGE_TRIPS; ++t) {
            const uint32_t j = threadIdx.x + (uint32_t)t * FS_BLOCK;
            if (j < bhi[r] - blo[r]) put(r, j, S.v[r][t]);
        }
}

// The density -> force hand-off (fs_device.h StepParams::block_bounds): the 8-word record of block `blk` holds the block-wide
// ranges as [lo0, lo1, lo2, hi0, hi1, hi2].
__device__ __forceinline__ void store_block_bounds(const StepParams& P, uint32_t blk, const uint32_t* blo, const uint32_t* bhi) {
    uint32_t* bb = P.block_bounds + 8u * blk;
    bb[0] = blo[0]; bb[1] = blo[1]; bb[2] = blo[2]; bb[3] = bhi[0]; bb[4] = bhi[1]; bb[5] = bhi[2];
}
__device__ __forceinline__ void load_block_bounds(const StepParams& P, uint32_t blk, uint32_t* blo, uint32_t* bhi) {
    const uint32_t* bb = P.block_bounds + 8u * blk;
    blo[0] = bb[0]; blo[1] = bb[1]; blo[2] = bb[2]; bhi[0] = bb[3]; bhi[1] = bb[4]; bhi[2] = bb[5];
}

// The record's ranges, and whether all three fit a tile of `tile` entries (what block_tile_bounds() says of the same ranges).
__device__ __forceinline__ bool recorded_tile_bounds(const StepParams& P, uint32_t blk, uint32_t* blo, uint32_t* bhi, uint32_t tile) {
    load_block_bounds(P, blk, blo, bhi);
    return bhi[0] - blo[0] <= tile && bhi[1] - blo[1] <= tile && bhi[2] - blo[2] <= tile;
}

// ------------------------------------------------------------ the driver
// A pass that adds per-candidate terms over the rows the density pass visits (k_density / k_density_edge and k_surface_tension,
// kernels_density.hip; k_diffuse, kernels_diffuse.hip) is its terms object plus walk_lane, walk_bounds and walk_rows, once each.
// The 3D counterpart is fs_sweep3.h (sweep3_lane / sweep3_planes).
// The lane of block `blk` of n particles: sorted slot i, its position, its cell — (u, v) of the cell-id layout: (x, y) unless the
// handle is a transposed slab rank — and its three row ranges.  A dead lane (i >= n) shadows particle ii = n - 1: it loads what a
// live lane loads, walks nothing (`live` goes into lane_row_ranges), reaches every barrier and stores nothing: the pass returns on
// !live after walk_rows.  walk_lane is its two halves in a row; a pass with more to load of particle ii (k_diffuse: its channel
// values) calls the halves itself and loads in between, in flight with `me` and ahead of the round trips to the cell table.
struct WalkLane { uint32_t i, ii; bool live; float2 me; uint32_t lo_fix, cx, cy; int32_t cg; RowRanges R; };
__device__ __forceinline__ WalkLane walk_lane_particle(uint32_t blk, uint32_t n, const float2* __restrict__ pred) {
    WalkLane L;
    L.i = blk * FS_BLOCK + threadIdx.x; L.live = L.i < n; L.ii = L.live ? L.i : n - 1;
    L.me = pred[L.ii];              // issued first: the quirk's two dependent scalar loads run beside it
    return L;
}
__device__ __forceinline__ void walk_lane_rows(const StepParams& P, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                               const u64* __restrict__ pairs, WalkLane& L) {
    L.lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
    uv_local(P, L.me, &L.cx, &L.cy, &L.cg);
    L.R = lane_row_ranges(P, cs, L.lo_fix, L.cx, L.cy, L.live);
}
__device__ __forceinline__ WalkLane walk_lane(const StepParams& P, uint32_t blk, uint32_t n, const float2* __restrict__ pred,
                                              const uint32_t* __restrict__ cs, const uint32_t* __restrict__ start_ref,
                                              const u64* __restrict__ pairs) {
    WalkLane L = walk_lane_particle(blk, n, pred);
    walk_lane_rows(P, cs, start_ref, pairs, L);
    return L;
}

// The block-wide ranges and whether all three fit a tile of `tile` entries.  RECORDED: the record of this step's density pass where there
// is one (it reduced the same ranges over the same 256 particles), else reduced over s_red[24], as the density pass itself always does.
template <bool RECORDED> __device__ __forceinline__ bool walk_bounds(const StepParams& P, uint32_t blk, const RowRanges& R, uint32_t* s_red,
                                                                     uint32_t* blo, uint32_t* bhi, uint32_t tile) {
    if (RECORDED && P.block_bounds) return recorded_tile_bounds(P, blk, blo, bhi, tile);
    return block_tile_bounds(R, s_red, blo, bhi, tile);
}

// The walk: candidates row by row, index ascending.  `fit`: the three block-wide rows go to LDS in two halves (above) and, behind
// the barrier, every lane's terms come from there; else every lane sweeps its own ranges in global memory.  Terms has
//   fetch(k)        what is staged of candidate k, read from global memory
//   put(r, j, c)    write it to slot j of row r in LDS
//   row(r, k, hi)   the terms of the staged candidates in slots [k, hi) of row r: the pass's own unrolling, adds in index order
//   one(k)          the terms of candidate k from global memory
// PRIO: the level the kernel raised its waves to for the load phase, or 0 (fs_device.h); lowered where that phase ends.
template <int PRIO, class Terms>
__device__ __forceinline__ void walk_rows(const RowRanges& R, const uint32_t* blo, const uint32_t* bhi, bool fit, Terms& T) {
    if (fit) {
        StagedRows<decltype(T.fetch(0u))> S;
        stage_rows_load(S, blo, bhi, [&](uint32_t k) { return T.fetch(k); });
        stage_rows_store(S, blo, bhi, [&](int r, uint32_t j, const decltype(T.fetch(0u))& c) { T.put(r, j, c); });
        __syncthreads();
        wave_prio_lower<PRIO>();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const bool any = R.lo[r] < R.hi[r];
            const uint32_t hi = any ? R.hi[r] - blo[r] : 0u, k = any ? R.lo[r] - blo[r] : 0u;
            T.row(r, k, hi);
        }
    } else {
        wave_prio_lower<PRIO>();
#pragma unroll
        for (int r = 0; r < 3; ++r)
            for (uint32_t k = R.lo[r]; k < R.hi[r]; ++k) T.one(k);
    }
}

// The neighbour weight w_j = m / rho_j of the passes behind the density pass, in two halves, so that the staging loads every
// candidate's operand before it forms the first weight: the one word read per candidate, and the weight from it.
template <bool MASS1> __device__ __forceinline__ float walk_weight_operand(const float2* __restrict__ rho2, const float* __restrict__ rho_arr, uint32_t j) {
    if (MASS1) return rho2[j].y;                    // +-RN(1/rho_j): the sign is the density pass's safe bit
    return rho_arr ? rho_arr[j] : rho2[j].x;        // rho_j.  rho_arr: tolerance mode (rho2 = {pressure, 1/rho})
}
template <bool MASS1> __device__ __forceinline__ float walk_weight_of(const StepParams& P, float d) {
    if (MASS1) return fabsf(d);                     // RN(1/rho_j) == RN(1.0f / rho_j)
    return __fdiv_rn(P.mass, d);
}

struct AosParticle { float2 position, predicted, velocity; float density; uint32_t grid; };   // ParticleInstance, 32 B

}  // namespace fsd

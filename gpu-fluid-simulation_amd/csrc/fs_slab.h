// fs_slab.h — device helpers of the slab kernels only (kernels_slab.hip, kernels_strip.hip, and k_cs_fixreorder<true>'s owned
// flag): the cell key inside a rank's window, the global column of a stored key, the halo / leaver rules of the pack and the
// reader of a received record.  (slab_advances and EdgeBlocks live in fs_device.h: the density and force passes use them.)
#pragma once
#include "fs_device.h"

namespace fsd {

#define SL_BLOCK 256
static inline uint32_t sl_blocks(uint32_t n) { return (n + SL_BLOCK - 1) / SL_BLOCK; }

// Cell key of a predicted position inside the window (owned + 2 ghost columns per side), DEAD outside it.
__device__ __forceinline__ uint32_t slab_key(const StepParams& P, float2 pred, uint32_t* cx_global) {
    uint32_t cx, cy;
    xy_of_point(P, pred, &cx, &cy);
    *cx_global = cx;
    const int32_t lo = (int32_t)P.own_lo - 2, hi = (int32_t)P.own_hi + 2;
    if ((int32_t)cx < lo || (int32_t)cx >= hi || cy >= P.grid_h) return FS_DEAD_KEY;
    return key_of_local(P, (uint32_t)((int32_t)cx - P.col_origin), cy);
}
// Global column (and row) of a stored key; is that column owned?
__device__ __forceinline__ int32_t global_col(const StepParams& P, uint32_t key, uint32_t* cy_out = nullptr) {
    uint32_t cxl, cy;
    key_to_local(P, key, &cxl, &cy);
    if (cy_out) *cy_out = cy;
    return (int32_t)cxl + P.col_origin;
}
__device__ __forceinline__ bool owns_col(const StepParams& P, int32_t cg) { return cg >= (int32_t)P.own_lo && cg < (int32_t)P.own_hi; }

// EdgeBlocks of the edge columns (`edges`; cs: the cell table, column-major ids) or of all `nblocks` blocks.
__device__ __forceinline__ EdgeBlocks edge_blocks_or_all(const StepParams& P, bool edges, const uint32_t* __restrict__ cs, uint32_t nblocks) {
    EdgeBlocks E;
    E.eL = 0u; E.eR = 0u; E.nb = nblocks;
    if (edges) E = edge_blocks(P, cs, *P.n_live, 0u);
    return E;
}

// Which neighbours need an owned particle predicted into global column cxg (bit 0: left, bit 1: right): migrants and the
// 2-column ghost halo.  (A leaver must land inside the neighbour's slab and not in ITS far halo: checked by the receiver.)
__device__ __forceinline__ unsigned char halo_flags(const StepParams& P, uint32_t cxg, bool has_left, bool has_right) {
    unsigned char f = 0;
    if (has_left && cxg < P.own_lo + 2u) f |= 1;
    if (has_right && cxg + 2u >= P.own_hi) f |= 2;
    return f;
}
// ... and one that leaves the window where there is no neighbour has left the domain partition: `lost`.
__device__ __forceinline__ void count_leavers(const StepParams& P, uint32_t cxg, bool has_left, bool has_right, uint32_t* __restrict__ counters) {
    if (!has_left && cxg < P.own_lo) atomicAdd(&counters[2], 1u);
    if (!has_right && cxg >= P.own_hi) atomicAdd(&counters[2], 1u);
}

// A message: 16-byte header, then R records {pos, vel}.
struct SlabHeader { uint32_t count, overflow, pad0, pad1; };
static inline float4* records(const SlabHeader* h) { return h ? (float4*)(h + 1) : nullptr; }

// Thread j of an unpack launch over both messages (left: j in [0, R), right: [R, 2R)).  The constructor picks the side, clamps
// the header's count to R and counts a set overflow flag once per message; read() — only where has() — copies the record to
// where the kernel wants it, returns its key (slab_key) and counts what both unpack kernels count: a record beyond window + halo (`lost`) and a migrant that lands
// in the two owned columns at the FAR edge, which the other neighbour would have needed as well (`far_halo`).
struct ReceivedRecord {
    bool in_range, right;
    uint32_t jj, cnt;
    const float4* rec;
    __device__ __forceinline__ ReceivedRecord(uint32_t j, uint32_t R, const SlabHeader* __restrict__ hdr_left, const float4* __restrict__ rec_left,
                                              const SlabHeader* __restrict__ hdr_right, const float4* __restrict__ rec_right,
                                              uint32_t* __restrict__ counters)
        : in_range(j < 2u * R), right(j >= R), jj(right ? j - R : j), cnt(0), rec(right ? rec_right : rec_left) {
        const SlabHeader* hdr = right ? hdr_right : hdr_left;
        if (in_range && hdr) { cnt = hdr->count < R ? hdr->count : R; if (jj == 0 && hdr->overflow) atomicAdd(&counters[3], 1u); }
    }
    __device__ __forceinline__ bool has() const { return in_range && jj < cnt; }
    __device__ __forceinline__ uint32_t read(const StepParams& P, float2* __restrict__ pos_to, float2* __restrict__ vel_to, uint32_t* __restrict__ counters, uint32_t* cx_global) const {
        const float4 r = rec[jj];
        const float2 pos = make_float2(r.x, r.y), vel = make_float2(r.z, r.w);
        *pos_to = pos;
        *vel_to = vel;
        uint32_t cxg;
        const uint32_t key = slab_key(P, predict_pos(P, pos, vel), &cxg);
        if (key == FS_DEAD_KEY) atomicAdd(&counters[2], 1u);
        if (!right && cxg + 2u >= P.own_hi && cxg < P.own_hi) atomicAdd(&counters[4], 1u);
        if (right && cxg < P.own_lo + 2u && cxg >= P.own_lo) atomicAdd(&counters[4], 1u);
        *cx_global = cxg;
        return key;
    }
};

}  // namespace fsd

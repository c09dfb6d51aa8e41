// fs_sample3.h — what the two 3D samplers share (kernels_sample3d.hip: k3_sample, the fs3_sample records; kernels_sample_attr3d.hip:
// k3_sample_attr, the tracking channels): the workgroup size and the wave tiles a grid of voxels is taken in.  One lane per query in
// both, so the ORDER of the queries decides the speed: lanes of a wave that fall into the same or adjacent cells walk the same cache
// lines and leave the loops together, and a grid is therefore taken in wave tiles that are compact in every axis that has extent.
#pragma once
#include "fs_3d.h"

namespace fsd {

#define B3S 256                    // workgroup: four waves, one query per lane

// The 256 threads of a workgroup over a GRID tile: the low bits of the lane (then of the wave) number go to x, the next to y,
// the rest to z.  lane = log2 extents of a wave's tile (they sum to 6), wave = those of the 2 x 2 (x 1) waves of a workgroup.
struct Sample3Tile {
    uint32_t lx, ly, wx, wy;       // log2: lane bits in x, in y (z: the rest); wave bits in x, in y (z: the rest)
    uint32_t tx, ty, tz;           // log2 extents of the workgroup's tile
    uint32_t nbx, nby;             // workgroup tiles along x, along y
};

// The voxel of this thread in a GRID launch and its centre (fs_sample_grid's expression per axis); false: the thread lies in the
// masked part of an edge tile.
__device__ __forceinline__ bool sample3_tile_voxel(const Sample3Tile& T, float3 wmin, float3 wmax, uint32_t width, uint32_t height,
                                                   uint32_t depth, size_t* q, float* x, float* y, float* z) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bi = blockIdx.x % T.nbx, bj = (blockIdx.x / T.nbx) % T.nby, bk = blockIdx.x / (T.nbx * T.nby);
    const uint32_t i = (bi << T.tx) + ((wave & ((1u << T.wx) - 1u)) << T.lx) + (lane & ((1u << T.lx) - 1u));
    const uint32_t j = (bj << T.ty) + (((wave >> T.wx) & ((1u << T.wy) - 1u)) << T.ly) + ((lane >> T.lx) & ((1u << T.ly) - 1u));
    const uint32_t k = (bk << T.tz) + ((wave >> (T.wx + T.wy)) << (6u - T.lx - T.ly)) + (lane >> (T.lx + T.ly));
    if (i >= width || j >= height || k >= depth) return false;        // edge tiles are masked
    *q = ((size_t)k * height + j) * width + i;
    *x = wmin.x + __fdiv_rn((float)i + 0.5f, (float)width) * (wmax.x - wmin.x);
    *y = wmin.y + __fdiv_rn((float)j + 0.5f, (float)height) * (wmax.y - wmin.y);
    *z = wmin.z + __fdiv_rn((float)k + 0.5f, (float)depth) * (wmax.z - wmin.z);
    return true;
}

// The wave tile of a view: six lane bits dealt round-robin (x, y, z) to the axes that have extent — 4 x 4 x 4 voxels for a
// volume, 8 x 8 for a slice, 64 in a row for a line —, then the two wave bits of the workgroup the same way (8 x 8 x 4,
// 16 x 16, 256).
inline Sample3Tile sample3_tile(uint32_t width, uint32_t height, uint32_t depth) {
    const bool has[3] = {width > 1u, height > 1u || (width <= 1u && depth <= 1u), depth > 1u};
    uint32_t lane[3] = {0, 0, 0}, wave[3] = {0, 0, 0};
    int a = 0;
    for (int bit = 0; bit < 8; ++bit) {
        while (!has[a]) a = (a + 1) % 3;
        (bit < 6 ? lane : wave)[a] += 1u;
        a = (a + 1) % 3;
    }
    Sample3Tile T;
    T.lx = lane[0]; T.ly = lane[1]; T.wx = wave[0]; T.wy = wave[1];
    T.tx = lane[0] + wave[0]; T.ty = lane[1] + wave[1]; T.tz = lane[2] + wave[2];
    T.nbx = (width + (1u << T.tx) - 1u) >> T.tx;
    T.nby = (height + (1u << T.ty) - 1u) >> T.ty;
    return T;
}
// Workgroups of a GRID launch over the view the tile was made for.
inline uint32_t sample3_tile_blocks(const Sample3Tile& T, uint32_t depth) {
    return T.nbx * T.nby * ((depth + (1u << T.tz) - 1u) >> T.tz);
}

}  // namespace fsd

// kernels_collide3d.hip — producer of the 3D collider (build extension): a w x h x d u8 voxel mask (> 128: solid,
// the threshold of the 2D producer, src/main.rs:403-515) to the push field of the force pass's COLLIDE tail (kernels_force3d.hip
// collide3) by an EXACT Euclidean distance transform in index space.  Three separable passes in u32 arithmetic, stated in
// include/fluidsim.h "3D colliders"; the result is fully determined, ties included:
//   k3c_pass_x  per row (j, k):    the free i' minimising |i - i'|
//   k3c_pass_y  per column (i, k): over the rows' answers, minimising (x - i)^2 + (j' - j)^2
//   k3c_pass_z  per pillar (i, j): over the columns' answers, minimising (x - i)^2 + (y - j)^2 + (k' - k)^2 -> the push vector
// One line per workgroup, staged in LDS (an extent is at most COLLIDER3_MAX_EXTENT of fs_3d.h),
// targets beyond the workgroup looped, brute force over the line
// in ascending order with a strict `<`: ties go to the smaller coordinate.  No atomics, no waiting between workgroups; off the step
// path.  Squared index distances are at most 3 * 1023^2 < 2^22.
#include <hip/hip_runtime.h>

#include "fs_3d.h"

namespace fsd {

#define B3X 256
#define C3_NONE 0xFFFFFFFFu      // no free voxel in the line(s) so far

__device__ __forceinline__ uint32_t sq_diff(uint32_t a, uint32_t b) { const uint32_t d = a > b ? a - b : b - a; return d * d; }

__global__ __launch_bounds__(B3X) void k3c_pass_x(const uint8_t* __restrict__ mask, uint32_t w, uint32_t* __restrict__ near_x) {
    __shared__ uint32_t s_free[COLLIDER3_MAX_EXTENT];
    const size_t base = (size_t)blockIdx.x * w;                          // row (j, k) = blockIdx.x: contiguous
    for (uint32_t t = threadIdx.x; t < w; t += B3X) s_free[t] = mask[base + t] > 128 ? 0u : 1u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < w; i += B3X) {
        uint32_t best = C3_NONE, bd = C3_NONE;
        for (uint32_t t = 0; t < w; ++t) {
            const uint32_t d = t > i ? t - i : i - t;
            if (s_free[t] && d < bd) { bd = d; best = t; }
        }
        near_x[base + i] = best;
    }
}

__global__ __launch_bounds__(B3X) void k3c_pass_y(const uint32_t* __restrict__ near_x, uint32_t w, uint32_t h,
                                                  uint32_t* __restrict__ near_xy) {
    __shared__ uint32_t s_x[COLLIDER3_MAX_EXTENT];
    const uint32_t i = blockIdx.x % w, k = blockIdx.x / w;               // column (i, k): stride w
    const size_t base = (size_t)k * h * w + i;
    for (uint32_t t = threadIdx.x; t < h; t += B3X) s_x[t] = near_x[base + (size_t)t * w];
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < h; j += B3X) {
        uint32_t best = C3_NONE, bd = C3_NONE;
        for (uint32_t t = 0; t < h; ++t) {
            const uint32_t x = s_x[t];
            const uint32_t d = sq_diff(x & 0xFFFFu, i) + sq_diff(t, j);  // x == NONE: masked below
            if (x != C3_NONE && d < bd) { bd = d; best = x | (t << 16); }
        }
        near_xy[base + (size_t)j * w] = best;
    }
}

__global__ __launch_bounds__(B3X) void k3c_pass_z(const uint32_t* __restrict__ near_xy, uint32_t w, uint32_t h, uint32_t d,
                                                  float vx, float vy, float vz, float4* __restrict__ field) {
    __shared__ uint32_t s_xy[COLLIDER3_MAX_EXTENT];
    const uint32_t i = blockIdx.x % w, j = blockIdx.x / w;               // pillar (i, j): stride w * h
    const size_t base = (size_t)j * w + i, plane = (size_t)w * h;
    for (uint32_t t = threadIdx.x; t < d; t += B3X) s_xy[t] = near_xy[base + t * plane];
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < d; k += B3X) {
        uint32_t bx = i, by = j, bz = k, bd = C3_NONE;                   // no free voxel anywhere (the host refuses it): +0
        for (uint32_t t = 0; t < d; ++t) {
            const uint32_t xy = s_xy[t], x = xy & 0xFFFFu, y = xy >> 16;
            const uint32_t dd = sq_diff(x, i) + sq_diff(y, j) + sq_diff(t, k);
            if (xy != C3_NONE && dd < bd) { bd = dd; bx = x; by = y; bz = t; }
        }
        float4 f;
        f.x = (float)((int)bx - (int)i) * vx; f.y = (float)((int)by - (int)j) * vy; f.z = (float)((int)bz - (int)k) * vz;
        f.w = 0.0f;
        field[base + k * plane] = f;
    }
}

void launch3_collider_from_mask(hipStream_t st, const ColliderMask3& Q) {
    hipLaunchKernelGGL(k3c_pass_x, dim3(Q.h * Q.d), dim3(B3X), 0, st, Q.mask, Q.w, Q.near_x);
    hipLaunchKernelGGL(k3c_pass_y, dim3(Q.w * Q.d), dim3(B3X), 0, st, Q.near_x, Q.w, Q.h, Q.near_xy);
    hipLaunchKernelGGL(k3c_pass_z, dim3(Q.w * Q.h), dim3(B3X), 0, st, Q.near_xy, Q.w, Q.h, Q.d, Q.vx, Q.vy, Q.vz, Q.field);
}

}  // namespace fsd

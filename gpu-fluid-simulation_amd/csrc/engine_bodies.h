// engine_bodies.h — what engine_features.hip (the 2D handle) and engine_3d_features.hip (the 3D handle) share of the moving
// bodies and of the mask producer behind them and the 3D colliders (§18), beyond BodySlots and BodyLoads in engine.h:
// plain functions over the pieces of a handle they work on.  Each handle's file keeps its entry points, the order of its checks
// and its messages.
#pragma once
#include <cmath>

#include "engine.h"
#include "fs_3d.h"

namespace fsd {

// n packed floats: every one finite (a motion) ...
inline bool all_finite(const float* f, int n) {
    for (int k = 0; k < n; ++k) if (!std::isfinite(f[k])) return false;
    return true;
}
// ... every one finite and > 0 (the extent of a body's box)
inline bool all_positive(const float* f, int n) {
    for (int k = 0; k < n; ++k) if (!(std::isfinite(f[k]) && f[k] > 0.0f)) return false;
    return true;
}

// a mask the producer accepts: some pixel or voxel is free (not > 128)
inline bool mask_has_free(const uint8_t* mask, size_t cells) {
    for (size_t k = 0; k < cells; ++k) if (!(mask[k] > 128)) return true;
    return false;
}

// The producer's staging and scratch for a mask of `cells`; they live for the call that makes them.
struct MaskStaging {
    DevArray<uint8_t> mask;
    DevArray<uint32_t> near_x, near_xy;
    hipError_t alloc(size_t cells) {
        hipError_t e = mask.alloc(cells);
        if (e == hipSuccess) e = near_x.alloc(cells);
        return e == hipSuccess ? near_xy.alloc(cells) : e;
    }
};

// The producer of §18 on a host mask, blocking: the push field of a w x h x d mask over a box of `size` into `field` (device,
// w * h * d vectors).  The stream is synchronised before the caller frees the staging, whatever happened.
inline fs_status mask_to_field3(hipStream_t st, const uint8_t* mask, uint32_t w, uint32_t h, uint32_t d, fs_vec3 size, float4* field,
                                const MaskStaging& stage) {
    ColliderMask3 Q;
    Q.mask = stage.mask.p; Q.w = w; Q.h = h; Q.d = d;
    Q.vx = size.x / (float)w; Q.vy = size.y / (float)h; Q.vz = size.z / (float)d;
    Q.near_x = stage.near_x.p; Q.near_xy = stage.near_xy.p; Q.field = field;
    hipError_t e = hipMemcpyAsync(stage.mask.p, mask, (size_t)w * h * d, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { launch3_collider_from_mask(st, Q); e = hipGetLastError(); }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? FS_OK : fail(FS_ERR_DEVICE, hipGetErrorString(e));
}

}  // namespace fsd

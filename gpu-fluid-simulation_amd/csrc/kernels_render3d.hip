// kernels_render3d.hip — 3D surface rendering (build extension): one ray per pixel marched through the density
// field of the 3D fluid until it crosses `iso`, the crossing refined by bisection, and ONE full field sample (kernels_sample3d.hip's
// statement: density, gradient, Shepard velocity) at the hit.  Reads the cell-sorted state the last step left on the device
// (pred with the density in .w, vel, cs).  No reference counterpart (the reference is 2D only).
//
// Statement (include/fluidsim.h "3D surface rendering"), f32 without contraction, sqrt and / correctly rounded, pixel (i, j):
//   u = ((float)i + 0.5f) / (float)width - 0.5f;  v likewise with j and height
//   perspective:  o = eye;  D.a = (forward.a + u * right.a) + v * up.a        orthographic:  o.a = (eye.a + u * right.a) + v * up.a;  D = forward
//   len = sqrt((D.x*D.x + D.y*D.y) + D.z*D.z);  d.a = D.a / len;  x(t).a = o.a + t * d.a;  t_k = t_near + (float)k * ds
//   K = the smallest k < max_steps with density(x(t_k)) >= iso;  none: a miss;  K == 0: t = t_0, hit 2;
//   else lo = t_{K-1}, hi = t_K, `refine` times mid = 0.5f * (lo + hi), density(x(mid)) >= iso ? hi = mid : lo = mid;  t = hi, hit 1
//   S = sample(x(t));  normal = -S.gradient / |S.gradient|;  velocity = S.velocity / S.weight
//
// One lane per ray keeps every sum in the statement's order.  A wave is an 8 x 8 pixel tile and a workgroup of four waves
// 16 x 16 (the slice tile of sample3_tile), so the lanes of a wave walk the same or adjacent cells at every march step.  The
// march evaluates the density only: the nine row ranges of the 27-cell walk are read first (18 independent loads of cs), a
// sample whose ranges are all empty is +0 < iso and costs nothing more, and a candidate costs one 16-byte load of pred: no
// velocity, no division.  The full sample runs once per hit ray, in k3_sample's expression order.
//
// The two walks (density3_at, sample3_at) live in fs_field3.h, shared with the surface extractor (kernels_mesh3d.hip).
#include "fs_field3.h"

namespace fsd {

struct SurfaceHit3 {               // fs3_surface_hit (include/fluidsim.h), 40 bytes
    float t, density, nx, ny, nz, vx, vy, vz;
    uint32_t steps, hit;
};
static_assert(sizeof(SurfaceHit3) == 40, "fs3_surface_hit is 40 bytes");

#define B3R 256                    // workgroup: four waves of 8 x 8 pixels, 16 x 16

template <bool ORTHO>
__global__ __launch_bounds__(B3R) void k3_render_surface(Params3 P, Surface3Query Q, uint32_t nbx,
                                                              const float4* __restrict__ pred, const float4* __restrict__ vel,
                                                              const uint32_t* __restrict__ cs, SurfaceHit3* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bi = blockIdx.x % nbx, bj = blockIdx.x / nbx;
    const uint32_t i = (bi << 4) + ((wave & 1u) << 3) + (lane & 7u);
    const uint32_t j = (bj << 4) + ((wave >> 1) << 3) + (lane >> 3);
    if (i >= Q.width || j >= Q.height) return;                      // edge tiles are masked
    const float u = __fdiv_rn((float)i + 0.5f, (float)Q.width) - 0.5f;
    const float v = __fdiv_rn((float)j + 0.5f, (float)Q.height) - 0.5f;
    float ox, oy, oz, Dx, Dy, Dz;
    if (ORTHO) {
        ox = (Q.eye.x + u * Q.right.x) + v * Q.up.x; oy = (Q.eye.y + u * Q.right.y) + v * Q.up.y; oz = (Q.eye.z + u * Q.right.z) + v * Q.up.z;
        Dx = Q.forward.x; Dy = Q.forward.y; Dz = Q.forward.z;
    } else {
        ox = Q.eye.x; oy = Q.eye.y; oz = Q.eye.z;
        Dx = (Q.forward.x + u * Q.right.x) + v * Q.up.x; Dy = (Q.forward.y + u * Q.right.y) + v * Q.up.y; Dz = (Q.forward.z + u * Q.right.z) + v * Q.up.z;
    }
    const float len = sqrt_rn((Dx * Dx + Dy * Dy) + Dz * Dz);
    const float dx = __fdiv_rn(Dx, len), dy = __fdiv_rn(Dy, len), dz = __fdiv_rn(Dz, len);
    const float iso = Q.iso;
    // the march: the first k whose sample reaches iso
    uint32_t K = 0u;
    for (; K < Q.max_steps; ++K) {
        const float t = Q.t_near + (float)K * Q.ds;                 // a product, never a running sum
        if (density3_at(P, ox + t * dx, oy + t * dy, oz + t * dz, pred, cs) >= iso) break;
    }
    SurfaceHit3 r;
    r.t = 0.0f; r.density = 0.0f; r.nx = 0.0f; r.ny = 0.0f; r.nz = 0.0f; r.vx = 0.0f; r.vy = 0.0f; r.vz = 0.0f;
    r.steps = K; r.hit = 0u;
    if (K < Q.max_steps) {
        float t = Q.t_near + (float)K * Q.ds;
        r.hit = 2u;
        if (K > 0u) {
            float lo = Q.t_near + (float)(K - 1u) * Q.ds, hi = t;
            for (uint32_t b = 0u; b < Q.refine; ++b) {
                const float mid = 0.5f * (lo + hi);
                if (density3_at(P, ox + mid * dx, oy + mid * dy, oz + mid * dz, pred, cs) >= iso) hi = mid; else lo = mid;
            }
            t = hi;
            r.hit = 1u;
        }
        const FullSample3 S = sample3_at(P, ox + t * dx, oy + t * dy, oz + t * dz, pred, vel, cs);
        const float gl = sqrt_rn((S.gx * S.gx + S.gy * S.gy) + S.gz * S.gz);
        r.t = t; r.density = S.density;
        if (gl > 0.0f) { r.nx = __fdiv_rn(-S.gx, gl); r.ny = __fdiv_rn(-S.gy, gl); r.nz = __fdiv_rn(-S.gz, gl); }
        if (S.weight > 0.0f) { r.vx = __fdiv_rn(S.vx, S.weight); r.vy = __fdiv_rn(S.vy, S.weight); r.vz = __fdiv_rn(S.vz, S.weight); }
    }
    out[(size_t)j * Q.width + i] = r;
}

void launch3_render_surface(hipStream_t st, const Params3& P, const Arrays3& A, const Surface3Query& Q) {
    const uint32_t nbx = (Q.width + 15u) >> 4, nby = (Q.height + 15u) >> 4;    // width * height <= 2^26: the product fits
    if (Q.orthographic)
        hipLaunchKernelGGL(k3_render_surface<true>, dim3(nbx * nby), dim3(B3R), 0, st, P, Q, nbx, A.pred, A.vel, A.cs, (SurfaceHit3*)Q.out);
    else
        hipLaunchKernelGGL(k3_render_surface<false>, dim3(nbx * nby), dim3(B3R), 0, st, P, Q, nbx, A.pred, A.vel, A.cs, (SurfaceHit3*)Q.out);
}

}  // namespace fsd

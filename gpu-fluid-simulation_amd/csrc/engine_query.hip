// engine_query.hip — what walks a single-domain handle's cell table off the step path, behind fs_sim::walk_ready: the
// density-splat renderer and field sampling (§13).  Blocking forms stage device memory in DevArray locals and
// synchronise the stream before those go out of scope.
#include <hip/hip_runtime.h>

#include "engine.h"

using namespace fsd;

extern "C" fs_status fs_render_density(fs_sim* s, const fs_view* view, float* rgba_host) {
    if (!s || !view || !rgba_host) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "render on a slab handle");
    FS_JOIN(s);
    if (view->width == 0 || view->height == 0 || (uint64_t)view->width * view->height > (1ull << 28))
        return fail(FS_ERR_INVALID, "bad image size");
    // an upload writes the records in upload order under the previous sort's cell table: a walk would pair old ranges with new arrays
    if (!s->walk_ready) return fail(FS_ERR_INVALID, "render needs a step since create and since the last upload of particles or start indices");
    FS_HIP(hipSetDevice(s->device));
    const size_t npix = (size_t)view->width * view->height;
    DevArray<float4> dimg;
    FS_HIP(dimg.alloc(npix));
    const fsd::StepParams P = make_params(*s, s->uniform);
    // after a step: `pred` = predicted positions of this step, `vel` = updated velocities (what the
    // reference's fragment shader sees in in_particles at draw time)
    fsd::launch_render_density(s->stream, P, make_float2(view->world_min.x, view->world_min.y),
                               make_float2(view->world_max.x, view->world_max.y), view->width, view->height, s->pred.p,
                               s->vel.p, s->cs.p, s->start_ref.p, s->pairs.p, dimg.p);
    hipError_t e = hipMemcpyAsync(rgba_host, dimg.p, npix * sizeof(float4), hipMemcpyDeviceToHost, s->stream);
    const hipError_t es = hipStreamSynchronize(s->stream);      // before the image is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    return sort_health(s);        // the image is in `rgba_host` either way; FS_ERR_DEVICE says the order it was walked in is not to be trusted
}

// ---- field sampling ---------------------------------------------------------------------------------
namespace {
// Argument and state checks the three calls share, in the order the header lists them.  *go = false: n == 0, nothing to do.
fs_status sample_check(fs_sim* s, const void* points_or_view, size_t n, const void* out, const float* attr_out, bool* go) {
    *go = false;
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "sampling: single-domain handles only (not built for slab handles)");
    if (attr_out && s->trk.channels <= 0) return fail(FS_ERR_INVALID, "sampling: attr_out needs tracking with at least one channel");
    if (n == 0) return FS_OK;
    if (!points_or_view || !out) return fail(FS_ERR_INVALID, "null argument");
    if (n > ((size_t)1 << 28)) return fail(FS_ERR_INVALID, "sampling: more than 2^28 points");
    if (!s->walk_ready) return fail(FS_ERR_INVALID, "sampling needs a step since create and since the last upload of particles or start indices");
    *go = true;
    return FS_OK;
}

// Enqueue the kernel on the simulation's stream.  points_dev == nullptr: the pixel centres of `view`.
fs_status sample_enqueue(fs_sim* s, const fs_vec2* points_dev, const fs_view* view, size_t n, fs_sample* out_dev, float* attr_out_dev) {
    static_assert(sizeof(fs_sample) == 24, "fs_sample is 24 bytes");
    fsd::SampleQuery Q;
    Q.n = (uint32_t)n;
    Q.points = (const float2*)points_dev;
    if (view) {
        Q.wmin = make_float2(view->world_min.x, view->world_min.y);
        Q.wmax = make_float2(view->world_max.x, view->world_max.y);
        Q.width = view->width; Q.height = view->height;
    }
    Q.out = out_dev; Q.attr_out = attr_out_dev;
    fsd::SampleState S;
    // after a step: `pred` = its predicted positions, `vel` = its new velocities (as fs_render_density); keys and densities
    // from where that step left them
    S.pred = s->pred.p; S.vel = s->vel.p;
    S.rho2 = s->rho2.p; S.rho = s->rho_in_rho2 ? nullptr : s->rho.p;
    S.cs = s->cs.p; S.start_ref = s->start_ref.p; S.pairs = s->pairs.p;
    if (attr_out_dev) {
        S.channels = s->trk.channels;
        S.attr = s->trk.channel(0, s->capacity); S.attr_stride = s->capacity;
    }
    fsd::launch_sample(s->stream, make_params(*s, s->uniform), Q, S);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// The blocking forms (fs_host.h staged_query): points == nullptr: the grid of `view`.
fs_status sample_host(fs_sim* s, const fs_vec2* points, const fs_view* view, size_t n, fs_sample* out, float* attr_out) {
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(staged_query(s->stream, points, n, out, attr_out, attr_out ? (size_t)s->trk.channels : 0,
                        [&](const fs_vec2* dpts, fs_sample* dout, float* dattr) {
                            return sample_enqueue(s, dpts, points ? nullptr : view, n, dout, dattr);
                        }));
    return sort_health(s);
}
}  // namespace

extern "C" {

fs_status fs_sample_points(fs_sim* s, const fs_vec2* points, size_t n, fs_sample* out, float* attr_out) {
    bool go;
    const fs_status r = sample_check(s, points, n, out, attr_out, &go);
    if (r != FS_OK || !go) return r;
    return sample_host(s, points, nullptr, n, out, attr_out);
}

fs_status fs_sample_points_device(fs_sim* s, const fs_vec2* points_dev, size_t n, fs_sample* out_dev, float* attr_out_dev) {
    bool go;
    const fs_status r = sample_check(s, points_dev, n, out_dev, attr_out_dev, &go);
    if (r != FS_OK || !go) return r;
    FS_HIP(hipSetDevice(s->device));
    return sample_enqueue(s, points_dev, nullptr, n, out_dev, attr_out_dev);
}

fs_status fs_sample_grid(fs_sim* s, const fs_view* view, fs_sample* out, float* attr_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "sampling: single-domain handles only (not built for slab handles)");
    if (!view) return fail(FS_ERR_INVALID, "null argument");
    if (view->width == 0 || view->height == 0 || (uint64_t)view->width * view->height > (1ull << 28))
        return fail(FS_ERR_INVALID, "bad grid size");
    const size_t n = (size_t)view->width * view->height;
    bool go;
    const fs_status r = sample_check(s, view, n, out, attr_out, &go);
    if (r != FS_OK || !go) return r;
    return sample_host(s, nullptr, view, n, out, attr_out);
}

}  // extern "C"

// engine_3d_query.hip — what walks a 3D handle's cell table off the step path, behind fs_sim3::sample_stale: field sampling
//  and its tracking channels (§20), surface rendering (§16), surface extraction (§17).  Blocking forms stage
// device memory through fs_host.h (staged_query for points in, download_records for a kernel's output) and end in sort_health3.
#include <hip/hip_runtime.h>

#include "engine_3d.h"

using fsd::fail;
using fsd::params3_common;
using fsd::sort_health3;
namespace {
// ---- field sampling (§14) and the tracking channels in it (§20) ------------------------------------------------------------
// How either family puts its kernel on the simulation's stream.  points_dev == nullptr: the voxel centres of `view`.
fs_status sample3_enqueue(fs_sim3* s, const fs_vec3* points_dev, const fs3_view* view, size_t n, fs3_sample* out_dev, float*) {
    static_assert(sizeof(fs3_sample) == 40 && sizeof(fs_vec3) == 12, "fs3_sample is 40 bytes, fs_vec3 three floats");
    fsd::Sample3Query Q;
    Q.n = (uint32_t)n;
    Q.points = (const float*)points_dev;
    if (view) fsd::set_view3(&Q, *view);
    Q.out = out_dev;
    fsd::launch3_sample(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

fs_status sample3_attr_enqueue(fs_sim3* s, const fs_vec3* points_dev, const fs3_view* view, size_t n, float* weight_dev, float* attr_dev) {
    fsd::Sample3AttrQuery Q;
    Q.n = (uint32_t)n;
    Q.points = (const float*)points_dev;
    if (view) fsd::set_view3(&Q, *view);
    Q.channels = s->trk.channels;
    Q.attr = s->trk.channel(0, s->cap); Q.attr_stride = s->cap;
    Q.weight_out = weight_dev; Q.attr_out = attr_dev;
    fsd::launch3_sample_attr(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

enum Sample3Form { POINTS, POINTS_DEVICE, GRID };

// One sampling call of either family: its checks in the order the header lists them, then the kernel — enqueued at once on device
// pointers, else through the staging of the blocking forms (fs_host.h staged_query).  GRID: the voxel centres of `view`, n = width
// * height * depth; else n points.  channels: the family of §20, whose `out` (the weights) may be null and whose attr_out may not.
template <class Rec, class Enqueue>
fs_status sample3_call(fs_sim3* s, Sample3Form form, const fs_vec3* points, const fs3_view* view, size_t n, Rec* out, float* attr_out,
                       bool channels, Enqueue enqueue) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (form == GRID) {
        if (!view) return fail(FS_ERR_INVALID, "null argument");
        const uint64_t wh = (uint64_t)view->width * view->height;
        if (wh == 0 || view->depth == 0 || wh > (1ull << 28) || wh * view->depth > (1ull << 28)) return fail(FS_ERR_INVALID, "bad grid size");
        n = (size_t)(wh * view->depth);
    }
    if (channels && s->trk.channels <= 0) return fail(FS_ERR_INVALID, "sampling: the channels need tracking with at least one channel");
    if (n == 0) return FS_OK;
    if ((form != GRID && !points) || !(channels ? (const void*)attr_out : (const void*)out)) return fail(FS_ERR_INVALID, "null argument");
    if (n > ((size_t)1 << 28)) return fail(FS_ERR_INVALID, "sampling: more than 2^28 points");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "sampling needs a step since create and since the last upload of particles");
    FS_HIP(hipSetDevice(s->device));
    if (form == POINTS_DEVICE) return enqueue(s, points, nullptr, n, out, attr_out);
    FS_TRY(fsd::staged_query(s->stream, points, n, out, attr_out, channels ? (size_t)s->trk.channels : 0,
                             [&](const fs_vec3* dpts, Rec* dout, float* dattr) { return enqueue(s, dpts, points ? nullptr : view, n, dout, dattr); }));
    return sort_health3(s);
}

// ---- surface rendering (§16) ------------------------------------------------------------------------------------------------
// The checks of both calls, in the order the header lists them.
fs_status surface3_check(const fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, const void* out) {
    static_assert(sizeof(fs3_camera) == 64 && sizeof(fs3_surface_params) == 20 && sizeof(fs3_surface_hit) == 40, "3D surface rendering records");
    if (!s || !cam || !sp || !out) return fail(FS_ERR_INVALID, "null argument");
    const uint64_t wh = (uint64_t)cam->width * cam->height;
    if (wh == 0 || wh > (1ull << 26)) return fail(FS_ERR_INVALID, "bad image size");
    if (cam->reserved != 0) return fail(FS_ERR_INVALID, "camera: reserved must be 0");
    if (cam->orthographic != 0 && cam->orthographic != 1) return fail(FS_ERR_INVALID, "camera: orthographic must be 0 or 1");
    if (!std::isfinite(sp->iso) || !(sp->iso > 0.0f)) return fail(FS_ERR_INVALID, "surface params: iso must be finite and > 0");
    if (!std::isfinite(sp->t_near) || !(sp->t_near >= 0.0f)) return fail(FS_ERR_INVALID, "surface params: t_near must be finite and >= 0");
    if (!std::isfinite(sp->ds) || !(sp->ds > 0.0f)) return fail(FS_ERR_INVALID, "surface params: ds must be finite and > 0");
    if (sp->max_steps < 1u || sp->max_steps > 4096u) return fail(FS_ERR_INVALID, "surface params: max_steps must be 1 .. 4096");
    if (sp->refine > 24u) return fail(FS_ERR_INVALID, "surface params: refine must be 0 .. 24");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "rendering needs a step since create and since the last upload of particles");
    return FS_OK;
}

fs_status surface3_enqueue(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out_dev) {
    fsd::Surface3Query Q;
    Q.eye = make_float3(cam->eye.x, cam->eye.y, cam->eye.z);
    Q.forward = make_float3(cam->forward.x, cam->forward.y, cam->forward.z);
    Q.right = make_float3(cam->right.x, cam->right.y, cam->right.z);
    Q.up = make_float3(cam->up.x, cam->up.y, cam->up.z);
    Q.width = cam->width; Q.height = cam->height; Q.orthographic = cam->orthographic;
    Q.iso = sp->iso; Q.t_near = sp->t_near; Q.ds = sp->ds; Q.max_steps = sp->max_steps; Q.refine = sp->refine;
    Q.out = out_dev;
    fsd::launch3_render_surface(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// ---- surface extraction (§17) -----------------------------------------------------------------------------------------------
// The checks of both calls, in the order the header lists them.
fs_status mesh3_check(const fs_sim3* s, const fs3_view* view, float iso, const void* verts, uint32_t vert_cap, const void* tris,
                      uint32_t tri_cap, const void* counts) {
    static_assert(sizeof(fs3_mesh_vertex) == 40, "fs3_mesh_vertex is 40 bytes");
    if (!s || !view || !counts) return fail(FS_ERR_INVALID, "null argument");
    if (view->width < 2u || view->height < 2u || view->depth < 2u) return fail(FS_ERR_INVALID, "bad lattice size: an extent < 2");
    const uint64_t wh = (uint64_t)view->width * view->height;
    if (wh > (1ull << 26) || wh * view->depth > (1ull << 26)) return fail(FS_ERR_INVALID, "bad lattice size: more than 2^26 nodes");
    if (!std::isfinite(iso) || !(iso > 0.0f)) return fail(FS_ERR_INVALID, "extraction: iso must be finite and > 0");
    if ((!verts && vert_cap) || (!tris && tri_cap)) return fail(FS_ERR_INVALID, "extraction: null array with a non-zero capacity");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "extraction needs a step since create and since the last upload of particles");
    return FS_OK;
}

// The query of a checked call on the handle's scratch, which grows here and nowhere else.
fs_status mesh3_query(fs_sim3* s, const fs3_view* view, float iso, fsd::Mesh3Query* Q) {
    FS_TRY(s->mesh.reserve((size_t)view->width * view->height * view->depth));
    fsd::set_view3(Q, *view);
    Q->iso = iso;
    Q->field = s->mesh.field.p; Q->rank = s->mesh.rank.p; Q->sums = s->mesh.sums.p;
    return FS_OK;
}

// Field, count and scan passes: {V, T} into Q.counts.
fs_status mesh3_count(fs_sim3* s, const fsd::Mesh3Query& Q) {
    fsd::launch3_mesh_count(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// Vertices (which also leaves every active cell's rank for the faces), then faces: whatever part has room.
fs_status mesh3_emit(fs_sim3* s, const fsd::Mesh3Query& Q) {
    if (Q.vert_cap == 0u && Q.tri_cap == 0u) return FS_OK;
    fsd::launch3_mesh_verts(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    if (Q.tri_cap != 0u) fsd::launch3_mesh_faces(s->stream, Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace

extern "C" {

fs_status fs3_sample_points(fs_sim3* s, const fs_vec3* points, size_t n, fs3_sample* out) {
    return sample3_call(s, POINTS, points, nullptr, n, out, nullptr, false, sample3_enqueue);
}
fs_status fs3_sample_points_device(fs_sim3* s, const fs_vec3* points_dev, size_t n, fs3_sample* out_dev) {
    return sample3_call(s, POINTS_DEVICE, points_dev, nullptr, n, out_dev, nullptr, false, sample3_enqueue);
}
fs_status fs3_sample_grid(fs_sim3* s, const fs3_view* view, fs3_sample* out) {
    return sample3_call(s, GRID, nullptr, view, 0, out, nullptr, false, sample3_enqueue);
}
// weight_out may be null
fs_status fs3_sample_attr_points(fs_sim3* s, const fs_vec3* points, size_t n, float* weight_out, float* attr_out) {
    return sample3_call(s, POINTS, points, nullptr, n, weight_out, attr_out, true, sample3_attr_enqueue);
}
fs_status fs3_sample_attr_points_device(fs_sim3* s, const fs_vec3* points_dev, size_t n, float* weight_out_dev, float* attr_out_dev) {
    return sample3_call(s, POINTS_DEVICE, points_dev, nullptr, n, weight_out_dev, attr_out_dev, true, sample3_attr_enqueue);
}
fs_status fs3_sample_attr_grid(fs_sim3* s, const fs3_view* view, float* weight_out, float* attr_out) {
    return sample3_call(s, GRID, nullptr, view, 0, weight_out, attr_out, true, sample3_attr_enqueue);
}

fs_status fs3_render_surface(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out) {
    FS_TRY(surface3_check(s, cam, sp, out));
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(fsd::download_records(s->stream, (size_t)cam->width * cam->height, out,
                                 [&](fs3_surface_hit* dout) { return surface3_enqueue(s, cam, sp, dout); }));
    return sort_health3(s);
}

fs_status fs3_render_surface_device(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out_dev) {
    FS_TRY(surface3_check(s, cam, sp, out_dev));
    FS_HIP(hipSetDevice(s->device));
    return surface3_enqueue(s, cam, sp, out_dev);
}

fs_status fs3_extract_surface_device(fs_sim3* s, const fs3_view* view, float iso, fs3_mesh_vertex* verts_dev, uint32_t vert_cap,
                                     uint32_t* tris_dev, uint32_t tri_cap, uint32_t* counts_dev) {
    FS_TRY(mesh3_check(s, view, iso, verts_dev, vert_cap, tris_dev, tri_cap, counts_dev));
    FS_HIP(hipSetDevice(s->device));
    fsd::Mesh3Query Q;
    FS_TRY(mesh3_query(s, view, iso, &Q));
    Q.counts = counts_dev; Q.verts = verts_dev; Q.vert_cap = vert_cap; Q.tris = tris_dev; Q.tri_cap = tri_cap;
    fsd::launch3_mesh_count(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    return mesh3_emit(s, Q);
}

// Blocking: the counts first (field, count and scan passes), then what fits of either array through the download helper.
fs_status fs3_extract_surface(fs_sim3* s, const fs3_view* view, float iso, fs3_mesh_vertex* verts, uint32_t vert_cap, uint32_t* tris,
                              uint32_t tri_cap, uint32_t counts[2]) {
    FS_TRY(mesh3_check(s, view, iso, verts, vert_cap, tris, tri_cap, counts));
    FS_HIP(hipSetDevice(s->device));
    fsd::Mesh3Query Q;
    FS_TRY(mesh3_query(s, view, iso, &Q));
    uint32_t vt[2] = {0u, 0u};
    FS_TRY(fsd::download_records(s->stream, 2, vt, [&](uint32_t* dcounts) { Q.counts = dcounts; return mesh3_count(s, Q); }));
    const uint32_t nv = vt[0] < vert_cap ? vt[0] : vert_cap, nt = vt[1] < tri_cap ? vt[1] : tri_cap;
    Q.vert_cap = nv; Q.tri_cap = 0u;
    if (nv) FS_TRY(fsd::download_records(s->stream, nv, verts, [&](fs3_mesh_vertex* dverts) { Q.verts = dverts; return mesh3_emit(s, Q); }));
    if (nt) {
        Q.verts = nullptr; Q.vert_cap = 0u; Q.tri_cap = nt;
        FS_TRY(fsd::download_records(s->stream, 3 * (size_t)nt, tris, [&](uint32_t* dtris) {
            Q.tris = dtris;
            if (nv) { fsd::launch3_mesh_faces(s->stream, Q); FS_HIP(hipGetLastError()); return FS_OK; }   // the ranks are there
            return mesh3_emit(s, Q);
        }));
    }
    counts[0] = vt[0]; counts[1] = vt[1];
    return sort_health3(s);
}

}  // extern "C"

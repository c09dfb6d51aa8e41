// engine_3d_features.hip — the opt-in features the 3D step enqueues for (their state: engine_3d.h, one struct each): colliders
// (DESIGN.md §18), moving bodies (§23) and their loads (§26), surface tension (§19), particle tracking (§20), channel diffusion and buoyancy (§28) and, on top of tracking,
// fs3_download_particles_by_id.
#include <hip/hip_runtime.h>

#include <vector>

#include "engine_3d.h"
#include "engine_bodies.h"

using fsd::DevArray;
using fsd::fail;
using fsd::sort_health3;
namespace {
// The checks the two collider setters share, in the order the header lists them (the handle first, by the caller).
fs_status collider3_check(const void* array, uint32_t w, uint32_t h, uint32_t d) {
    const uint32_t top = fsd::COLLIDER3_MAX_EXTENT;
    if (!array) return fail(FS_ERR_INVALID, "null argument");
    if (w == 0u || h == 0u || d == 0u || w > top || h > top || d > top) return fail(FS_ERR_INVALID, "collider: an extent of 0 or above 1024");
    return FS_OK;
}

// Checks 3 and 4 of the two body constructors (the handle and the pointers first, by the caller).
fs_status body3_check(uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent) {
    FS_TRY(collider3_check(&extent, w, h, d));
    if (!fsd::all_positive(&extent.x, 3)) return fail(FS_ERR_INVALID, "body: a box extent that is not finite and > 0");
    return FS_OK;
}

// The per-body calls' checks: the handle and the pointers (`null`), then the slot.
fs_status body3_slot(const fs_sim3* s, bool null, uint32_t body) {
    if (!s || null) return fail(FS_ERR_INVALID, "null argument");
    if (!s->bodies.has(body)) return fail(FS_ERR_INVALID, "body: the slot holds no body");
    return FS_OK;
}

// A produced or uploaded field becomes the body of `slot`: identity pose at the origin, at rest.
void body3_install(fs_sim3* s, uint32_t slot, DevArray<float4>&& field, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent) {
    fs_sim3::Bodies::Slot& b = s->bodies.slot[slot];
    b.field = std::move(field);
    b.w = w; b.h = h; b.d = d; b.extent = extent;
    b.motion = fs3_body_motion{};
    b.motion.rot[0] = b.motion.rot[4] = b.motion.rot[8] = 1.0f;
}

// The field in use as w * h * d fs_vec3 on the host.  Blocking.
fs_status collider3_read(fs_sim3* s, fs_vec3* dst) { return fsd::download_vec3(s->stream, s->collider.field.p, s->collider.voxels(), dst); }

// ids (attr = false) or one channel, host <-> the arrays of the last enqueued step.  Blocking.
fs_status track3_copy(fs_sim3* s, int channel, bool attr, void* host, size_t n, bool upload) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->trk.copy(s->stream, s->n, s->cap, channel, attr, host, n, upload));
    return upload ? FS_OK : sort_health3(s);
}

// The checks every setter and getter of channel diffusion and buoyancy starts with: the handle and the pointers (`null`), then tracking on.
fs_status diffusion3_handle(const fs_sim3* s, bool null) {
    if (!s || null) return fail(FS_ERR_INVALID, "null argument");
    if (!s->trk.on()) return fail(FS_ERR_INVALID, "diffusion: tracking is off (fs3_track_enable with at least one channel first)");
    return FS_OK;
}
}  // namespace

extern "C" {

// ---- 3D colliders -------------------------------------------------------------------------------------
fs_status fs3_collider_upload(fs_sim3* s, const fs_vec3* field, uint32_t w, uint32_t h, uint32_t d) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(collider3_check(field, w, h, d));
    const size_t voxels = (size_t)w * h * d;
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[voxels]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    for (size_t k = 0; k < voxels; ++k) {
        const fs_vec3 f = field[k];
        if (!std::isfinite(f.x) || !std::isfinite(f.y) || !std::isfinite(f.z)) return fail(FS_ERR_INVALID, "collider: non-finite component");
        host[k] = make_float4(f.x, f.y, f.z, 0.0f);
    }
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->collider.reserve(s->stream, voxels));
    // on the stream: after the steps in flight, before the steps to come
    FS_HIP(hipMemcpyAsync(s->collider.field.p, host.get(), voxels * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    s->collider.set(w, h, d);
    return FS_OK;
}

fs_status fs3_collider_from_mask(fs_sim3* s, const uint8_t* mask, uint32_t w, uint32_t h, uint32_t d, fs_vec3* field_host) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(collider3_check(mask, w, h, d));
    const size_t voxels = (size_t)w * h * d;
    if (!fsd::mask_has_free(mask, voxels)) return fail(FS_ERR_INVALID, "collider: the mask has no free voxel");
    FS_HIP(hipSetDevice(s->device));
    fsd::MaskStaging stage;
    if (stage.alloc(voxels) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "collider: device staging");
    }
    FS_TRY(s->collider.reserve(s->stream, voxels));
    const fs_status r = mask_to_field3(s->stream, mask, w, h, d, s->st.size, s->collider.field.p, stage);
    if (r != FS_OK) { s->collider.clear(); return r; }
    s->collider.set(w, h, d);
    return field_host ? collider3_read(s, field_host) : FS_OK;
}

fs_status fs3_collider_clear(fs_sim3* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipStreamSynchronize(s->stream));       // the steps in flight read the field
    s->collider.clear();
    s->collider.field.release();
    return FS_OK;
}

fs_status fs3_collider_dims(const fs_sim3* s, uint32_t* w, uint32_t* h, uint32_t* d) {
    if (!s || !w || !h || !d) return fail(FS_ERR_INVALID, "null argument");
    *w = s->collider.w; *h = s->collider.h; *d = s->collider.d;
    return FS_OK;
}

fs_status fs3_collider_download(fs_sim3* s, fs_vec3* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (s->collider.w == 0u) return fail(FS_ERR_INVALID, "collider: none is set");
    if (n != s->collider.voxels()) return fail(FS_ERR_INVALID, "collider: n must be w * h * d");
    FS_HIP(hipSetDevice(s->device));
    return collider3_read(s, dst);
}

// ---- 3D moving bodies -----------------------------------------------------------------------------------
fs_status fs3_body_create(fs_sim3* s, const fs_vec3* field, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent, uint32_t* body_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (!field || !body_out) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(body3_check(w, h, d, extent));
    const size_t voxels = (size_t)w * h * d;
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[voxels]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    for (size_t k = 0; k < voxels; ++k) {
        const fs_vec3 f = field[k];
        if (!std::isfinite(f.x) || !std::isfinite(f.y) || !std::isfinite(f.z)) return fail(FS_ERR_INVALID, "body: non-finite component");
        host[k] = make_float4(f.x, f.y, f.z, 0.0f);
    }
    const uint32_t slot = s->bodies.free_slot();
    if (slot == FS3_MAX_BODIES) return fail(FS_ERR_INVALID, "body: no free slot");
    FS_HIP(hipSetDevice(s->device));
    DevArray<float4> dev;
    if (dev.alloc(voxels) != hipSuccess) { (void)hipGetLastError(); return fail(FS_ERR_OOM, "body: device field"); }
    FS_HIP(hipMemcpyAsync(dev.p, host.get(), voxels * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    body3_install(s, slot, std::move(dev), w, h, d, extent);
    *body_out = slot;
    return FS_OK;
}

fs_status fs3_body_create_from_mask(fs_sim3* s, const uint8_t* mask, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent,
                                    fs_vec3* field_host, uint32_t* body_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (!mask || !body_out) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(body3_check(w, h, d, extent));
    const size_t voxels = (size_t)w * h * d;
    if (!fsd::mask_has_free(mask, voxels)) return fail(FS_ERR_INVALID, "body: the mask has no free voxel");
    const uint32_t slot = s->bodies.free_slot();
    if (slot == FS3_MAX_BODIES) return fail(FS_ERR_INVALID, "body: no free slot");
    FS_HIP(hipSetDevice(s->device));
    fsd::MaskStaging stage;
    DevArray<float4> dev;
    if (stage.alloc(voxels) != hipSuccess || dev.alloc(voxels) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "body: device staging");
    }
    FS_TRY(mask_to_field3(s->stream, mask, w, h, d, extent, dev.p, stage));
    if (field_host) FS_TRY(fsd::download_vec3(s->stream, dev.p, voxels, field_host));
    body3_install(s, slot, std::move(dev), w, h, d, extent);
    *body_out = slot;
    return FS_OK;
}

fs_status fs3_body_set_motion(fs_sim3* s, uint32_t body, const fs3_body_motion* m) {
    FS_TRY(body3_slot(s, !m, body));
    // 18 floats, nothing between them (static_assert below)
    if (!fsd::all_finite(&m->centre.x, 18)) return fail(FS_ERR_INVALID, "body: non-finite motion");
    s->bodies.slot[body].motion = *m;           // host memory only: the next enqueue takes it by value
    return FS_OK;
}
static_assert(sizeof(fs3_body_motion) == 18 * sizeof(float), "fs3_body_motion is 18 packed floats");
static_assert(fsd::BODIES3_MAX == FS3_MAX_BODIES, "Bodies3 holds every slot of the ABI");

fs_status fs3_body_get_motion(const fs_sim3* s, uint32_t body, fs3_body_motion* out) {
    FS_TRY(body3_slot(s, !out, body));
    *out = s->bodies.slot[body].motion;
    return FS_OK;
}

fs_status fs3_body_dims(const fs_sim3* s, uint32_t body, uint32_t* w, uint32_t* h, uint32_t* d, fs_vec3* extent) {
    FS_TRY(body3_slot(s, !w || !h || !d || !extent, body));
    const fs_sim3::Bodies::Slot& b = s->bodies.slot[body];
    *w = b.w; *h = b.h; *d = b.d; *extent = b.extent;
    return FS_OK;
}

fs_status fs3_body_download(fs_sim3* s, uint32_t body, fs_vec3* dst, size_t n) {
    FS_TRY(body3_slot(s, !dst, body));
    const fs_sim3::Bodies::Slot& b = s->bodies.slot[body];
    if (n != b.voxels()) return fail(FS_ERR_INVALID, "body: n must be w * h * d");
    FS_HIP(hipSetDevice(s->device));
    return fsd::download_vec3(s->stream, b.field.p, n, dst);
}

fs_status fs3_body_destroy(fs_sim3* s, uint32_t body) {
    FS_TRY(body3_slot(s, false, body));
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipStreamSynchronize(s->stream));       // the steps in flight read the field
    fs_sim3::Bodies::Slot& b = s->bodies.slot[body];
    b.w = b.h = b.d = 0;
    b.field.release();
    FS_HIP(s->bodies.loads.zero(s->stream, body));                // before the slot can be reused (a new body starts at zero)
    return FS_OK;
}

uint32_t fs3_body_count(const fs_sim3* s) { return s ? s->bodies.count() : 0u; }

// ---- 3D body loads ------------------------------------------------------------------------------------
static_assert(sizeof(fs3_body_load) == 9 * 8, "fs3_body_load: the kernel's eight words and steps");
const char* const LOADS3_OFF = "body loads: not enabled (fs3_body_loads_enable)";

fs_status fs3_body_loads_enable(fs_sim3* s, int on) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (on) FS_HIP(hipSetDevice(s->device));
    return s->bodies.loads.enable(s->stream, on != 0);
}

int fs3_body_loads_enabled(const fs_sim3* s) { return s && s->bodies.loads.on ? 1 : 0; }

fs_status fs3_body_loads(fs_sim3* s, uint32_t body, fs3_body_load* out, int reset) {
    FS_TRY(body3_slot(s, !out, body));
    fs_sim3::Bodies::Loads& L = s->bodies.loads;
    if (!L.on) return fail(FS_ERR_INVALID, LOADS3_OFF);
    FS_HIP(hipSetDevice(s->device));
    unsigned long long w[fsd::BODY3_LOAD_WORDS];
    uint64_t steps;
    FS_TRY(L.read(s->stream, body, reset != 0, w, &steps));
    for (int a = 0; a < 3; ++a) { out->impulse_q[a] = (int64_t)w[a]; out->angular_q[a] = (int64_t)w[3 + a]; }
    out->hits = w[6]; out->dropped = w[7];
    out->steps = steps;
    return FS_OK;
}

fs_status fs3_body_loads_device(fs_sim3* s, const void** words) {
    if (!s || !words) return fail(FS_ERR_INVALID, "null argument");
    if (!s->bodies.loads.on) return fail(FS_ERR_INVALID, LOADS3_OFF);
    *words = s->bodies.loads.words.p;
    return FS_OK;
}

// ---- 3D surface tension -------------------------------------------------------------------------------
fs_status fs3_set_surface_tension(fs_sim3* s, int enable, float coefficient, float threshold) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (!enable) { s->tension.on = false; return FS_OK; }          // the two floats are not looked at
    if (std::isnan(coefficient)) return fail(FS_ERR_INVALID, "surface tension: coefficient is NaN");
    if (std::isnan(threshold)) return fail(FS_ERR_INVALID, "surface tension: threshold is NaN");
    if (!s->tension.st.p) {
        FS_HIP(hipSetDevice(s->device));
        if (s->tension.st.alloc(s->cap) != hipSuccess) {
            (void)hipGetLastError();
            s->tension.st.release();
            return fail(FS_ERR_OOM, "surface tension: device array");
        }
    }
    if (!s->tension.on) s->tension.valid = false;                  // fs3_download_surface_tension waits for a step of this enable
    s->tension.on = true; s->tension.sigma = coefficient; s->tension.tau = threshold;
    return FS_OK;
}

int fs3_surface_tension_enabled(const fs_sim3* s) { return (s && s->tension.on) ? 1 : 0; }

fs_status fs3_surface_tension_params(const fs_sim3* s, float* coefficient, float* threshold) {
    if (!s || !coefficient || !threshold) return fail(FS_ERR_INVALID, "null argument");
    if (!s->tension.on) return fail(FS_ERR_INVALID, "surface tension: not enabled");
    *coefficient = s->tension.sigma; *threshold = s->tension.tau;
    return FS_OK;
}

fs_status fs3_download_surface_tension(fs_sim3* s, fs_vec3* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (!s->tension.on) return fail(FS_ERR_INVALID, "surface tension: not enabled");
    if (!s->tension.valid) return fail(FS_ERR_INVALID, "surface tension: no step since surface tension was last enabled");
    if (n != s->n) return fail(FS_ERR_INVALID, "surface tension: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(fsd::download_vec3(s->stream, s->tension.st.p, n, dst));
    return sort_health3(s);
}

// ---- 3D particle tracking -----------------------------------------------------------------------------
fs_status fs3_track_enable(fs_sim3* s, int channels) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->trk.enable(s->stream, s->n, s->cap, channels));
    s->diffusion.clear();           // the channels start over: so do their conductivities and the buoyancy channel
    return FS_OK;
}

fs_status fs3_track_disable(fs_sim3* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    s->trk.channels = -1;           // the arrays stay allocated until the handle is destroyed
    s->diffusion.clear();
    return FS_OK;
}

int fs3_track_channels(const fs_sim3* s) { return s ? s->trk.channels : -1; }

fs_status fs3_track_download_ids(fs_sim3* s, uint32_t* dst, size_t n) { return track3_copy(s, 0, false, dst, n, false); }
fs_status fs3_track_upload_ids(fs_sim3* s, const uint32_t* src, size_t n) { return track3_copy(s, 0, false, (void*)src, n, true); }
fs_status fs3_track_download_attr(fs_sim3* s, int channel, float* dst, size_t n) { return track3_copy(s, channel, true, dst, n, false); }
fs_status fs3_track_upload_attr(fs_sim3* s, int channel, const float* src, size_t n) { return track3_copy(s, channel, true, (void*)src, n, true); }

fs_status fs3_track_ids_device(fs_sim3* s, const uint32_t** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->cap, 0, false, (const void**)out);
}

fs_status fs3_track_attr_device(fs_sim3* s, int channel, const float** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->cap, channel, true, (const void**)out);
}

// ---- 3D channel diffusion and buoyancy ------------------------------------------------------------------
fs_status fs3_set_diffusion(fs_sim3* s, int channel, float conductivity) {
    FS_TRY(diffusion3_handle(s, false));
    if (channel < 0 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "diffusion: no such channel");
    if (!std::isfinite(conductivity) || conductivity < 0.0f) return fail(FS_ERR_INVALID, "diffusion: a conductivity that is negative or not finite");
    s->diffusion.kappa[channel] = conductivity;     // host memory only: the next enqueue takes it by value
    return FS_OK;
}

fs_status fs3_get_diffusion(const fs_sim3* s, int channel, float* conductivity) {
    FS_TRY(diffusion3_handle(s, !conductivity));
    if (channel < 0 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "diffusion: no such channel");
    *conductivity = s->diffusion.kappa[channel];
    return FS_OK;
}

fs_status fs3_set_buoyancy(fs_sim3* s, int channel, float beta, float reference) {
    FS_TRY(diffusion3_handle(s, false));
    if (channel < -1 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "buoyancy: no such channel");
    if (!std::isfinite(beta) || !std::isfinite(reference)) return fail(FS_ERR_INVALID, "buoyancy: beta or reference not finite");
    fs_sim3::Diffusion& d = s->diffusion;
    if (channel >= 0 && !d.fb.p) {
        FS_HIP(hipSetDevice(s->device));
        if (d.fb.alloc(s->cap) != hipSuccess) {
            (void)hipGetLastError();
            d.fb.release();
            return fail(FS_ERR_OOM, "buoyancy: force buffer");
        }
    }
    if (channel != d.buoy) d.valid = false;         // fs3_download_buoyancy waits for a step of this setting
    d.buoy = channel;
    d.beta = channel >= 0 ? beta : 0.0f;
    d.reference = channel >= 0 ? reference : 0.0f;
    return FS_OK;
}

fs_status fs3_get_buoyancy(const fs_sim3* s, int* channel, float* beta, float* reference) {
    FS_TRY(diffusion3_handle(s, !channel || !beta || !reference));
    *channel = s->diffusion.buoy; *beta = s->diffusion.beta; *reference = s->diffusion.reference;
    return FS_OK;
}

fs_status fs3_download_buoyancy(fs_sim3* s, fs_vec3* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (s->diffusion.buoy < 0) return fail(FS_ERR_INVALID, "buoyancy: no channel is set");
    if (!s->diffusion.valid) return fail(FS_ERR_INVALID, "buoyancy: no step with a buoyancy channel since the channel was last set");
    if (n != s->n) return fail(FS_ERR_INVALID, "buoyancy: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(fsd::download_vec3(s->stream, s->diffusion.fb.p, n, dst));
    return sort_health3(s);
}

/* Off the step path: two downloads and a scatter on the host, so entries of dst that no id names are never written. */
fs_status fs3_download_particles_by_id(fs_sim3* s, fs3_particle* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    if (!s->trk.on()) return fail(FS_ERR_INVALID, "tracking is off (enable it first)");
    std::vector<fs3_particle> rec;
    std::vector<uint32_t> ids;
    try { rec.resize(s->n); ids.resize(s->n); } catch (const std::bad_alloc&) { return fail(FS_ERR_OOM, "host staging"); }
    FS_TRY(fs3_download_particles(s, rec.data(), rec.size()));
    FS_TRY(fs3_track_download_ids(s, ids.data(), ids.size()));
    fsd::Tracking::scatter_by_id(ids, rec, dst, n);
    return FS_OK;
}

}  // extern "C"

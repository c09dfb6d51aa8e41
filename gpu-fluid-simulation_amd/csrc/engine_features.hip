// engine_features.hip — the opt-in per-step features of a single-domain handle: surface tension, particle
// tracking (§12), channel diffusion and buoyancy (§27), moving bodies (§24) and their loads (§25).  Their state and what the step
// enqueues for them: SurfaceTension / Tracking / Diffusion / Bodies (engine.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "engine_bodies.h"

using namespace fsd;

extern "C" {

fs_status fs_set_surface_tension(fs_sim* s, int enable) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "surface tension: single-domain handles only (not built for slab handles)");
    if (enable && !s->st.on) {
        if (!s->st.stf.p) {
            FS_HIP(hipSetDevice(s->device));
            FS_HIP(s->st.stf.alloc(s->capacity));
        }
        s->st.valid = false;        // fs_download_surface_tension waits for a step of this enable
    }
    s->st.on = enable != 0;
    return FS_OK;
}

int fs_surface_tension_enabled(const fs_sim* s) { return (s && s->st.on) ? 1 : 0; }

fs_status fs_download_surface_tension(fs_sim* s, fs_vec2* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (!s->st.valid) return fail(FS_ERR_INVALID, "surface tension: no step with surface tension since the handle was created or ST was last enabled");
    if (n != s->n) return fail(FS_ERR_INVALID, "surface tension: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    static_assert(sizeof(fs_vec2) == sizeof(float2), "fs_vec2 is two f32");
    if (n) FS_HIP(hipMemcpyAsync(dst, s->st.stf.p, n * sizeof(fs_vec2), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return sort_health(s);
}

// ---- particle tracking ----------------------------------------------------------------------------
fs_status fs_track_enable(fs_sim* s, int channels) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "tracking: single-domain handles only (not built for slab handles)");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->trk.enable(s->stream, s->n, s->capacity, channels));
    s->dif.clear();                 // the channels start over: so do their conductivities and the buoyancy channel
    return FS_OK;
}

fs_status fs_track_disable(fs_sim* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    s->trk.channels = -1;           // the arrays stay allocated until the handle is destroyed
    s->dif.clear();
    return FS_OK;
}

int fs_track_channels(const fs_sim* s) { return s ? s->trk.channels : -1; }

}  // extern "C"

// ---- channel diffusion and buoyancy ---------------------------------------------------------------------------
namespace {
const char* const DIF_SLAB = "diffusion: single-domain handles only (not built for slab handles)";

// The checks every call of the feature starts with: the handle ("null"), the slab refusal, tracking on.
fs_status diffusion_handle(const fs_sim* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, DIF_SLAB);
    if (!s->trk.on()) return fail(FS_ERR_INVALID, "diffusion: tracking is off (fs_track_enable with at least one channel first)");
    return FS_OK;
}
}  // namespace

extern "C" {

fs_status fs_set_diffusion(fs_sim* s, int channel, float conductivity) {
    FS_TRY(diffusion_handle(s));
    if (channel < 0 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "diffusion: no such channel");
    if (!std::isfinite(conductivity) || conductivity < 0.0f) return fail(FS_ERR_INVALID, "diffusion: a conductivity that is negative or not finite");
    s->dif.kappa[channel] = conductivity;       // host memory only: the next enqueue takes it by value
    return FS_OK;
}

fs_status fs_get_diffusion(const fs_sim* s, int channel, float* conductivity) {
    FS_TRY(diffusion_handle(s));
    if (!conductivity) return fail(FS_ERR_INVALID, "null argument");
    if (channel < 0 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "diffusion: no such channel");
    *conductivity = s->dif.kappa[channel];
    return FS_OK;
}

fs_status fs_set_buoyancy(fs_sim* s, int channel, float beta, float reference) {
    FS_TRY(diffusion_handle(s));
    if (channel < -1 || channel >= s->trk.channels) return fail(FS_ERR_INVALID, "buoyancy: no such channel");
    if (!std::isfinite(beta) || !std::isfinite(reference)) return fail(FS_ERR_INVALID, "buoyancy: beta or reference not finite");
    if (channel >= 0 && !s->dif.fb.p) {
        FS_HIP(hipSetDevice(s->device));
        if (s->dif.fb.alloc(s->capacity) != hipSuccess) { (void)hipGetLastError(); return fail(FS_ERR_OOM, "buoyancy: force buffer"); }
    }
    if (channel != s->dif.buoy) s->dif.valid = false;       // fs_download_buoyancy waits for a step of this setting
    s->dif.buoy = channel;
    s->dif.beta = channel >= 0 ? beta : 0.0f;
    s->dif.reference = channel >= 0 ? reference : 0.0f;
    return FS_OK;
}

fs_status fs_get_buoyancy(const fs_sim* s, int* channel, float* beta, float* reference) {
    FS_TRY(diffusion_handle(s));
    if (!channel || !beta || !reference) return fail(FS_ERR_INVALID, "null argument");
    *channel = s->dif.buoy; *beta = s->dif.beta; *reference = s->dif.reference;
    return FS_OK;
}

fs_status fs_download_buoyancy(fs_sim* s, fs_vec2* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, DIF_SLAB);
    if (!s->dif.valid) return fail(FS_ERR_INVALID, "buoyancy: no step with a buoyancy channel since the handle was created or the channel was last set");
    if (n != s->n) return fail(FS_ERR_INVALID, "buoyancy: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    if (n) FS_HIP(hipMemcpyAsync(dst, s->dif.fb.p, n * sizeof(fs_vec2), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return sort_health(s);
}

}  // extern "C"

namespace {
// ids (attr = false) or one channel, host <-> the arrays of the last enqueued step.  Blocking.
fs_status track_copy(fs_sim* s, int channel, bool attr, void* host, size_t n, bool upload) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->trk.copy(s->stream, s->n, s->capacity, channel, attr, host, n, upload));
    return upload ? FS_OK : sort_health(s);
}
}  // namespace

extern "C" {

fs_status fs_track_download_ids(fs_sim* s, uint32_t* dst, size_t n) { return track_copy(s, 0, false, dst, n, false); }
fs_status fs_track_upload_ids(fs_sim* s, const uint32_t* src, size_t n) { return track_copy(s, 0, false, (void*)src, n, true); }
fs_status fs_track_download_attr(fs_sim* s, int channel, float* dst, size_t n) { return track_copy(s, channel, true, dst, n, false); }
fs_status fs_track_upload_attr(fs_sim* s, int channel, const float* src, size_t n) { return track_copy(s, channel, true, (void*)src, n, true); }

fs_status fs_track_ids_device(fs_sim* s, const uint32_t** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->capacity, 0, false, (const void**)out);
}

fs_status fs_track_attr_device(fs_sim* s, int channel, const float** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->capacity, channel, true, (const void**)out);
}

/* Off the step path: two downloads and a scatter on the host, so entries of dst that no id names are never written. */
fs_status fs_download_particles_by_id(fs_sim* s, fs_particle* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    if (!s->trk.on()) return fail(FS_ERR_INVALID, "tracking is off (fs_track_enable)");
    std::vector<fs_particle> rec;
    std::vector<uint32_t> ids;
    try { rec.resize(s->n); ids.resize(s->n); } catch (const std::bad_alloc&) { return fail(FS_ERR_OOM, "host staging"); }
    FS_TRY(fs_download_particles(s, rec.data(), rec.size()));
    if (s->n) {
        FS_TRY(fs_track_download_ids(s, ids.data(), ids.size()));
    }
    Tracking::scatter_by_id(ids, rec, dst, n);
    return FS_OK;
}

}  // extern "C"

// ---- 2D moving bodies -----------------------------------------------------------------------------------
namespace {
const char* const BODY_SLAB = "body: single-domain handles only (not built for slab handles)";

// Checks 4 and 5 of the two body constructors (the handle and the pointers first, by the caller).
fs_status body_check(uint32_t w, uint32_t h, fs_vec2 extent) {
    if (w == 0u || h == 0u || w > 1024u || h > 1024u) return fail(FS_ERR_INVALID, "body: w or h of 0 or above 1024");
    if (!all_positive(&extent.x, 2)) return fail(FS_ERR_INVALID, "body: a box extent that is not finite and > 0");
    return FS_OK;
}

// A produced or uploaded field becomes the body of `slot`: identity pose at the origin, at rest.
void body_install(fs_sim* s, uint32_t slot, DevArray<float2>&& field, uint32_t w, uint32_t h, fs_vec2 extent) {
    Bodies::Slot& b = s->bodies.slot[slot];
    b.field = std::move(field);
    b.w = w; b.h = h; b.extent = extent;
    b.motion = fs_body_motion{};
    b.motion.rot[0] = b.motion.rot[3] = 1.0f;
}

// host -> a fresh device field, blocking on the handle's stream
fs_status body_upload(fs_sim* s, const fs_vec2* host, size_t pixels, DevArray<float2>* dev) {
    static_assert(sizeof(fs_vec2) == sizeof(float2), "fs_vec2 is two f32");
    if (dev->alloc(pixels) != hipSuccess) { (void)hipGetLastError(); return fail(FS_ERR_OOM, "body: device field"); }
    FS_HIP(hipMemcpyAsync(dev->p, host, pixels * sizeof(float2), hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

// The per-body calls' checks 1, 2 and 8 (the pointers between them, by the caller through `null`).
fs_status body_slot(const fs_sim* s, bool null, uint32_t body) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, BODY_SLAB);
    if (null) return fail(FS_ERR_INVALID, "null argument");
    if (!s->bodies.has(body)) return fail(FS_ERR_INVALID, "body: the slot holds no body");
    return FS_OK;
}
}  // namespace

extern "C" {

fs_status fs_body_create(fs_sim* s, const fs_vec2* field, uint32_t w, uint32_t h, fs_vec2 extent, uint32_t* body_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, BODY_SLAB);
    if (!field || !body_out) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(body_check(w, h, extent));
    const size_t pixels = (size_t)w * h;
    for (size_t k = 0; k < pixels; ++k)
        if (!std::isfinite(field[k].x) || !std::isfinite(field[k].y)) return fail(FS_ERR_INVALID, "body: non-finite component");
    const uint32_t slot = s->bodies.free_slot();
    if (slot == FS_MAX_BODIES) return fail(FS_ERR_INVALID, "body: no free slot");
    FS_HIP(hipSetDevice(s->device));
    DevArray<float2> dev;
    FS_TRY(body_upload(s, field, pixels, &dev));
    body_install(s, slot, std::move(dev), w, h, extent);
    *body_out = slot;
    return FS_OK;
}
static_assert(FS_BODY_LOAD_SHIFT == BODY_LOAD_SHIFT && sizeof(fs_body_load) == 6 * 8, "fs_body_load: the kernel's five words and steps");

// The producer of "3D colliders" (mask_to_field3, engine_bodies.h: one library, one transform) on the w x h x 1 mask over a box
// of (extent.x, extent.y, 1); its z component is +0 everywhere and is dropped on the host, between the two blocking copies.
fs_status fs_body_create_from_mask(fs_sim* s, const uint8_t* mask, uint32_t w, uint32_t h, fs_vec2 extent, fs_vec2* field_host,
                                   uint32_t* body_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, BODY_SLAB);
    if (!mask || !body_out) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(body_check(w, h, extent));
    const size_t pixels = (size_t)w * h;
    if (!mask_has_free(mask, pixels)) return fail(FS_ERR_INVALID, "body: the mask has no free pixel");
    const uint32_t slot = s->bodies.free_slot();
    if (slot == FS_MAX_BODIES) return fail(FS_ERR_INVALID, "body: no free slot");
    FS_HIP(hipSetDevice(s->device));
    std::unique_ptr<float4[]> host4(new (std::nothrow) float4[pixels]);
    std::unique_ptr<fs_vec2[]> host2(new (std::nothrow) fs_vec2[pixels]);
    if (!host4 || !host2) return fail(FS_ERR_OOM, "host allocation failed");
    MaskStaging stage;
    DevArray<float4> field4;
    if (stage.alloc(pixels) != hipSuccess || field4.alloc(pixels) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "body: device staging");
    }
    FS_TRY(mask_to_field3(s->stream, mask, w, h, 1u, fs_vec3{extent.x, extent.y, 1.0f}, field4.p, stage));
    hipError_t e = hipMemcpyAsync(host4.get(), field4.p, pixels * sizeof(float4), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    for (size_t k = 0; k < pixels; ++k) host2[k] = fs_vec2{host4[k].x, host4[k].y};
    DevArray<float2> dev;
    FS_TRY(body_upload(s, host2.get(), pixels, &dev));
    if (field_host) std::memcpy(field_host, host2.get(), pixels * sizeof(fs_vec2));
    body_install(s, slot, std::move(dev), w, h, extent);
    *body_out = slot;
    return FS_OK;
}

fs_status fs_body_set_motion(fs_sim* s, uint32_t body, const fs_body_motion* m) {
    FS_TRY(body_slot(s, !m, body));
    // 9 floats, nothing between them (static_assert below)
    if (!all_finite(&m->centre.x, 9)) return fail(FS_ERR_INVALID, "body: non-finite motion");
    s->bodies.slot[body].motion = *m;           // host memory only: the next enqueue takes it by value
    return FS_OK;
}
static_assert(sizeof(fs_body_motion) == 9 * sizeof(float), "fs_body_motion is 9 packed floats");
static_assert(fsd::BODIES2_MAX == FS_MAX_BODIES, "Bodies2 holds every slot of the ABI");

fs_status fs_body_get_motion(const fs_sim* s, uint32_t body, fs_body_motion* out) {
    FS_TRY(body_slot(s, !out, body));
    *out = s->bodies.slot[body].motion;
    return FS_OK;
}

fs_status fs_body_dims(const fs_sim* s, uint32_t body, uint32_t* w, uint32_t* h, fs_vec2* extent) {
    FS_TRY(body_slot(s, !w || !h || !extent, body));
    const Bodies::Slot& b = s->bodies.slot[body];
    *w = b.w; *h = b.h; *extent = b.extent;
    return FS_OK;
}

fs_status fs_body_download(fs_sim* s, uint32_t body, fs_vec2* dst, size_t n) {
    FS_TRY(body_slot(s, !dst, body));
    const Bodies::Slot& b = s->bodies.slot[body];
    if (n != b.pixels()) return fail(FS_ERR_INVALID, "body: n must be w * h");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipMemcpyAsync(dst, b.field.p, n * sizeof(fs_vec2), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

fs_status fs_body_destroy(fs_sim* s, uint32_t body) {
    FS_TRY(body_slot(s, false, body));
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipStreamSynchronize(s->stream));       // the steps in flight read the field
    Bodies::Slot& b = s->bodies.slot[body];
    b.w = b.h = 0;
    b.field.release();
    FS_HIP(s->bodies.loads.zero(s->stream, body));                // before the slot can be reused (a new body starts at zero)
    return FS_OK;
}

uint32_t fs_body_count(const fs_sim* s) { return s ? s->bodies.count() : 0u; }

// ---- 2D body loads ----
fs_status fs_body_loads_enable(fs_sim* s, int on) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, BODY_SLAB);
    if (on) FS_HIP(hipSetDevice(s->device));
    return s->bodies.loads.enable(s->stream, on != 0);
}

int fs_body_loads_enabled(const fs_sim* s) { return s && s->bodies.loads.on ? 1 : 0; }

fs_status fs_body_loads(fs_sim* s, uint32_t body, fs_body_load* out, int reset) {
    FS_TRY(body_slot(s, !out, body));
    Bodies::Loads& L = s->bodies.loads;
    if (!L.on) return fail(FS_ERR_INVALID, "body loads: not enabled (fs_body_loads_enable)");
    FS_HIP(hipSetDevice(s->device));
    unsigned long long w[BODY_LOAD_WORDS];
    uint64_t steps;
    FS_TRY(L.read(s->stream, body, reset != 0, w, &steps));
    out->impulse_q[0] = (int64_t)w[0]; out->impulse_q[1] = (int64_t)w[1];
    out->angular_q = (int64_t)w[2];
    out->hits = w[3]; out->dropped = w[4];
    out->steps = steps;
    return FS_OK;
}

fs_status fs_body_loads_device(fs_sim* s, const void** words) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, BODY_SLAB);
    if (!words) return fail(FS_ERR_INVALID, "null argument");
    if (!s->bodies.loads.on) return fail(FS_ERR_INVALID, "body loads: not enabled (fs_body_loads_enable)");
    *words = s->bodies.loads.words.p;
    return FS_OK;
}

}  // extern "C"

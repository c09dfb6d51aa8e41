// engine_features.hip — the opt-in per-step features of a single-domain handle: surface tension and particle
// tracking (§12).  Their state and what the step enqueues for them: SurfaceTension / Tracking (engine.h).
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "engine.h"

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
    return FS_OK;
}

fs_status fs_track_disable(fs_sim* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    s->trk.channels = -1;           // the arrays stay allocated until the handle is destroyed
    return FS_OK;
}

int fs_track_channels(const fs_sim* s) { return s ? s->trk.channels : -1; }

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

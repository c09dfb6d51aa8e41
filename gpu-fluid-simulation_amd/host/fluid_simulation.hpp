// fluid_simulation.hpp — C++ host-side mirror of the reference's Rust interface for the hot
// path, layered on the C ABI (include/fluidsim.h).  Header-only; links libfluidsim_hip.so.
//
// The reference host code is Rust (src/simulation.rs, src/buffer.rs); this image has no Rust
// toolchain, so the host layer above the C ABI is C++ with the same names, argument meaning
// and error behaviour.  (The Rust twin is shipped as source in ../rust/.)
//
//   FluidSimulation::new_(settings)      <- FluidSimulation::new      src/simulation.rs:139
//   FluidSimulation::tick(tick_settings) <- FluidSimulation::tick     src/simulation.rs:459
//   FluidSimulation::tick_count()        <- pub tick: u32             src/simulation.rs:12
//   particles()/start_indices()/uniform()<- simulation_bg / simulation_settings_bg  :542-559
//   force_field_texture_write()          <- force_field_texture() + queue.write_buffer  :562, renderer.rs:497-502
//   ResizableBuffer<T>, SSBO<T>          <- src/buffer.rs:9-173
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fluidsim.h"

namespace fluidsim {

// The reference panics (unwrap / ilog2(0)); across a C ABI that becomes a status, and in this
// C++ mirror an exception carrying it.
struct Error : std::runtime_error {
    fs_status status;
    Error(fs_status s, const char* msg) : std::runtime_error(std::string("fluidsim: ") + msg), status(s) {}
};
inline void check(fs_status s) { if (s != FS_OK) throw Error(s, fs_last_error()); }

using SimulationSettings = fs_settings;   // src/simulation.rs:95-104
using TickSettings = fs_tick_settings;    // src/simulation.rs:107-122
using ParticleInstance = fs_particle;     // src/simulation.rs:126-135
using SimulationUniform = fs_uniform;     // src/simulation.rs:53-90
using Sample = fs_sample;                 // build extension: field sampling

// Defaults: src/main.rs:48-54, src/renderer.rs:16.
inline SimulationSettings default_settings() {
    return SimulationSettings{100000u, 0.1f, 0.2f, fs_vec2{53.0f, 53.0f}, fs_uvec2{1024u, 1024u}};
}
// Defaults: src/renderer.rs:374-388.
inline TickSettings default_tick_settings() {
    TickSettings t{};
    t.delta = 1.0f / 120.0f; t.gravity = fs_vec2{0.0f, 0.0f}; t.mass = 1.0f; t.pressure_constant = 50.0f;
    t.rest_density = 0.0f; t.damping_factor = 0.1f; t.viscosity_coefficient = 25.0f;
    t.surface_tension_treshold = 0.1f; t.surface_tension_coefficient = 35.0f; t.mouse_force_radius = 5.0f;
    t.mouse_force_power = 150.0f; t.mouse_pos = fs_vec2{0.0f, 0.0f}; t.mouse_state = 0;
    return t;
}

class FluidSimulation {
public:
    // FluidSimulation::new(&device, settings): `device` is a HIP ordinal here.
    static FluidSimulation new_(int device, const SimulationSettings& settings) {
        FluidSimulation s;
        check(fs_create(&settings, device, &s.h_));
        return s;
    }
    static FluidSimulation with_options(const SimulationSettings& settings, const fs_options& opts) {
        FluidSimulation s;
        check(fs_create_ex(&settings, &opts, &s.h_));
        return s;
    }
    FluidSimulation(FluidSimulation&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    FluidSimulation& operator=(FluidSimulation&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    FluidSimulation(const FluidSimulation&) = delete;
    FluidSimulation& operator=(const FluidSimulation&) = delete;
    ~FluidSimulation() { reset(); }

    // tick(&mut self, queue, encoder, settings): enqueues on the simulation's HIP stream and
    // returns immediately (the reference only records; submit is src/main.rs:226).
    void tick(const TickSettings& t) { check(fs_step(h_, &t)); }
    void wait() { check(fs_sync(h_)); }                       // device.poll(Wait), src/main.rs:79
    uint32_t tick_count() const { return fs_tick_count(h_); }
    uint32_t particle_count() const { return fs_particle_count(h_); }

    // Device pointers for a renderer (the bind-group accessors of the reference).
    const ParticleInstance* particles() { const fs_particle* p = nullptr; check(fs_particles_device(h_, &p)); return p; }
    const uint32_t* start_indices(size_t* count = nullptr) { const uint32_t* p = nullptr; check(fs_start_indices_device(h_, &p, count)); return p; }
    SimulationUniform uniform() const { SimulationUniform u; check(fs_get_uniform(h_, &u)); return u; }
    void force_field_texture_write(const fs_vec2* field, uint32_t w, uint32_t h) { check(fs_upload_force_field(h_, field, w, h)); }

    std::vector<ParticleInstance> download() {
        std::vector<ParticleInstance> v(particle_count());
        check(fs_download_particles(h_, v.data(), v.size()));
        return v;
    }
    void upload(const std::vector<ParticleInstance>& v) { check(fs_upload_particles(h_, v.data(), v.size())); }
    // Build extension, NOT in the reference: colour-field surface tension (include/fluidsim.h), single-domain handles.
    void set_surface_tension(bool enable) { check(fs_set_surface_tension(h_, enable ? 1 : 0)); }
    bool surface_tension_enabled() const { return fs_surface_tension_enabled(h_) != 0; }
    // channel diffusion and buoyancy: tracking must be on; track / untrack clear the settings
    void set_diffusion(int channel, float conductivity) { check(fs_set_diffusion(h_, channel, conductivity)); }
    float diffusion(int channel) const { float k = 0.0f; check(fs_get_diffusion(h_, channel, &k)); return k; }
    void set_buoyancy(int channel, float beta, float reference = 0.0f) { check(fs_set_buoyancy(h_, channel, beta, reference)); }
    void clear_buoyancy() { check(fs_set_buoyancy(h_, -1, 0.0f, 0.0f)); }
    bool buoyancy(int* channel, float* beta, float* reference) const {      // false: no buoyancy channel
        check(fs_get_buoyancy(h_, channel, beta, reference));
        return *channel >= 0;
    }
    std::vector<fs_vec2> buoyancy_forces() {                                 // the last buoyancy step's fb per particle, download order
        std::vector<fs_vec2> v(particle_count());
        check(fs_download_buoyancy(h_, v.data(), v.size()));
        return v;
    }
    std::vector<fs_vec2> surface_tension_forces() {
        std::vector<fs_vec2> v(particle_count());
        check(fs_download_surface_tension(h_, v.data(), v.size()));
        return v;
    }
    // Build extension, NOT in the reference: particle tracking (include/fluidsim.h), single-domain handles.  Every particle gets
    // an id (its current slot) and `channels` float attributes (all 0) that follow it through the sort of every later step.
    void track(int channels = 0) { check(fs_track_enable(h_, channels)); }
    void untrack() { check(fs_track_disable(h_)); }
    int track_channels() const { return fs_track_channels(h_); }   // -1: off
    std::vector<uint32_t> particle_ids() {
        std::vector<uint32_t> v(particle_count());
        check(fs_track_download_ids(h_, v.data(), v.size()));
        return v;
    }
    void set_particle_ids(const std::vector<uint32_t>& v) { check(fs_track_upload_ids(h_, v.data(), v.size())); }
    std::vector<float> attribute(int channel) {
        std::vector<float> v(particle_count());
        check(fs_track_download_attr(h_, channel, v.data(), v.size()));
        return v;
    }
    void set_attribute(int channel, const std::vector<float>& v) { check(fs_track_upload_attr(h_, channel, v.data(), v.size())); }
    const uint32_t* particle_ids_device() { const uint32_t* p = nullptr; check(fs_track_ids_device(h_, &p)); return p; }
    const float* attribute_device(int channel) { const float* p = nullptr; check(fs_track_attr_device(h_, channel, &p)); return p; }
    // dst[id] = the record of the particle with that id; entries that no id names are left as they are
    void download_by_id(std::vector<ParticleInstance>& dst) { check(fs_download_particles_by_id(h_, dst.data(), dst.size())); }
    // 2D particle count: `capacity` slots of which particle_count() are live.  reserve: grow-only, blocking, everything observable
    // is preserved; refused once a renderer hand-off is registered (size that handle with fs_options.capacity).  emit /
    // emit_nozzle append behind the live particles (count + n <= capacity), the nozzle's nu x nv records generated on the
    // device (nv == 1: a line).  remove_box (lo <= position <= hi on both axes) and remove (flags[i] != 0, one per particle)
    // are blocking stable compactions and return how many particles went.
    uint32_t capacity() const { return fs_capacity(h_); }
    void reserve(uint32_t capacity) { check(fs_reserve(h_, capacity)); }
    void emit(const std::vector<ParticleInstance>& v) { check(fs_emit_particles(h_, v.data(), v.size())); }
    void emit_nozzle(const fs_nozzle& nozzle) { check(fs_emit_nozzle(h_, &nozzle)); }
    uint32_t remove_box(fs_vec2 lo, fs_vec2 hi) { uint32_t n = 0; check(fs_remove_in_box(h_, &lo, &hi, &n)); return n; }
    uint32_t remove(const std::vector<uint8_t>& flags) { uint32_t n = 0; check(fs_remove_flagged(h_, flags.data(), flags.size(), &n)); return n; }
    uint32_t next_id() const { return fs_track_next_id(h_); }       // of the next emitted particle while tracking is on; 0: off
    // Build extension, NOT in the reference: 2D moving bodies (include/fluidsim.h), single-domain handles.  w * h push vectors in
    // world units over the body's own box [-extent/2, extent/2] in the body frame.  add_body* return the slot (the lowest free one
    // of 0 .. FS_MAX_BODIES - 1) and block; the body starts at the origin with the identity pose, at rest.  set_body_motion: host
    // memory only, for the ticks enqueued afterwards; the engine does not advance the pose.
    uint32_t add_body(const std::vector<fs_vec2>& field, uint32_t w, uint32_t h, fs_vec2 extent) {
        if (field.size() != (size_t)w * h) throw std::invalid_argument("add_body: field.size() != w * h");
        uint32_t slot = 0;
        check(fs_body_create(h_, field.data(), w, h, extent, &slot));
        return slot;
    }
    uint32_t add_body_mask(const std::vector<uint8_t>& mask, uint32_t w, uint32_t h, fs_vec2 extent) {
        if (mask.size() != (size_t)w * h) throw std::invalid_argument("add_body_mask: mask.size() != w * h");
        uint32_t slot = 0;
        check(fs_body_create_from_mask(h_, mask.data(), w, h, extent, nullptr, &slot));
        return slot;
    }
    void set_body_motion(uint32_t body, const fs_body_motion& motion) { check(fs_body_set_motion(h_, body, &motion)); }
    fs_body_motion body_motion(uint32_t body) const { fs_body_motion m{}; check(fs_body_get_motion(h_, body, &m)); return m; }
    std::vector<fs_vec2> body_field(uint32_t body) {
        uint32_t w = 0, h = 0;
        fs_vec2 extent{};
        check(fs_body_dims(h_, body, &w, &h, &extent));
        std::vector<fs_vec2> v((size_t)w * h);
        check(fs_body_download(h_, body, v.data(), v.size()));
        return v;
    }
    void remove_body(uint32_t body) { check(fs_body_destroy(h_, body)); }
    uint32_t body_count() const { return fs_body_count(h_); }
    // Build extension: 2D body loads (include/fluidsim.h).  The impulse and angular impulse the fluid hands each body, as 64-bit
    // fixed-point sums (2^-FS_BODY_LOAD_SHIFT per unit particle mass); enabling zeroes them, the particles stay the same bytes.
    void enable_body_loads(bool on = true) { check(fs_body_loads_enable(h_, on ? 1 : 0)); }
    bool body_loads_enabled() const { return fs_body_loads_enabled(h_) != 0; }
    fs_body_load body_loads(uint32_t body, bool reset = false) {          // blocking
        fs_body_load l{};
        check(fs_body_loads(h_, body, &l, reset ? 1 : 0));
        return l;
    }
    const void* body_loads_device() { const void* p = nullptr; check(fs_body_loads_device(h_, &p)); return p; }
    // Build extension: fluid diagnostics (include/fluidsim.h).  Momentum, energy, centre of mass, density range, bounding box,
    // channel sums and a count of non-finite particles as exact integer words, reduced on the GPU; observing only.
    fs_stats stats() { fs_stats r{}; check(fs_stats_read(h_, &r)); return r; }                 // blocking
    void stats_device(fs_stats* out_dev) { check(fs_stats_device(h_, out_dev)); }              // stream-ordered, no host read
    // Build extension, NOT in the reference: field sampling (include/fluidsim.h), single-domain handles.  Density, Shepard weight,
    // un-normalised velocity sum, neighbour count and cell of the fluid at any points; `attr` (may be null) receives the channel
    // sums, channel c of query k at c * n + k.  Needs a tick since creation / the last upload.  Coherently ordered points are
    // sampled several times faster than shuffled ones.
    std::vector<Sample> sample(const std::vector<fs_vec2>& points, std::vector<float>* attr = nullptr) {
        std::vector<Sample> out(points.size());
        if (attr) attr->assign((size_t)(track_channels() > 0 ? track_channels() : 0) * points.size(), 0.0f);
        check(fs_sample_points(h_, points.data(), points.size(), out.data(), attr ? attr->data() : nullptr));
        return out;
    }
    // ... at the pixel centres of `view` (fs_render_density's mapping), row-major; bit-identical to sample() on those points
    std::vector<Sample> sample_grid(const fs_view& view, std::vector<float>* attr = nullptr) {
        const size_t n = (size_t)view.width * view.height;
        std::vector<Sample> out(n);
        if (attr) attr->assign((size_t)(track_channels() > 0 ? track_channels() : 0) * n, 0.0f);
        check(fs_sample_grid(h_, &view, out.data(), attr ? attr->data() : nullptr));
        return out;
    }
    // ... with device pointers, enqueued on the simulation's stream after the ticks in flight; non-blocking
    void sample_device(const fs_vec2* points_dev, size_t n, Sample* out_dev, float* attr_out_dev = nullptr) {
        check(fs_sample_points_device(h_, points_dev, n, out_dev, attr_out_dev));
    }
    fs_sim* handle() { return h_; }

private:
    FluidSimulation() = default;
    void reset() { if (h_) fs_destroy(h_); h_ = nullptr; }
    fs_sim* h_ = nullptr;
};

// Build extension, NOT in the reference (2D only): the 3D step (include/fluidsim.h fs3_*) and its field sampling.
using Sample3 = fs3_sample;
using Camera3 = fs3_camera;               // build extension: 3D surface rendering
using SurfaceParams3 = fs3_surface_params;
using SurfaceHit3 = fs3_surface_hit;
static_assert(sizeof(Camera3) == 64 && sizeof(SurfaceParams3) == 20 && sizeof(SurfaceHit3) == 40, "3D surface rendering records");
using MeshVertex3 = fs3_mesh_vertex;      // build extension: 3D surface extraction
static_assert(sizeof(MeshVertex3) == 40, "fs3_mesh_vertex is 40 bytes");
struct Mesh3 {
    std::vector<MeshVertex3> vertices;
    std::vector<uint32_t> triangles;      // three indices per triangle, outward winding
};
class FluidSimulation3D {
public:
    static FluidSimulation3D new_(int device, const fs3_settings& settings, fs_vec3 initial_offset = fs_vec3{0.0f, 0.0f, 0.0f},
                                  int math_mode = FS_MATH_IEEE) {
        FluidSimulation3D s;
        check(fs3_create_ex(&settings, device, initial_offset, math_mode, &s.h_));
        return s;
    }
    FluidSimulation3D(FluidSimulation3D&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    FluidSimulation3D& operator=(FluidSimulation3D&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    FluidSimulation3D(const FluidSimulation3D&) = delete;
    FluidSimulation3D& operator=(const FluidSimulation3D&) = delete;
    ~FluidSimulation3D() { reset(); }

    void tick(const fs3_tick_settings& t) { check(fs3_step(h_, &t)); }
    void wait() { check(fs3_sync(h_)); }
    uint32_t tick_count() const { return fs3_tick_count(h_); }
    uint32_t particle_count() const { return fs3_particle_count(h_); }
    void* stream() const { return fs3_stream(h_); }
    std::vector<fs3_particle> download() {
        std::vector<fs3_particle> v(particle_count());
        check(fs3_download_particles(h_, v.data(), v.size()));
        return v;
    }
    void upload(const std::vector<fs3_particle>& v) { check(fs3_upload_particles(h_, v.data(), v.size())); }
    // 3D field sampling: density, Shepard weight, un-normalised velocity sum, density gradient (-gradient is the outward normal),
    // neighbour count and cell of the fluid at any points.  Needs a tick since creation / the last upload.  Coherently ordered
    // points are sampled several times faster than shuffled ones.
    std::vector<Sample3> sample(const std::vector<fs_vec3>& points) {
        std::vector<Sample3> out(points.size());
        check(fs3_sample_points(h_, points.data(), points.size(), out.data()));
        return out;
    }
    // ... at the voxel centres of `view`, voxel (i, j, k) at (k * height + j) * width + i; bit-identical to sample() on those points
    std::vector<Sample3> sample_grid(const fs3_view& view) {
        std::vector<Sample3> out((size_t)view.width * view.height * view.depth);
        check(fs3_sample_grid(h_, &view, out.data()));
        return out;
    }
    // ... with device pointers, enqueued on the simulation's stream after the ticks in flight; non-blocking
    void sample_device(const fs_vec3* points_dev, size_t n, Sample3* out_dev) { check(fs3_sample_points_device(h_, points_dev, n, out_dev)); }
    // 3D surface rendering: ray-marches the density's iso-surface into a G-buffer (distance, density, outward normal, Shepard
    // velocity, march index, hit kind), pixel (i, j) at j * width + i.  Blocking; needs a tick since creation / the last upload.
    std::vector<SurfaceHit3> render_surface(const Camera3& camera, const SurfaceParams3& params) {
        std::vector<SurfaceHit3> out((size_t)camera.width * camera.height);
        check(fs3_render_surface(h_, &camera, &params, out.data()));
        return out;
    }
    // ... into a device buffer, enqueued on the simulation's stream after the ticks in flight; non-blocking
    void render_surface_device(const Camera3& camera, const SurfaceParams3& params, SurfaceHit3* out_dev) {
        check(fs3_render_surface_device(h_, &camera, &params, out_dev));
    }
    // 3D surface extraction: surface nets over the width x height x depth lattice nodes of `view` (each >= 2), at exact size in
    // two calls: the counts, then the arrays.  Blocking; needs a tick since creation / the last upload.
    Mesh3 extract_surface(const fs3_view& view, float iso) {
        uint32_t counts[2] = {0, 0};
        check(fs3_extract_surface(h_, &view, iso, nullptr, 0, nullptr, 0, counts));
        Mesh3 m;
        m.vertices.resize(counts[0]);
        m.triangles.resize(3 * (size_t)counts[1]);
        if (counts[0] || counts[1])
            check(fs3_extract_surface(h_, &view, iso, counts[0] ? m.vertices.data() : nullptr, counts[0],
                                      counts[1] ? m.triangles.data() : nullptr, counts[1], counts));
        return m;
    }
    // ... into device buffers (vert_cap records, 3 * tri_cap indices, two counts), enqueued on the simulation's stream after the
    // ticks in flight; no host read.  The counts are always the full ones.
    void extract_surface_device(const fs3_view& view, float iso, MeshVertex3* verts_dev, uint32_t vert_cap, uint32_t* tris_dev,
                                uint32_t tri_cap, uint32_t* counts_dev) {
        check(fs3_extract_surface_device(h_, &view, iso, verts_dev, vert_cap, tris_dev, tri_cap, counts_dev));
    }
    // 3D colliders: w * h * d push vectors in world units over the whole domain, voxel (i, j, k) at (k * h + j) * w + i, zero = free
    // space.  Blocking; holds for the ticks enqueued afterwards.  set_collider_mask: from a voxel mask (> 128: solid).
    void set_collider(const std::vector<fs_vec3>& field, uint32_t w, uint32_t h, uint32_t d) {
        if (field.size() != (size_t)w * h * d) throw std::invalid_argument("set_collider: field.size() != w * h * d");
        check(fs3_collider_upload(h_, field.data(), w, h, d));
    }
    void set_collider_mask(const std::vector<uint8_t>& mask, uint32_t w, uint32_t h, uint32_t d) {
        if (mask.size() != (size_t)w * h * d) throw std::invalid_argument("set_collider_mask: mask.size() != w * h * d");
        check(fs3_collider_from_mask(h_, mask.data(), w, h, d, nullptr));
    }
    void clear_collider() { check(fs3_collider_clear(h_)); }
    std::vector<fs_vec3> collider() {      // empty when none is set
        uint32_t w = 0, h = 0, d = 0;
        check(fs3_collider_dims(h_, &w, &h, &d));
        std::vector<fs_vec3> v((size_t)w * h * d);
        if (!v.empty()) check(fs3_collider_download(h_, v.data(), v.size()));
        return v;
    }
    // 3D moving bodies: w * h * d push vectors over the body's own box [-extent/2, extent/2] in the body frame, the layout of
    // set_collider.  add_body* return the slot (the lowest free one of 0 .. FS3_MAX_BODIES - 1) and block; the body starts at the
    // origin with the identity pose, at rest.  set_body_motion: host memory only, for the ticks enqueued afterwards; the engine
    // does not advance the pose.
    uint32_t add_body(const std::vector<fs_vec3>& field, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent) {
        if (field.size() != (size_t)w * h * d) throw std::invalid_argument("add_body: field.size() != w * h * d");
        uint32_t slot = 0;
        check(fs3_body_create(h_, field.data(), w, h, d, extent, &slot));
        return slot;
    }
    uint32_t add_body_mask(const std::vector<uint8_t>& mask, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent) {
        if (mask.size() != (size_t)w * h * d) throw std::invalid_argument("add_body_mask: mask.size() != w * h * d");
        uint32_t slot = 0;
        check(fs3_body_create_from_mask(h_, mask.data(), w, h, d, extent, nullptr, &slot));
        return slot;
    }
    void set_body_motion(uint32_t body, const fs3_body_motion& motion) { check(fs3_body_set_motion(h_, body, &motion)); }
    fs3_body_motion body_motion(uint32_t body) const { fs3_body_motion m{}; check(fs3_body_get_motion(h_, body, &m)); return m; }
    std::vector<fs_vec3> body_field(uint32_t body) {
        uint32_t w = 0, h = 0, d = 0;
        fs_vec3 extent{};
        check(fs3_body_dims(h_, body, &w, &h, &d, &extent));
        std::vector<fs_vec3> v((size_t)w * h * d);
        check(fs3_body_download(h_, body, v.data(), v.size()));
        return v;
    }
    void remove_body(uint32_t body) { check(fs3_body_destroy(h_, body)); }
    uint32_t body_count() const { return fs3_body_count(h_); }
    // 3D body loads (include/fluidsim.h "3D body loads"): what the fluid hands each body, summed on the GPU in fixed point.
    void enable_body_loads(bool on = true) { check(fs3_body_loads_enable(h_, on ? 1 : 0)); }
    bool body_loads_enabled() const { return fs3_body_loads_enabled(h_) != 0; }
    fs3_body_load body_loads(uint32_t body, bool reset = false) {         // blocking
        fs3_body_load l{};
        check(fs3_body_loads(h_, body, &l, reset ? 1 : 0));
        return l;
    }
    const void* body_loads_device() { const void* p = nullptr; check(fs3_body_loads_device(h_, &p)); return p; }
    // 3D fluid diagnostics (include/fluidsim.h "3D fluid diagnostics"): the 2D record with three components; observing only.
    fs3_stats stats() { fs3_stats r{}; check(fs3_stats_read(h_, &r)); return r; }              // blocking
    void stats_device(fs3_stats* out_dev) { check(fs3_stats_device(h_, out_dev)); }            // stream-ordered, no host read
    // 3D surface tension: colour-field CSF with coefficient sigma and threshold tau, for the ticks enqueued afterwards.
    void set_surface_tension(float coefficient, float threshold = 0.0f) { check(fs3_set_surface_tension(h_, 1, coefficient, threshold)); }
    void clear_surface_tension() { check(fs3_set_surface_tension(h_, 0, 0.0f, 0.0f)); }
    bool surface_tension_enabled() const { return fs3_surface_tension_enabled(h_) != 0; }
    std::pair<float, float> surface_tension_params() const {      // (coefficient, threshold); throws when the feature is off
        float c = 0.0f, t = 0.0f;
        check(fs3_surface_tension_params(h_, &c, &t));
        return {c, t};
    }
    std::vector<fs_vec3> surface_tension_forces() {               // the last step's force per particle, download order
        std::vector<fs_vec3> v(particle_count());
        check(fs3_download_surface_tension(h_, v.data(), v.size()));
        return v;
    }
    // 3D channel diffusion and buoyancy: tracking must be on; track / untrack clear the settings
    void set_diffusion(int channel, float conductivity) { check(fs3_set_diffusion(h_, channel, conductivity)); }
    float diffusion(int channel) const { float k = 0.0f; check(fs3_get_diffusion(h_, channel, &k)); return k; }
    void set_buoyancy(int channel, float beta, float reference = 0.0f) { check(fs3_set_buoyancy(h_, channel, beta, reference)); }
    void clear_buoyancy() { check(fs3_set_buoyancy(h_, -1, 0.0f, 0.0f)); }
    bool buoyancy(int* channel, float* beta, float* reference) const {      // false: no buoyancy channel
        check(fs3_get_buoyancy(h_, channel, beta, reference));
        return *channel >= 0;
    }
    std::vector<fs_vec3> buoyancy_forces() {                                 // the last buoyancy step's fb per particle, download order
        std::vector<fs_vec3> v(particle_count());
        check(fs3_download_buoyancy(h_, v.data(), v.size()));
        return v;
    }
    // 3D particle count: `capacity` slots of which particle_count() are live.  reserve: grow-only, blocking, everything observable
    // is preserved.  emit / emit_nozzle append behind the live particles (count + n <= capacity), the nozzle's layer of nu x nv
    // records generated on the device.  remove_box (lo <= position <= hi on every axis) and remove (flags[i] != 0, one per
    // particle in download order) are blocking and stable, and return how many particles went.
    uint32_t capacity() const { return fs3_capacity(h_); }
    void reserve(uint32_t capacity) { check(fs3_reserve(h_, capacity)); }
    void emit(const std::vector<fs3_particle>& v) { check(fs3_emit_particles(h_, v.data(), v.size())); }
    void emit_nozzle(const fs3_nozzle& nozzle) { check(fs3_emit_nozzle(h_, &nozzle)); }
    uint32_t remove_box(fs_vec3 lo, fs_vec3 hi) { uint32_t n = 0; check(fs3_remove_in_box(h_, &lo, &hi, &n)); return n; }
    uint32_t remove(const std::vector<uint8_t>& flags) { uint32_t n = 0; check(fs3_remove_flagged(h_, flags.data(), flags.size(), &n)); return n; }
    uint32_t next_id() const { return fs3_track_next_id(h_); }      // of the next emitted particle while tracking is on; 0: off
    // 3D particle tracking: every particle gets an id (its current slot) and `channels` float attributes (all 0) that follow it
    // through the sort of every later tick.
    void track(int channels = 0) { check(fs3_track_enable(h_, channels)); }
    void untrack() { check(fs3_track_disable(h_)); }
    int track_channels() const { return fs3_track_channels(h_); }   // -1: off
    std::vector<uint32_t> particle_ids() {
        std::vector<uint32_t> v(particle_count());
        check(fs3_track_download_ids(h_, v.data(), v.size()));
        return v;
    }
    void set_particle_ids(const std::vector<uint32_t>& v) { check(fs3_track_upload_ids(h_, v.data(), v.size())); }
    std::vector<float> attribute(int channel) {
        std::vector<float> v(particle_count());
        check(fs3_track_download_attr(h_, channel, v.data(), v.size()));
        return v;
    }
    void set_attribute(int channel, const std::vector<float>& v) { check(fs3_track_upload_attr(h_, channel, v.data(), v.size())); }
    const uint32_t* particle_ids_device() { const uint32_t* p = nullptr; check(fs3_track_ids_device(h_, &p)); return p; }
    const float* attribute_device(int channel) { const float* p = nullptr; check(fs3_track_attr_device(h_, channel, &p)); return p; }
    // dst[id] = the record of the particle with that id; entries that no id names are left as they are
    void download_by_id(std::vector<fs3_particle>& dst) { check(fs3_download_particles_by_id(h_, dst.data(), dst.size())); }
    // 3D channel sampling: the un-normalised SPH sums of the tracking channels at any points, channel c of query q at c * n + q;
    // `weight` (may be null) receives the Shepard denominators.  Needs track(channels >= 1) and a tick since the last upload.
    std::vector<float> sample_attr(const std::vector<fs_vec3>& points, std::vector<float>* weight = nullptr) {
        std::vector<float> attr((size_t)(track_channels() > 0 ? track_channels() : 0) * points.size(), 0.0f);
        if (weight) weight->assign(points.size(), 0.0f);
        check(fs3_sample_attr_points(h_, points.data(), points.size(), weight ? weight->data() : nullptr, attr.data()));
        return attr;
    }
    // ... at the voxel centres of `view` (sample_grid's order); bit-identical to sample_attr() on those points
    std::vector<float> sample_attr_grid(const fs3_view& view, std::vector<float>* weight = nullptr) {
        const size_t n = (size_t)view.width * view.height * view.depth;
        std::vector<float> attr((size_t)(track_channels() > 0 ? track_channels() : 0) * n, 0.0f);
        if (weight) weight->assign(n, 0.0f);
        check(fs3_sample_attr_grid(h_, &view, weight ? weight->data() : nullptr, attr.data()));
        return attr;
    }
    // ... with device pointers, enqueued on the simulation's stream after the ticks in flight; non-blocking
    void sample_attr_device(const fs_vec3* points_dev, size_t n, float* weight_out_dev, float* attr_out_dev) {
        check(fs3_sample_attr_points_device(h_, points_dev, n, weight_out_dev, attr_out_dev));
    }
    fs_sim3* handle() { return h_; }

private:
    FluidSimulation3D() = default;
    void reset() { if (h_) fs3_destroy(h_); h_ = nullptr; }
    fs_sim3* h_ = nullptr;
};

// ResizableBuffer<T> — src/buffer.rs:17-88.
template <class T>
class ResizableBuffer {
public:
    ResizableBuffer(const char* name, int device, size_t len) { check(fs_buffer_create(device, sizeof(T), len, name, &b_)); }
    ~ResizableBuffer() { if (b_) fs_buffer_destroy(b_); }
    ResizableBuffer(const ResizableBuffer&) = delete;
    ResizableBuffer& operator=(const ResizableBuffer&) = delete;
    bool resize(size_t new_cap) { int r = 0; check(fs_buffer_resize(b_, new_cap, &r)); return r != 0; }   // :46-67
    void write(size_t offset, const T* data, size_t count) { check(fs_buffer_write(b_, offset, data, count)); }  // :70-87
    size_t len() const { return fs_buffer_len(b_); }
    T* buffer() const { return static_cast<T*>(fs_buffer_device_ptr(b_)); }
protected:
    fs_buffer* b_ = nullptr;
};

// SSBO<T> — src/buffer.rs:9-14,91-173: a ResizableBuffer plus its binding; with HIP the
// "bind group" is just the device pointer.
template <class T>
class SSBO : public ResizableBuffer<T> {
public:
    using ResizableBuffer<T>::ResizableBuffer;
    void resize(size_t new_cap) { if (new_cap > this->len()) (void)ResizableBuffer<T>::resize(new_cap); }  // :127-150
    void update(const T* data, size_t count) { this->write(0, data, count); }                              // :153-155
    T* bind_group() const { return this->buffer(); }                                                       // :162-164
};

}  // namespace fluidsim

/*
 * fluidsim.h — C ABI of the MI355X-native SPH fluid-step engine.
 *
 * This is the drop-in boundary for the reference's per-tick hot path
 * (rookieCookies/gpu-fluid-simulation).  Every entry point cites the reference
 * interface it replaces as file:line relative to the reference tree.  Plain
 * pointers and sizes only; no C++/torch types cross this boundary; nothing here
 * throws or aborts — every call returns an fs_status.
 *
 * Reference surface mirrored here:
 *   FluidSimulation::new      src/simulation.rs:139-455
 *   FluidSimulation::tick     src/simulation.rs:459-539
 *   accessors                 src/simulation.rs:542-564
 *   ParticleInstance (32 B)   src/simulation.rs:126-135, funcs.wgsl:1-8
 *   SimulationUniform (120 B) src/simulation.rs:53-90,   funcs.wgsl:17-51
 *   SimulationSettings        src/simulation.rs:95-104
 *   TickSettings              src/simulation.rs:107-122
 *   ResizableBuffer<T>/SSBO<T> src/buffer.rs:9-173
 */
#ifndef FLUIDSIM_H
#define FLUIDSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 2

/* ------------------------------------------------------------------ status */
typedef enum fs_status {
    FS_OK = 0,
    FS_ERR_INVALID = 1,      /* bad argument; N <= 1 (reference panics: simulation.rs:323-324) */
    FS_ERR_DEVICE = 2,       /* HIP runtime error (message in fs_last_error) */
    FS_ERR_OOM = 3,          /* device or host allocation failed */
    FS_ERR_UNSUPPORTED = 4,  /* option combination not built */
    FS_ERR_COMM = 5          /* RCCL error, or librccl could not be loaded (fs_comm_*, fs_slab_exchange) */
} fs_status;

/* ------------------------------------------------------------------- PODs */
typedef struct fs_vec2 { float x, y; } fs_vec2;
typedef struct fs_vec3 { float x, y, z; } fs_vec3;
typedef struct fs_uvec2 { uint32_t x, y; } fs_uvec2;

/* SimulationSettings — src/simulation.rs:95-104 (same fields, same order). */
typedef struct fs_settings {
    uint32_t particle_count;
    float particle_spacing;
    float smoothing_radius;
    fs_vec2 size;
    fs_uvec2 texture_size;
} fs_settings;

/* TickSettings — src/simulation.rs:107-122 (same fields, same order). */
typedef struct fs_tick_settings {
    float delta;
    fs_vec2 gravity;
    float mass;
    float pressure_constant;
    float rest_density;
    float damping_factor;
    float viscosity_coefficient;
    float surface_tension_treshold;     /* sic — spelling follows the reference */
    float surface_tension_coefficient;
    float mouse_force_radius;
    float mouse_force_power;
    fs_vec2 mouse_pos;
    int32_t mouse_state;
} fs_tick_settings;

/* ParticleInstance — src/simulation.rs:126-135; 32 bytes, offsets 0/8/16/24/28. */
typedef struct fs_particle {
    fs_vec2 position;
    fs_vec2 predicted_position;
    fs_vec2 velocity;
    float density;
    uint32_t grid;
} fs_particle;

/* SimulationUniform — src/simulation.rs:53-90; 120 bytes. */
typedef struct fs_uniform {
    float delta;
    uint32_t particle_count;
    float sqr_radius;
    uint32_t frame_time;
    fs_vec2 gravity;
    fs_vec2 bounds;
    fs_vec2 mouse_pos;
    float smoothing_radius;
    float particle_mass;
    float pressure_constant;
    float rest_density;
    float damping_factor;
    float viscosity_coefficient;
    float surface_tension_treshold;
    float surface_tension_coefficient;
    float poly6_kernel_volume;
    float poly6_kernel_derivative;
    float poly6_kernel_laplacian;
    float spiky_kernel_derivative;
    float viscosity_kernel;
    int32_t mouse_state;
    float mouse_force_radius;
    float mouse_force_power;
    uint32_t grid_w;
    uint32_t grid_h;
    fs_vec2 texture_size;
} fs_uniform;

/* SortUniform payload — src/simulation.rs:40-50 (without the 240-byte pad). */
typedef struct fs_sort_step {
    uint32_t group_width;
    uint32_t group_height;
    uint32_t step_index;
    uint32_t num_values;
} fs_sort_step;

/* Build-defined options (NOT in the reference; defaults reproduce the reference). */
typedef enum fs_sort_mode {
    FS_SORT_BITONIC = 0,   /* reference network (sort.wgsl:27-51): bit-exact permutation */
    FS_SORT_COUNTING = 1   /* O(N) cell counting sort; stable within a cell */
} fs_sort_mode;

typedef enum fs_math_mode {
    FS_MATH_IEEE = 0,      /* correctly rounded / and sqrt, no contraction: bit-identical to the CPU oracle */
    FS_MATH_WGSL_ULP = 1,  /* native rcp / sqrt in the force pass (<= ~1.5 ulp): within WGSL's own accuracy
                              contract for the reference shaders (division 2.5 ULP, sqrt 2 ULP), not bit-exact */
    FS_MATH_TOLERANCE = 2  /* density and force terms re-associated for speed (FMA, one rsqrt per pair, pressure and
                              1/density precomputed per particle): positions / velocities / densities within
                              rtol 1e-5, atol 1e-4*h of the IEEE oracle per step (north_star's float contract);
                              cell keys and start_indices remain bit-exact.  Never the default. */
} fs_math_mode;

typedef struct fs_options {
    int32_t device;            /* HIP device ordinal */
    int32_t sort_mode;         /* fs_sort_mode */
    int32_t ref_quirks;        /* 1 = reproduce compute.wgsl:49-55 stale cell-start behaviour */
    int32_t math_mode;         /* fs_math_mode (default FS_MATH_IEEE) */
    fs_vec2 initial_offset;    /* translation added to the reference lattice (dam-break scene) */
    uint32_t capacity;         /* particle slots to allocate (0 = particle_count); multi-GPU slabs */
    uint32_t reserved1;
} fs_options;

typedef struct fs_sim fs_sim;       /* opaque: one simulation, one HIP stream */
typedef struct fs_buffer fs_buffer; /* opaque: ResizableBuffer<T> */

/* ------------------------------------------------------------- lifecycle */
/* FluidSimulation::new (src/simulation.rs:139): builds the reference lattice
 * (:147-163), zeroed start_indices (:204-209) and force field (:213-218).
 * device = HIP ordinal.  N <= 1 -> FS_ERR_INVALID (reference: ilog2(0) panic);
 * N (or options.capacity) > 2^28 -> FS_ERR_INVALID (32-bit byte offsets in the kernels). */
fs_status fs_create(const fs_settings* settings, int device, fs_sim** out);
fs_status fs_create_ex(const fs_settings* settings, const fs_options* opts, fs_sim** out);
void fs_options_default(fs_options* opts);
/* Drop of FluidSimulation (Renderer owns it: src/renderer.rs:31). */
void fs_destroy(fs_sim* sim);

/* --------------------------------------------------------------- stepping */
/* FluidSimulation::tick (src/simulation.rs:459-539).  Pre-increments `tick`,
 * builds the 120-byte uniform (:470-497) and enqueues the whole pass chain on
 * the simulation's stream.  Non-blocking, like the reference (which only
 * records into a CommandEncoder; submit happens at src/main.rs:226).
 * FS_ERR_DEVICE from fs_step / fs_timed_steps is terminal for the handle: besides HIP runtime errors it reports that the
 * sort's stand-by kernel (csrc/kernels_sort_global.inc k_late_fallback, a persistent launch with a bounded-spin grid barrier)
 * timed out on a barrier in an EARLIER step — the host learns of it from the device's report a few steps later, and the
 * particle order of every step since is undefined.  Destroy the handle and re-create it (or re-upload a checkpoint into
 * a new one); no further call on the old handle is meaningful.  fs_sort_plan_info.timeouts counts such events
 * (0 on a healthy device: the grid is <= 128 workgroups on 256 CUs, all co-resident). */
fs_status fs_step(fs_sim* sim, const fs_tick_settings* tick);
/* device.poll(Wait) equivalent (src/main.rs:79). */
fs_status fs_sync(fs_sim* sim);
/* pub tick: u32 (src/simulation.rs:12). */
uint32_t fs_tick_count(const fs_sim* sim);
uint32_t fs_particle_count(const fs_sim* sim);
/* grid_w / grid_h (src/simulation.rs:140-141). */
fs_status fs_grid_dims(const fs_sim* sim, uint32_t* grid_w, uint32_t* grid_h);
/* The HIP stream the pass chain runs on (hipStream_t as void*). */
void* fs_stream(const fs_sim* sim);

/* ------------------------------------------- data the renderer consumes */
/* simulation_bg binding 0 (src/simulation.rs:552-559; fluid_shader.wgsl:38-75):
 * cell-sorted 32-byte AoS records, device pointer.  The engine keeps SoA state;
 * the AoS view is materialised on the stream by this call. */
fs_status fs_particles_device(fs_sim* sim, const fs_particle** out);
/* simulation_bg binding 1: start_indices u32[grid_w*grid_h] (persistent, never cleared). */
fs_status fs_start_indices_device(fs_sim* sim, const uint32_t** out, size_t* count);
/* simulation_settings_bg (src/simulation.rs:552-554): last uniform written by fs_step. */
fs_status fs_get_uniform(const fs_sim* sim, fs_uniform* out);
/* force_field_texture() (src/simulation.rs:562-564) + queue.write_buffer (src/renderer.rs:497-502). */
fs_status fs_upload_force_field(fs_sim* sim, const fs_vec2* field, uint32_t w, uint32_t h);

/* ---- hand-off without a host round trip --------------------------------------------
 * The reference's renderer binds the simulation's particle and start_indices buffers directly
 * (simulation_bg: src/simulation.rs:552-559, used at src/renderer.rs:457-458; fluid_shader.wgsl:38-75).
 * fs_export_handle gives a consumer in ANOTHER process (or another API) the same thing: an interprocess
 * handle of the device allocation holding the cell-sorted 32-byte records / the start_indices table.
 * Registering the particle export switches the engine to a LIVE AoS view: from the next fs_step on the force pass
 * writes the ParticleInstance records itself (no export pass, no copy); the consumer reads them after fs_sync
 * (or after its own wait on the step).  `ipc` is a hipIpcMemHandle_t (HIP consumers: fs_import_open);
 * `dmabuf_fd` is a dma-buf file descriptor of the same range for external-memory import by Vulkan / wgpu
 * (-1 when the runtime cannot export one); the caller owns and closes it. */
enum { FS_EXPORT_PARTICLES = 0, FS_EXPORT_START_INDICES = 1 };
typedef struct fs_mem_handle {
    uint8_t ipc[64];
    uint64_t bytes;       /* size of the exported range: particle_count * 32, or grid_w * grid_h * 4 */
    int32_t device;       /* HIP ordinal the allocation lives on */
    int32_t dmabuf_fd;
} fs_mem_handle;
fs_status fs_export_handle(fs_sim* sim, int which, fs_mem_handle* out);
/* Consumer side (any process with a HIP device): map an exported range, read from it, unmap. */
fs_status fs_import_open(const fs_mem_handle* handle, int device, void** dev_ptr);
fs_status fs_import_read(const void* dev_ptr, size_t offset, void* dst, size_t bytes);   /* blocking copy to host */
fs_status fs_import_close(void* dev_ptr);

/* Host copies (checkpoint / tests).  Blocking.  n = number of records. */
fs_status fs_download_particles(fs_sim* sim, fs_particle* dst, size_t n);
fs_status fs_upload_particles(fs_sim* sim, const fs_particle* src, size_t n);
fs_status fs_download_start_indices(fs_sim* sim, uint32_t* dst, size_t n);
fs_status fs_upload_start_indices(fs_sim* sim, const uint32_t* src, size_t n);

/* ------------------------------------------------- host-side mirrors (pure) */
/* Initial lattice, src/simulation.rs:147-163, f32 arithmetic as written. */
fs_status fs_reference_lattice(const fs_settings* settings, fs_vec2 offset, fs_particle* dst, size_t n);
/* Sort schedule, src/simulation.rs:323-347.  Returns the number of steps
 * S(S+1)/2; fills up to `cap` entries when dst != NULL. */
size_t fs_sort_schedule(uint32_t particle_count, fs_sort_step* dst, size_t cap);
/* Uniform construction, src/simulation.rs:470-497. */
fs_status fs_build_uniform(const fs_settings* settings, const fs_tick_settings* tick,
                           uint32_t tick_count, fs_uniform* out);

/* ------------------------------------------- obstacle field producer */
/* generate_smooth_gradient_field (src/main.rs:403-515): u8 mask (> 128 = obstacle source; none ->
 * the image border) -> per-pixel vector to the nearest source, by the reference's two-pass raster
 * propagation, reproduced exactly.  `field_host` may be NULL; with `sim` the result is also
 * written straight into the simulation's force field (the renderer's write_buffer,
 * src/renderer.rs:497-502), in which case (w, h) must equal settings.texture_size.  sim may be
 * NULL (then `device` selects the GPU).  Limits: h <= 1024, w < 65536.  The sweep is inherently sequential along
 * x + 2y (a pixel depends on its left / upper neighbours' RESULTS), so it runs as ONE workgroup — one thread per image
 * row, ~3 w + 2 h barrier steps — on one CU: ~1 ms at 1024^2, off the per-tick path (the reference runs it on a CPU
 * thread per rendered frame). */
fs_status fs_generate_force_field(fs_sim* sim, int device, const uint8_t* image, uint32_t w, uint32_t h,
                                  fs_vec2* field_host);

/* ------------------------------------------------- renderer hand-off */
/* Headless version of the reference's density-splat fragment shader (fluid_shader.wgsl:27-102):
 * per pixel a 5x5-cell walk over the cell-sorted particles, Gaussian splat of density and
 * speed, colour ramp.  The reference draws a full-screen quad through an orthographic
 * projection over the whole domain with +y down (src/renderer.rs:558-561); `fs_view` is that
 * mapping made explicit: pixel (i, j) samples world_min + ((i+0.5)/width, (j+0.5)/height) *
 * (world_max - world_min).  Output: width*height RGBA f32 (straight alpha), host memory.
 *
 * The pixel's cell is funcs.wgsl:212-214 in f32 with the true division (saturating f32 -> u32, so a point left of or above
 * the domain falls into column / row 1); window cell (X, Y) = ((u32)(cx + ox), (u32)(cy + oy)) is skipped when X >= grid_w
 * or Y >= grid_h.  A view may overhang the domain, lie outside it (every pixel 0), be flipped (world_max < world_min) or
 * degenerate (world_min == world_max).  For coordinates that are not finite or larger than 2^30 * smoothing_radius in
 * magnitude the pixel values are unspecified; no memory outside the handle's arrays is read for any coordinate.
 *
 * Single-domain handles only (FS_ERR_UNSUPPORTED on a slab handle).  FS_ERR_INVALID before the first fs_step and between
 * fs_upload_particles / fs_upload_start_indices and the next fs_step: an upload leaves the records in upload order under
 * the previous step's cell table (the precondition of fs_sample_*).  FS_ERR_DEVICE after the sort's stand-by kernel
 * reported a grid-barrier time-out (the handle is dead, as for fs_step). */
typedef struct fs_view {
    fs_vec2 world_min, world_max;
    uint32_t width, height;
} fs_view;
fs_status fs_render_density(fs_sim* sim, const fs_view* view, float* rgba_host);

/* -------------------------------------------------------------- profiling */
/* Per-pass device time measured with hipEvents on the simulation's stream. */
/* FS_PASS_BOUNDARY: slab handles only — the part of a step that runs after the halo exchange (overlapped step: waiting for
 * the incoming messages + the boundary strips); 0 on every other handle. */
enum { FS_PASS_PREDICT_KEY = 0, FS_PASS_SORT = 1, FS_PASS_REORDER = 2, FS_PASS_DENSITY = 3,
       FS_PASS_FORCE = 4, FS_PASS_BOUNDARY = 5, FS_PASS_COUNT = 6 };
fs_status fs_profile_enable(fs_sim* sim, int enable);
/* Accumulated milliseconds per pass since the last reset and number of steps. */
fs_status fs_profile_read(fs_sim* sim, double ms[FS_PASS_COUNT], uint64_t* steps, int reset);
/* Time `steps` consecutive fs_step calls with one hipEvent pair on the stream. */
fs_status fs_timed_steps(fs_sim* sim, const fs_tick_settings* tick, uint32_t steps, double* ms_total);

/* ------------------------------------------------ surface tension (build extension, opt-in) */
/* NOT in the reference: its calculate_surface_tension (compute.wgsl:303-498) is dead code whose gradient is identically
 * zero.  Enabled, every step runs a colour-field continuum-surface-force pass (Mueller, Charypar & Gross 2003, §4.4) with
 * the density pass's 2D poly6 kernel, after the density pass and before the force pass, and move_particle adds its force:
 * ax = (fp.x + fv.x) + st.x.  For sorted slot i with predicted position x, over the neighbours j the density pass visits
 * (same cells, same order, same start-index rules, i itself included), in f32 without contraction:
 *     o = q_j - x, r2 = o.o, skipped when r2 > h2;  d = h2 - r2;  w = m / rho_j (this step's clamped density)
 *     n += w * (((Cg*d)*d) * o)          Cg = poly6_kernel_derivative = 24/(pi h^8)
 *     L += w * ((Cl*d) * (3*r2 - h2))    Cl = 2 Cg
 *     |n| = sqrt(n.n);  st = (|n| > surface_tension_treshold && |n| > 0) ? ((-surface_tension_coefficient * L) / |n|) n : 0
 * Bit-exact in FS_MATH_IEEE; the other math modes keep their per-step contract.  Off by default (the knobs alone change
 * nothing).  Single-domain 2D handles only: a slab handle gets FS_ERR_UNSUPPORTED.  The pass's time falls inside the
 * FS_PASS_FORCE interval of fs_profile_read.  See DESIGN.md §11.
 * fs_set_surface_tension: takes effect for steps enqueued after the call (the first enable allocates 8 B per particle).
 * fs_download_surface_tension: the last step's st, one fs_vec2 per particle in fs_download_particles' slot order; n must equal
 * the particle count.  FS_ERR_INVALID when no step with surface tension has been enqueued since the handle was created or
 * since surface tension was last enabled.  Blocking. */
fs_status fs_set_surface_tension(fs_sim* sim, int enable);
int fs_surface_tension_enabled(const fs_sim* sim);
fs_status fs_download_surface_tension(fs_sim* sim, fs_vec2* dst, size_t n);

/* ------------------------------------------------ particle tracking (build extension, opt-in) */
/* NOT in the reference: every step cell-sorts the records and they carry no id, so "index i" names a different particle after
 * every tick.  With tracking on, the handle keeps per particle a uint32_t id and C float channels (0 <= C <=
 * FS_TRACK_MAX_CHANNELS), stored in slot order (fs_download_particles' order) and permuted by every step exactly as the
 * records are.  Let src[i] be the slot, in the order before a step, of the particle which that step places in slot i (the
 * permutation the step's sort applies: the bitonic network's in FS_SORT_BITONIC, the stable sort's in FS_SORT_COUNTING).
 * After the step:
 *     id[i]      = id_before[src[i]]
 *     attr[c][i] = attr_before[c][src[i]]      for c < C      (bit copies: NaN payloads, -0 and denormals survive)
 * Nothing else reads or writes them: the simulation state is bit-identical with tracking on or off, in every math mode, with
 * or without surface tension.  One gather pass per step, timed inside the FS_PASS_REORDER interval of fs_profile_read; with
 * tracking off no launch and no allocation.  Single-domain 2D handles only: a slab handle gets FS_ERR_UNSUPPORTED from
 * fs_track_enable.  See DESIGN.md §12.
 *
 * fs_upload_particles does NOT touch ids or channels: it replaces the records of slots, and identity stays with the slot, so
 * download -> edit -> upload keeps every id.
 *
 * fs_track_enable: allocates on first use (8 B + 8 B per channel, per particle) and (re)initialises id[i] = i (the slot held
 *   at the moment of the call, i.e. fs_download_particles' current order) and every channel to +0.0f.  Calling it again
 *   re-initialises, also with another channel count.  channels < 0 or > FS_TRACK_MAX_CHANNELS: FS_ERR_INVALID.  Takes effect
 *   for steps enqueued after the call and is ordered after the steps already in flight.
 * fs_track_disable: later steps do not carry; the read calls below then return FS_ERR_INVALID.  Off is the default.
 * fs_track_channels: -1 when off, else C.
 * fs_track_download_* / fs_track_upload_*: blocking host copies in slot order.  n must equal the particle count and channel must
 *   be < C, else FS_ERR_INVALID.  Uploaded ids are the caller's business (any uint32_t, duplicates allowed).
 * fs_track_ids_device / fs_track_attr_device: device pointers to the arrays of the last enqueued step (stream-ordered on
 *   fs_stream), for a renderer on the same device.  Valid until the next fs_step / fs_timed_steps / upload / enable: the
 *   arrays ping-pong, as fs_particles_device's view may.
 * fs_download_particles_by_id: dst[id[i]] = particle[i] for every slot with id[i] < n; entries of dst that no id names are
 *   left exactly as the caller passed them; with duplicate ids it is unspecified which record wins.  n is the length of dst
 *   and need not equal the particle count.  Blocking; off the step path. */
#define FS_TRACK_MAX_CHANNELS 4
fs_status fs_track_enable(fs_sim* sim, int channels);
fs_status fs_track_disable(fs_sim* sim);
int fs_track_channels(const fs_sim* sim);
fs_status fs_track_download_ids(fs_sim* sim, uint32_t* dst, size_t n);
fs_status fs_track_upload_ids(fs_sim* sim, const uint32_t* src, size_t n);
fs_status fs_track_download_attr(fs_sim* sim, int channel, float* dst, size_t n);
fs_status fs_track_upload_attr(fs_sim* sim, int channel, const float* src, size_t n);
fs_status fs_track_ids_device(fs_sim* sim, const uint32_t** out);
fs_status fs_track_attr_device(fs_sim* sim, int channel, const float** out);
fs_status fs_download_particles_by_id(fs_sim* sim, fs_particle* dst, size_t n);

/* ------------------------------------------------ field sampling (build extension, opt-in by being called) */
/* NOT in the reference: every other read-out is indexed by slot.  These calls evaluate the fluid at arbitrary points: the
 * reference's calculate_density_at_point (funcs.wgsl:157-203) at a point that need not be a particle, and the SPH interpolants
 * sum_j (m / rho_j) W_j f_j of the velocity and of the tracking channels.  The result is a pure function of the state the handle
 * holds after its last step — what fs_download_particles (p[k]), fs_download_start_indices (S), fs_get_uniform and
 * fs_track_download_attr (attr[c]) return — in every math mode and sort mode.  With n = particle_count, h = smoothing_radius,
 * h2 = h * h, m = particle_mass, Cv = 4.0f / (PI * powf(h, 8.0f)) (the density pass's coefficient), all f32 without contraction,
 * for a query point x:
 *     (cx, cy) = (u32_sat(floor((x.x + bounds.x * 0.5f) / h)) + 1, likewise y)         wrapping + 1 (funcs.wgsl:212-214)
 *     cell = cy * grid_w + cx                                                          wrapping u32
 *     density = weight = velocity = a_c = +0.0f;  neighbours = 0
 *     for oy in -1, 0, 1:  for ox in -1, 0, 1:
 *         X = (u32)(cx + ox);  Y = (u32)(cy + oy);  skipped when X >= grid_w or Y >= grid_h      (fs_render_density's rule)
 *         id = Y * grid_w + X;  k = S[id]
 *         while k < n and p[k].grid == id:                                             (a stale S[id] included: ref_quirks)
 *             d = p[k].predicted_position - x;  r2 = d.x * d.x + d.y * d.y
 *             if not (r2 > h2):
 *                 e = h2 - r2;  W = ((Cv * e) * e) * e
 *                 density += m * W
 *                 t = (m / p[k].density) * W                                           IEEE division by the stored density
 *                 weight += t;  velocity += t * p[k].velocity;  a_c += t * attr[c][k];  neighbours += 1
 *             k += 1
 * `velocity` and the channel sums are returned un-normalised; dividing by `weight` gives the Shepard-normalised value.  At a
 * particle's own predicted position, fmax(fmax(density, EPSILON), 0.1f) is that particle's stored density, bit for bit, in
 * FS_MATH_IEEE.  Non-finite query coordinates give unspecified values (and no out-of-bounds access).  See DESIGN.md §13.
 *
 * fs_sample_points: host pointers, blocking.
 * fs_sample_points_device: device pointers on the handle's device; enqueued on fs_stream(sim) after the steps in flight;
 *   non-blocking, no allocation, no host read — for a consumer on the same GPU.  The buffers must stay valid until the stream
 *   has passed the call.
 * fs_sample_grid: host output, blocking; pixel (i, j) is fs_render_density's point
 *   world_min + (((float)i + 0.5f) / (float)width) * (world_max - world_min), stored at out[j * width + i]; bit-identical to
 *   fs_sample_points on those points.
 * attr_out may be NULL; else attr_out[c * n + k] = a_c of query k for c < fs_track_channels(sim) (n = width * height for a grid).
 * Query order decides the speed, not the result: points in a coherent order (a grid, sorted by cell, slot order) are sampled
 * several times faster than the same points shuffled.  Nothing is sorted behind the caller's back.
 * Checks, in this order: NULL handle -> FS_ERR_INVALID; slab handle -> FS_ERR_UNSUPPORTED; (grid) NULL or zero-sized view, or
 * width * height > 2^28 -> FS_ERR_INVALID; attr_out != NULL with tracking off or zero channels -> FS_ERR_INVALID; n == 0 ->
 * FS_OK, nothing touched; NULL points / out -> FS_ERR_INVALID; n > 2^28 -> FS_ERR_INVALID; no step enqueued since create or since
 * the last fs_upload_particles / fs_upload_start_indices (records and cell table would not belong together) -> FS_ERR_INVALID. */
typedef struct fs_sample {        /* 24 bytes */
    float density;                /* sum m W */
    float weight;                 /* sum (m / rho_j) W: the Shepard denominator */
    fs_vec2 velocity;             /* sum (m / rho_j) W v_j, un-normalised */
    uint32_t neighbours;          /* candidates with r2 <= h2 */
    uint32_t cell;                /* cell id of the query point */
} fs_sample;
fs_status fs_sample_points(fs_sim* sim, const fs_vec2* points, size_t n, fs_sample* out, float* attr_out);
fs_status fs_sample_points_device(fs_sim* sim, const fs_vec2* points_dev, size_t n, fs_sample* out_dev, float* attr_out_dev);
fs_status fs_sample_grid(fs_sim* sim, const fs_view* view, fs_sample* out, float* attr_out);

/* ------------------------------------------------ 2D particle count (build extension, opt-in by being called) */
/* A particle count that changes at run time: a tap that fills a tank, an outflow, a scene assembled from blocks of fluid.  The
 * 2D counterpart of "3D particle count" below, clause for clause.  A handle has `capacity` slots (fs_options.capacity at create,
 * at least settings.particle_count) and a live count <= capacity; after fs_create both are settings.particle_count.
 * fs_particle_count returns the live count, and every step, transfer and query works on exactly that many particles;
 * fs_uniform.particle_count follows it.  The live count is always known to the host: emission has a size the caller gives,
 * removal is a blocking call that returns how many particles went.  The step's passes are unchanged, in both sort modes, and a
 * handle that never calls these functions launches exactly the kernels it launched before, with the same arguments.
 * FS_ABI_VERSION is unchanged.  Single-domain handles only: on a slab handle every call below is FS_ERR_INVALID right after
 * the NULL check (a slab's count belongs to the exchange; fs_capacity and fs_track_next_id only read).  See DESIGN.md §22.
 *
 * fs_reserve: grow-only and blocking.  capacity > 2^28 is FS_ERR_INVALID; capacity <= fs_capacity is FS_OK and does nothing.
 * Every per-slot array gets `capacity` slots; the records, the tick, start_indices, the force field, ids and channels, the last
 * step's surface-tension forces and the validity of the queries are preserved bit for bit.  Everything new is allocated before
 * anything old is released: on FS_ERR_OOM the handle is exactly what it was.  Device pointers handed out by fs_track_*_device
 * die.  On a handle with a renderer hand-off registered (fs_export_handle(FS_EXPORT_PARTICLES)) fs_reserve is FS_ERR_INVALID,
 * whatever the capacity: the exported allocation cannot move.  Such a caller sizes the handle with fs_options.capacity at create.
 *
 * fs_emit_particles: appends n host records at slots [count, count + n), stored as fs_upload_particles stores them, all five
 * fields as given; ordered on fs_stream after the steps in flight, and back only when `src` has been read.  In this order: a NULL
 * handle is FS_ERR_INVALID; n == 0 is FS_OK and touches nothing; a NULL src is FS_ERR_INVALID; count + n > capacity is
 * FS_ERR_INVALID and changes nothing.
 *
 * fs_emit_nozzle: the same append of M = nu * nv records generated on the device, no host array and no transfer.  For q in
 * [0, M), in f32 without contraction:
 *     a = q % nu;  b = q / nu;  sa = ((float)a + 0.5f) - 0.5f * (float)nu;  sb = ((float)b + 0.5f) - 0.5f * (float)nv
 *     position.c = (origin.c + sa * u.c) + sb * v.c;  predicted_position = position;  velocity = nozzle.velocity
 *     density = +0;  grid = 0;  stored at slot count + q
 * nv == 1 is a line of particles, the usual 2D tap; nv > 1 a block of fluid.  Positions outside the box are legal: the step's
 * clamps deal with them as with an upload.  FS_ERR_INVALID, in this order: a NULL handle or nozzle; nu == 0, nv == 0 or
 * nu * nv > 2^28; any of the 8 floats not finite; count + M > capacity (nothing changes).  Enqueued on fs_stream; with
 * FS_SORT_BITONIC it waits for the steps in flight only when the count crosses a power of two, with FS_SORT_COUNTING never.
 *
 * fs_remove_in_box / fs_remove_flagged: blocking.  Slot i goes when lo.a <= position.a && position.a <= hi.a on both axes
 * (inclusive edges; a NaN coordinate is never removed; the test runs on the device), or when flags_host[i] != 0, where n must
 * equal the count (else FS_ERR_INVALID).  The survivors keep their relative order; position, predicted position, velocity,
 * density, grid and, with tracking on, ids and every channel move as bit copies.  *removed receives the number removed.  Fewer
 * than 2 survivors: FS_ERR_INVALID, *removed = 0, nothing changes.  Nothing matches: FS_OK, *removed = 0, nothing changes at
 * all (the queries stay valid).  NULL arguments are FS_ERR_INVALID.
 *
 * After any call that changed the count: fs_render_density, fs_sample_* and fs_sample_grid return FS_ERR_INVALID until the next
 * step, fs_download_surface_tension until the next step with the pass on, and pointers from fs_track_*_device are dead.
 * fs_upload_particles still clamps to the live count and never grows it.  start_indices is sized by the grid and persistent: no
 * call here touches it, so after a removal it may name slots >= count (the stale-start quirk of ref_quirks = 1 then clamps to
 * the cell's count, as it always did).  Slots behind the live count keep whatever they held; no result depends on them.
 *
 * Renderer hand-off: emission and removal are allowed on a handle with a hand-off registered.  The exported view then holds the
 * new state, for the new count, after the next step (or after the next fs_particles_device, which re-materialises it); between
 * the change and that, its contents are unspecified.  The exported allocation has `capacity` records and never moves: the IPC
 * handle names all of it, so an importer reads the new count's records at the address it already has.  fs_mem_handle.bytes and
 * the dma-buf descriptor cover the live count at the time of the export only: a consumer of the descriptor calls
 * fs_export_handle again after the count has grown past that.
 *
 * Tracking: fs_track_enable sets next_id to the live count at the call; every particle emitted while tracking is on gets
 * id = next_id++ in emission order (wrapping u32) and +0.0f in every channel; fs_track_upload_ids does not touch next_id;
 * removal compacts ids and channels with the records.  fs_track_next_id: next_id, or 0 when tracking is off. */
fs_status fs_reserve(fs_sim* sim, uint32_t capacity);
uint32_t fs_capacity(const fs_sim* sim);
fs_status fs_emit_particles(fs_sim* sim, const fs_particle* src, size_t n);
typedef struct fs_nozzle {        /* 40 bytes */
    fs_vec2 origin, u, v, velocity;
    uint32_t nu, nv;
} fs_nozzle;
fs_status fs_emit_nozzle(fs_sim* sim, const fs_nozzle* nozzle);
fs_status fs_remove_in_box(fs_sim* sim, const fs_vec2* lo, const fs_vec2* hi, uint32_t* removed);
fs_status fs_remove_flagged(fs_sim* sim, const uint8_t* flags_host, size_t n, uint32_t* removed);
uint32_t fs_track_next_id(const fs_sim* sim);

/* ------------------------------------------------ 2D moving bodies (build extension, opt-in by being created) */
/* Kinematic rigid bodies for the 2D step: a wave-maker paddle, a stirrer, a piston, a gate.  The 2D counterpart of "3D moving
 * bodies" below.  Up to FS_MAX_BODIES per handle, each a small W x H field of push vectors, field[j * W + i], a zero vector is
 * free space, over the body's own box [-extent/2, extent/2] in the BODY frame, with a pose and a velocity the host sets per step.
 * The vectors are in world units of the body frame — not the pixel units of the force texture (fs_upload_force_field), which
 * stays what it was: one domain-wide static field, pushed out inside move_particle.  The fluid feels the body (one-way
 * coupling): the engine neither integrates the pose nor computes forces on the body — it can REPORT what the fluid hands each
 * body, see "2D body loads" below, and a host that integrates the pose from that closes the loop.  A handle without a body
 * launches exactly the kernels it launched before and computes the same bits.
 *
 * With bodies present, a step is B_7(...B_0(step(state))): the whole reference step first, its texture push-out and its wall
 * clamp included, then the operator of each existing body in ascending slot order, on the position p and the velocity v the step
 * is about to leave.  All arithmetic is f32 without contraction, `/` and `sqrt` are correctly rounded, u32_sat as in "3D
 * colliders"; b.a = bounds.a * 0.5f are the half-bounds of the step (its own bs_x, bs_y) and damping the tick's damping_factor.
 * Per body: c = centre, rij = rot[2*i + j] (world = R * local), u = velocity, w = angular_velocity, hb.a = extent.a * 0.5f (on
 * the host, once), W_x = W, W_y = H.
 *     d.a  = p.a - c.a
 *     q.x  = r00*d.x + r10*d.y;   q.y = r01*d.x + r11*d.y                    (q = R^T d: the body frame)
 *     if !(fabsf(q.x) <= hb.x && fabsf(q.y) <= hb.y): unchanged              (NaN: unchanged; on an edge: inside)
 *     ia = min(u32_sat(((q.a + hb.a) / extent.a) * (float)W_a), W_a - 1)
 *     g  = field[iy * W + ix];   if g.x == 0 && g.y == 0: unchanged
 *     len = sqrt(g.x*g.x + g.y*g.y);   if !(len > 0): unchanged              (a vector whose squares underflow is free space)
 *     f.x = r00*g.x + r01*g.y;   f.y = r10*g.x + r11*g.y                     (R g: back to the world)
 *     n.a = f.a / len
 *     p.a = p.a + f.a
 *     s.a = p.a - c.a                                                        (the pushed position)
 *     us.x = u.x - w*s.y;   us.y = u.y + w*s.x                               (the body surface's velocity there)
 *     r.a = v.a - us.a
 *     rn  = r.x*n.x + r.y*n.y
 *     k   = (1.0f - damping) * rn
 *     v.a = us.a + (r.a - k*n.a)
 *     per axis, x then y: if fabsf(p.a) > b.a { p.a = b.a * sign(p.a); v.a *= -1.0f * damping }
 * predicted_position, density and grid are not touched, and neither is start_indices.  All three math modes (FS_MATH_IEEE,
 * FS_MATH_WGSL_ULP, FS_MATH_TOLERANCE) run this same IEEE operator.  The engine does not check that rot is a rotation, only that
 * it is finite.  A pushed particle keeps the body surface's velocity along the normal, so a moving wall hands momentum over.
 * The lines above hold at every operand a call accepts; nothing is flushed, ranged or special-cased.  f32 denormals count: an
 * extent of 2^-149 gives hb = 0 (only q == 0 is inside), and with an extent of 1e-40 the quotient of two denormals is 0.5.  A
 * vector whose squares overflow has len = +inf and n = 0: the particle is pushed (onto a wall) and keeps v = us + r.  damping is
 * used as the tick gives it, also outside [0, 1].  The plain step zeroes a NaN velocity, clamps the speed and clamps a position
 * onto the walls, so at an ordinary damping B_0 meets a finite velocity and a position that is finite or NaN; a later operator
 * can meet the NaN, infinite or enormous velocity an earlier one left, and computes with it as written.
 *
 * fs_body_create: a field made by the caller.  fs_body_create_from_mask: the exact distance transform of "3D colliders" on a
 * w x h x 1 mask over the body's box, the z component dropped — the same passes, the same tie rules, s_a = extent.a / (float)W_a,
 * a mask value > 128 is solid; `field_host` (may be NULL) receives the field, w * h fs_vec2.  It is not the chamfer of
 * fs_generate_force_field, which works in pixel units and is not exact.  *body_out is the lowest free slot in
 * 0 .. FS_MAX_BODIES - 1; slots are stable (destroying body 1 leaves body 2 as body 2).  A new body has the identity pose at the
 * origin and zero velocities.
 *
 * Checks, in this order, FS_ERR_INVALID unless stated; a refused call changes nothing:
 *  1. NULL handle.
 *  2. A slab handle -> FS_ERR_UNSUPPORTED (single-domain handles only).
 *  3. NULL array or out pointer (field, mask, body_out, motion, dst, or one of the three of fs_body_dims).
 *  4. w or h of 0 or above 1024.
 *  5. A component of the box `extent` that is not finite and > 0.
 *  6. A non-finite field component, or a mask without a free pixel.
 *  7. No free slot.
 *  8. The per-body calls: a slot that holds no body (fs_body_download then: n != w * h).
 *  9. fs_body_set_motion: any non-finite float.
 *
 * create*, download and destroy are blocking and ordered on fs_stream(sim); destroy synchronises before freeing, because steps
 * in flight read the field.  fs_body_set_motion touches host memory only: a step (fs_step, and every step of fs_timed_steps)
 * takes every body's motion by value when it is enqueued, so setting a different pose before each of several un-synchronised
 * steps is the intended use.  The pose holds until it is set again.  Nothing here makes rendering or sampling stale; particles
 * emitted inside a body (fs_emit_*) are pushed by the next step.  With a renderer hand-off registered
 * (fs_export_handle(FS_EXPORT_PARTICLES)) the exported records hold the pushed positions and velocities.  The time of the
 * operators falls inside FS_PASS_FORCE.  FS_ABI_VERSION is unchanged.  See DESIGN.md §24. */
#define FS_MAX_BODIES 8
typedef struct fs_body_motion {
    fs_vec2 centre;            /* world position of the body box's centre */
    float   rot[4];            /* row-major R, world = R * local; the caller supplies a rotation, the engine checks only finiteness */
    fs_vec2 velocity;          /* of the centre, world units per second */
    float   angular_velocity;  /* rad/s, counter-clockwise in (x, y) */
} fs_body_motion;
fs_status fs_body_create(fs_sim* sim, const fs_vec2* field_host, uint32_t w, uint32_t h, fs_vec2 extent, uint32_t* body_out);
fs_status fs_body_create_from_mask(fs_sim* sim, const uint8_t* mask_host, uint32_t w, uint32_t h, fs_vec2 extent,
                                   fs_vec2* field_host /* may be NULL */, uint32_t* body_out);
fs_status fs_body_set_motion(fs_sim* sim, uint32_t body, const fs_body_motion* motion);
fs_status fs_body_get_motion(const fs_sim* sim, uint32_t body, fs_body_motion* out);
fs_status fs_body_dims(const fs_sim* sim, uint32_t body, uint32_t* w, uint32_t* h, fs_vec2* extent);
fs_status fs_body_download(fs_sim* sim, uint32_t body, fs_vec2* dst, size_t n);              /* n == w*h */
fs_status fs_body_destroy(fs_sim* sim, uint32_t body);
uint32_t  fs_body_count(const fs_sim* sim);                                                  /* 0 for a NULL handle */

/* ------------------------------------------------ 2D body loads (build extension, opt-in per handle) */
/* The impulse and the angular impulse the fluid gives each body of "2D moving bodies", summed on the GPU inside the bodies' own
 * pass.  fs_body_loads_enable(sim, on) turns them on or off.  While off, a step launches exactly the kernels it launches without
 * this section and leaves the same bytes.  While on, the particle state is still byte for byte that of "2D moving bodies": loads
 * only observe.
 *
 * A HIT of body b is a particle that reaches the line `p.a = p.a + f.a` of the operator B_b above.  With that section's names:
 *   v0   the velocity on entry to B_b: after the step and after the operators of the lower slots (their wall re-clamp included);
 *   v1.a = us.a + (r.a - k*n.a): the velocity B_b computes, BEFORE its wall re-clamp — what the wall does is not the body's load;
 *   s.a  = p.a - c.a: the pushed position relative to the centre, before the re-clamp.
 * f32 without contraction, one operation per line:
 *     j.x = v0.x - v1.x;   j.y = v0.y - v1.y     (impulse on the body per unit particle mass: minus the particle's velocity change)
 *     t0 = s.x * j.y;   t1 = s.y * j.x;   tz = t0 - t1     (angular impulse about the body's centre, counter-clockwise positive)
 * The positional push p += f carries no momentum and is not counted.
 *
 * Fixed point: Q(x) is the signed 64-bit integer nearest to x * 2^FS_BODY_LOAD_SHIFT, ties to even (the product is exact in f32,
 * so every correctly rounded route gives the same integer).  If any of j.x, j.y, tz is NaN or fails fabsf(x) < 16384.0f (2^14),
 * the hit adds nothing to the three sums and is counted in `dropped`; its particle is moved exactly as without loads.  Per body
 * the engine keeps five 64-bit words: sum Q(j.x), sum Q(j.y), sum Q(tz), hits (every hit, dropped ones included) and dropped,
 * each sum modulo 2^64 over all hits of all steps since the words were last zeroed.  |Q| < 2^34 and a step has at most 2^28
 * particles, so one step cannot wrap; at |j| < 2^7 and 16 M hits per step wrapping is thousands of steps away.  The engine does
 * not guard it: read with reset != 0 often enough.  Integer sums are associative, so the words are ONE defined value whatever the
 * order of lanes, waves and workgroups: identical from run to run and equal to a host sum of Q over the hits.
 * Momentum handed to body b = impulse_q * 2^-FS_BODY_LOAD_SHIFT * (the mass of one particle), in world units.
 *
 * Enabling (also when already on) zeroes every slot's words and `steps`.  A body created while loads are on starts at zero; a
 * destroyed slot's words are zeroed before the slot can be reused.  Steps taken while loads are off count nothing, and disabling
 * keeps the words (they cannot be read until the next enable, which zeroes them).  fs_body_loads is blocking and ordered on
 * fs_stream(sim): it returns the words behind every step enqueued so far; reset != 0 zeroes that slot's words and `steps` behind
 * the read, on the stream.  fs_body_loads_device hands out the device address of FS_MAX_BODIES x 5 64-bit words, by slot, in the
 * order above, for a consumer on the stream: it holds the finished values once any step has completed (the step's last launch
 * folds the pass's partial sums into it; the address is stable until the handle is destroyed).
 *
 * Checks, in this order, FS_ERR_INVALID unless stated; a refused call changes nothing:
 *  1. NULL handle (fs_body_loads_enabled: 0).
 *  2. A slab handle -> FS_ERR_UNSUPPORTED.
 *  3. NULL out pointer (`out`, `words`).
 *  4. fs_body_loads: a slot that holds no body.
 *  5. fs_body_loads, fs_body_loads_device: loads are not enabled ("not enabled").
 * FS_ABI_VERSION is unchanged.  See DESIGN.md §25. */
#define FS_BODY_LOAD_SHIFT 20
typedef struct fs_body_load {
    int64_t  impulse_q[2];   /* sum Q(j.x), sum Q(j.y): times 2^-20 times the particle mass = momentum handed to the body */
    int64_t  angular_q;      /* sum Q(tz) */
    uint64_t hits, dropped;
    uint64_t steps;          /* steps enqueued with loads on since the words were zeroed (host-side count) */
} fs_body_load;
fs_status fs_body_loads_enable(fs_sim* sim, int on);
int       fs_body_loads_enabled(const fs_sim* sim);                                         /* 0 for a NULL handle */
fs_status fs_body_loads(fs_sim* sim, uint32_t body, fs_body_load* out, int reset);           /* blocking */
fs_status fs_body_loads_device(fs_sim* sim, const void** words);

/* ------------------------------------------------ multi-GPU slab mode (build extension) */
/* NOT in the reference (single wgpu device, src/renderer.rs:108-133).  SURVEY.md §8e: a rank
 * owns the global cell columns [own_lo, own_hi) of the grid (src/simulation.rs:140-141) and
 * exchanges one fixed-size message per neighbour per step (migrants + 2-column ghost halo).
 * Messages are device buffers of fs_slab_message_bytes(); the caller moves them between
 * ranks (RCCL send/recv).  A step = fs_slab_pack -> exchange -> fs_slab_step, all
 * asynchronous on the simulation's stream; counts stay on the device. */
typedef struct fs_slab_config {
    uint32_t own_lo, own_hi;      /* owned window in global cell columns */
    uint32_t has_left, has_right; /* neighbours present */
    uint32_t capacity;            /* particle slots of the local array (incl. 2*recv_capacity) */
    uint32_t recv_capacity;       /* records per incoming message */
    uint32_t max_cols;            /* widest owned window this handle must support (re-balancing) */
    uint32_t sort_mode;           /* low byte: 0 = default (counting sort), 1 + fs_sort_mode selects explicitly; flags (counting sort
                                     only, default: the edge-first step) | FS_SLAB_SERIAL: the serial step (pack -> exchange ->
                                     everything), | FS_SLAB_STRIPS: the boundary-strips step, | FS_SLAB_ROWMAJOR: row-major cell ids
                                     even where a slab edge has a neighbour (FS_SLAB_MODE / FS_SLAB_TRANSPOSE override) */
} fs_slab_config;
#define FS_SLAB_SERIAL 0x100u
#define FS_SLAB_STRIPS 0x200u
#define FS_SLAB_ROWMAJOR 0x400u

typedef struct fs_slab_counters {
    uint32_t n_live;        /* live slots after the last step (owned + ghosts; overlapped step: the sorted prefix, i.e. the
                               carried-over particles — ghosts and this step's migrants live outside it) */
    uint32_t lost;          /* particles that left slab + halo in one step (must stay 0) */
    uint32_t overflow;      /* message capacity exceeded, or owned particles stranded past the main slots
                               (n_live > capacity - 2*recv_capacity at the next pack); must stay 0 */
    uint32_t far_halo;      /* migrants that landed in the receiver's far halo zone, or (overlapped step) within 2 columns
                               of its interior: the boundary zone was too narrow for their speed (must stay 0) */
} fs_slab_counters;

fs_status fs_slab_create(const fs_settings* global_settings, int device, const fs_slab_config* cfg, fs_sim** out);
/* Initial owned particles (host AoS records, any order). */
fs_status fs_slab_upload_owned(fs_sim* sim, const fs_particle* src, size_t n);
/* Move the owned window (re-balancing); takes effect at the next fs_slab_pack.  Until then fs_slab_download and
 * fs_slab_column_histogram still describe the stored state in the window it was built with. */
fs_status fs_slab_set_window(fs_sim* sim, uint32_t own_lo, uint32_t own_hi);
size_t fs_slab_message_bytes(const fs_sim* sim);
/* Begin a step: predict, classify, fill the two outgoing device messages (NULL = no neighbour).  Three step modes
 * (fs_slab_overlapped(): 1 edge-first — the default with the counting sort —, 2 strips, 0 serial; fs_slab_config.sort_mode
 * flags, FS_SLAB_MODE in the environment), one call pattern: fs_slab_pack -> exchange -> fs_slab_step.
 *   EDGE-FIRST (1): fs_slab_step forks after its reorder pass — the handle's exchange stream (fs_slab_comm_stream) advances
 *     the owned columns within the boundary zone of a neighboured edge first and builds the NEXT tick's two messages from
 *     their new state right away, into the buffers the last fs_slab_pack was given; the interior columns' density / force
 *     launches run beside that on the simulation's stream.  The next fs_slab_pack finds the messages built (same buffers,
 *     same delta, same window: otherwise it builds them itself) and only classifies the interior columns' slots for the sort.
 *     Keep the send buffers of a step untouched until the next fs_slab_pack returns, and exchange on the exchange stream
 *     (fs_slab_exchange does; other transports: fs_slab_comm_begin / _end).
 *   STRIPS (2): ghosts never enter the rank's sorted array; fs_slab_pack also enqueues sort, reorder, density and the interior
 *     columns' force launch; fs_slab_step finishes the boundary columns on a small second array after the exchange.
 *   SERIAL (0): pack, exchange and the whole step one after the other on the simulation's stream. */
fs_status fs_slab_pack(fs_sim* sim, const fs_tick_settings* tick, void* send_left, void* send_right);
/* Finish the step with the two incoming device messages (NULL = no neighbour). */
fs_status fs_slab_step(fs_sim* sim, const void* recv_left, const void* recv_right);
/* Step mode (see fs_slab_pack); owned columns per neighboured edge in the boundary zone (default 4, at least 3; set it to
 * 3 + the columns the fastest particle can cross in one step — a migrant that lands closer than 3 columns to the interior
 * is counted in fs_slab_counters.far_halo; a window edge moved by fs_slab_set_window widens the next step's zone by itself). */
int fs_slab_overlapped(const fs_sim* sim);
fs_status fs_slab_set_boundary_cols(fs_sim* sim, uint32_t cols);
uint32_t fs_slab_boundary_cols(const fs_sim* sim);
/* Transport hooks of the overlapped step (no-ops on a serial handle, where the simulation's own stream orders the exchange):
 * fs_slab_comm_begin makes fs_slab_comm_stream() wait for the packed messages; the caller issues its send / recv on THAT
 * stream; fs_slab_comm_end records their completion, which the next fs_slab_step waits for.  fs_slab_exchange does all three.
 * fs_slab_wait_packed blocks the host until the outgoing messages are complete (transports that stage through the host). */
void* fs_slab_comm_stream(const fs_sim* sim);
fs_status fs_slab_comm_begin(fs_sim* sim);
fs_status fs_slab_comm_end(fs_sim* sim);
fs_status fs_slab_wait_packed(fs_sim* sim);
fs_status fs_slab_counters_read(fs_sim* sim, fs_slab_counters* out);   /* blocking */
/* Live records (global cell keys) and their owned flags; blocking.  Returns n_live. */
fs_status fs_slab_download(fs_sim* sim, fs_particle* dst, uint8_t* owned, size_t cap, uint32_t* n_live);
/* Largest |velocity| among the owned particles (sizes the outer-edge margin between two re-balancing
 * steps: a wall-side slab must contain everything that can move before the next one); blocking. */
fs_status fs_slab_max_speed(fs_sim* sim, float* out);
/* Per-global-column particle counts of the owned columns (others untouched); blocking. */
fs_status fs_slab_column_histogram(fs_sim* sim, uint32_t* hist, size_t grid_w_global);

/* The three re-balancing inputs above without reading anything back: enqueued on the simulation's stream, results stay in
 * DEVICE buffers of the caller — hist_dev[grid_w_global] (zero outside the owned window) and stats_dev[4] = {lost,
 * overflow, far_halo, bits of the largest owned |velocity|}, all four MAX-reducible as u32.  All-reduce them on the
 * same stream (fs_comm_allreduce: SUM for the histogram, MAX for the stats) and read both once. */
fs_status fs_slab_rebalance_stats(fs_sim* sim, uint32_t* stats_dev, uint32_t* hist_dev, size_t grid_w_global);

/* ---- native RCCL transport (csrc/comm.hip): one process per GPU, any host language --------------------------
 * fs_comm_unique_id on rank 0 -> ship the 128 bytes to every rank -> fs_comm_init everywhere; then per step
 * fs_slab_pack -> fs_slab_exchange -> fs_slab_step.  The exchange is one grouped ncclSend/ncclRecv set on the
 * simulation's stream (left_rank / right_rank < 0 = no neighbour on that side); with left_rank == right_rank ==
 * own rank it is a self-exchange (recv_right receives send_right, recv_left receives send_left).  RCCL failures
 * return FS_ERR_COMM with the RCCL message in fs_last_error().  fs_comm_allreduce (in place, on the simulation's
 * stream) serves the re-balancing histogram / violation counters. */
#define FS_COMM_ID_BYTES 128
typedef struct fs_comm fs_comm;
enum { FS_COMM_U32 = 0, FS_COMM_U64 = 1, FS_COMM_F32 = 2 };
enum { FS_COMM_SUM = 0, FS_COMM_MAX = 1 };
fs_status fs_comm_unique_id(uint8_t id[FS_COMM_ID_BYTES]);
fs_status fs_comm_init(int device, int rank, int world, const uint8_t id[FS_COMM_ID_BYTES], fs_comm** out);
void fs_comm_destroy(fs_comm* comm);
fs_status fs_slab_exchange(fs_sim* sim, fs_comm* comm, int left_rank, int right_rank, const void* send_left,
                           const void* send_right, void* recv_left, void* recv_right);
fs_status fs_comm_allreduce(fs_sim* sim, fs_comm* comm, void* device_buf, size_t count, int dtype, int op);

/* ------------------------------------------------------------ 3D extension */
/* NOT in the reference (2D only).  Build-defined per SURVEY.md Appendix B.3: same pass
 * chain and kernel shapes with a third coordinate, 27-cell sweep, clean cell starts, no
 * mouse force; an obstacle field only on request ("3D colliders" below).  Normative statement: oracle/sph_oracle3d.cpp. */
typedef struct fs3_settings {
    uint32_t particle_count;      /* must be a cube (side^3) for the built-in lattice */
    float particle_spacing;
    float smoothing_radius;
    fs_vec3 size;
} fs3_settings;

typedef struct fs3_tick_settings {
    float delta;
    fs_vec3 gravity;
    float mass;
    float pressure_constant;
    float rest_density;
    float damping_factor;
    float viscosity_coefficient;
} fs3_tick_settings;

typedef struct fs3_particle {      /* 48 bytes */
    fs_vec3 position;
    fs_vec3 predicted_position;
    fs_vec3 velocity;
    float density;
    uint32_t grid;
    uint32_t pad;
} fs3_particle;

typedef struct fs_sim3 fs_sim3;

fs_status fs3_create(const fs3_settings* settings, int device, fs_vec3 initial_offset, fs_sim3** out);
/* math_mode: FS_MATH_IEEE (default of fs3_create: bit-identical to oracle/sph_oracle3d.cpp) or FS_MATH_TOLERANCE (density
 * and force terms re-associated as in 2D: rtol 1e-5 per step against the 3D oracle, cell keys bit-exact).  The 3D
 * statement has no reference counterpart, so "exact" here means exact against this repository's own 3D oracle. */
fs_status fs3_create_ex(const fs3_settings* settings, int device, fs_vec3 initial_offset, int math_mode, fs_sim3** out);
void fs3_destroy(fs_sim3* sim);
fs_status fs3_step(fs_sim3* sim, const fs3_tick_settings* tick);
fs_status fs3_sync(fs_sim3* sim);
uint32_t fs3_tick_count(const fs_sim3* sim);
uint32_t fs3_particle_count(const fs_sim3* sim);
fs_status fs3_grid_dims(const fs_sim3* sim, uint32_t* w, uint32_t* h, uint32_t* d);
fs_status fs3_download_particles(fs_sim3* sim, fs3_particle* dst, size_t n);
fs_status fs3_upload_particles(fs_sim3* sim, const fs3_particle* src, size_t n);
fs_status fs3_reference_lattice(const fs3_settings* settings, fs_vec3 offset, fs3_particle* dst, size_t n);
fs_status fs3_timed_steps(fs_sim3* sim, const fs3_tick_settings* tick, uint32_t steps, double* ms_total);
fs_status fs3_profile_enable(fs_sim3* sim, int enable);
fs_status fs3_profile_read(fs_sim3* sim, double ms[FS_PASS_COUNT], uint64_t* steps, int reset);
/* The simulation's HIP stream (hipStream_t): every fs3_* call of this handle is enqueued on it, as fs_stream for a 2D handle. */
void* fs3_stream(const fs_sim3* sim);

/* ------------------------------------------------ 3D field sampling (build extension, opt-in by being called) */
/* The 3D counterpart of "field sampling" above, with the density gradient (the surface normal of an iso-surface extractor or
 * ray-marcher) and with volumes and slices as the grid form.  The result is a pure function of the state an fs_sim3 holds after
 * its last step: the records p[k] that fs3_download_particles returns (sorted by `grid` after a step), the grid dimensions, the
 * settings, and the `mass` of the tick passed to the last fs3_step / fs3_timed_steps (the handle keeps it).  It holds in both
 * math modes.  With n = particle_count, h = smoothing_radius, h2 = h * h, m = mass,
 * C6 = 315.0f / (64.0f * PI3 * powf(h, 9.0f)) (the oracle's and the step's poly6: host libm, PI3 = 3.14159265359f),
 * Cg = 6.0f * C6, everything f32 without contraction, for a query point x:
 *     (cx, cy, cz) = u32_sat(floor((x.a + size.a * 0.5f) / h)) + 1   per axis, TRUE division, wrapping + 1   (oracle cell_xyz)
 *     cell = (cz * grid_h + cy) * grid_w + cx                                               wrapping u32
 *     density = weight = +0.0f; velocity = gradient = (+0,+0,+0); neighbours = 0
 *     for oz in -1,0,1: for oy in -1,0,1: for ox in -1,0,1:
 *         X = cx+ox, Y = cy+oy, Z = cz+oz (wrapping u32); skipped when X >= grid_w or Y >= grid_h or Z >= grid_d
 *         id = (Z * grid_h + Y) * grid_w + X
 *         for the slots k with p[k].grid == id, ascending:
 *             d = p[k].predicted_position - x;  r2 = d.x*d.x + d.y*d.y + d.z*d.z
 *             if not (r2 > h2):
 *                 e = h2 - r2;  W = ((C6 * e) * e) * e
 *                 density += m * W
 *                 g = m * ((Cg * e) * e);  gradient.a += g * d.a          (= grad_x of sum m W; the outward normal is -gradient)
 *                 t = (m / p[k].density) * W                              IEEE division by the stored density
 *                 weight += t;  velocity.a += t * p[k].velocity.a;  neighbours += 1
 * A skipped candidate is a branch, not an added zero: velocity and gradient terms can be -0.  Velocity is returned
 * un-normalised; dividing by `weight` gives the Shepard value.  The known answer that ties the sampler to the step is the
 * density identity, in FS_MATH_IEEE: at p[i].predicted_position, fmax(fmax(density, 1.19209290e-07f), 0.1f) equals p[i].density
 * bit for bit — walk order and term are those of oracle/sph_oracle3d.cpp step3, which adds +0 for candidates outside the radius,
 * and that cannot change a non-negative sum.  Non-finite coordinates give unspecified values and no out-of-bounds access.
 *
 * fs3_sample_points: host pointers, blocking.
 * fs3_sample_points_device: device pointers on the handle's device; enqueued on fs3_stream(sim) after the steps in flight;
 *   stream-ordered, non-blocking, no allocation, no host read.  The buffers must stay valid until the stream has passed the call.
 * fs3_sample_grid: host output, blocking.  Voxel (i, j, k) is the point
 *   world_min + (((float)i + 0.5f) / (float)width) * (world_max - world_min), likewise per axis (fs_sample_grid's expression),
 *   stored at out[(k * height + j) * width + i]; bit-identical to fs3_sample_points on those points.  A slice is depth == 1 with
 *   world_min.z == world_max.z: the expression then gives exactly that z.
 * Query order decides the speed, not the result (see "field sampling").  Nothing is sorted behind the caller's back.
 * Checks, in this order: NULL handle -> FS_ERR_INVALID; (grid) NULL view, a zero extent, or width * height * depth > 2^28 ->
 * FS_ERR_INVALID; n == 0 -> FS_OK, nothing touched; NULL points / out -> FS_ERR_INVALID; n > 2^28 -> FS_ERR_INVALID; no step
 * enqueued since create or since the last fs3_upload_particles with n > 0 (a partial upload counts: records and cell table would
 * not belong together) -> FS_ERR_INVALID.  See DESIGN.md §14. */
typedef struct fs3_sample {       /* 40 bytes; offsets 0/4/8/20/32/36 */
    float density;                /* sum m W */
    float weight;                 /* sum (m / rho_j) W: the Shepard denominator */
    fs_vec3 velocity;             /* sum (m / rho_j) W v_j, un-normalised */
    fs_vec3 gradient;             /* grad_x of sum m W */
    uint32_t neighbours;          /* candidates with r2 <= h2 */
    uint32_t cell;                /* cell id of the query point */
} fs3_sample;
typedef struct fs3_view {
    fs_vec3 world_min, world_max;
    uint32_t width, height, depth;
} fs3_view;
fs_status fs3_sample_points(fs_sim3* sim, const fs_vec3* points, size_t n, fs3_sample* out);
fs_status fs3_sample_points_device(fs_sim3* sim, const fs_vec3* points_dev, size_t n, fs3_sample* out_dev);
fs_status fs3_sample_grid(fs_sim3* sim, const fs3_view* view, fs3_sample* out);

/* ------------------------------------------------ 3D particle tracking (build extension, opt-in) */
/* The 3D counterpart of "particle tracking" above: every fs3_step cell-sorts the records and they carry no id, so "index i" names
 * a different particle after every tick.  With tracking on, the handle keeps per particle a uint32_t id and C float channels
 * (0 <= C <= FS_TRACK_MAX_CHANNELS), stored in slot order (fs3_download_particles' order) and permuted by every step exactly as the
 * records are.  Let src[i] be the slot, in the order before a step, of the particle which that step places in slot i (the
 * permutation the step's sort applies: the bitonic network's; the 3D engine has no other sort).  After the step:
 *     id[i]      = id_before[src[i]]
 *     attr[c][i] = attr_before[c][src[i]]      for c < C      (bit copies: NaN payloads, -0 and denormals survive)
 * Nothing else reads or writes them: the simulation state is bit-identical with tracking on or off, in both math modes, with
 * or without a collider or surface tension.  One gather pass per step, timed inside the FS_PASS_REORDER interval of
 * fs3_profile_read; with tracking off no launch and no allocation.  See DESIGN.md §20.
 *
 * fs3_upload_particles does NOT touch ids or channels: it replaces the records of slots, and identity stays with the slot, so
 * download -> edit -> upload keeps every id.
 *
 * fs3_track_enable: allocates on first use (8 B + 8 B per channel, per particle) and (re)initialises id[i] = i (the slot held
 *   at the moment of the call, i.e. fs3_download_particles' current order) and every channel to +0.0f.  Calling it again
 *   re-initialises, also with another channel count.  channels < 0 or > FS_TRACK_MAX_CHANNELS: FS_ERR_INVALID.  Takes effect
 *   for steps enqueued after the call and is ordered after the steps already in flight.
 * fs3_track_disable: later steps do not carry; the read calls below then return FS_ERR_INVALID.  Off is the default.
 * fs3_track_channels: -1 when off, else C.
 * fs3_track_download_* / fs3_track_upload_*: blocking host copies in slot order.  n must equal the particle count and channel
 *   must be < C, else FS_ERR_INVALID.  Uploaded ids are the caller's business (any uint32_t, duplicates allowed).
 * fs3_track_ids_device / fs3_track_attr_device: device pointers to the arrays of the last enqueued step (stream-ordered on
 *   fs3_stream), for a renderer on the same device.  Valid until the next fs3_step / fs3_timed_steps / upload / enable: the
 *   arrays ping-pong.
 * fs3_download_particles_by_id: dst[id[i]] = particle[i] for every slot with id[i] < n; entries of dst that no id names are
 *   left exactly as the caller passed them; with duplicate ids it is unspecified which record wins.  n is the length of dst
 *   and need not equal the particle count.  Blocking; off the step path. */
fs_status fs3_track_enable(fs_sim3* sim, int channels);
fs_status fs3_track_disable(fs_sim3* sim);
int fs3_track_channels(const fs_sim3* sim);
fs_status fs3_track_download_ids(fs_sim3* sim, uint32_t* dst, size_t n);
fs_status fs3_track_upload_ids(fs_sim3* sim, const uint32_t* src, size_t n);
fs_status fs3_track_download_attr(fs_sim3* sim, int channel, float* dst, size_t n);
fs_status fs3_track_upload_attr(fs_sim3* sim, int channel, const float* src, size_t n);
fs_status fs3_track_ids_device(fs_sim3* sim, const uint32_t** out);
fs_status fs3_track_attr_device(fs_sim3* sim, int channel, const float** out);
fs_status fs3_download_particles_by_id(fs_sim3* sim, fs3_particle* dst, size_t n);

/* ------------------------------------------------ 3D channel diffusion and buoyancy (build extension, opt-in) */
/* The 3D form of "channel diffusion and buoyancy" below: with these calls a tracking channel of an fs_sim3 may diffuse between
 * neighbours (heat, dye, salinity) and one channel may feed back into the motion as a Boussinesq buoyancy force.  See DESIGN.md §28.
 *
 * Tracking must be on with C >= 1 channels.  Per channel c < C there is a conductivity kappa_c >= 0; 0, the default, means the
 * channel does not diffuse.  At most one channel b is the buoyancy channel, with expansion coefficient beta and reference value
 * A0; the default is none.  The pass runs in every step after the density pass — and after the surface-tension pass when that is
 * on — and before the force pass.
 *
 * Inputs: the sorted slots' predicted positions q; this step's clamped densities rho, the values the force pass divides by; the
 * channel values A_c as the step's carry delivered them; h2 = h * h, m = the tick's mass, Cg = 6.0f * poly6 (the Cg of "3D surface
 * tension"), delta and gravity of the tick.
 *
 * Diffusion.  For sorted slot i with predicted position x, over the candidates j the density pass visits (27 cells, z outer, then
 * y, x inner, ascending slots inside a cell, cells outside the grid skipped, i itself included), in f32 without contraction, `/`
 * correctly rounded, sums starting at +0.0f:
 *     ox = q_j.x - x.x;  oy = q_j.y - x.y;  oz = q_j.z - x.z;  r2 = ox*ox + oy*oy + oz*oz
 *     if (r2 > h2) skip                          (a NaN r2 is admitted, as in "3D surface tension")
 *     d  = h2 - r2
 *     w  = m / rho_j
 *     wk = w * ((Cg * d) * d)
 *     for each diffusing channel c:  acc_c += wk * (A_c[j] - A_c[i])
 * and then, with u_i = 1.0f / rho_i and g_c = (2.0f * kappa_c) * delta formed once on the host in f32,
 *     A_c'[i] = A_c[i] + (g_c * acc_c) * u_i
 * Jacobi semantics: every A_c[j] read is the value before the pass.  A skipped candidate is skipped by a select, never multiplied
 * by zero: its A may be a NaN.  A channel with kappa_c = 0 is neither read nor written: NaN payloads, -0.0 and denormals survive
 * bit for bit.  The weight is non-negative and symmetric in i and j; its second moment is 3 (twice the sum approximates the
 * Laplacian of A) and it integrates to 9 / h^2: for a uniform fluid at rho0 the explicit update is a convex combination of the
 * neighbours' values while kappa_c * delta <= rho0 h^2 / 18.  The engine does not enforce the limit.
 *
 * Buoyancy.  With a = A_b[i], the value before the pass,
 *     s  = beta * (A0 - a);  rs = rho_i * s
 *     bv = (rs * gravity.x, rs * gravity.y, rs * gravity.z)
 *     fb = surface tension on ? (st.x + bv.x, st.y + bv.y, st.z + bv.z) : bv
 * and the integrate line is that of "3D surface tension" with fb where it has st: acc.a = (fp.a + fv.a * viscosity_coefficient)
 * + fb.a; everything after it is unchanged.  With no buoyancy channel the force pass gets what it gets without these calls.
 *
 * Bit-exact in FS_MATH_IEEE.  FS_MATH_TOLERANCE handles run this same IEEE pass on their own densities.  With nothing set a
 * handle allocates nothing and launches exactly the kernels it launched before, with the same arguments.  The pass's time falls
 * inside the FS_PASS_FORCE interval of fs3_profile_read.  FS_ABI_VERSION is unchanged.
 *
 * fs3_set_diffusion / fs3_set_buoyancy: host settings, taking effect for the steps enqueued after the call (channel = -1
 *   switches buoyancy off and ignores the two floats' values; the first buoyancy channel allocates 16 B per slot, which
 *   fs3_reserve grows).  fs3_track_enable (also a re-initialising one) and fs3_track_disable clear every conductivity and the
 *   buoyancy channel.
 * fs3_get_diffusion / fs3_get_buoyancy: the values in use (channel -1, beta 0, reference 0: no buoyancy channel).
 * FS_ERR_INVALID for these four, in this order: a NULL handle or pointer; tracking off; channel outside [0, C) (fs3_set_buoyancy:
 *   outside [-1, C)); a conductivity that is negative or not finite; a beta or reference that is not finite.
 * fs3_download_buoyancy: the last step's fb, under the rules of fs3_download_surface_tension: one fs_vec3 per particle in
 *   fs3_download_particles' slot order.  Blocking.  FS_ERR_INVALID, in this order: a NULL argument; no buoyancy channel is set; no
 *   step has been enqueued since it was set (or since the particle count changed); n != the particle count.
 *   fs3_download_surface_tension keeps returning st alone. */
fs_status fs3_set_diffusion(fs_sim3* sim, int channel, float conductivity);
fs_status fs3_get_diffusion(const fs_sim3* sim, int channel, float* conductivity);
fs_status fs3_set_buoyancy(fs_sim3* sim, int channel, float beta, float reference);   /* channel = -1: off */
fs_status fs3_get_buoyancy(const fs_sim3* sim, int* channel, float* beta, float* reference);
fs_status fs3_download_buoyancy(fs_sim3* sim, fs_vec3* dst, size_t n);

/* ------------------------------------------------ 3D channel sampling (build extension, opt-in by being called) */
/* The SPH interpolant of the tracking channels at arbitrary points: what shows a carried dye, age or temperature on a slice, on a
 * ray-marched surface (sample at the hit points) or on a mesh (sample at the vertices).  The statement is that of "3D field
 * sampling" with the same cells, order, skip rules and `r2 > h2` branch, the same W and the same
 *     t = (m / p[k].density) * W                                  IEEE division by the stored density, f32 without contraction
 * and, with attr[c] what fs3_track_download_attr returns and C = fs3_track_channels(sim), for an in-radius candidate k:
 *     weight += t;  a_c += t * attr[c][k]      for c < C
 * The sums start at +0.0f; a skipped candidate is a branch, not an added zero.  The results are un-normalised: a_c / weight is the
 * Shepard value.  Two identities follow, bit for bit, on the same points: `weight` is fs3_sample.weight; a channel that holds
 * 1.0f in every slot sums to `weight`, and channels that hold the stored velocity.x / .y / .z of every slot sum to
 * fs3_sample.velocity.  A pure function of the stored state, in both math modes.
 *
 * Outputs: attr_out[c * n + q] = a_c of query q (n = width * height * depth for a grid, voxel order and voxel centres those of
 * fs3_sample_grid); weight_out may be NULL, else weight_out[q] = weight.
 * fs3_sample_attr_points / fs3_sample_attr_grid: host pointers, blocking; the grid form is bit-identical to the point form on
 *   fs3_sample_grid's voxel centres.
 * fs3_sample_attr_points_device: device pointers on the handle's device; enqueued on fs3_stream(sim) after the steps in flight;
 *   stream-ordered, non-blocking, no allocation, no host read.  The buffers must stay valid until the stream has passed the call.
 * Checks, in this order: NULL handle -> FS_ERR_INVALID; (grid) NULL view, a zero extent, or width * height * depth > 2^28 ->
 * FS_ERR_INVALID; tracking off or C == 0 -> FS_ERR_INVALID; n == 0 -> FS_OK, nothing touched; NULL points / attr_out ->
 * FS_ERR_INVALID; n > 2^28 -> FS_ERR_INVALID; no step enqueued since create or since the last fs3_upload_particles with n > 0 ->
 * FS_ERR_INVALID.  See DESIGN.md §20. */
fs_status fs3_sample_attr_points(fs_sim3* sim, const fs_vec3* points, size_t n, float* weight_out, float* attr_out);
fs_status fs3_sample_attr_points_device(fs_sim3* sim, const fs_vec3* points_dev, size_t n, float* weight_out_dev, float* attr_out_dev);
fs_status fs3_sample_attr_grid(fs_sim3* sim, const fs3_view* view, float* weight_out, float* attr_out);

/* ------------------------------------------------ 3D surface rendering (build extension, opt-in by being called) */
/* A headless ray-marcher over the field of "3D field sampling": one ray per pixel is marched through the density until it reaches
 * `iso`, the crossing is refined by bisection, and one full sample at the hit gives the G-buffer record (distance, density,
 * outward normal, Shepard velocity).  Shading is the caller's.  All arithmetic is f32 without contraction.  `sqrt` and `/` are
 * correctly rounded.  `density(x)` is the `density` sum of the "3D field sampling" statement at point `x`, and `sample(x)` is that
 * statement's full record.  The state is exactly that statement's: the records, the grid, the settings and the mass of the last
 * step.
 *
 * For pixel (i, j), stored at out[j * width + i]:
 *     u = ((float)i + 0.5f) / (float)width  - 0.5f;   v = ((float)j + 0.5f) / (float)height - 0.5f
 *     perspective:  o = eye;                                   D.a = (forward.a + u * right.a) + v * up.a
 *     orthographic: o.a = (eye.a + u * right.a) + v * up.a;    D = forward
 *     len = sqrt((D.x*D.x + D.y*D.y) + D.z*D.z);   d.a = D.a / len;   x(t).a = o.a + t * d.a
 *     t_k = t_near + (float)k * ds                 k = 0 .. max_steps-1   (a product, never a running sum)
 *     K = the smallest k with density(x(t_k)) >= iso
 *     no such k:  record = {t 0, density 0, normal 0, velocity 0, steps max_steps, hit 0}
 *     K == 0:     t = t_0, hit = 2
 *     K  > 0:     lo = t_{K-1}, hi = t_K; `refine` times: mid = 0.5f * (lo + hi); density(x(mid)) >= iso ? hi = mid : lo = mid;   t = hi, hit = 1
 *     S = sample(x(t));  density = S.density;  gl = sqrt((gx*gx + gy*gy) + gz*gz) of S.gradient
 *     normal.a = gl > 0 ? (-S.gradient.a) / gl : +0;   velocity.a = S.weight > 0 ? S.velocity.a / S.weight : +0;   steps = K
 *
 * Which samples the kernel actually evaluates is its own business.  It may skip any t_k for which it can prove density < iso, for
 * instance when the point's 27 cells hold no particle, so the sum is exactly +0 and iso > 0.  The record must not change.  `steps`
 * is defined by K, not by work done, so it stays implementation-independent.
 *
 * Pixels with len == 0 or with non-finite camera or ray values get unspecified records.  No out-of-bounds access is allowed in
 * those cases.
 *
 * Checks, in this order:
 *  1. NULL handle, camera, params or `out` -> FS_ERR_INVALID.
 *  2. width * height == 0 or > 2^26, reserved != 0, or orthographic not 0 or 1 -> FS_ERR_INVALID.
 *  3. A params field outside the ranges below, NaN included -> FS_ERR_INVALID.
 *  4. No step since create or since the last fs3_upload_particles with n > 0 (the rule of "3D field sampling") -> FS_ERR_INVALID.
 *
 * fs3_render_surface: host output, blocking.  fs3_render_surface_device: device output on the handle's device; enqueued on
 * fs3_stream(sim) after the steps in flight; stream-ordered, non-blocking, no allocation, no host read.  If the call is not used,
 * there is no launch and no allocation.  See DESIGN.md §16. */
typedef struct fs3_camera {       /* 64 bytes */
    fs_vec3 eye, forward, right, up;   /* right / up span the whole image (they carry field of view and aspect) */
    uint32_t width, height;
    int32_t orthographic;              /* 0: perspective, rays leave `eye`; 1: parallel rays along `forward` */
    uint32_t reserved;                 /* must be 0 */
} fs3_camera;
typedef struct fs3_surface_params { /* 20 bytes */
    float iso;            /* density threshold, finite, > 0 */
    float t_near;         /* finite, >= 0 */
    float ds;             /* march step, finite, > 0 */
    uint32_t max_steps;   /* 1 .. 4096 */
    uint32_t refine;      /* bisection iterations, 0 .. 24 */
} fs3_surface_params;
typedef struct fs3_surface_hit {  /* 40 bytes; offsets 0/4/8/20/32/36 */
    float t;              /* ray parameter of the hit (distance from the ray origin: directions are normalised) */
    float density;        /* sum m W at the hit point */
    fs_vec3 normal;       /* -gradient / |gradient|, outward */
    fs_vec3 velocity;     /* Shepard-normalised */
    uint32_t steps;       /* index k of the first march sample with density >= iso; max_steps on a miss */
    uint32_t hit;         /* 0 miss, 1 surface bracketed (and refined), 2 the first sample was already inside */
} fs3_surface_hit;
fs_status fs3_render_surface(fs_sim3* sim, const fs3_camera* camera, const fs3_surface_params* params, fs3_surface_hit* out_host);
fs_status fs3_render_surface_device(fs_sim3* sim, const fs3_camera* camera, const fs3_surface_params* params, fs3_surface_hit* out_dev);

/* ------------------------------------------------ 3D surface extraction (build extension, opt-in by being called) */
/* The iso-surface of the density as an indexed triangle mesh, by surface nets (the dual method): one vertex per lattice cell the
 * surface crosses, one quad per interior lattice edge it crosses.  No case tables; the output is fully determined by the statement
 * below.  All arithmetic is f32 without contraction, `/` and `sqrt` are correctly rounded.  `density(x)` and `sample(x)` are those
 * of "3D field sampling", and the state is that statement's: the records, the grid, the settings and the mass of the last step.
 *
 * Lattice.  An fs3_view with width, height, depth >= 2 gives W x H x D NODES.  Node (i, j, k) is fs3_sample_grid's voxel centre:
 *     N_a(i) = world_min.a + (((float)i + 0.5f) / (float)W) * (world_max.a - world_min.a)     per axis a with its own extent
 *     F(i,j,k) = density(node), byte-equal to fs3_sample_grid(view).density;   inside(i,j,k) = F >= iso
 * Cells.  The lattice has (W-1)(H-1)(D-1) cells; cell (i, j, k) has the corner nodes (i+a, j+b, k+c), a, b, c in {0, 1}.  A cell
 * is ACTIVE when its eight corners are neither all inside nor all outside.
 * Vertex of an active cell.  Its twelve edges are visited in this order: the four x-edges at (y0, z0) = (0,0), (1,0), (0,1), (1,1);
 * the four y-edges at (x0, z0) in the same order; the four z-edges at (x0, y0) in the same order.  An edge runs from its low
 * corner a to its high corner b along its axis.  With sx = sy = sz = +0 and c = 0, an edge with inside(a) != inside(b) adds:
 *     tt = (iso - Fa) / (Fb - Fa);   c += 1
 *     x-edge: sx += tt; sy += (float)y0; sz += (float)z0          (y-edge: sy += tt; sx += (float)x0; sz += (float)z0;  z likewise)
 * Then, per axis a with the cell's index i_a:
 *     l.a = s_a / (float)c;   position.a = N_a(i_a) + l.a * (N_a(i_a + 1) - N_a(i_a))
 *     S = sample(position);   density = S.density;   normal and velocity from S exactly as in fs3_surface_hit:
 *     normal.a = gl > 0 ? (-S.gradient.a) / gl : +0 with gl = sqrt((gx*gx + gy*gy) + gz*gz);  velocity.a = S.weight > 0 ? S.velocity.a / S.weight : +0
 * Vertex order is ascending cell index (k*(H-1) + j)*(W-1) + i; a vertex's index is its rank among the active cells.
 * Faces.  Take the lattice edge from node n = (i, j, k) along axis A in {x, y, z}; (u, v) are the next two axes cyclically:
 * x -> (y, z), y -> (z, x), z -> (x, y).  The edge is INTERIOR when its u- and v-coordinates are both >= 1 and at most the last
 * node index minus 1 (the four cells around it then exist).  An interior edge whose two end nodes differ in `inside` emits one
 * quad of those four cells' vertices, the cells at the edge's low A-coordinate and at (u, v) offsets
 *     A = (u-1, v-1), B = (u, v-1), C = (u, v), D = (u-1, v)
 * in the order (A, B, C, D) when the low node is inside — counter-clockwise seen from +A, outward — and (A, D, C, B) otherwise.
 * Quad q becomes the triangles 2q = (v0, v1, v2) and 2q+1 = (v0, v2, v3).  Quad order is ascending 3 * ((k*H + j)*W + i) + A.
 * Edges on the lattice's boundary emit nothing: a surface that leaves the view is left open there.  Orientation is defined in
 * index space: a view flipped in an odd number of axes mirrors the winding, which is the caller's business.
 *
 * counts[0] = V and counts[1] = T are always the full counts.  Vertices [0, min(V, vert_cap)) and triangles [0, min(T, tri_cap))
 * are written (3 indices per triangle); a written triangle may name an unwritten vertex; nothing past those ranges is touched.
 * `verts` may be NULL only when vert_cap == 0, `tris` only when tri_cap == 0; both capacities 0 is a count query.  FS_OK whether or
 * not the capacities sufficed: the caller compares the counts with its capacities.
 *
 * Checks, in this order:
 *  1. NULL handle, view or counts -> FS_ERR_INVALID.
 *  2. An extent < 2, or width * height * depth > 2^26 -> FS_ERR_INVALID.
 *  3. iso not finite or not > 0 -> FS_ERR_INVALID.
 *  4. A NULL array with a non-zero capacity -> FS_ERR_INVALID.
 *  5. No step since create or since the last fs3_upload_particles with n > 0 (the rule of "3D field sampling") -> FS_ERR_INVALID.
 *
 * fs3_extract_surface: host pointers, blocking.  fs3_extract_surface_device: device pointers on the handle's device (counts_dev
 * included); enqueued on fs3_stream(sim) after the steps in flight; stream-ordered, no host read.  The scratch (node field,
 * per-node ranks, workgroup sums) belongs to the handle and grows — allocates — only when a lattice has more nodes than any
 * earlier one on that handle; otherwise the call only enqueues.  Non-finite view coordinates give unspecified records and no
 * out-of-bounds access.  Which node densities the kernels actually evaluate is their own business, as in the ray-marcher; the
 * records must not change.  If the call is not used, there is no launch and no allocation.  See DESIGN.md §17. */
typedef struct fs3_mesh_vertex {   /* 40 bytes; offsets 0/12/24/36 */
    fs_vec3 position;             /* in the active cell's box */
    fs_vec3 normal;               /* -gradient / |gradient|, outward */
    fs_vec3 velocity;             /* Shepard-normalised */
    float density;                /* sum m W at `position` */
} fs3_mesh_vertex;
fs_status fs3_extract_surface(fs_sim3* sim, const fs3_view* view, float iso, fs3_mesh_vertex* verts, uint32_t vert_cap,
                              uint32_t* tris /* 3 per triangle */, uint32_t tri_cap, uint32_t counts[2] /* V, T */);
fs_status fs3_extract_surface_device(fs_sim3* sim, const fs3_view* view, float iso, fs3_mesh_vertex* verts_dev, uint32_t vert_cap,
                                     uint32_t* tris_dev, uint32_t tri_cap, uint32_t* counts_dev /* [2] */);

/* ------------------------------------------------ 3D colliders (build extension, opt-in by being set) */
/* Static obstacles for the 3D step: the 3D counterpart of the 2D force texture (read by move_particle, compute.wgsl:127-140;
 * produced by generate_smooth_gradient_field, src/main.rs:403-515).  A collider is a W x H x D voxel field of push vectors in world
 * units over the whole domain [-size/2, size/2]; voxel (i, j, k) is field[(k * H + j) * W + i]; a zero vector is free space.  A
 * handle that never sets one launches exactly the kernels it launched before and computes the same bits.
 *
 * With a collider set, a step is the step without one followed, per particle, by the operator C below on the position p and the
 * velocity v that step stores (after its wall clamp): new state = C(step(state)).  All arithmetic is f32 without contraction, `/`
 * and `sqrt` are correctly rounded; b.a = size.a * 0.5f are the half-bounds of the step; u32_sat is the conversion of the cell
 * coordinates (oracle/sph_oracle3d.cpp cell_xyz: NaN and negatives -> 0, >= 2^32 -> 2^32 - 1, else truncation).
 *     ia = min(u32_sat(((p.a + b.a) / size.a) * (float)W_a), W_a - 1)            per axis a (W_x = W, W_y = H, W_z = D)
 *     f  = field[(iz * H + iy) * W + ix]
 *     if f.x != 0 || f.y != 0 || f.z != 0:
 *         len = sqrt((f.x*f.x + f.y*f.y) + f.z*f.z)
 *         if len > 0:                                      (a vector whose squares all underflow is treated as zero)
 *             n.a = f.a / len
 *             p.a = p.a + f.a
 *             vn  = (v.x*n.x + v.y*n.y) + v.z*n.z
 *             k   = (1.0f - damping_factor) * vn           (compute.wgsl:137-138 with a third coordinate)
 *             v.a = v.a - k * n.a
 *             per axis, in x, y, z order: if fabsf(p.a) > b.a { p.a = b.a * sign(p.a); v.a *= -1.0f * damping_factor }
 * predicted_position, density and grid are not touched.  The order is integrate, clamp, push, clamp (the reference's 2D order is
 * push, then its only clamp): the 3D oracle plus this operator on the CPU is then the whole statement.  The lookup uses the new,
 * clamped position; every index is clamped as well, so no value of p reads outside the field.
 *
 * fs3_collider_upload: a field made by the caller.  fs3_collider_from_mask: the field of a u8 voxel mask (> 128: solid, the 2D
 * producer's threshold; same layout), made on the GPU by an exact Euclidean distance transform in INDEX space — three separable
 * passes in u32 arithmetic, so every bit is determined:
 *     X: a(i,j,k) = the free i' in row (j,k) minimising |i - i'|, ties to the smaller i'; none if the row has no free voxel
 *     Y: over j' with a(i,j',k) defined, minimise (a(i,j',k) - i)^2 + (j' - j)^2, ties to the smaller j';  b = (a(i,j',k), j')
 *     Z: over k' with b(i,j,k') defined, minimise (b.x - i)^2 + (b.y - j)^2 + (k' - k)^2, ties to the smaller k';  c = (b.x, b.y, k')
 *     field(i,j,k).a = (float)((int)c.a - (int)i_a) * s_a,   s_a = size.a / (float)W_a       (a free voxel's nearest is itself: +0)
 * The squared index distance to c is the minimum over all free voxels; the tie rules only pick among equals.  "Nearest" is in
 * index space: with voxels that are not cubes it need not be the nearest free voxel in world space.  A solid voxel's vector
 * reaches the CENTRE-to-centre offset of its nearest free voxel.  `field_host` (may be NULL) receives the field, w * h * d fs_vec3.
 *
 * Checks, in this order:
 *  1. NULL handle -> FS_ERR_INVALID.
 *  2. NULL array (field, mask, dst, or one of the three extent pointers) -> FS_ERR_INVALID.
 *  3. An extent of 0 or above 1024 -> FS_ERR_INVALID.
 *  4. fs3_collider_upload: a non-finite component -> FS_ERR_INVALID.  fs3_collider_from_mask: a mask without a free voxel ->
 *     FS_ERR_INVALID.  Either way the collider set before stays as it was.
 * fs3_collider_download: FS_ERR_INVALID when no collider is set or n != w * h * d.  fs3_collider_dims: 0, 0, 0 when none.
 *
 * The calls are blocking, like fs3_upload_particles, and ordered on fs3_stream(sim): they take effect for the steps enqueued
 * afterwards, after the steps already in flight, which never see a half-replaced field.  A second upload replaces the first and
 * allocates only if the field grew; fs3_collider_clear frees it.  Setting or clearing a collider does NOT make sampling, rendering
 * or extraction stale (the records and the cell table still belong together).  The time of the operator falls inside
 * FS_PASS_FORCE.  FS_ABI_VERSION is unchanged.  See DESIGN.md §18. */
fs_status fs3_collider_upload(fs_sim3* sim, const fs_vec3* field_host, uint32_t w, uint32_t h, uint32_t d);
fs_status fs3_collider_from_mask(fs_sim3* sim, const uint8_t* mask_host, uint32_t w, uint32_t h, uint32_t d, fs_vec3* field_host /* may be NULL */);
fs_status fs3_collider_clear(fs_sim3* sim);
fs_status fs3_collider_dims(const fs_sim3* sim, uint32_t* w, uint32_t* h, uint32_t* d);      /* 0,0,0 when none */
fs_status fs3_collider_download(fs_sim3* sim, fs_vec3* dst, size_t n);                       /* n == w*h*d; FS_ERR_INVALID when none */

/* ------------------------------------------------ 3D moving bodies (build extension, opt-in by being created) */
/* Kinematic rigid bodies for the 3D step: up to FS3_MAX_BODIES per handle, each a small W x H x D voxel field of push vectors
 * (the layout of "3D colliders": field[(k * H + j) * W + i], a zero vector is free space) over the body's own box
 * [-extent/2, extent/2] in the BODY frame, with a pose and a velocity the host sets per step.  The fluid feels the body (one-way
 * coupling): the engine neither integrates the pose nor computes forces on the body.  A handle without a body launches exactly
 * the kernels it launched before and computes the same bits.
 *
 * With bodies present, a step is B_7(...B_0(C(step(state)))): the static collider C first if one is set, then the operator of
 * each existing body in ascending slot order, on the position p and the velocity v the step is about to store.  All arithmetic is
 * f32 without contraction, `/` and `sqrt` are correctly rounded, u32_sat as in "3D colliders"; b.a are the half-bounds of the
 * step and damping the tick's damping_factor.  Per body: c = centre, rij = rot[3*i + j] (world = R * local), u = velocity,
 * w = angular_velocity, hb.a = extent.a * 0.5f (on the host, once), W_x = W, W_y = H, W_z = D.
 *     d.a  = p.a - c.a
 *     q.x  = (r00*d.x + r10*d.y) + r20*d.z                                   (q = R^T d: the body frame)
 *     q.y  = (r01*d.x + r11*d.y) + r21*d.z
 *     q.z  = (r02*d.x + r12*d.y) + r22*d.z
 *     if !(fabsf(q.x) <= hb.x && fabsf(q.y) <= hb.y && fabsf(q.z) <= hb.z): unchanged      (NaN: unchanged; on a face: inside)
 *     ia = min(u32_sat(((q.a + hb.a) / extent.a) * (float)W_a), W_a - 1)
 *     g  = field[(iz * H + iy) * W + ix];   if g.x == 0 && g.y == 0 && g.z == 0: unchanged
 *     len = sqrt((g.x*g.x + g.y*g.y) + g.z*g.z);   if !(len > 0): unchanged
 *     f.x = (r00*g.x + r01*g.y) + r02*g.z;  f.y = (r10*g.x + r11*g.y) + r12*g.z;  f.z = (r20*g.x + r21*g.y) + r22*g.z
 *     n.a = f.a / len
 *     p.a = p.a + f.a
 *     s.a = p.a - c.a                                                        (the pushed position)
 *     us.x = u.x + (w.y*s.z - w.z*s.y);  us.y = u.y + (w.z*s.x - w.x*s.z);  us.z = u.z + (w.x*s.y - w.y*s.x)
 *     r.a = v.a - us.a
 *     rn  = (r.x*n.x + r.y*n.y) + r.z*n.z
 *     k   = (1.0f - damping) * rn
 *     v.a = us.a + (r.a - k*n.a)
 *     per axis, in x, y, z order: if fabsf(p.a) > b.a { p.a = b.a * sign(p.a); v.a *= -1.0f * damping }
 * predicted_position, density and grid are not touched.  FS_MATH_TOLERANCE handles run the same IEEE operator, as they do C.
 * The engine does not check that rot is a rotation, only that it is finite.  As in "2D moving bodies", the lines hold at every
 * operand a call accepts: denormal extents are not flushed, a vector whose squares overflow has n = 0, damping is used as given,
 * and an operator computes as written with the NaN, infinite or enormous velocity an earlier one left.
 *
 * fs3_body_create: a field made by the caller.  fs3_body_create_from_mask: the producer of "3D colliders" on the body's box —
 * the same three passes, the same tie rules, s_a = extent.a / (float)W_a; `field_host` (may be NULL) receives the field.
 * *body_out is the lowest free slot in 0 .. FS3_MAX_BODIES - 1; slots are stable (destroying body 1 leaves body 2 as body 2).  A
 * new body has the identity pose at the origin and zero velocities.
 *
 * Checks, in this order, all FS_ERR_INVALID; a refused call changes nothing:
 *  1. NULL handle.
 *  2. NULL array or out pointer (field, mask, body_out, motion, dst, or one of the four of fs3_body_dims).
 *  3. An extent (w, h, d) of 0 or above 1024.
 *  4. A component of the box `extent` that is not finite and > 0.
 *  5. A non-finite field component, or a mask without a free voxel.
 *  6. No free slot.
 *  7. The per-body calls: a slot that holds no body (fs3_body_download then: n != w * h * d).
 *  8. fs3_body_set_motion: any non-finite float.
 *
 * create*, download and destroy are blocking and ordered on fs3_stream(sim), exactly as the fs3_collider_* calls are; destroy
 * synchronises before freeing, because steps in flight read the field.  fs3_body_set_motion touches host memory only: a step takes
 * every body's motion by value when it is enqueued, so setting a different pose before each of several un-synchronised steps is
 * the intended use.  The pose holds until it is set again.  Nothing here makes sampling, rendering or extraction stale; particles
 * emitted inside a body are pushed by the next step.  The time of the operators falls inside FS_PASS_FORCE.  FS_ABI_VERSION is
 * unchanged.  See DESIGN.md §23. */
#define FS3_MAX_BODIES 8
typedef struct fs3_body_motion {
    fs_vec3 centre;            /* world position of the body box's centre */
    float   rot[9];            /* row-major R, world = R * local; the caller supplies a rotation, the engine checks only finiteness */
    fs_vec3 velocity;          /* of the centre, world units per second */
    fs_vec3 angular_velocity;  /* world frame, rad/s */
} fs3_body_motion;
fs_status fs3_body_create(fs_sim3* sim, const fs_vec3* field_host, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent, uint32_t* body_out);
fs_status fs3_body_create_from_mask(fs_sim3* sim, const uint8_t* mask_host, uint32_t w, uint32_t h, uint32_t d, fs_vec3 extent,
                                    fs_vec3* field_host /* may be NULL */, uint32_t* body_out);
fs_status fs3_body_set_motion(fs_sim3* sim, uint32_t body, const fs3_body_motion* motion);
fs_status fs3_body_get_motion(const fs_sim3* sim, uint32_t body, fs3_body_motion* out);
fs_status fs3_body_dims(const fs_sim3* sim, uint32_t body, uint32_t* w, uint32_t* h, uint32_t* d, fs_vec3* extent);
fs_status fs3_body_download(fs_sim3* sim, uint32_t body, fs_vec3* dst, size_t n);            /* n == w*h*d */
fs_status fs3_body_destroy(fs_sim3* sim, uint32_t body);
uint32_t  fs3_body_count(const fs_sim3* sim);                                                /* 0 for a NULL handle */

/* ------------------------------------------------ 3D body loads (build extension, opt-in per handle) */
/* The 3D form of "2D body loads": the impulse and the angular impulse the fluid gives each body of "3D moving bodies", summed on
 * the GPU inside the bodies' own pass.  fs3_body_loads_enable(sim, on) turns them on or off.  While off, a step launches exactly
 * the kernels it launches without this section and leaves the same bytes.  While on, the particle state is still byte for byte
 * that of "3D moving bodies": loads only observe.
 *
 * A HIT of body b is a particle that reaches the line `p.a = p.a + f.a` of the operator B_b above.  With that section's names:
 *   v0   the velocity on entry to B_b: after the step, after the static collider C if one is set, and after the operators of the
 *        lower slots (their wall re-clamp included);
 *   v1.a = us.a + (r.a - k*n.a): the velocity B_b computes, BEFORE its wall re-clamp — what the wall does is not the body's load;
 *   s.a  = p.a - c.a: the pushed position relative to the centre, before the re-clamp.
 * f32 without contraction, one operation per line:
 *     j.a = v0.a - v1.a                                     (a = x, y, z; impulse on the body per unit particle mass)
 *     t.x = s.y*j.z - s.z*j.y     (two products, then one subtraction; the same for the others)
 *     t.y = s.z*j.x - s.x*j.z
 *     t.z = s.x*j.y - s.y*j.x     (angular impulse about the body's centre, world frame)
 * The positional push p += f carries no momentum and is not counted.
 *
 * Fixed point: Q and the drop rule are those of "2D body loads", FS_BODY_LOAD_SHIFT reused: Q(x) is the signed 64-bit integer
 * nearest to x * 2^20, ties to even.  If any of the SIX values j.x, j.y, j.z, t.x, t.y, t.z is NaN or fails
 * fabsf(x) < 16384.0f, the hit adds nothing to the six sums and is counted in `dropped`; its particle is moved exactly as
 * without loads.  Per body the engine keeps EIGHT 64-bit words, in this order:
 *     sum Q(j.x), sum Q(j.y), sum Q(j.z), sum Q(t.x), sum Q(t.y), sum Q(t.z), hits (dropped ones included), dropped
 * each modulo 2^64 over all hits of all steps since the words were last zeroed.  Integer sums are associative, so the words are
 * ONE defined value whatever the order of lanes, waves and workgroups.  Momentum handed to body b = impulse_q * 2^-20 * (the mass
 * of one particle); angular momentum about its centre likewise from angular_q.
 *
 * Enabling (also when already on) zeroes every slot's words and `steps`.  A body created while loads are on starts at zero; a
 * destroyed slot's words are zeroed before the slot can be reused.  Steps taken while loads are off count nothing, and disabling
 * keeps the words (they cannot be read until the next enable, which zeroes them).  fs3_body_loads is blocking and ordered on
 * fs3_stream(sim): it returns the words behind every step enqueued so far; reset != 0 zeroes that slot's words and `steps` behind
 * the read, on the stream.  fs3_body_loads_device hands out the device address of FS3_MAX_BODIES x 8 64-bit words, by slot, in the
 * order above, for a consumer on the stream: it holds the finished values once any step has completed (the step's last launch
 * folds the pass's partial sums into it; the address is stable until the handle is destroyed).
 *
 * Checks, in this order, all FS_ERR_INVALID (a 3D handle has no slab form); a refused call changes nothing:
 *  1. NULL handle (fs3_body_loads_enabled: 0).
 *  2. NULL out pointer (`out`, `words`).
 *  3. fs3_body_loads: a slot that holds no body.
 *  4. fs3_body_loads, fs3_body_loads_device: loads are not enabled ("not enabled").
 * The time of both launches falls inside FS_PASS_FORCE.  FS_ABI_VERSION is unchanged.  See DESIGN.md §26. */
typedef struct fs3_body_load {
    int64_t  impulse_q[3];   /* sum Q(j.x), sum Q(j.y), sum Q(j.z) */
    int64_t  angular_q[3];   /* sum Q(t.x), sum Q(t.y), sum Q(t.z) */
    uint64_t hits, dropped;
    uint64_t steps;          /* steps enqueued with loads on since the words were zeroed (host-side count), as in 2D */
} fs3_body_load;             /* 72 bytes */
fs_status fs3_body_loads_enable(fs_sim3* sim, int on);
int       fs3_body_loads_enabled(const fs_sim3* sim);                                        /* 0 for a NULL handle */
fs_status fs3_body_loads(fs_sim3* sim, uint32_t body, fs3_body_load* out, int reset);        /* blocking */
fs_status fs3_body_loads_device(fs_sim3* sim, const void** words);

/* ------------------------------------------------ 3D surface tension (build extension, opt-in) */
/* The 3D form of the 2D step's opt-in surface tension above: a colour-field continuum-surface-force pass (Mueller, Charypar &
 * Gross 2003, §4.4) with the 3D poly6 kernel of the 3D step, W = C (h^2 - r^2)^3, C = 315/(64 pi h^9).  Enabled, every step runs
 * the pass after its density pass and before its force pass, and the integrate step adds its force:
 *     acc.a = (fp.a + fv.a * viscosity_coefficient) + st.a
 * (the division by rho_i, gravity, the NaN reset, the speed clamp, the walls and the collider operator follow unchanged).
 * fs3_tick_settings has no surface-tension knobs: sigma (coefficient) and tau (threshold) come from fs3_set_surface_tension.
 *
 * For sorted slot i with predicted position x, over the neighbours j the density pass visits (27 cells, z outer, then y, x inner,
 * ascending slots inside a cell, cells outside the grid skipped, i itself included), in f32 without contraction, `/` and sqrt
 * correctly rounded, all sums starting at +0:
 *     ox = q_j.x - x.x; oy = q_j.y - x.y; oz = q_j.z - x.z;  r2 = ox*ox + oy*oy + oz*oz;  skipped when r2 > h2
 *     d = h2 - r2;  w = m / rho_j                      (rho_j: this step's clamped density; m: the tick's mass)
 *     k = (Cg * d) * d;   n.a += w * (k * o.a)          Cg = 6.0f * poly6 (poly6 = C as the step computes it on the host)
 *     lk = (Cg * d) * ((7.0f * r2) - h2x3);  L += w * lk   h2x3 = 3.0f * h2
 *     nl = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)
 *     st = (nl > tau && nl > 0) ? s * n with s = (-sigma * L) / nl : 0
 * Bit-exact in FS_MATH_IEEE.  FS_MATH_TOLERANCE handles run the same IEEE pass on their own densities and keep their per-step
 * contract.  Off by default: a handle that never enables it launches exactly the kernels it launched before, with the same
 * arguments.  The pass's time falls inside the FS_PASS_FORCE interval of fs3_profile_read.  FS_ABI_VERSION is unchanged.  See
 * DESIGN.md §19.
 *
 * fs3_set_surface_tension: takes effect for the steps enqueued after the call (no synchronisation: steps already in flight
 * keep the values they were enqueued with).  The first enable allocates 16 B per particle.  enable == 0 ignores the two floats
 * and returns the handle to the launches of a handle that never enabled it.  FS_ERR_INVALID for a NULL handle, then for a NaN
 * coefficient, then for a NaN threshold (infinities and negative values are taken as they are).
 * fs3_surface_tension_params: the values in use; FS_ERR_INVALID for a NULL argument or when the feature is off.
 * fs3_download_surface_tension: the last step's st, one fs_vec3 per particle in fs3_download_particles' slot order.  Blocking.
 * FS_ERR_INVALID, in this order: a NULL argument; the feature is off; no step has been enqueued since it was last enabled;
 * n != the particle count. */
fs_status fs3_set_surface_tension(fs_sim3* sim, int enable, float coefficient, float threshold);
int fs3_surface_tension_enabled(const fs_sim3* sim);
fs_status fs3_surface_tension_params(const fs_sim3* sim, float* coefficient, float* threshold);
fs_status fs3_download_surface_tension(fs_sim3* sim, fs_vec3* dst, size_t n);

/* ------------------------------------------------ 3D particle count (build extension, opt-in by being called) */
/* A particle count that changes at run time: a tap, an outflow, a count that is no cube.  A handle has `capacity` slots and a
 * live count <= capacity; after fs3_create both are settings.particle_count.  fs3_particle_count returns the live count, and
 * every step, transfer and query works on exactly that many particles.  The live count is always known to the host: emission
 * has a size the caller gives, removal is a blocking call that returns how many particles went.  The step's passes are
 * unchanged, and a handle that never calls these functions launches exactly the kernels it launched before, with the same
 * arguments.  FS_ABI_VERSION is unchanged.  See DESIGN.md §21.
 *
 * fs3_reserve: grow-only and blocking.  capacity <= fs3_capacity is FS_OK and does nothing; capacity > 2^28 is FS_ERR_INVALID.
 * Every per-slot array gets `capacity` slots; the records, the tick, ids and channels, the last step's surface-tension forces,
 * the collider and the validity of the queries are preserved bit for bit.  Everything new is allocated before anything old is
 * released: on FS_ERR_OOM the handle is exactly what it was.  Device pointers handed out by fs3_track_*_device die.
 *
 * fs3_emit_particles: appends n host records at slots [count, count + n), stored as fs3_upload_particles stores them, all
 * fields as given; ordered on fs3_stream after the steps in flight, and back only when `src` has been read.  In this order: a NULL
 * handle is FS_ERR_INVALID; n == 0 is FS_OK and touches nothing; a NULL src is FS_ERR_INVALID; count + n > capacity is
 * FS_ERR_INVALID and changes nothing.
 *
 * fs3_emit_nozzle: the same append of M = nu * nv records generated on the device, no host array and no transfer.  For q in
 * [0, M), in f32 without contraction:
 *     a = q % nu;  b = q / nu;  sa = ((float)a + 0.5f) - 0.5f * (float)nu;  sb = ((float)b + 0.5f) - 0.5f * (float)nv
 *     position.c = (origin.c + sa * u.c) + sb * v.c;  predicted_position = position;  velocity = nozzle.velocity
 *     density = +0;  grid = 0;  stored at slot count + q
 * Positions outside the box are legal: the step's clamps deal with them as with an upload.  FS_ERR_INVALID, in this order: a
 * NULL handle or nozzle; nu == 0, nv == 0 or nu * nv > 2^28; any of the 12 floats not finite; count + M > capacity (nothing
 * changes).  Enqueued on fs3_stream; it waits for the steps in flight only when the count crosses a power of two.
 *
 * fs3_remove_in_box / fs3_remove_flagged: blocking.  Slot i goes when lo.a <= position.a && position.a <= hi.a on every axis
 * (inclusive edges; a NaN coordinate is never removed; the test runs on the device), or when flags_host[i] != 0, where n must
 * equal the count (else FS_ERR_INVALID).  The survivors keep their relative order; position, predicted position and density,
 * velocity, key and, with tracking on, ids and every channel move as bit copies.  *removed receives the number removed.  Fewer
 * than 2 survivors: FS_ERR_INVALID, *removed = 0, nothing changes.  Nothing matches: FS_OK, *removed = 0, nothing changes at
 * all (the queries stay valid).  NULL arguments are FS_ERR_INVALID.
 *
 * After any call that changed the count: the queries (fs3_sample_*, fs3_sample_attr_*, fs3_render_surface*,
 * fs3_extract_surface*) return FS_ERR_INVALID until the next step, fs3_download_surface_tension until the next step with the
 * pass on, and pointers from fs3_track_*_device are dead.  fs3_upload_particles still clamps to the live count and never grows it.
 *
 * Tracking: fs3_track_enable sets next_id to the live count at the call; every particle emitted while tracking is on gets
 * id = next_id++ in emission order (wrapping u32) and +0.0f in every channel; fs3_track_upload_ids does not touch next_id;
 * removal compacts ids and channels with the records.  fs3_track_next_id: next_id, or 0 when tracking is off. */
fs_status fs3_reserve(fs_sim3* sim, uint32_t capacity);
uint32_t fs3_capacity(const fs_sim3* sim);
fs_status fs3_emit_particles(fs_sim3* sim, const fs3_particle* src, size_t n);
typedef struct fs3_nozzle {       /* 56 bytes */
    fs_vec3 origin, u, v, velocity;
    uint32_t nu, nv;
} fs3_nozzle;
fs_status fs3_emit_nozzle(fs_sim3* sim, const fs3_nozzle* nozzle);
fs_status fs3_remove_in_box(fs_sim3* sim, const fs_vec3* lo, const fs_vec3* hi, uint32_t* removed);
fs_status fs3_remove_flagged(fs_sim3* sim, const uint8_t* flags_host, size_t n, uint32_t* removed);
uint32_t fs3_track_next_id(const fs_sim3* sim);

/* ------------------------------------------------------- ResizableBuffer */
/* ResizableBuffer<T>::new (src/buffer.rs:27-43). */
fs_status fs_buffer_create(int device, size_t elem_size, size_t len, const char* name, fs_buffer** out);
/* ::resize (src/buffer.rs:46-67): grow-only, copies old contents, clamps to the
 * device maximum with a warning.  *resized = 0 when new_cap < len. */
fs_status fs_buffer_resize(fs_buffer* buf, size_t new_cap, int* resized);
/* ::write (src/buffer.rs:70-87): data longer than the buffer is trimmed (and
 * logged); offset-aware superset of the reference check. */
fs_status fs_buffer_write(fs_buffer* buf, size_t offset, const void* data, size_t count);
fs_status fs_buffer_read(fs_buffer* buf, size_t offset, void* dst, size_t count);
size_t fs_buffer_len(const fs_buffer* buf);      /* SSBO::len (src/buffer.rs:170-172) */
void* fs_buffer_device_ptr(const fs_buffer* buf); /* bind_group() equivalent (src/buffer.rs:162-164) */
void fs_buffer_destroy(fs_buffer* buf);

/* ------------------------------------------------------------- self-tests */
/* Bit-exact parity makes the force pass divide-bound; three identities let it keep IEEE results
 * with far fewer instructions, and each is PROVEN by enumeration on the GPU before it is used:
 *  - division by the two loop-invariant constants (2h^3, h^2; funcs.wgsl:119) as a 3-instruction
 *    form: every f32 numerator the kernel can feed it (2^-60 <= |x| <= c, both signs) is checked
 *    against `/` for the handle's constants when the handle is created;
 *  - RN(1/b) on [2^-20, 2^20] as v_rcp_f32 + one Newton step and RN(sqrt(x)) on [2^-40, 2^40] as
 *    v_sqrt_f32 + one Newton/Markstein correction: every f32 of both ranges is checked at create;
 *  - a/b from y = RN(1/b) as q0 = a*y, q = fma(fma(-q0, b, a), y, q0): holds for all 2^46 mantissa
 *    pairs (tools/div_markstein.hip, profiles/r01_f_div_by_rcp_exhaustive.txt), used inside range
 *    guards; operands outside the guards take the true division.
 * fs_selftest_constdiv exposes the first enumeration (mismatch count for constant c, reciprocal y,
 * range [lo, hi]); fs_constdiv_status returns bit 0 / 1 = proof succeeded for 2h^3 / h^2, bit 2 / 3
 * = for the lean reciprocal / square root, bit 4 = for the cell size h of the cell-coordinate quotients (funcs.wgsl:212-214,
 * numerators 2^-60 .. 4 x the larger bound) (31 = everything in use). */
fs_status fs_selftest_constdiv(int device, float c, float y, float lo, float hi, uint32_t* mismatches);
int fs_constdiv_status(const fs_sim* sim);
/* The engine's sort (the reference network of sort.wgsl:27-51 on (key << 32 | index) pairs) run on `n` caller-supplied
 * pairs, host memory, in place.  `fuse_stage` < 0: the engine's default late-stage plan; 0: per-stage launches only;
 * k: the shifted merge from stage k (kernels_sort.hip); k | 0x100: the same with the single stand-by launch instead of
 * the per-stage ones.  plan[0] / plan[1] (may be NULL): how often the device-side
 * certificate chose the shifted merge / the per-stage plan for this call (0, 0 when no plan was in play).  Blocking. */
fs_status fs_selftest_sort(int device, uint64_t* pairs, uint32_t n, int fuse_stage, uint32_t plan[2]);
/* The host policy that picks the sort's late-stage plan (csrc/sort_policy.h), replayed on the CPU against a model of the
 * flow: `required[i]` is the lowest stage whose window the moves of step i fit (a stage more doubles the window); the
 * certificate of step i, run at the stage the policy chose, passes iff stage >= required[i], fit class min(3, stage -
 * required[i]); its report reaches the policy `lag` steps later (the engine keeps at most 4 steps in flight).
 * Outputs per step: the stage chosen, 1 where the single stand-by launch was in the stream.  No device is touched. */
fs_status fs_selftest_sort_policy(uint32_t log2_count, int start_back, uint32_t lag, const uint32_t* required, size_t steps,
                                  uint32_t* stage_out, uint32_t* single_out);

/* Diagnostics of the sort's late-stage plan (csrc/kernels_sort.hip, k_late_cert in csrc/kernels_sort_global.inc): the network's last stages run as one shifted
 * merge when a device-side certificate allows it, as per-stage launches otherwise.  Counts since create.  Blocking. */
typedef struct fs_sort_plan_info {
    uint32_t shifted;        /* sorts that took the shifted merge */
    uint32_t per_stage;      /* sorts whose certificate failed (per-stage plan: separate launches or the stand-by kernel) */
    uint32_t standby_runs;   /* of those, done by the single stand-by kernel */
    uint32_t stage;          /* first stage the shifted merge currently replaces (0: engine default) */
    uint32_t standby_single; /* 1: the single stand-by launch is in use instead of the per-stage launches */
    uint32_t timeouts;       /* stand-by grid-barrier time-outs (0 on a healthy device) */
    uint32_t wide_tiles;     /* 4096-element tiles whose keys spanned >= 2^20 - 1 cells (an uploaded, unordered state on a large grid):
                                left by the packed first kernel to the 64-bit one */
} fs_sort_plan_info;
fs_status fs_sort_plan_read(fs_sim* sim, fs_sort_plan_info* out);

/* ------------------------------------------------ channel diffusion and buoyancy (build extension, opt-in) */
/* NOT in the reference.  Without these calls a tracking channel is a passive label: nothing changes it, nothing reads it.  With
 * them a channel may diffuse between neighbours (heat, dye, salinity) and one channel may feed back into the motion as a
 * Boussinesq buoyancy force.  2D single-domain handles only; see DESIGN.md §27.
 *
 * Tracking must be on with C >= 1 channels.  Per channel c < C there is a conductivity kappa_c >= 0; 0, the default, means the
 * channel does not diffuse.  At most one channel b is the buoyancy channel, with expansion coefficient beta and reference value
 * A0; the default is none.  The pass runs in every step after the density pass — and after the surface-tension pass when that is
 * on — and before the force pass.
 *
 * Inputs: the sorted slots' predicted positions q; this step's clamped densities rho, the values the force pass divides by; the
 * channel values A_c as the step's carry (the tracking pass) delivered them; from the uniform h2 = sqr_radius, m = particle_mass,
 * Cg = poly6_kernel_derivative = 24/(pi h^8), delta and gravity.
 *
 * Diffusion.  For slot i, over the neighbours j the density pass visits (same cells, same order, same start-index rules, the
 * stale-start quirk under ref_quirks = 1 included, i itself included), in f32 without contraction, sums starting at +0.0f:
 *     ox = q_j.x - q_i.x;  oy = q_j.y - q_i.y;  r2 = ox*ox + oy*oy
 *     if (r2 > h2) skip                          (a NaN r2 is admitted, as by the surface-tension pass)
 *     d  = h2 - r2
 *     w  = m / rho_j                             (IEEE division; == |1/rho_j| as the density pass rounds it when m == 1)
 *     wk = w * ((Cg * d) * d)
 *     for each diffusing channel c:  acc_c += wk * (A_c[j] - A_c[i])
 * and then, with u_i = 1.0f / rho_i (IEEE) and g_c = (2.0f * kappa_c) * delta formed once on the host in f32,
 *     A_c'[i] = A_c[i] + (g_c * acc_c) * u_i
 * Jacobi semantics: every A_c[j] read is the value before the pass.  A skipped candidate is skipped, not multiplied by zero: its
 * A may be a NaN.  A channel with kappa_c = 0 is not written at all: NaN payloads, -0.0 and denormals survive bit for bit.
 * This is the Cleary-Monaghan / Brookshaw form with the poly6 gradient, (x_ij . grad W_ij) / r^2 = -Cg d^2: no square root, no
 * singularity at r = 0, non-negative weights, symmetric in i and j, so sum_i A_i is conserved in exact arithmetic where the
 * neighbour relation is symmetric.  The second moment of the weight is 2 (the sum approximates the Laplacian of A) and the
 * effective diffusivity is kappa_c / rho_i.  For a uniform fluid at rho0 the explicit update is a convex combination of the
 * neighbours' values while kappa_c * delta <= rho0 h^2 / 16 (the weight integrates to 8 / h^2); the engine does not enforce it.
 *
 * Buoyancy.  With a = A_b[i], the value before the pass,
 *     s  = beta * (A0 - a)
 *     bx = (rho_i * s) * gravity.x;  by = (rho_i * s) * gravity.y
 *     fb = surface tension on ? (st.x + bx, st.y + by) : (bx, by)
 * and move_particle uses ax = (fp.x + fv.x) + fb.x (likewise y) where the surface-tension step uses st; everything after it is
 * unchanged.  After the division by rho_i a hot particle gains -beta (a - A0) gravity delta of velocity.
 *
 * With buoyancy off the particle state, start_indices and ids are byte-identical with diffusion on or off, in every math mode
 * and both sort modes.  With nothing set a handle launches what it always did and allocates nothing.  FS_MATH_WGSL_ULP and
 * FS_MATH_TOLERANCE run this same IEEE pass (tolerance mode on its own densities).  The pass's time falls inside the
 * FS_PASS_FORCE interval of fs_profile_read.
 *
 * fs_set_diffusion / fs_set_buoyancy: host settings, taking effect for the steps enqueued after the call (channel = -1 switches
 *   buoyancy off; the first buoyancy channel allocates 8 B per particle).  fs_track_enable (also a re-initialising one) and
 *   fs_track_disable clear every conductivity and the buoyancy channel.
 * fs_get_diffusion / fs_get_buoyancy: the values in use (channel -1, beta 0, reference 0: no buoyancy channel).
 * fs_download_buoyancy: the last step's fb, under the rules of fs_download_surface_tension: one fs_vec2 per particle in
 *   fs_download_particles' slot order, n must equal the particle count, FS_ERR_INVALID when no step with a buoyancy channel has
 *   been enqueued since the handle was created, since the channel was last chosen, or since the count changed.  Blocking.
 * FS_ERR_INVALID: a NULL handle or argument ("null" in fs_last_error), tracking off, channel outside [0, C) (fs_set_buoyancy:
 *   outside [-1, C)), a conductivity that is negative or not finite, a beta or reference that is not finite.  A slab handle gets
 *   FS_ERR_UNSUPPORTED. */
fs_status fs_set_diffusion(fs_sim* sim, int channel, float conductivity);
fs_status fs_get_diffusion(const fs_sim* sim, int channel, float* conductivity);
fs_status fs_set_buoyancy(fs_sim* sim, int channel, float beta, float reference);   /* channel = -1: off */
fs_status fs_get_buoyancy(const fs_sim* sim, int* channel, float* beta, float* reference);
fs_status fs_download_buoyancy(fs_sim* sim, fs_vec2* dst, size_t n);

/* ------------------------------------------------ fluid diagnostics (build extension, opt-in by being called) */
/* NOT in the reference.  What the fluid as a whole is doing, reduced on the GPU without a download: momentum, kinetic energy,
 * centre of mass, density range, bounding box, the sums and ranges of the tracking channels, and a count of particles that are
 * not finite.  Single-domain handles, 2D and 3D ("3D fluid diagnostics" below is this section with three components); see
 * DESIGN.md §29.  A handle that never calls it launches exactly the kernels it launches without this section and allocates nothing.
 *
 * The result is a pure function of
 *   - the n = fs_particle_count records r[i] that fs_download_particles would return at that point of the stream,
 *   - with tracking on, the `channels` float arrays that fs_track_download_attr would return,
 *   - the tick count,
 * and of nothing else: no sort mode, no math mode, no order of particles, lanes, waves or workgroups.  All arithmetic is f32
 * without contraction, one operation per line.
 *
 * Fixed point and ordering.  Q(x) is the Q of "2D body loads": the signed 64-bit integer nearest to x * 2^FS_STATS_SHIFT, ties to
 * even; exact for |x| < 2^14.  |Q| < 2^34 and n <= 2^28, so no sum can wrap within one call.  in(x) means: not NaN and
 * fabsf(x) < 16384.0f.  Extremes follow the total order of the bit patterns of non-NaN floats, so -0 is below +0: the engine maps a
 * float to the usual order-preserving u32 key and reduces keys with integer min and max, and each extreme is ONE defined value
 * too.  Maxima start from -inf and minima from +inf, and stay there when nothing contributes.
 *
 * Per record i, with p its position, v its velocity and rho its density:
 *   - if any of the five floats is NaN or +-inf: nonfinite += 1, and the record contributes to nothing else;
 *   - otherwise  a = v.x*v.x;  b = v.y*v.y;  e = a + b   (e may be +inf);
 *     speed2_max takes e, density_min / density_max take rho, pos_min.a / pos_max.a take p.a, each as it is;
 *   - if in() holds for v.x, v.y, p.x, p.y, e and rho:  momentum_q[a] += Q(v.a);  energy_q += Q(e);  position_q[a] += Q(p.a);
 *     density_q += Q(rho);  otherwise dropped += 1 and the record is added to no sum.
 * count = n, and count - nonfinite - dropped is the number of records in every sum: every mean has one denominator.
 *
 * Per tracking channel c < channels (channels = 0 with tracking off), over all n slots, whatever the record is: a NaN or +-inf value
 * counts in attr_dropped[c] only; a finite value A enters attr_min[c] and attr_max[c]; with in(A) it adds Q(A) to attr_q[c],
 * without it counts in attr_dropped[c].  Entries with c >= channels are 0 (integers) and the starting values (floats).
 * tick = fs_tick_count; pad = 0.
 *
 * What a host derives from the words (mass and gravity are the step's):
 *     momentum         = mass * momentum_q * 2^-20
 *     kinetic energy   = 0.5 * mass * energy_q * 2^-20
 *     potential energy = -mass * (gravity . position_q) * 2^-20
 *     mean density, centre of mass = density_q, position_q * 2^-20 / (count - nonfinite - dropped)
 *     largest speed    = sqrtf(speed2_max)      — with the cell side h, a CFL time step: delta = courant * h / largest speed
 *
 * The calls work in every state of a handle: before the first step (the lattice), after fs_upload_particles (partial uploads
 * included), after steps in both sort modes and all three math modes, with a renderer hand-off live, after fs_reserve, fs_emit_* and
 * fs_remove_* (n is the live count, not the capacity), with tracking on or off.  They never move or write particle state: the
 * arrays are read in place, no record copy is made, and they may be called any number of times between steps.
 *
 * fs_stats_read: blocking; the record behind everything enqueued so far lands in `out`.
 * fs_stats_device: stream-ordered on fs_stream(sim) and without a host read: two launches that leave the record at `out_dev`, which
 *   is memory of the handle's device, 8-byte aligned, and must stay valid until the stream has passed the call.  The first call of
 *   either form allocates the handle's scratch (under 1 MB), later calls allocate nothing.
 * Checks, in this order; a refused call changes nothing:
 *  1. NULL handle -> FS_ERR_INVALID.
 *  2. A slab handle -> FS_ERR_UNSUPPORTED.
 *  3. NULL out pointer -> FS_ERR_INVALID.
 * FS_ABI_VERSION is unchanged. */
#define FS_STATS_SHIFT 20
typedef struct fs_stats {          /* 208 bytes */
    uint64_t count, nonfinite, dropped;
    int64_t  momentum_q[2], energy_q, position_q[2], density_q;
    float    speed2_max, density_min, density_max;
    fs_vec2  pos_min, pos_max;
    uint32_t tick;
    int64_t  attr_q[4];
    uint64_t attr_dropped[4];
    float    attr_min[4], attr_max[4];
    uint32_t channels, pad;
} fs_stats;
fs_status fs_stats_read(fs_sim* sim, fs_stats* out);           /* blocking */
fs_status fs_stats_device(fs_sim* sim, fs_stats* out_dev);     /* stream-ordered on fs_stream(sim), no host read */

/* ------------------------------------------------ 3D fluid diagnostics (build extension, opt-in by being called) */
/* "fluid diagnostics" above on an fs_sim3, with three components where 2D has two: seven floats decide nonfinite,
 * c = v.z*v.z and e = (a + b) + c, in() is asked of v.x, v.y, v.z, p.x, p.y, p.z, e and rho, the records are those of
 * fs3_download_particles and the channels those of fs3_track_download_attr.  The same rules for the calls; there is no 3D slab
 * handle, so the checks are 1 and 3. */
typedef struct fs3_stats {         /* 232 bytes */
    uint64_t count, nonfinite, dropped;
    int64_t  momentum_q[3], energy_q, position_q[3], density_q;
    float    speed2_max, density_min, density_max;
    fs_vec3  pos_min, pos_max;
    uint32_t tick;
    int64_t  attr_q[4];
    uint64_t attr_dropped[4];
    float    attr_min[4], attr_max[4];
    uint32_t channels, pad;
} fs3_stats;
fs_status fs3_stats_read(fs_sim3* sim, fs3_stats* out);        /* blocking */
fs_status fs3_stats_device(fs_sim3* sim, fs3_stats* out_dev);  /* stream-ordered on fs3_stream(sim), no host read */

/* ----------------------------------------------------------------- errors */
const char* fs_last_error(void);  /* thread-local, never NULL */
int fs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDSIM_H */

//! Rust binding a maintainer of rookieCookies/gpu-fluid-simulation would add to run the
//! per-tick SPH step on an MI355X through `libfluidsim_hip.so` (C ABI: include/fluidsim.h).
//! Same type names, fields and method names as src/simulation.rs and src/buffer.rs so that
//! `renderer.rs` keeps compiling: `FluidSimulation::new(device, settings)`, `.tick(settings)`,
//! `.tick` (as `tick_count()`), `SimulationUniform`, `ResizableBuffer<T>`, `SSBO<T>`.
//! NOT BUILT in this repository's image (no Rust toolchain) — source only.  It cannot drift
//! silently: tests/test_rust_shim.py parses the `extern "C"` block below and checks every symbol,
//! its arity and its pointer / scalar shape against include/fluidsim.h and the built library.
#![allow(non_camel_case_types)]
use std::ffi::{c_char, c_int, c_void, CStr, CString};
use std::marker::PhantomData;

#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)] pub struct Vec2 { pub x: f32, pub y: f32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)] pub struct Vec3 { pub x: f32, pub y: f32, pub z: f32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)] pub struct UVec2 { pub x: u32, pub y: u32 }

/// src/simulation.rs:95-104
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct SimulationSettings {
    pub particle_count: u32, pub particle_spacing: f32, pub smoothing_radius: f32,
    pub size: Vec2, pub texture_size: UVec2,
}
/// src/simulation.rs:107-122
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct TickSettings {
    pub delta: f32, pub gravity: Vec2, pub mass: f32, pub pressure_constant: f32, pub rest_density: f32,
    pub damping_factor: f32, pub viscosity_coefficient: f32, pub surface_tension_treshold: f32,
    pub surface_tension_coefficient: f32, pub mouse_force_radius: f32, pub mouse_force_power: f32,
    pub mouse_pos: Vec2, pub mouse_state: i32,
}
/// src/simulation.rs:126-135 (32 bytes)
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct ParticleInstance {
    pub position: Vec2, pub predicted_position: Vec2, pub velocity: Vec2, pub density: f32, pub grid: u32,
}
const _: () = assert!(std::mem::size_of::<ParticleInstance>() == 32);

/// src/simulation.rs:53-90 — the 120-byte uniform the renderer binds as `simulation_settings_bg`
/// (src/simulation.rs:552-554, src/renderer.rs:171,457; WGSL `Uniforms`, funcs.wgsl:17-51).
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct SimulationUniform {
    pub delta: f32, pub particle_count: u32, pub sqr_radius: f32, pub frame_time: u32,
    pub gravity: Vec2, pub bounds: Vec2, pub mouse_pos: Vec2,
    pub smoothing_radius: f32, pub particle_mass: f32, pub pressure_constant: f32, pub rest_density: f32,
    pub damping_factor: f32, pub viscosity_coefficient: f32,
    pub surface_tension_treshold: f32, pub surface_tension_coefficient: f32,
    pub poly6_kernel_volume: f32, pub poly6_kernel_derivative: f32, pub poly6_kernel_laplacian: f32,
    pub spiky_kernel_derivative: f32, pub viscosity_kernel: f32,
    pub mouse_state: i32, pub mouse_force_radius: f32, pub mouse_force_power: f32,
    pub grid_w: u32, pub grid_h: u32, pub texture_size: Vec2,
}
const _: () = assert!(std::mem::size_of::<SimulationUniform>() == 120);

/// SortUniform payload, src/simulation.rs:40-50 (without the 240-byte pad).
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct SortStep { pub group_width: u32, pub group_height: u32, pub step_index: u32, pub num_values: u32 }

/// fs_options (build-defined; the defaults reproduce the reference).
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct Options {
    pub device: i32, pub sort_mode: i32, pub ref_quirks: i32, pub math_mode: i32,
    pub initial_offset: Vec2, pub capacity: u32, pub reserved1: u32,
}
pub const SORT_BITONIC: i32 = 0;
pub const SORT_COUNTING: i32 = 1;
pub const MATH_IEEE: i32 = 0;
pub const MATH_WGSL_ULP: i32 = 1;
pub const MATH_TOLERANCE: i32 = 2;

/// fs_view: the renderer's orthographic full-domain camera (src/renderer.rs:558-561) made explicit.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct View { pub world_min: Vec2, pub world_max: Vec2, pub width: u32, pub height: u32 }

/// fs_sample: the fluid at one query point (build extension, include/fluidsim.h "field sampling"); 24 bytes.
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)]
pub struct Sample { pub density: f32, pub weight: f32, pub velocity: Vec2, pub neighbours: u32, pub cell: u32 }
const _: () = assert!(std::mem::size_of::<Sample>() == 24);

/// fs_mem_handle: interprocess / external-memory handle of a device buffer of the simulation (80 bytes).
#[repr(C)] #[derive(Clone, Copy)]
pub struct MemHandle { pub ipc: [u8; 64], pub bytes: u64, pub device: i32, pub dmabuf_fd: i32 }
const _: () = assert!(std::mem::size_of::<MemHandle>() == 80);
pub const EXPORT_PARTICLES: c_int = 0;
pub const EXPORT_START_INDICES: c_int = 1;

/// fs_sort_plan_info: diagnostics of the sort's late-stage plan.
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct SortPlanInfo { pub shifted: u32, pub per_stage: u32, pub standby_runs: u32, pub stage: u32, pub standby_single: u32, pub timeouts: u32, pub wide_tiles: u32 }

/// fs_slab_config / fs_slab_counters (multi-GPU slabs; not in the reference).
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct SlabConfig { pub own_lo: u32, pub own_hi: u32, pub has_left: u32, pub has_right: u32, pub capacity: u32, pub recv_capacity: u32, pub max_cols: u32, pub sort_mode: u32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct SlabCounters { pub n_live: u32, pub lost: u32, pub overflow: u32, pub far_halo: u32 }

/// 3D extension PODs (fs3_*; not in the reference).
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct Settings3 { pub particle_count: u32, pub particle_spacing: f32, pub smoothing_radius: f32, pub size: Vec3 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct TickSettings3 { pub delta: f32, pub gravity: Vec3, pub mass: f32, pub pressure_constant: f32, pub rest_density: f32, pub damping_factor: f32, pub viscosity_coefficient: f32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct Particle3 { pub position: Vec3, pub predicted_position: Vec3, pub velocity: Vec3, pub density: f32, pub grid: u32, pub pad: u32 }
/// fs3_sample: the 3D fluid at one query point (build extension, include/fluidsim.h "3D field sampling"); 40 bytes.
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)]
pub struct Sample3 { pub density: f32, pub weight: f32, pub velocity: Vec3, pub gradient: Vec3, pub neighbours: u32, pub cell: u32 }
const _: () = assert!(std::mem::size_of::<Sample3>() == 40);
/// fs3_view: a box and its voxel counts; a slice is `depth == 1` with `world_min.z == world_max.z`.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct View3 { pub world_min: Vec3, pub world_max: Vec3, pub width: u32, pub height: u32, pub depth: u32 }
const _: () = assert!(std::mem::size_of::<Particle3>() == 48);
/// fs3_camera: the rays of a `width` x `height` image (build extension, include/fluidsim.h "3D surface rendering"); 64 bytes.
/// `right` / `up` span the whole image; `orthographic` 0: rays leave `eye`, 1: parallel rays along `forward`; `reserved` is 0.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct Camera3 { pub eye: Vec3, pub forward: Vec3, pub right: Vec3, pub up: Vec3, pub width: u32, pub height: u32, pub orthographic: i32, pub reserved: u32 }
/// fs3_surface_params: iso > 0, t_near >= 0, ds > 0, max_steps 1 ..= 4096, refine 0 ..= 24; 20 bytes.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct SurfaceParams3 { pub iso: f32, pub t_near: f32, pub ds: f32, pub max_steps: u32, pub refine: u32 }
/// fs_nozzle: `nu` x `nv` particles centred on `origin`, spaced by `u` and `v` (include/fluidsim.h "2D particle count"); 40 bytes.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct Nozzle { pub origin: Vec2, pub u: Vec2, pub v: Vec2, pub velocity: Vec2, pub nu: u32, pub nv: u32 }
const _: () = assert!(std::mem::size_of::<Nozzle>() == 40);
/// fs3_nozzle: a layer of `nu` x `nv` particles centred on `origin`, spaced by `u` and `v` (include/fluidsim.h "3D particle count"); 56 bytes.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct Nozzle3 { pub origin: Vec3, pub u: Vec3, pub v: Vec3, pub velocity: Vec3, pub nu: u32, pub nv: u32 }
const _: () = assert!(std::mem::size_of::<Nozzle3>() == 56);
/// fs3_body_motion: pose and velocity of a moving body (build extension, include/fluidsim.h "3D moving bodies"); 72 bytes.
/// `rot`: row-major R, world = R * local; the engine checks only that it is finite.
#[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
pub struct BodyMotion3 { pub centre: Vec3, pub rot: [f32; 9], pub velocity: Vec3, pub angular_velocity: Vec3 }
const _: () = assert!(std::mem::size_of::<BodyMotion3>() == 72);
impl Default for BodyMotion3 {
    /// The motion of a new body: the identity pose at the origin, at rest.
    fn default() -> Self {
        BodyMotion3 { centre: Vec3::default(), rot: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], velocity: Vec3::default(), angular_velocity: Vec3::default() }
    }
}
/// fs_body_motion: pose and velocity of a 2D moving body (build extension, include/fluidsim.h "2D moving bodies"); 36 bytes.
/// `rot`: row-major R, world = R * local; the engine checks only that it is finite.  `angular_velocity`: rad/s, counter-clockwise.
#[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
pub struct BodyMotion { pub centre: Vec2, pub rot: [f32; 4], pub velocity: Vec2, pub angular_velocity: f32 }
const _: () = assert!(std::mem::size_of::<BodyMotion>() == 36);
impl Default for BodyMotion {
    /// The motion of a new body: the identity pose at the origin, at rest.
    fn default() -> Self {
        BodyMotion { centre: Vec2::default(), rot: [1.0, 0.0, 0.0, 1.0], velocity: Vec2::default(), angular_velocity: 0.0 }
    }
}
/// fs_body_load: what the fluid handed one 2D body (build extension, include/fluidsim.h "2D body loads"); 48 bytes.  The three
/// sums are in units of 2^-BODY_LOAD_SHIFT per unit particle mass, modulo 2^64.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct BodyLoad { pub impulse_q: [i64; 2], pub angular_q: i64, pub hits: u64, pub dropped: u64, pub steps: u64 }
const _: () = assert!(std::mem::size_of::<BodyLoad>() == 48);
/// FS_BODY_LOAD_SHIFT
pub const BODY_LOAD_SHIFT: u32 = 20;
impl BodyLoad {
    /// Momentum handed to the body: `impulse_q * 2^-20 * mass`, `mass` the mass of one particle.
    pub fn impulse(&self, mass: f64) -> [f64; 2] {
        let k = mass / (1u64 << BODY_LOAD_SHIFT) as f64;
        [self.impulse_q[0] as f64 * k, self.impulse_q[1] as f64 * k]
    }
    /// Angular momentum about the body's centre handed to the body, counter-clockwise positive.
    pub fn angular_impulse(&self, mass: f64) -> f64 { self.angular_q as f64 * mass / (1u64 << BODY_LOAD_SHIFT) as f64 }
}
/// fs_stats: the fluid diagnostics of a 2D handle (build extension, include/fluidsim.h "fluid diagnostics"); 208 bytes.  The `_q`
/// words are sums of Q(x) = rint(x * 2^STATS_SHIFT) over the records that are finite and in range.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct Stats {
    pub count: u64, pub nonfinite: u64, pub dropped: u64,
    pub momentum_q: [i64; 2], pub energy_q: i64, pub position_q: [i64; 2], pub density_q: i64,
    pub speed2_max: f32, pub density_min: f32, pub density_max: f32,
    pub pos_min: Vec2, pub pos_max: Vec2,
    pub tick: u32,
    pub attr_q: [i64; 4], pub attr_dropped: [u64; 4], pub attr_min: [f32; 4], pub attr_max: [f32; 4],
    pub channels: u32, pub pad: u32,
}
const _: () = assert!(std::mem::size_of::<Stats>() == 208);
/// fs3_stats: the same record with three components; 232 bytes.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct Stats3 {
    pub count: u64, pub nonfinite: u64, pub dropped: u64,
    pub momentum_q: [i64; 3], pub energy_q: i64, pub position_q: [i64; 3], pub density_q: i64,
    pub speed2_max: f32, pub density_min: f32, pub density_max: f32,
    pub pos_min: Vec3, pub pos_max: Vec3,
    pub tick: u32,
    pub attr_q: [i64; 4], pub attr_dropped: [u64; 4], pub attr_min: [f32; 4], pub attr_max: [f32; 4],
    pub channels: u32, pub pad: u32,
}
const _: () = assert!(std::mem::size_of::<Stats3>() == 232);
/// FS_STATS_SHIFT
pub const STATS_SHIFT: u32 = 20;
impl Stats {
    /// The number of records in every sum: the one denominator of every mean.
    pub fn summed(&self) -> u64 { self.count - self.nonfinite - self.dropped }
    /// `sqrtf(speed2_max)`; 0 when no finite record contributed.
    pub fn max_speed(&self) -> f32 { if self.speed2_max == f32::NEG_INFINITY { 0.0 } else { self.speed2_max.sqrt() } }
    /// `0.5 * mass * energy_q * 2^-20`, `mass` the mass of one particle.
    pub fn kinetic_energy(&self, mass: f64) -> f64 { 0.5 * mass * self.energy_q as f64 / (1u64 << STATS_SHIFT) as f64 }
}
impl Stats3 {
    pub fn summed(&self) -> u64 { self.count - self.nonfinite - self.dropped }
    pub fn max_speed(&self) -> f32 { if self.speed2_max == f32::NEG_INFINITY { 0.0 } else { self.speed2_max.sqrt() } }
    pub fn kinetic_energy(&self, mass: f64) -> f64 { 0.5 * mass * self.energy_q as f64 / (1u64 << STATS_SHIFT) as f64 }
}
/// fs3_body_load: what the fluid handed one 3D body (build extension, include/fluidsim.h "3D body loads"); 72 bytes.  The six
/// sums are in units of 2^-BODY_LOAD_SHIFT per unit particle mass, modulo 2^64; `angular_q` is about the body's centre, world frame.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct Body3Load { pub impulse_q: [i64; 3], pub angular_q: [i64; 3], pub hits: u64, pub dropped: u64, pub steps: u64 }
const _: () = assert!(std::mem::size_of::<Body3Load>() == 72);
impl Body3Load {
    /// Momentum handed to the body: `impulse_q * 2^-20 * mass`, `mass` the mass of one particle.
    pub fn impulse(&self, mass: f64) -> [f64; 3] {
        let k = mass / (1u64 << BODY_LOAD_SHIFT) as f64;
        [self.impulse_q[0] as f64 * k, self.impulse_q[1] as f64 * k, self.impulse_q[2] as f64 * k]
    }
    /// Angular momentum about the body's centre handed to the body, world frame.
    pub fn angular_impulse(&self, mass: f64) -> [f64; 3] {
        let k = mass / (1u64 << BODY_LOAD_SHIFT) as f64;
        [self.angular_q[0] as f64 * k, self.angular_q[1] as f64 * k, self.angular_q[2] as f64 * k]
    }
}
/// FS_MAX_BODIES: the body slots of a 2D handle.
pub const MAX_BODIES: u32 = 8;
/// FS3_MAX_BODIES: the body slots of a 3D handle.
pub const MAX_BODIES3: u32 = 8;
/// fs3_surface_hit: one pixel of the G-buffer; 40 bytes, offsets 0/4/8/20/32/36.  `hit` 0: miss, 1: bracketed and refined, 2: the first sample was inside.
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)]
pub struct SurfaceHit3 { pub t: f32, pub density: f32, pub normal: Vec3, pub velocity: Vec3, pub steps: u32, pub hit: u32 }
const _: () = assert!(std::mem::size_of::<Camera3>() == 64 && std::mem::size_of::<SurfaceParams3>() == 20 && std::mem::size_of::<SurfaceHit3>() == 40);
/// fs3_mesh_vertex: one vertex of an extracted iso-surface (build extension, include/fluidsim.h "3D surface extraction"); 40 bytes, offsets 0/12/24/36.
#[repr(C)] #[derive(Clone, Copy, Default, Debug, PartialEq)]
pub struct MeshVertex3 { pub position: Vec3, pub normal: Vec3, pub velocity: Vec3, pub density: f32 }
const _: () = assert!(std::mem::size_of::<MeshVertex3>() == 40);

#[repr(C)] pub struct fs_sim { _p: [u8; 0] }
#[repr(C)] pub struct fs_sim3 { _p: [u8; 0] }
#[repr(C)] pub struct fs_buffer { _p: [u8; 0] }
#[repr(C)] pub struct fs_comm { _p: [u8; 0] }

pub const PASS_COUNT: usize = 6;   // FS_PASS_COUNT (the sixth, FS_PASS_BOUNDARY, is non-zero on slab handles only)
/// fs_slab_config.sort_mode | SLAB_SERIAL: the serial slab step instead of the overlapped one.
pub const SLAB_SERIAL: u32 = 0x100;
pub const COMM_ID_BYTES: usize = 128;

// Every entry point of include/fluidsim.h, in the header's order.
extern "C" {
    // lifecycle — FluidSimulation::new / Drop (src/simulation.rs:139, src/renderer.rs:31)
    fn fs_create(settings: *const SimulationSettings, device: c_int, out: *mut *mut fs_sim) -> c_int;
    fn fs_create_ex(settings: *const SimulationSettings, opts: *const Options, out: *mut *mut fs_sim) -> c_int;
    fn fs_options_default(opts: *mut Options);
    fn fs_destroy(sim: *mut fs_sim);
    // stepping — FluidSimulation::tick (src/simulation.rs:459-539)
    fn fs_step(sim: *mut fs_sim, tick: *const TickSettings) -> c_int;
    fn fs_sync(sim: *mut fs_sim) -> c_int;
    fn fs_tick_count(sim: *const fs_sim) -> u32;
    fn fs_particle_count(sim: *const fs_sim) -> u32;
    fn fs_grid_dims(sim: *const fs_sim, grid_w: *mut u32, grid_h: *mut u32) -> c_int;
    fn fs_stream(sim: *const fs_sim) -> *mut c_void;
    // data the renderer consumes (src/simulation.rs:542-564)
    fn fs_particles_device(sim: *mut fs_sim, out: *mut *const ParticleInstance) -> c_int;
    fn fs_start_indices_device(sim: *mut fs_sim, out: *mut *const u32, count: *mut usize) -> c_int;
    fn fs_get_uniform(sim: *const fs_sim, out: *mut SimulationUniform) -> c_int;
    fn fs_upload_force_field(sim: *mut fs_sim, field: *const Vec2, w: u32, h: u32) -> c_int;
    fn fs_export_handle(sim: *mut fs_sim, which: c_int, out: *mut MemHandle) -> c_int;
    fn fs_import_open(handle: *const MemHandle, device: c_int, dev_ptr: *mut *mut c_void) -> c_int;
    fn fs_import_read(dev_ptr: *const c_void, offset: usize, dst: *mut c_void, bytes: usize) -> c_int;
    fn fs_import_close(dev_ptr: *mut c_void) -> c_int;
    fn fs_download_particles(sim: *mut fs_sim, dst: *mut ParticleInstance, n: usize) -> c_int;
    fn fs_upload_particles(sim: *mut fs_sim, src: *const ParticleInstance, n: usize) -> c_int;
    fn fs_download_start_indices(sim: *mut fs_sim, dst: *mut u32, n: usize) -> c_int;
    fn fs_upload_start_indices(sim: *mut fs_sim, src: *const u32, n: usize) -> c_int;
    // host-side mirrors (pure)
    fn fs_reference_lattice(settings: *const SimulationSettings, offset: Vec2, dst: *mut ParticleInstance, n: usize) -> c_int;
    fn fs_sort_schedule(particle_count: u32, dst: *mut SortStep, cap: usize) -> usize;
    fn fs_build_uniform(settings: *const SimulationSettings, tick: *const TickSettings, tick_count: u32, out: *mut SimulationUniform) -> c_int;
    // obstacle field producer, headless density splat
    fn fs_generate_force_field(sim: *mut fs_sim, device: c_int, image: *const u8, w: u32, h: u32, field_host: *mut Vec2) -> c_int;
    fn fs_render_density(sim: *mut fs_sim, view: *const View, rgba_host: *mut f32) -> c_int;
    fn fs_sample_points(sim: *mut fs_sim, points: *const Vec2, n: usize, out: *mut Sample, attr_out: *mut f32) -> c_int;
    fn fs_sample_points_device(sim: *mut fs_sim, points_dev: *const Vec2, n: usize, out_dev: *mut Sample, attr_out_dev: *mut f32) -> c_int;
    fn fs_sample_grid(sim: *mut fs_sim, view: *const View, out: *mut Sample, attr_out: *mut f32) -> c_int;
    // 2D particle count
    fn fs_reserve(sim: *mut fs_sim, capacity: u32) -> c_int;
    fn fs_capacity(sim: *const fs_sim) -> u32;
    fn fs_emit_particles(sim: *mut fs_sim, src: *const ParticleInstance, n: usize) -> c_int;
    fn fs_emit_nozzle(sim: *mut fs_sim, nozzle: *const Nozzle) -> c_int;
    fn fs_remove_in_box(sim: *mut fs_sim, lo: *const Vec2, hi: *const Vec2, removed: *mut u32) -> c_int;
    fn fs_remove_flagged(sim: *mut fs_sim, flags_host: *const u8, n: usize, removed: *mut u32) -> c_int;
    fn fs_track_next_id(sim: *const fs_sim) -> u32;
    fn fs_body_create(sim: *mut fs_sim, field_host: *const Vec2, w: u32, h: u32, extent: Vec2, body_out: *mut u32) -> c_int;
    fn fs_body_create_from_mask(sim: *mut fs_sim, mask_host: *const u8, w: u32, h: u32, extent: Vec2, field_host: *mut Vec2, body_out: *mut u32) -> c_int;
    fn fs_body_set_motion(sim: *mut fs_sim, body: u32, motion: *const BodyMotion) -> c_int;
    fn fs_body_get_motion(sim: *const fs_sim, body: u32, out: *mut BodyMotion) -> c_int;
    fn fs_body_dims(sim: *const fs_sim, body: u32, w: *mut u32, h: *mut u32, extent: *mut Vec2) -> c_int;
    fn fs_body_download(sim: *mut fs_sim, body: u32, dst: *mut Vec2, n: usize) -> c_int;
    fn fs_body_destroy(sim: *mut fs_sim, body: u32) -> c_int;
    fn fs_body_count(sim: *const fs_sim) -> u32;
    fn fs_body_loads_enable(sim: *mut fs_sim, on: c_int) -> c_int;
    fn fs_body_loads_enabled(sim: *const fs_sim) -> c_int;
    fn fs_body_loads(sim: *mut fs_sim, body: u32, out: *mut BodyLoad, reset: c_int) -> c_int;
    fn fs_body_loads_device(sim: *mut fs_sim, words: *mut *const c_void) -> c_int;
    fn fs_stats_read(sim: *mut fs_sim, out: *mut Stats) -> c_int;
    fn fs_stats_device(sim: *mut fs_sim, out_dev: *mut Stats) -> c_int;
    // profiling
    fn fs_profile_enable(sim: *mut fs_sim, enable: c_int) -> c_int;
    fn fs_profile_read(sim: *mut fs_sim, ms: *mut f64, steps: *mut u64, reset: c_int) -> c_int;
    fn fs_timed_steps(sim: *mut fs_sim, tick: *const TickSettings, steps: u32, ms_total: *mut f64) -> c_int;
    // surface tension (build extension, opt-in)
    fn fs_set_surface_tension(sim: *mut fs_sim, enable: c_int) -> c_int;
    fn fs_surface_tension_enabled(sim: *const fs_sim) -> c_int;
    fn fs_download_surface_tension(sim: *mut fs_sim, dst: *mut Vec2, n: usize) -> c_int;
    fn fs_set_diffusion(sim: *mut fs_sim, channel: c_int, conductivity: f32) -> c_int;
    fn fs_get_diffusion(sim: *const fs_sim, channel: c_int, conductivity: *mut f32) -> c_int;
    fn fs_set_buoyancy(sim: *mut fs_sim, channel: c_int, beta: f32, reference: f32) -> c_int;
    fn fs_get_buoyancy(sim: *const fs_sim, channel: *mut c_int, beta: *mut f32, reference: *mut f32) -> c_int;
    fn fs_download_buoyancy(sim: *mut fs_sim, dst: *mut Vec2, n: usize) -> c_int;
    // particle tracking (build extension, opt-in)
    fn fs_track_enable(sim: *mut fs_sim, channels: c_int) -> c_int;
    fn fs_track_disable(sim: *mut fs_sim) -> c_int;
    fn fs_track_channels(sim: *const fs_sim) -> c_int;
    fn fs_track_download_ids(sim: *mut fs_sim, dst: *mut u32, n: usize) -> c_int;
    fn fs_track_upload_ids(sim: *mut fs_sim, src: *const u32, n: usize) -> c_int;
    fn fs_track_download_attr(sim: *mut fs_sim, channel: c_int, dst: *mut f32, n: usize) -> c_int;
    fn fs_track_upload_attr(sim: *mut fs_sim, channel: c_int, src: *const f32, n: usize) -> c_int;
    fn fs_track_ids_device(sim: *mut fs_sim, out: *mut *const u32) -> c_int;
    fn fs_track_attr_device(sim: *mut fs_sim, channel: c_int, out: *mut *const f32) -> c_int;
    fn fs_download_particles_by_id(sim: *mut fs_sim, dst: *mut ParticleInstance, n: usize) -> c_int;
    // multi-GPU slab mode
    fn fs_slab_create(global_settings: *const SimulationSettings, device: c_int, cfg: *const SlabConfig, out: *mut *mut fs_sim) -> c_int;
    fn fs_slab_upload_owned(sim: *mut fs_sim, src: *const ParticleInstance, n: usize) -> c_int;
    fn fs_slab_set_window(sim: *mut fs_sim, own_lo: u32, own_hi: u32) -> c_int;
    fn fs_slab_message_bytes(sim: *const fs_sim) -> usize;
    fn fs_slab_pack(sim: *mut fs_sim, tick: *const TickSettings, send_left: *mut c_void, send_right: *mut c_void) -> c_int;
    fn fs_slab_step(sim: *mut fs_sim, recv_left: *const c_void, recv_right: *const c_void) -> c_int;
    fn fs_slab_overlapped(sim: *const fs_sim) -> c_int;
    fn fs_slab_set_boundary_cols(sim: *mut fs_sim, cols: u32) -> c_int;
    fn fs_slab_boundary_cols(sim: *const fs_sim) -> u32;
    fn fs_slab_comm_stream(sim: *const fs_sim) -> *mut c_void;
    fn fs_slab_comm_begin(sim: *mut fs_sim) -> c_int;
    fn fs_slab_comm_end(sim: *mut fs_sim) -> c_int;
    fn fs_slab_wait_packed(sim: *mut fs_sim) -> c_int;
    fn fs_slab_counters_read(sim: *mut fs_sim, out: *mut SlabCounters) -> c_int;
    fn fs_slab_download(sim: *mut fs_sim, dst: *mut ParticleInstance, owned: *mut u8, cap: usize, n_live: *mut u32) -> c_int;
    fn fs_slab_max_speed(sim: *mut fs_sim, out: *mut f32) -> c_int;
    fn fs_slab_column_histogram(sim: *mut fs_sim, hist: *mut u32, grid_w_global: usize) -> c_int;
    fn fs_slab_rebalance_stats(sim: *mut fs_sim, stats: *mut u32, hist: *mut u32, grid_w_global: usize) -> c_int;
    // native RCCL transport
    fn fs_comm_unique_id(id: *mut u8) -> c_int;
    fn fs_comm_init(device: c_int, rank: c_int, world: c_int, id: *const u8, out: *mut *mut fs_comm) -> c_int;
    fn fs_comm_destroy(comm: *mut fs_comm);
    fn fs_slab_exchange(sim: *mut fs_sim, comm: *mut fs_comm, left_rank: c_int, right_rank: c_int,
                        send_left: *const c_void, send_right: *const c_void,
                        recv_left: *mut c_void, recv_right: *mut c_void) -> c_int;
    fn fs_comm_allreduce(sim: *mut fs_sim, comm: *mut fs_comm, device_buf: *mut c_void, count: usize, dtype: c_int, op: c_int) -> c_int;
    // 3D extension
    fn fs3_create(settings: *const Settings3, device: c_int, initial_offset: Vec3, out: *mut *mut fs_sim3) -> c_int;
    fn fs3_create_ex(settings: *const Settings3, device: c_int, initial_offset: Vec3, math_mode: c_int, out: *mut *mut fs_sim3) -> c_int;
    fn fs3_destroy(sim: *mut fs_sim3);
    fn fs3_step(sim: *mut fs_sim3, tick: *const TickSettings3) -> c_int;
    fn fs3_sync(sim: *mut fs_sim3) -> c_int;
    fn fs3_tick_count(sim: *const fs_sim3) -> u32;
    fn fs3_particle_count(sim: *const fs_sim3) -> u32;
    fn fs3_grid_dims(sim: *const fs_sim3, w: *mut u32, h: *mut u32, d: *mut u32) -> c_int;
    fn fs3_download_particles(sim: *mut fs_sim3, dst: *mut Particle3, n: usize) -> c_int;
    fn fs3_upload_particles(sim: *mut fs_sim3, src: *const Particle3, n: usize) -> c_int;
    fn fs3_reference_lattice(settings: *const Settings3, offset: Vec3, dst: *mut Particle3, n: usize) -> c_int;
    fn fs3_timed_steps(sim: *mut fs_sim3, tick: *const TickSettings3, steps: u32, ms_total: *mut f64) -> c_int;
    fn fs3_profile_enable(sim: *mut fs_sim3, enable: c_int) -> c_int;
    fn fs3_profile_read(sim: *mut fs_sim3, ms: *mut f64, steps: *mut u64, reset: c_int) -> c_int;
    fn fs3_stream(sim: *const fs_sim3) -> *mut c_void;
    fn fs3_sample_points(sim: *mut fs_sim3, points: *const Vec3, n: usize, out: *mut Sample3) -> c_int;
    fn fs3_sample_points_device(sim: *mut fs_sim3, points_dev: *const Vec3, n: usize, out_dev: *mut Sample3) -> c_int;
    fn fs3_sample_grid(sim: *mut fs_sim3, view: *const View3, out: *mut Sample3) -> c_int;
    fn fs3_track_enable(sim: *mut fs_sim3, channels: c_int) -> c_int;
    fn fs3_track_disable(sim: *mut fs_sim3) -> c_int;
    fn fs3_track_channels(sim: *const fs_sim3) -> c_int;
    fn fs3_track_download_ids(sim: *mut fs_sim3, dst: *mut u32, n: usize) -> c_int;
    fn fs3_track_upload_ids(sim: *mut fs_sim3, src: *const u32, n: usize) -> c_int;
    fn fs3_track_download_attr(sim: *mut fs_sim3, channel: c_int, dst: *mut f32, n: usize) -> c_int;
    fn fs3_track_upload_attr(sim: *mut fs_sim3, channel: c_int, src: *const f32, n: usize) -> c_int;
    fn fs3_track_ids_device(sim: *mut fs_sim3, out: *mut *const u32) -> c_int;
    fn fs3_track_attr_device(sim: *mut fs_sim3, channel: c_int, out: *mut *const f32) -> c_int;
    fn fs3_download_particles_by_id(sim: *mut fs_sim3, dst: *mut Particle3, n: usize) -> c_int;
    fn fs3_sample_attr_points(sim: *mut fs_sim3, points: *const Vec3, n: usize, weight_out: *mut f32, attr_out: *mut f32) -> c_int;
    fn fs3_sample_attr_points_device(sim: *mut fs_sim3, points_dev: *const Vec3, n: usize, weight_out_dev: *mut f32, attr_out_dev: *mut f32) -> c_int;
    fn fs3_sample_attr_grid(sim: *mut fs_sim3, view: *const View3, weight_out: *mut f32, attr_out: *mut f32) -> c_int;
    fn fs3_render_surface(sim: *mut fs_sim3, camera: *const Camera3, params: *const SurfaceParams3, out_host: *mut SurfaceHit3) -> c_int;
    fn fs3_render_surface_device(sim: *mut fs_sim3, camera: *const Camera3, params: *const SurfaceParams3, out_dev: *mut SurfaceHit3) -> c_int;
    fn fs3_extract_surface(sim: *mut fs_sim3, view: *const View3, iso: f32, verts: *mut MeshVertex3, vert_cap: u32, tris: *mut u32, tri_cap: u32, counts: *mut u32) -> c_int;
    fn fs3_extract_surface_device(sim: *mut fs_sim3, view: *const View3, iso: f32, verts_dev: *mut MeshVertex3, vert_cap: u32, tris_dev: *mut u32, tri_cap: u32, counts_dev: *mut u32) -> c_int;
    fn fs3_collider_upload(sim: *mut fs_sim3, field_host: *const Vec3, w: u32, h: u32, d: u32) -> c_int;
    fn fs3_collider_from_mask(sim: *mut fs_sim3, mask_host: *const u8, w: u32, h: u32, d: u32, field_host: *mut Vec3) -> c_int;
    fn fs3_collider_clear(sim: *mut fs_sim3) -> c_int;
    fn fs3_collider_dims(sim: *const fs_sim3, w: *mut u32, h: *mut u32, d: *mut u32) -> c_int;
    fn fs3_collider_download(sim: *mut fs_sim3, dst: *mut Vec3, n: usize) -> c_int;
    fn fs3_body_create(sim: *mut fs_sim3, field_host: *const Vec3, w: u32, h: u32, d: u32, extent: Vec3, body_out: *mut u32) -> c_int;
    fn fs3_body_create_from_mask(sim: *mut fs_sim3, mask_host: *const u8, w: u32, h: u32, d: u32, extent: Vec3, field_host: *mut Vec3, body_out: *mut u32) -> c_int;
    fn fs3_body_set_motion(sim: *mut fs_sim3, body: u32, motion: *const BodyMotion3) -> c_int;
    fn fs3_body_get_motion(sim: *const fs_sim3, body: u32, out: *mut BodyMotion3) -> c_int;
    fn fs3_body_dims(sim: *const fs_sim3, body: u32, w: *mut u32, h: *mut u32, d: *mut u32, extent: *mut Vec3) -> c_int;
    fn fs3_body_download(sim: *mut fs_sim3, body: u32, dst: *mut Vec3, n: usize) -> c_int;
    fn fs3_body_destroy(sim: *mut fs_sim3, body: u32) -> c_int;
    fn fs3_body_count(sim: *const fs_sim3) -> u32;
    fn fs3_body_loads_enable(sim: *mut fs_sim3, on: c_int) -> c_int;
    fn fs3_body_loads_enabled(sim: *const fs_sim3) -> c_int;
    fn fs3_body_loads(sim: *mut fs_sim3, body: u32, out: *mut Body3Load, reset: c_int) -> c_int;
    fn fs3_body_loads_device(sim: *mut fs_sim3, words: *mut *const c_void) -> c_int;
    fn fs3_stats_read(sim: *mut fs_sim3, out: *mut Stats3) -> c_int;
    fn fs3_stats_device(sim: *mut fs_sim3, out_dev: *mut Stats3) -> c_int;
    fn fs3_set_surface_tension(sim: *mut fs_sim3, enable: c_int, coefficient: f32, threshold: f32) -> c_int;
    fn fs3_surface_tension_enabled(sim: *const fs_sim3) -> c_int;
    fn fs3_surface_tension_params(sim: *const fs_sim3, coefficient: *mut f32, threshold: *mut f32) -> c_int;
    fn fs3_download_surface_tension(sim: *mut fs_sim3, dst: *mut Vec3, n: usize) -> c_int;
    fn fs3_set_diffusion(sim: *mut fs_sim3, channel: c_int, conductivity: f32) -> c_int;
    fn fs3_get_diffusion(sim: *const fs_sim3, channel: c_int, conductivity: *mut f32) -> c_int;
    fn fs3_set_buoyancy(sim: *mut fs_sim3, channel: c_int, beta: f32, reference: f32) -> c_int;
    fn fs3_get_buoyancy(sim: *const fs_sim3, channel: *mut c_int, beta: *mut f32, reference: *mut f32) -> c_int;
    fn fs3_download_buoyancy(sim: *mut fs_sim3, dst: *mut Vec3, n: usize) -> c_int;
    fn fs3_reserve(sim: *mut fs_sim3, capacity: u32) -> c_int;
    fn fs3_capacity(sim: *const fs_sim3) -> u32;
    fn fs3_emit_particles(sim: *mut fs_sim3, src: *const Particle3, n: usize) -> c_int;
    fn fs3_emit_nozzle(sim: *mut fs_sim3, nozzle: *const Nozzle3) -> c_int;
    fn fs3_remove_in_box(sim: *mut fs_sim3, lo: *const Vec3, hi: *const Vec3, removed: *mut u32) -> c_int;
    fn fs3_remove_flagged(sim: *mut fs_sim3, flags_host: *const u8, n: usize, removed: *mut u32) -> c_int;
    fn fs3_track_next_id(sim: *const fs_sim3) -> u32;
    // ResizableBuffer<T> (src/buffer.rs)
    fn fs_buffer_create(device: c_int, elem_size: usize, len: usize, name: *const c_char, out: *mut *mut fs_buffer) -> c_int;
    fn fs_buffer_resize(buf: *mut fs_buffer, new_cap: usize, resized: *mut c_int) -> c_int;
    fn fs_buffer_write(buf: *mut fs_buffer, offset: usize, data: *const c_void, count: usize) -> c_int;
    fn fs_buffer_read(buf: *mut fs_buffer, offset: usize, dst: *mut c_void, count: usize) -> c_int;
    fn fs_buffer_len(buf: *const fs_buffer) -> usize;
    fn fs_buffer_device_ptr(buf: *const fs_buffer) -> *mut c_void;
    fn fs_buffer_destroy(buf: *mut fs_buffer);
    // self-tests and diagnostics
    fn fs_selftest_constdiv(device: c_int, c: f32, y: f32, lo: f32, hi: f32, mismatches: *mut u32) -> c_int;
    fn fs_constdiv_status(sim: *const fs_sim) -> c_int;
    fn fs_selftest_sort(device: c_int, pairs: *mut u64, n: u32, fuse_stage: c_int, plan: *mut u32) -> c_int;
    fn fs_selftest_sort_policy(log2_count: u32, start_back: c_int, lag: u32, required: *const u32, steps: usize,
                               stage_out: *mut u32, single_out: *mut u32) -> c_int;
    fn fs_sort_plan_read(sim: *mut fs_sim, out: *mut SortPlanInfo) -> c_int;
    // errors
    fn fs_last_error() -> *const c_char;
    fn fs_abi_version() -> c_int;
}

fn check(status: c_int) {
    if status != 0 {
        // the reference unwrap()s everywhere; keep the panic-on-error behaviour on the Rust side
        let msg = unsafe { CStr::from_ptr(fs_last_error()) }.to_string_lossy().into_owned();
        panic!("fluidsim status {status}: {msg}");
    }
}

pub fn abi_version() -> i32 { unsafe { fs_abi_version() } }

pub struct FluidSimulation { raw: *mut fs_sim, settings: SimulationSettings }

impl FluidSimulation {
    /// `FluidSimulation::new(&wgpu::Device, SimulationSettings)` — src/simulation.rs:139.
    pub fn new(hip_device: i32, settings: SimulationSettings) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe { fs_create(&settings, hip_device, &mut raw) });
        Self { raw, settings }
    }
    /// The same with the build-defined options (sort mode, math mode, lattice offset, capacity).
    pub fn with_options(settings: SimulationSettings, opts: Options) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe { fs_create_ex(&settings, &opts, &mut raw) });
        Self { raw, settings }
    }
    pub fn default_options() -> Options { let mut o = Options::default(); unsafe { fs_options_default(&mut o) }; o }
    /// `tick(&mut self, &Queue, &mut CommandEncoder, TickSettings)` — src/simulation.rs:459.  Enqueues; does not wait.
    pub fn tick(&mut self, settings: TickSettings) { check(unsafe { fs_step(self.raw, &settings) }); }
    /// `device.poll(Wait)` — src/main.rs:79.
    pub fn wait(&mut self) { check(unsafe { fs_sync(self.raw) }); }
    /// `pub tick: u32` — src/simulation.rs:12.
    pub fn tick_count(&self) -> u32 { unsafe { fs_tick_count(self.raw) } }
    pub fn particle_count(&self) -> u32 { unsafe { fs_particle_count(self.raw) } }
    pub fn settings(&self) -> SimulationSettings { self.settings }
    /// `grid_w`, `grid_h` — src/simulation.rs:140-141.
    pub fn grid_dims(&self) -> (u32, u32) {
        let (mut w, mut h) = (0u32, 0u32); check(unsafe { fs_grid_dims(self.raw, &mut w, &mut h) }); (w, h)
    }
    /// `simulation_settings_bg()` — src/simulation.rs:552-554: the uniform of the last tick, by value.
    pub fn simulation_uniform(&self) -> SimulationUniform {
        let mut u = SimulationUniform::default(); check(unsafe { fs_get_uniform(self.raw, &mut u) }); u
    }
    /// The uniform `tick` would build (src/simulation.rs:470-497) without stepping.
    pub fn build_uniform(settings: &SimulationSettings, tick: &TickSettings, tick_count: u32) -> SimulationUniform {
        let mut u = SimulationUniform::default(); check(unsafe { fs_build_uniform(settings, tick, tick_count, &mut u) }); u
    }
    /// `simulation_bg()` binding 0 — src/simulation.rs:556-559: device pointer to the cell-sorted 32-byte records.
    pub fn particles_device(&mut self) -> *const ParticleInstance {
        let mut p = std::ptr::null(); check(unsafe { fs_particles_device(self.raw, &mut p) }); p
    }
    /// `simulation_bg()` binding 1: `start_indices`.
    pub fn start_indices_device(&mut self) -> (*const u32, usize) {
        let (mut p, mut n) = (std::ptr::null(), 0usize);
        check(unsafe { fs_start_indices_device(self.raw, &mut p, &mut n) }); (p, n)
    }
    /// `force_field_texture()` + `queue.write_buffer` — src/simulation.rs:562, src/renderer.rs:497-502.
    pub fn write_force_field(&mut self, field: &[Vec2], w: u32, h: u32) {
        assert_eq!(field.len(), (w * h) as usize);
        check(unsafe { fs_upload_force_field(self.raw, field.as_ptr(), w, h) });
    }
    /// `generate_smooth_gradient_field` (src/main.rs:403-515) on the GPU, straight into the force field.
    pub fn set_obstacle_image(&mut self, image: &[u8], w: u32, h: u32) {
        assert_eq!(image.len(), (w * h) as usize);
        check(unsafe { fs_generate_force_field(self.raw, 0, image.as_ptr(), w, h, std::ptr::null_mut()) });
    }
    /// One-copy hand-off for a wgpu renderer: `queue.write_buffer(&particles, 0, cast_slice(&v))`.
    pub fn download_particles(&mut self) -> Vec<ParticleInstance> {
        let mut v = vec![ParticleInstance::default(); self.particle_count() as usize];
        check(unsafe { fs_download_particles(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn upload_particles(&mut self, src: &[ParticleInstance]) { check(unsafe { fs_upload_particles(self.raw, src.as_ptr(), src.len()) }); }
    /// Build extension, NOT in the reference: colour-field surface tension from the tick's surface_tension_* knobs
    /// (include/fluidsim.h), for the steps enqueued after this call.  Single-domain handles.
    pub fn set_surface_tension(&mut self, enable: bool) { check(unsafe { fs_set_surface_tension(self.raw, enable as c_int) }); }
    pub fn surface_tension_enabled(&self) -> bool { unsafe { fs_surface_tension_enabled(self.raw) != 0 } }
    /// The last step's surface-tension force per particle, in `download_particles` order.
    pub fn surface_tension_forces(&mut self) -> Vec<Vec2> {
        let mut v = vec![Vec2 { x: 0.0, y: 0.0 }; self.particle_count() as usize];
        check(unsafe { fs_download_surface_tension(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    /// Build extension, NOT in the reference: diffusion and buoyancy of the tracking channels (include/fluidsim.h).  Channel
    /// `channel` diffuses between neighbours with this conductivity (0: not at all) in the steps after the call.  Tracking must
    /// be on; `track` and `untrack` clear every conductivity and the buoyancy channel.
    pub fn set_diffusion(&mut self, channel: u32, conductivity: f32) { check(unsafe { fs_set_diffusion(self.raw, channel as c_int, conductivity) }); }
    pub fn diffusion(&self, channel: u32) -> f32 {
        let mut k = 0.0f32;
        check(unsafe { fs_get_diffusion(self.raw, channel as c_int, &mut k) }); k
    }
    /// The buoyancy channel: a particle with value a gains -beta (a - reference) gravity delta of velocity per step.
    pub fn set_buoyancy(&mut self, channel: u32, beta: f32, reference: f32) { check(unsafe { fs_set_buoyancy(self.raw, channel as c_int, beta, reference) }); }
    pub fn clear_buoyancy(&mut self) { check(unsafe { fs_set_buoyancy(self.raw, -1, 0.0, 0.0) }); }
    /// (channel, beta, reference) of the buoyancy channel, if one is set.
    pub fn buoyancy(&self) -> Option<(u32, f32, f32)> {
        let (mut c, mut b, mut r) = (0 as c_int, 0.0f32, 0.0f32);
        check(unsafe { fs_get_buoyancy(self.raw, &mut c, &mut b, &mut r) });
        if c < 0 { None } else { Some((c as u32, b, r)) }
    }
    /// What the last step with a buoyancy channel handed the force pass per particle, in `download_particles` order.
    pub fn buoyancy_forces(&mut self) -> Vec<Vec2> {
        let mut v = vec![Vec2 { x: 0.0, y: 0.0 }; self.particle_count() as usize];
        check(unsafe { fs_download_buoyancy(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    /// Build extension, NOT in the reference: particle tracking (include/fluidsim.h).  Every particle gets an id (its current
    /// slot) and `channels` f32 attributes (all 0.0) that follow it through the sort of every later step.  Single-domain handles.
    pub fn track(&mut self, channels: u32) { check(unsafe { fs_track_enable(self.raw, channels as c_int) }); }
    pub fn untrack(&mut self) { check(unsafe { fs_track_disable(self.raw) }); }
    /// `None` when tracking is off.
    pub fn track_channels(&self) -> Option<u32> {
        let c = unsafe { fs_track_channels(self.raw) };
        if c < 0 { None } else { Some(c as u32) }
    }
    /// The id of the particle in every slot, in `download_particles` order.
    pub fn particle_ids(&mut self) -> Vec<u32> {
        let mut v = vec![0u32; self.particle_count() as usize];
        check(unsafe { fs_track_download_ids(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn set_particle_ids(&mut self, ids: &[u32]) { check(unsafe { fs_track_upload_ids(self.raw, ids.as_ptr(), ids.len()) }); }
    pub fn attribute(&mut self, channel: u32) -> Vec<f32> {
        let mut v = vec![0f32; self.particle_count() as usize];
        check(unsafe { fs_track_download_attr(self.raw, channel as c_int, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn set_attribute(&mut self, channel: u32, values: &[f32]) {
        check(unsafe { fs_track_upload_attr(self.raw, channel as c_int, values.as_ptr(), values.len()) });
    }
    /// Device pointers to the arrays of the last enqueued step; valid until the next tick / upload / `track`.
    pub fn particle_ids_device(&mut self) -> *const u32 {
        let mut p: *const u32 = std::ptr::null();
        check(unsafe { fs_track_ids_device(self.raw, &mut p) }); p
    }
    pub fn attribute_device(&mut self, channel: u32) -> *const f32 {
        let mut p: *const f32 = std::ptr::null();
        check(unsafe { fs_track_attr_device(self.raw, channel as c_int, &mut p) }); p
    }
    /// `dst[id]` = the record of the particle with that id; entries of `dst` that no id names are left as they are.
    pub fn download_particles_by_id(&mut self, dst: &mut [ParticleInstance]) {
        check(unsafe { fs_download_particles_by_id(self.raw, dst.as_mut_ptr(), dst.len()) });
    }
    /// Build extension: 2D particle count (include/fluidsim.h).  `capacity` slots, of which `particle_count` are live.
    pub fn capacity(&self) -> u32 { unsafe { fs_capacity(self.raw) } }
    /// Room for `capacity` particles: grow-only, blocking, everything observable is preserved.  Refused on a handle with a
    /// renderer hand-off registered: size that one with `Options::capacity` at create.
    pub fn reserve(&mut self, capacity: u32) { check(unsafe { fs_reserve(self.raw, capacity) }); }
    /// Appends `src` behind the live particles, all fields as given; `particle_count + src.len() <= capacity`.
    pub fn emit(&mut self, src: &[ParticleInstance]) { check(unsafe { fs_emit_particles(self.raw, src.as_ptr(), src.len()) }); }
    /// Appends `nu * nv` particles generated on the device (`nv == 1`: a line, the usual 2D tap).
    pub fn emit_nozzle(&mut self, nozzle: &Nozzle) { check(unsafe { fs_emit_nozzle(self.raw, nozzle) }); }
    /// Removes every particle with `lo <= position <= hi` on both axes (blocking, stable); returns how many went.
    pub fn remove_box(&mut self, lo: Vec2, hi: Vec2) -> u32 { let mut n = 0u32; check(unsafe { fs_remove_in_box(self.raw, &lo, &hi, &mut n) }); n }
    /// Removes the particles whose flag (one per particle, download order) is non-zero (blocking, stable); returns how many went.
    pub fn remove(&mut self, flags: &[u8]) -> u32 { let mut n = 0u32; check(unsafe { fs_remove_flagged(self.raw, flags.as_ptr(), flags.len(), &mut n) }); n }
    /// The id the next emitted particle gets while tracking is on (0 when it is off).
    pub fn next_id(&self) -> u32 { unsafe { fs_track_next_id(self.raw) } }
    /// Build extension: 2D moving bodies (include/fluidsim.h).  `field`: `w * h` push vectors in world units over the body's own
    /// box `[-extent/2, extent/2]` in the body frame.  Returns the slot (the lowest free one of `0 .. MAX_BODIES`); blocking.  The
    /// body starts at the origin with the identity pose, at rest.
    pub fn add_body(&mut self, field: &[Vec2], w: u32, h: u32, extent: Vec2) -> u32 {
        assert_eq!(field.len(), (w as usize) * (h as usize));
        let mut slot = 0u32;
        check(unsafe { fs_body_create(self.raw, field.as_ptr(), w, h, extent, &mut slot) });
        slot
    }
    /// The body of a `w * h` mask (`> 128`: solid) over the box `extent`, by the exact distance transform of the 3D colliders.
    pub fn add_body_mask(&mut self, mask: &[u8], w: u32, h: u32, extent: Vec2) -> u32 {
        assert_eq!(mask.len(), (w as usize) * (h as usize));
        let mut slot = 0u32;
        check(unsafe { fs_body_create_from_mask(self.raw, mask.as_ptr(), w, h, extent, std::ptr::null_mut(), &mut slot) });
        slot
    }
    /// Pose and velocity for the ticks enqueued afterwards; host memory only.  The engine does not advance the pose.
    pub fn set_body_motion(&mut self, body: u32, motion: &BodyMotion) { check(unsafe { fs_body_set_motion(self.raw, body, motion) }); }
    pub fn body_motion(&self, body: u32) -> BodyMotion { let mut m = BodyMotion::default(); check(unsafe { fs_body_get_motion(self.raw, body, &mut m) }); m }
    /// `((w, h), extent)` of a body.
    pub fn body_dims(&self, body: u32) -> ((u32, u32), Vec2) {
        let (mut w, mut h, mut e) = (0u32, 0u32, Vec2::default());
        check(unsafe { fs_body_dims(self.raw, body, &mut w, &mut h, &mut e) });
        ((w, h), e)
    }
    /// A body's field, `w * h` vectors.  Blocking.
    pub fn body_field(&mut self, body: u32) -> Vec<Vec2> {
        let ((w, h), _) = self.body_dims(body);
        let mut v = vec![Vec2::default(); (w as usize) * (h as usize)];
        check(unsafe { fs_body_download(self.raw, body, v.as_mut_ptr(), v.len()) });
        v
    }
    /// Destroys a body and frees its slot; the other bodies keep theirs.  Blocking.
    pub fn remove_body(&mut self, body: u32) { check(unsafe { fs_body_destroy(self.raw, body) }); }
    pub fn body_count(&self) -> u32 { unsafe { fs_body_count(self.raw) } }
    /// Build extension: 2D body loads (include/fluidsim.h).  Turns the per-body sums of what the fluid hands each body on or off;
    /// enabling zeroes them.  The particles are the same bytes either way.
    pub fn enable_body_loads(&mut self, on: bool) { check(unsafe { fs_body_loads_enable(self.raw, on as c_int) }); }
    pub fn body_loads_enabled(&self) -> bool { unsafe { fs_body_loads_enabled(self.raw) != 0 } }
    /// A body's load words since they were last zeroed (blocking); `reset` zeroes them behind the read.
    pub fn body_loads(&mut self, body: u32, reset: bool) -> BodyLoad {
        let mut l = BodyLoad::default();
        check(unsafe { fs_body_loads(self.raw, body, &mut l, reset as c_int) });
        l
    }
    /// Device address of the `MAX_BODIES x 5` 64-bit words, by slot, for a consumer on the handle's stream.
    pub fn body_loads_device(&mut self) -> *const c_void {
        let mut p: *const c_void = std::ptr::null();
        check(unsafe { fs_body_loads_device(self.raw, &mut p) });
        p
    }
    /// Build extension: fluid diagnostics (include/fluidsim.h).  The record behind everything enqueued so far (blocking); the
    /// state is only read.
    pub fn stats(&mut self) -> Stats {
        let mut r = Stats::default();
        check(unsafe { fs_stats_read(self.raw, &mut r) });
        r
    }
    /// The same record to device memory at `out_dev` (8-byte aligned), stream-ordered and without a host read.
    pub fn stats_device(&mut self, out_dev: *mut Stats) { check(unsafe { fs_stats_device(self.raw, out_dev) }); }
    /// `start_indices` to the host (the renderer's second storage binding; u32[grid_w * grid_h]).
    pub fn download_start_indices(&mut self) -> Vec<u32> {
        let (w, h) = self.grid_dims();
        let mut v = vec![0u32; (w as usize) * (h as usize)];
        check(unsafe { fs_download_start_indices(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn upload_start_indices(&mut self, src: &[u32]) { check(unsafe { fs_upload_start_indices(self.raw, src.as_ptr(), src.len()) }); }
    /// Zero-copy hand-off: export the particle (or start_indices) allocation.  `dmabuf_fd` imports into Vulkan / wgpu
    /// as external memory (the buffers `simulation_bg` binds, src/simulation.rs:552-559); after this call the force
    /// pass writes the 32-byte records itself, so each frame costs no export pass and no PCIe copy.
    pub fn export(&mut self, which: c_int) -> MemHandle {
        let mut h = MemHandle { ipc: [0; 64], bytes: 0, device: 0, dmabuf_fd: -1 };
        check(unsafe { fs_export_handle(self.raw, which, &mut h) }); h
    }
    /// Headless `fluid_shader.wgsl:27-102`: width*height RGBA f32.  Needs a `tick` since create and since the last upload
    /// of particles or start indices (include/fluidsim.h).
    pub fn render_density(&mut self, view: &View) -> Vec<f32> {
        let mut v = vec![0f32; 4 * view.width as usize * view.height as usize];
        check(unsafe { fs_render_density(self.raw, view, v.as_mut_ptr()) }); v
    }
    /// Build extension, NOT in the reference: field sampling (include/fluidsim.h).  Density, Shepard weight, un-normalised
    /// velocity sum, neighbour count and cell of the fluid at `points`; with `attributes` also the channel sums, channel `c`
    /// of query `k` at `c * points.len() + k`.  Needs a tick since `new` / the last upload.  Coherently ordered points
    /// (sorted by cell, slot order) are sampled several times faster than shuffled ones.
    pub fn sample(&mut self, points: &[Vec2], attributes: bool) -> (Vec<Sample>, Vec<f32>) {
        let mut out = vec![Sample::default(); points.len()];
        let ch = if attributes { self.track_channels().unwrap_or(0) as usize } else { 0 };
        let mut attr = vec![0f32; ch * points.len()];
        let ap = if attributes { attr.as_mut_ptr() } else { std::ptr::null_mut() };
        check(unsafe { fs_sample_points(self.raw, points.as_ptr(), points.len(), out.as_mut_ptr(), ap) }); (out, attr)
    }
    /// `sample` at the pixel centres of `view` (`render_density`'s mapping), row-major; bit-identical to `sample` on those points.
    pub fn sample_grid(&mut self, view: &View, attributes: bool) -> (Vec<Sample>, Vec<f32>) {
        let n = view.width as usize * view.height as usize;
        let mut out = vec![Sample::default(); n];
        let ch = if attributes { self.track_channels().unwrap_or(0) as usize } else { 0 };
        let mut attr = vec![0f32; ch * n];
        let ap = if attributes { attr.as_mut_ptr() } else { std::ptr::null_mut() };
        check(unsafe { fs_sample_grid(self.raw, view, out.as_mut_ptr(), ap) }); (out, attr)
    }
    /// Device pointers on the simulation's device; enqueued on its stream after the ticks in flight, non-blocking.
    /// `attr_out_dev` may be null.  The buffers must stay valid until the stream has passed the call.
    pub unsafe fn sample_device(&mut self, points_dev: *const Vec2, n: usize, out_dev: *mut Sample, attr_out_dev: *mut f32) {
        check(fs_sample_points_device(self.raw, points_dev, n, out_dev, attr_out_dev));
    }
    pub fn profile(&mut self, enable: bool) { check(unsafe { fs_profile_enable(self.raw, enable as c_int) }); }
    pub fn profile_read(&mut self, reset: bool) -> ([f64; PASS_COUNT], u64) {
        let (mut ms, mut steps) = ([0f64; PASS_COUNT], 0u64);
        check(unsafe { fs_profile_read(self.raw, ms.as_mut_ptr(), &mut steps, reset as c_int) }); (ms, steps)
    }
    pub fn timed_steps(&mut self, settings: TickSettings, steps: u32) -> f64 {
        let mut ms = 0f64; check(unsafe { fs_timed_steps(self.raw, &settings, steps, &mut ms) }); ms
    }
    pub fn sort_plan(&mut self) -> SortPlanInfo { let mut i = SortPlanInfo::default(); check(unsafe { fs_sort_plan_read(self.raw, &mut i) }); i }
    pub fn constdiv_status(&self) -> i32 { unsafe { fs_constdiv_status(self.raw) } }
    pub fn stream(&self) -> *mut c_void { unsafe { fs_stream(self.raw) } }
    pub fn raw(&mut self) -> *mut fs_sim { self.raw }
}
impl Drop for FluidSimulation { fn drop(&mut self) { unsafe { fs_destroy(self.raw) } } }

/// The reference lattice (src/simulation.rs:147-163) and sort schedule (:323-347) without a device.
pub fn reference_lattice(settings: &SimulationSettings, offset: Vec2) -> Vec<ParticleInstance> {
    let mut v = vec![ParticleInstance::default(); settings.particle_count as usize];
    check(unsafe { fs_reference_lattice(settings, offset, v.as_mut_ptr(), v.len()) }); v
}
pub fn sort_schedule(particle_count: u32) -> Vec<SortStep> {
    let n = unsafe { fs_sort_schedule(particle_count, std::ptr::null_mut(), 0) };
    let mut v = vec![SortStep::default(); n];
    unsafe { fs_sort_schedule(particle_count, v.as_mut_ptr(), n) }; v
}

/// Consumer side of `FluidSimulation::export` in another HIP process.
pub struct Imported { ptr: *mut c_void }
impl Imported {
    pub fn open(handle: &MemHandle, hip_device: i32) -> Self { let mut p = std::ptr::null_mut(); check(unsafe { fs_import_open(handle, hip_device, &mut p) }); Self { ptr: p } }
    pub fn read(&self, offset: usize, dst: &mut [u8]) { check(unsafe { fs_import_read(self.ptr, offset, dst.as_mut_ptr() as *mut c_void, dst.len()) }); }
    pub fn device_ptr(&self) -> *mut c_void { self.ptr }
}
impl Drop for Imported { fn drop(&mut self) { unsafe { fs_import_close(self.ptr); } } }

/// `ResizableBuffer<T>` — src/buffer.rs:17-88, over HIP device memory.  The wgpu arguments
/// (`device`, `usage`, `belt`, `encoder`) have no counterpart: `hip_device` selects the GPU at
/// `new`, copies are ordered on the buffer's own stream.
pub struct ResizableBuffer<T: Copy> { raw: *mut fs_buffer, pub len: usize, marker: PhantomData<T> }
impl<T: Copy> ResizableBuffer<T> {
    /// src/buffer.rs:27-43
    pub fn new(name: &'static str, hip_device: i32, len: usize) -> Self {
        let cname = CString::new(name).unwrap();
        let mut raw = std::ptr::null_mut();
        check(unsafe { fs_buffer_create(hip_device, std::mem::size_of::<T>(), len, cname.as_ptr(), &mut raw) });
        Self { raw, len, marker: PhantomData }
    }
    /// src/buffer.rs:46-67: grow-only, keeps the contents, clamps to the device maximum (warning); false when `new_cap < len`.
    pub fn resize(&mut self, new_cap: usize) -> bool {
        let mut r: c_int = 0;
        check(unsafe { fs_buffer_resize(self.raw, new_cap, &mut r) });
        self.len = unsafe { fs_buffer_len(self.raw) };
        r != 0
    }
    /// src/buffer.rs:70-87: data longer than the buffer is trimmed (and logged).
    pub fn write(&self, offset: usize, data: &[T]) {
        check(unsafe { fs_buffer_write(self.raw, offset, data.as_ptr() as *const c_void, data.len()) });
    }
    pub fn read(&self, offset: usize, count: usize) -> Vec<T> {
        let mut v: Vec<T> = Vec::with_capacity(count);
        check(unsafe { fs_buffer_read(self.raw, offset, v.as_mut_ptr() as *mut c_void, count) });
        unsafe { v.set_len(count) }; v
    }
    /// `.buffer` (the wgpu::Buffer): here the device pointer.
    pub fn device_ptr(&self) -> *mut c_void { unsafe { fs_buffer_device_ptr(self.raw) } }
}
impl<T: Copy> Drop for ResizableBuffer<T> { fn drop(&mut self) { unsafe { fs_buffer_destroy(self.raw) } } }

/// `SSBO<T>` — src/buffer.rs:9-14,91-173: a `ResizableBuffer<T>` plus its binding.  HIP kernels take
/// pointers, so `bind_group()` is the device pointer and `layout()` the element size.
pub struct SSBO<T: Copy> { pub buffer: ResizableBuffer<T> }
impl<T: Copy> SSBO<T> {
    pub fn new(name: &'static str, hip_device: i32, data_len: usize) -> Self { Self { buffer: ResizableBuffer::new(name, hip_device, data_len) } }
    /// src/buffer.rs:129-152: no-op unless `new_cap > len`.
    pub fn resize(&mut self, new_cap: usize) { if new_cap > self.buffer.len { self.buffer.resize(new_cap); } }
    /// src/buffer.rs:155-157: `write(0, data)`.
    pub fn update(&self, data: &[T]) { self.write(0, data) }
    pub fn write(&self, offset: usize, data: &[T]) { self.buffer.write(offset, data) }
    pub fn bind_group(&self) -> *mut c_void { self.buffer.device_ptr() }
    pub fn layout(&self) -> usize { std::mem::size_of::<T>() }
    pub fn len(&self) -> usize { self.buffer.len }
}

/// One rank of the multi-GPU slab decomposition (fs_slab_*): pack -> Comm::exchange -> step.
pub struct SlabSimulation { raw: *mut fs_sim }
impl SlabSimulation {
    pub fn new(global: &SimulationSettings, hip_device: i32, cfg: &SlabConfig) -> Self {
        let mut raw = std::ptr::null_mut(); check(unsafe { fs_slab_create(global, hip_device, cfg, &mut raw) }); Self { raw }
    }
    pub fn upload_owned(&mut self, src: &[ParticleInstance]) { check(unsafe { fs_slab_upload_owned(self.raw, src.as_ptr(), src.len()) }); }
    pub fn set_window(&mut self, own_lo: u32, own_hi: u32) { check(unsafe { fs_slab_set_window(self.raw, own_lo, own_hi) }); }
    pub fn message_bytes(&self) -> usize { unsafe { fs_slab_message_bytes(self.raw) } }
    pub unsafe fn pack(&mut self, tick: &TickSettings, send_left: *mut c_void, send_right: *mut c_void) { check(fs_slab_pack(self.raw, tick, send_left, send_right)); }
    pub unsafe fn step(&mut self, recv_left: *const c_void, recv_right: *const c_void) { check(fs_slab_step(self.raw, recv_left, recv_right)); }
    /// Overlapped step (the default with the counting sort): `pack` also enqueues the interior columns' whole step, `step` the
    /// boundary strips; the exchange between them runs on `comm_stream()` (Comm::exchange does the hand-over itself).
    pub fn overlapped(&self) -> bool { unsafe { fs_slab_overlapped(self.raw) != 0 } }
    pub fn set_boundary_cols(&mut self, cols: u32) { check(unsafe { fs_slab_set_boundary_cols(self.raw, cols) }); }
    pub fn boundary_cols(&self) -> u32 { unsafe { fs_slab_boundary_cols(self.raw) } }
    pub fn comm_stream(&self) -> *mut c_void { unsafe { fs_slab_comm_stream(self.raw) } }
    pub fn comm_begin(&mut self) { check(unsafe { fs_slab_comm_begin(self.raw) }); }
    pub fn comm_end(&mut self) { check(unsafe { fs_slab_comm_end(self.raw) }); }
    pub fn wait_packed(&mut self) { check(unsafe { fs_slab_wait_packed(self.raw) }); }
    pub fn counters(&mut self) -> SlabCounters { let mut c = SlabCounters::default(); check(unsafe { fs_slab_counters_read(self.raw, &mut c) }); c }
    pub fn max_speed(&mut self) -> f32 { let mut v = 0f32; check(unsafe { fs_slab_max_speed(self.raw, &mut v) }); v }
    pub fn column_histogram(&mut self, hist: &mut [u32]) { check(unsafe { fs_slab_column_histogram(self.raw, hist.as_mut_ptr(), hist.len()) }); }
    /// Device-side re-balancing inputs for `Comm::allreduce`: `stats` = 4 u32 {lost, overflow, far_halo, max-speed bits}, `hist` = grid_w u32.
    pub unsafe fn rebalance_stats(&mut self, stats: *mut u32, hist: *mut u32, grid_w_global: usize) { check(fs_slab_rebalance_stats(self.raw, stats, hist, grid_w_global)); }
    pub fn download(&mut self, cap: usize) -> (Vec<ParticleInstance>, Vec<u8>) {
        let (mut rec, mut owned, mut n) = (vec![ParticleInstance::default(); cap], vec![0u8; cap], 0u32);
        check(unsafe { fs_slab_download(self.raw, rec.as_mut_ptr(), owned.as_mut_ptr(), cap, &mut n) });
        rec.truncate(n as usize); owned.truncate(n as usize); (rec, owned)
    }
    pub fn wait(&mut self) { check(unsafe { fs_sync(self.raw) }); }
    pub fn raw(&mut self) -> *mut fs_sim { self.raw }
}
impl Drop for SlabSimulation { fn drop(&mut self) { unsafe { fs_destroy(self.raw) } } }

/// One RCCL communicator per process / GPU (multi-GPU slab runs: fs_slab_pack -> Comm::exchange -> fs_slab_step).
pub struct Comm { raw: *mut fs_comm }
pub const COMM_U32: c_int = 0; pub const COMM_U64: c_int = 1; pub const COMM_F32: c_int = 2;
pub const COMM_SUM: c_int = 0; pub const COMM_MAX: c_int = 1;
impl Comm {
    pub fn unique_id() -> [u8; COMM_ID_BYTES] { let mut id = [0u8; COMM_ID_BYTES]; check(unsafe { fs_comm_unique_id(id.as_mut_ptr()) }); id }
    pub fn init(hip_device: i32, rank: i32, world: i32, id: &[u8; COMM_ID_BYTES]) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe { fs_comm_init(hip_device, rank, world, id.as_ptr(), &mut raw) }); Self { raw }
    }
    /// Grouped ncclSend/ncclRecv of the two fixed-size slab messages on the simulation's own stream.
    pub unsafe fn exchange(&self, sim: *mut fs_sim, left: i32, right: i32, send_left: *const c_void,
                           send_right: *const c_void, recv_left: *mut c_void, recv_right: *mut c_void) {
        check(fs_slab_exchange(sim, self.raw, left, right, send_left, send_right, recv_left, recv_right));
    }
    /// In-place all-reduce on the simulation's stream (re-balancing histogram / violation counters).
    pub unsafe fn allreduce(&self, sim: *mut fs_sim, device_buf: *mut c_void, count: usize, dtype: c_int, op: c_int) {
        check(fs_comm_allreduce(sim, self.raw, device_buf, count, dtype, op));
    }
}
impl Drop for Comm { fn drop(&mut self) { unsafe { fs_comm_destroy(self.raw) } } }

/// 3D extension (fs3_*; no reference counterpart).
pub struct FluidSimulation3D { raw: *mut fs_sim3 }
impl FluidSimulation3D {
    pub fn new(hip_device: i32, settings: Settings3, initial_offset: Vec3) -> Self {
        let mut raw = std::ptr::null_mut(); check(unsafe { fs3_create(&settings, hip_device, initial_offset, &mut raw) }); Self { raw }
    }
    pub fn with_math_mode(hip_device: i32, settings: Settings3, initial_offset: Vec3, math_mode: i32) -> Self {
        let mut raw = std::ptr::null_mut(); check(unsafe { fs3_create_ex(&settings, hip_device, initial_offset, math_mode, &mut raw) }); Self { raw }
    }
    pub fn tick(&mut self, t: TickSettings3) { check(unsafe { fs3_step(self.raw, &t) }); }
    pub fn wait(&mut self) { check(unsafe { fs3_sync(self.raw) }); }
    pub fn tick_count(&self) -> u32 { unsafe { fs3_tick_count(self.raw) } }
    pub fn particle_count(&self) -> u32 { unsafe { fs3_particle_count(self.raw) } }
    pub fn grid_dims(&self) -> (u32, u32, u32) { let (mut w, mut h, mut d) = (0, 0, 0); check(unsafe { fs3_grid_dims(self.raw, &mut w, &mut h, &mut d) }); (w, h, d) }
    pub fn download_particles(&mut self) -> Vec<Particle3> {
        let mut v = vec![Particle3::default(); self.particle_count() as usize];
        check(unsafe { fs3_download_particles(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn upload_particles(&mut self, src: &[Particle3]) { check(unsafe { fs3_upload_particles(self.raw, src.as_ptr(), src.len()) }); }
    pub fn reference_lattice(settings: &Settings3, offset: Vec3) -> Vec<Particle3> {
        let mut v = vec![Particle3::default(); settings.particle_count as usize];
        check(unsafe { fs3_reference_lattice(settings, offset, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn timed_steps(&mut self, t: TickSettings3, steps: u32) -> f64 { let mut ms = 0f64; check(unsafe { fs3_timed_steps(self.raw, &t, steps, &mut ms) }); ms }
    pub fn profile(&mut self, enable: bool) { check(unsafe { fs3_profile_enable(self.raw, enable as c_int) }); }
    pub fn profile_read(&mut self, reset: bool) -> ([f64; PASS_COUNT], u64) {
        let (mut ms, mut steps) = ([0f64; PASS_COUNT], 0u64);
        check(unsafe { fs3_profile_read(self.raw, ms.as_mut_ptr(), &mut steps, reset as c_int) }); (ms, steps)
    }
}
impl FluidSimulation3D {
    /// Build extension: 3D field sampling (include/fluidsim.h).  Density, Shepard weight, un-normalised velocity sum, density
    /// gradient (`-gradient` is the outward normal), neighbour count and cell of the fluid at `points`.  Needs a tick since
    /// `new` / the last upload.  Coherently ordered points are sampled several times faster than shuffled ones.
    pub fn sample(&mut self, points: &[Vec3]) -> Vec<Sample3> {
        let mut out = vec![Sample3::default(); points.len()];
        check(unsafe { fs3_sample_points(self.raw, points.as_ptr(), points.len(), out.as_mut_ptr()) }); out
    }
    /// `sample` at the voxel centres of `view`, voxel (i, j, k) at `(k * height + j) * width + i`; bit-identical to `sample` there.
    pub fn sample_grid(&mut self, view: &View3) -> Vec<Sample3> {
        let mut out = vec![Sample3::default(); view.width as usize * view.height as usize * view.depth as usize];
        check(unsafe { fs3_sample_grid(self.raw, view, out.as_mut_ptr()) }); out
    }
    /// Device pointers on the simulation's device; enqueued on its stream after the ticks in flight, non-blocking.
    /// The buffers must stay valid until the stream has passed the call.
    pub unsafe fn sample_device(&mut self, points_dev: *const Vec3, n: usize, out_dev: *mut Sample3) {
        check(fs3_sample_points_device(self.raw, points_dev, n, out_dev));
    }
    /// Build extension: 3D surface rendering (include/fluidsim.h).  Ray-marches the density's iso-surface into a G-buffer, pixel
    /// (i, j) at `j * width + i`.  Blocking; needs a tick since `new` / the last upload.
    pub fn render_surface(&mut self, camera: &Camera3, params: &SurfaceParams3) -> Vec<SurfaceHit3> {
        let mut out = vec![SurfaceHit3::default(); camera.width as usize * camera.height as usize];
        check(unsafe { fs3_render_surface(self.raw, camera, params, out.as_mut_ptr()) }); out
    }
    /// ... into a device buffer of `width * height` records; enqueued on the simulation's stream, non-blocking.
    pub unsafe fn render_surface_device(&mut self, camera: &Camera3, params: &SurfaceParams3, out_dev: *mut SurfaceHit3) {
        check(fs3_render_surface_device(self.raw, camera, params, out_dev));
    }
    /// Build extension: 3D surface extraction (include/fluidsim.h).  Surface nets over the `width` x `height` x `depth` lattice
    /// nodes of `view` (each >= 2): the vertices and the triangles (three indices each, outward winding) at exact size, in two
    /// calls: the counts, then the arrays.  Blocking; needs a tick since `new` / the last upload.
    pub fn extract_surface(&mut self, view: &View3, iso: f32) -> (Vec<MeshVertex3>, Vec<[u32; 3]>) {
        let mut counts = [0u32; 2];
        check(unsafe { fs3_extract_surface(self.raw, view, iso, std::ptr::null_mut(), 0, std::ptr::null_mut(), 0, counts.as_mut_ptr()) });
        let mut verts = vec![MeshVertex3::default(); counts[0] as usize];
        let mut tris = vec![[0u32; 3]; counts[1] as usize];
        if counts[0] != 0 || counts[1] != 0 {
            let vp = if verts.is_empty() { std::ptr::null_mut() } else { verts.as_mut_ptr() };
            let tp = if tris.is_empty() { std::ptr::null_mut() } else { tris.as_mut_ptr() as *mut u32 };
            check(unsafe { fs3_extract_surface(self.raw, view, iso, vp, counts[0], tp, counts[1], counts.as_mut_ptr()) });
        }
        (verts, tris)
    }
    /// ... into device buffers (`vert_cap` records, `3 * tri_cap` indices, two counts); enqueued on the simulation's stream, no
    /// host read.  The counts are always the full ones: compare them with the capacities once the stream has passed the call.
    pub unsafe fn extract_surface_device(&mut self, view: &View3, iso: f32, verts_dev: *mut MeshVertex3, vert_cap: u32, tris_dev: *mut u32, tri_cap: u32, counts_dev: *mut u32) {
        check(fs3_extract_surface_device(self.raw, view, iso, verts_dev, vert_cap, tris_dev, tri_cap, counts_dev));
    }
    /// Build extension: 3D colliders (include/fluidsim.h).  `field`: `w * h * d` push vectors in world units over the whole
    /// domain, voxel (i, j, k) at `(k * h + j) * w + i`, zero = free space.  Blocking; holds for the ticks enqueued afterwards.
    pub fn set_collider(&mut self, field: &[Vec3], w: u32, h: u32, d: u32) {
        assert_eq!(field.len(), w as usize * h as usize * d as usize);
        check(unsafe { fs3_collider_upload(self.raw, field.as_ptr(), w, h, d) });
    }
    /// ... from a voxel mask (> 128: solid): every solid voxel pushes to its nearest free voxel in index space.
    pub fn set_collider_mask(&mut self, mask: &[u8], w: u32, h: u32, d: u32) {
        assert_eq!(mask.len(), w as usize * h as usize * d as usize);
        check(unsafe { fs3_collider_from_mask(self.raw, mask.as_ptr(), w, h, d, std::ptr::null_mut()) });
    }
    pub fn clear_collider(&mut self) { check(unsafe { fs3_collider_clear(self.raw) }); }
    /// (w, h, d) of the collider, (0, 0, 0) when none is set.
    pub fn collider_dims(&self) -> (u32, u32, u32) { let (mut w, mut h, mut d) = (0, 0, 0); check(unsafe { fs3_collider_dims(self.raw, &mut w, &mut h, &mut d) }); (w, h, d) }
    /// The field in use; empty when none is set.
    pub fn collider(&mut self) -> Vec<Vec3> {
        let (w, h, d) = self.collider_dims();
        let mut v = vec![Vec3::default(); w as usize * h as usize * d as usize];
        if !v.is_empty() { check(unsafe { fs3_collider_download(self.raw, v.as_mut_ptr(), v.len()) }); }
        v
    }
    /// Build extension: 3D moving bodies (include/fluidsim.h).  `field`: `w * h * d` push vectors over the body's own box
    /// `[-extent/2, extent/2]` in the body frame, the layout of `set_collider`.  Returns the slot, the lowest free one of
    /// `0 .. MAX_BODIES3`.  Blocking.  The body starts at the origin with the identity pose, at rest.
    pub fn add_body(&mut self, field: &[Vec3], w: u32, h: u32, d: u32, extent: Vec3) -> u32 {
        assert_eq!(field.len(), w as usize * h as usize * d as usize);
        let mut slot = 0u32;
        check(unsafe { fs3_body_create(self.raw, field.as_ptr(), w, h, d, extent, &mut slot) });
        slot
    }
    /// ... from a voxel mask (> 128: solid) over the body's box: `set_collider_mask`'s producer.
    pub fn add_body_mask(&mut self, mask: &[u8], w: u32, h: u32, d: u32, extent: Vec3) -> u32 {
        assert_eq!(mask.len(), w as usize * h as usize * d as usize);
        let mut slot = 0u32;
        check(unsafe { fs3_body_create_from_mask(self.raw, mask.as_ptr(), w, h, d, extent, std::ptr::null_mut(), &mut slot) });
        slot
    }
    /// Pose and velocity of a body for the ticks enqueued afterwards; host memory only.  The engine does not advance the pose.
    pub fn set_body_motion(&mut self, body: u32, motion: &BodyMotion3) { check(unsafe { fs3_body_set_motion(self.raw, body, motion) }); }
    pub fn body_motion(&self, body: u32) -> BodyMotion3 { let mut m = BodyMotion3::default(); check(unsafe { fs3_body_get_motion(self.raw, body, &mut m) }); m }
    /// ((w, h, d), extent) of a body.
    pub fn body_dims(&self, body: u32) -> ((u32, u32, u32), Vec3) {
        let (mut w, mut h, mut d, mut e) = (0, 0, 0, Vec3::default());
        check(unsafe { fs3_body_dims(self.raw, body, &mut w, &mut h, &mut d, &mut e) });
        ((w, h, d), e)
    }
    /// A body's field.  Blocking.
    pub fn body_field(&mut self, body: u32) -> Vec<Vec3> {
        let ((w, h, d), _) = self.body_dims(body);
        let mut v = vec![Vec3::default(); w as usize * h as usize * d as usize];
        check(unsafe { fs3_body_download(self.raw, body, v.as_mut_ptr(), v.len()) });
        v
    }
    /// Destroys a body and frees its slot; the other bodies keep theirs.  Blocking.
    pub fn remove_body(&mut self, body: u32) { check(unsafe { fs3_body_destroy(self.raw, body) }); }
    pub fn body_count(&self) -> u32 { unsafe { fs3_body_count(self.raw) } }
    /// Build extension: 3D body loads (include/fluidsim.h).  Enabling zeroes every body's words; loads only observe.
    pub fn enable_body_loads(&mut self, on: bool) { check(unsafe { fs3_body_loads_enable(self.raw, on as c_int) }); }
    pub fn body_loads_enabled(&self) -> bool { unsafe { fs3_body_loads_enabled(self.raw) != 0 } }
    /// What the fluid handed `body` since its words were last zeroed.  Blocking; `reset` zeroes the slot behind the read.
    pub fn body_loads(&mut self, body: u32, reset: bool) -> Body3Load {
        let mut l = Body3Load::default();
        check(unsafe { fs3_body_loads(self.raw, body, &mut l, reset as c_int) });
        l
    }
    /// The device address of the 8 x 8 64-bit words, by slot, for a consumer on the handle's stream.
    pub fn body_loads_device(&mut self) -> *const c_void {
        let mut p: *const c_void = std::ptr::null();
        check(unsafe { fs3_body_loads_device(self.raw, &mut p) });
        p
    }
    /// Build extension: 3D fluid diagnostics (include/fluidsim.h).  Blocking; the state is only read.
    pub fn stats(&mut self) -> Stats3 {
        let mut r = Stats3::default();
        check(unsafe { fs3_stats_read(self.raw, &mut r) });
        r
    }
    /// The same record to device memory at `out_dev` (8-byte aligned), stream-ordered and without a host read.
    pub fn stats_device(&mut self, out_dev: *mut Stats3) { check(unsafe { fs3_stats_device(self.raw, out_dev) }); }
    /// Build extension: 3D surface tension (include/fluidsim.h), colour-field CSF with coefficient sigma and threshold tau,
    /// for the ticks enqueued afterwards.
    pub fn set_surface_tension(&mut self, coefficient: f32, threshold: f32) { check(unsafe { fs3_set_surface_tension(self.raw, 1, coefficient, threshold) }); }
    pub fn clear_surface_tension(&mut self) { check(unsafe { fs3_set_surface_tension(self.raw, 0, 0.0, 0.0) }); }
    pub fn surface_tension_enabled(&self) -> bool { unsafe { fs3_surface_tension_enabled(self.raw) != 0 } }
    /// (coefficient, threshold) in use, None when the feature is off.
    pub fn surface_tension_params(&self) -> Option<(f32, f32)> {
        if !self.surface_tension_enabled() { return None; }
        let (mut c, mut t) = (0.0f32, 0.0f32);
        check(unsafe { fs3_surface_tension_params(self.raw, &mut c, &mut t) }); Some((c, t))
    }
    /// The last step's surface-tension force per particle, in `download_particles` order.
    pub fn surface_tension_forces(&mut self) -> Vec<Vec3> {
        let mut v = vec![Vec3::default(); self.particle_count() as usize];
        check(unsafe { fs3_download_surface_tension(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    /// Build extension: 3D channel diffusion and buoyancy (include/fluidsim.h).  Channel `channel` diffuses between neighbours
    /// with this conductivity (0: not at all) in the steps after the call.  Tracking must be on; `track` and `untrack` clear
    /// every conductivity and the buoyancy channel.
    pub fn set_diffusion(&mut self, channel: u32, conductivity: f32) { check(unsafe { fs3_set_diffusion(self.raw, channel as c_int, conductivity) }); }
    pub fn diffusion(&self, channel: u32) -> f32 {
        let mut k = 0.0f32;
        check(unsafe { fs3_get_diffusion(self.raw, channel as c_int, &mut k) }); k
    }
    /// The buoyancy channel: a particle with value a gains -beta (a - reference) gravity delta of velocity per step.
    pub fn set_buoyancy(&mut self, channel: u32, beta: f32, reference: f32) { check(unsafe { fs3_set_buoyancy(self.raw, channel as c_int, beta, reference) }); }
    pub fn clear_buoyancy(&mut self) { check(unsafe { fs3_set_buoyancy(self.raw, -1, 0.0, 0.0) }); }
    /// (channel, beta, reference) of the buoyancy channel, if one is set.
    pub fn buoyancy(&self) -> Option<(u32, f32, f32)> {
        let (mut c, mut b, mut r) = (0 as c_int, 0.0f32, 0.0f32);
        check(unsafe { fs3_get_buoyancy(self.raw, &mut c, &mut b, &mut r) });
        if c < 0 { None } else { Some((c as u32, b, r)) }
    }
    /// What the last step with a buoyancy channel handed the force pass per particle, in `download_particles` order.
    pub fn buoyancy_forces(&mut self) -> Vec<Vec3> {
        let mut v = vec![Vec3::default(); self.particle_count() as usize];
        check(unsafe { fs3_download_buoyancy(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    /// Build extension: 3D particle count (include/fluidsim.h).  `capacity` slots, of which `particle_count` are live.
    pub fn capacity(&self) -> u32 { unsafe { fs3_capacity(self.raw) } }
    /// Room for `capacity` particles: grow-only, blocking, everything observable is preserved.
    pub fn reserve(&mut self, capacity: u32) { check(unsafe { fs3_reserve(self.raw, capacity) }); }
    /// Appends `src` behind the live particles, all fields as given; `particle_count + src.len() <= capacity`.
    pub fn emit(&mut self, src: &[Particle3]) { check(unsafe { fs3_emit_particles(self.raw, src.as_ptr(), src.len()) }); }
    /// Appends a layer of `nu * nv` particles generated on the device.
    pub fn emit_nozzle(&mut self, nozzle: &Nozzle3) { check(unsafe { fs3_emit_nozzle(self.raw, nozzle) }); }
    /// Removes every particle with `lo <= position <= hi` on every axis (blocking, stable); returns how many went.
    pub fn remove_box(&mut self, lo: Vec3, hi: Vec3) -> u32 { let mut n = 0u32; check(unsafe { fs3_remove_in_box(self.raw, &lo, &hi, &mut n) }); n }
    /// Removes the particles whose flag (one per particle, `download_particles` order) is non-zero; returns how many went.
    pub fn remove(&mut self, flags: &[u8]) -> u32 { let mut n = 0u32; check(unsafe { fs3_remove_flagged(self.raw, flags.as_ptr(), flags.len(), &mut n) }); n }
    /// The id the next emitted particle gets while tracking is on (0 when it is off).
    pub fn next_id(&self) -> u32 { unsafe { fs3_track_next_id(self.raw) } }
    /// Build extension: 3D particle tracking (include/fluidsim.h).  Every particle gets an id (its current slot) and `channels`
    /// f32 attributes (all 0.0) that follow it through the sort of every later step.
    pub fn track(&mut self, channels: u32) { check(unsafe { fs3_track_enable(self.raw, channels as c_int) }); }
    pub fn untrack(&mut self) { check(unsafe { fs3_track_disable(self.raw) }); }
    /// `None` when tracking is off.
    pub fn track_channels(&self) -> Option<u32> {
        let c = unsafe { fs3_track_channels(self.raw) };
        if c < 0 { None } else { Some(c as u32) }
    }
    /// The id of the particle in every slot, in `download_particles` order.
    pub fn particle_ids(&mut self) -> Vec<u32> {
        let mut v = vec![0u32; self.particle_count() as usize];
        check(unsafe { fs3_track_download_ids(self.raw, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn set_particle_ids(&mut self, ids: &[u32]) { check(unsafe { fs3_track_upload_ids(self.raw, ids.as_ptr(), ids.len()) }); }
    pub fn attribute(&mut self, channel: u32) -> Vec<f32> {
        let mut v = vec![0f32; self.particle_count() as usize];
        check(unsafe { fs3_track_download_attr(self.raw, channel as c_int, v.as_mut_ptr(), v.len()) }); v
    }
    pub fn set_attribute(&mut self, channel: u32, values: &[f32]) {
        check(unsafe { fs3_track_upload_attr(self.raw, channel as c_int, values.as_ptr(), values.len()) });
    }
    /// Device pointers to the arrays of the last enqueued step; valid until the next tick / upload / `track`.
    pub fn particle_ids_device(&mut self) -> *const u32 {
        let mut p: *const u32 = std::ptr::null();
        check(unsafe { fs3_track_ids_device(self.raw, &mut p) }); p
    }
    pub fn attribute_device(&mut self, channel: u32) -> *const f32 {
        let mut p: *const f32 = std::ptr::null();
        check(unsafe { fs3_track_attr_device(self.raw, channel as c_int, &mut p) }); p
    }
    /// `dst[id]` = the record of the particle with that id; entries of `dst` that no id names are left as they are.
    pub fn download_particles_by_id(&mut self, dst: &mut [Particle3]) {
        check(unsafe { fs3_download_particles_by_id(self.raw, dst.as_mut_ptr(), dst.len()) });
    }
    /// Build extension: 3D channel sampling (include/fluidsim.h).  (weights, sums): the Shepard denominators and the
    /// un-normalised SPH sums of the tracking channels at `points`, channel c of query q at `c * n + q`.  Needs
    /// `track(channels >= 1)` and a tick since the last upload.
    pub fn sample_attr(&mut self, points: &[Vec3]) -> (Vec<f32>, Vec<f32>) {
        let ch = self.track_channels().unwrap_or(0) as usize;
        let (mut w, mut a) = (vec![0f32; points.len()], vec![0f32; ch * points.len()]);
        check(unsafe { fs3_sample_attr_points(self.raw, points.as_ptr(), points.len(), w.as_mut_ptr(), a.as_mut_ptr()) }); (w, a)
    }
    /// `sample_attr` at the voxel centres of `view` (`sample_grid`'s order); bit-identical to `sample_attr` there.
    pub fn sample_attr_grid(&mut self, view: &View3) -> (Vec<f32>, Vec<f32>) {
        let n = view.width as usize * view.height as usize * view.depth as usize;
        let ch = self.track_channels().unwrap_or(0) as usize;
        let (mut w, mut a) = (vec![0f32; n], vec![0f32; ch * n]);
        check(unsafe { fs3_sample_attr_grid(self.raw, view, w.as_mut_ptr(), a.as_mut_ptr()) }); (w, a)
    }
    /// Device pointers on the simulation's device (`weight_out_dev` may be null); enqueued on its stream, non-blocking.
    pub unsafe fn sample_attr_device(&mut self, points_dev: *const Vec3, n: usize, weight_out_dev: *mut f32, attr_out_dev: *mut f32) {
        check(fs3_sample_attr_points_device(self.raw, points_dev, n, weight_out_dev, attr_out_dev));
    }
    pub fn stream(&self) -> *mut c_void { unsafe { fs3_stream(self.raw) } }
}
impl Drop for FluidSimulation3D { fn drop(&mut self) { unsafe { fs3_destroy(self.raw) } } }

/// Create-time proofs and the sort self-tests, for a Rust-side test suite.
pub mod selftest {
    use super::*;
    pub fn constdiv(hip_device: i32, c: f32, y: f32, lo: f32, hi: f32) -> u32 { let mut m = 0u32; check(unsafe { fs_selftest_constdiv(hip_device, c, y, lo, hi, &mut m) }); m }
    pub fn sort(hip_device: i32, pairs: &mut [u64], fuse_stage: i32) -> [u32; 2] {
        let mut plan = [0u32; 2];
        check(unsafe { fs_selftest_sort(hip_device, pairs.as_mut_ptr(), pairs.len() as u32, fuse_stage, plan.as_mut_ptr()) }); plan
    }
    pub fn sort_policy(log2_count: u32, start_back: i32, lag: u32, required: &[u32]) -> (Vec<u32>, Vec<u32>) {
        let (mut stage, mut single) = (vec![0u32; required.len()], vec![0u32; required.len()]);
        check(unsafe { fs_selftest_sort_policy(log2_count, start_back, lag, required.as_ptr(), required.len(), stage.as_mut_ptr(), single.as_mut_ptr()) });
        (stage, single)
    }
}

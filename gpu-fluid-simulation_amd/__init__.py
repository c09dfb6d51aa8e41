"""gpu-fluid-simulation_amd — MI355X-native SPH fluid-step engine (hot path of
rookieCookies/gpu-fluid-simulation) behind the C ABI in include/fluidsim.h.

This module is the thin Python host mirror used by tests and bench.py; it only
marshals arguments into libfluidsim_hip.so (hand-written HIP kernels).  There is
no CPU fallback: without the built extension (or without a GPU) calls raise.

Mirrors, by name and argument meaning:
  FluidSimulation.new / .tick / .tick_count   src/simulation.rs:139,459,12
  SimulationSettings / TickSettings           src/simulation.rs:95-122
  ResizableBuffer                             src/buffer.rs:17-88
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (  # noqa: F401
    FS_MATH_IEEE,
    FS_MATH_TOLERANCE,
    FS_MATH_WGSL_ULP,
    FS_SORT_BITONIC,
    FS_SORT_COUNTING,
    FS_SLAB_ROWMAJOR,
    FS_SLAB_SERIAL,
    FS_SLAB_STRIPS,
    MESH_VERTEX_DTYPE,
    PARTICLE3_DTYPE,
    PARTICLE_DTYPE,
    PASS_NAMES,
    SAMPLE3_DTYPE,
    SAMPLE_DTYPE,
    SURFACE_HIT_DTYPE,
    Camera3,
    ExtensionMissing,
    Nozzle3,
    Options,
    Settings,
    Settings3,
    SlabConfig,
    SurfaceParams3,
    SlabCounters,
    SortStep,
    TickSettings,
    TickSettings3,
    Uniform,
    UVec2,
    Vec2,
    Vec3,
    load_library,
)

__all__ = [
    "FluidSimulation", "ResizableBuffer", "SimulationSettings", "default_tick_settings", "dam_break_2d",
    "FluidSimError", "load_library", "PARTICLE_DTYPE", "SAMPLE_DTYPE", "SAMPLE3_DTYPE",
    "SURFACE_HIT_DTYPE", "look_at_camera", "shade_surface", "surface_hit_points", "MESH_VERTEX_DTYPE", "write_obj", "box_mask3d",
]


class FluidSimError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"fluidsim status {status}: {message}")
        self.status = status


def _check(lib, status):
    if status != _abi.FS_OK:
        raise FluidSimError(status, lib.fs_last_error().decode("utf-8", "replace"))


def SimulationSettings(particle_count=100_000, particle_spacing=0.1, smoothing_radius=0.2, size=(53.0, 53.0),
                       texture_size=(1024, 1024)):
    """Defaults: src/main.rs:48-54, src/renderer.rs:16."""
    return Settings(int(particle_count), float(particle_spacing), float(smoothing_radius),
                    Vec2(float(size[0]), float(size[1])), UVec2(int(texture_size[0]), int(texture_size[1])))


def default_tick_settings(**over):
    """Defaults: src/renderer.rs:374-388."""
    t = TickSettings(
        delta=np.float32(1.0) / np.float32(120.0), gravity=Vec2(0.0, 0.0), mass=1.0, pressure_constant=50.0,
        rest_density=0.0, damping_factor=0.1, viscosity_coefficient=25.0, surface_tension_treshold=0.1,
        surface_tension_coefficient=35.0, mouse_force_radius=5.0, mouse_force_power=150.0,
        mouse_pos=Vec2(0.0, 0.0), mouse_state=0)
    for k, v in over.items():
        if k in ("gravity", "mouse_pos"):
            v = Vec2(float(v[0]), float(v[1]))
        setattr(t, k, v)
    return t


def dam_break_2d(n):
    """The benchmark scene of SURVEY.md §8d: reference lattice + defaults, gravity on.

    Returns (settings, initial_offset, tick_settings).  All scene arithmetic in f32.
    """
    f = np.float32
    s, h = f(0.1), f(0.2)
    L = np.sqrt(f(n)) * s          # block side; exact for the square counts of the benchmark configs
    size = (f(2.0) * L, f(1.25) * L)
    off = (-size[0] / f(2) + L / f(2) + s / f(2), size[1] / f(2) - L / f(2) - s / f(2))
    settings = SimulationSettings(n, s, h, size, (1024, 1024))
    tick = default_tick_settings(gravity=(0.0, 9.81))
    return settings, (float(off[0]), float(off[1])), tick


def selftest_sort(keys, fuse_stage=-1, device=0):
    """The engine's sort (reference network, sort.wgsl:27-51) on bare u32 keys: (sorted_keys, perm, plan).

    plan = (calls that took the shifted late-stage merge, calls that took the per-stage plan); see
    csrc/kernels_sort_global.inc k_late_cert.  fuse_stage: -1 default plan, 0 per-stage only, k shifted merge from stage k.
    """
    lib = load_library()
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    pairs = (k.astype(np.uint64) << np.uint64(32)) | np.arange(k.shape[0], dtype=np.uint64)
    plan = (C.c_uint32 * 2)()
    _check(lib, lib.fs_selftest_sort(int(device), pairs.ctypes.data_as(C.c_void_p), k.shape[0], int(fuse_stage), plan))
    return (pairs >> np.uint64(32)).astype(np.uint32), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32), (plan[0], plan[1])


def selftest_sort_policy(required, log2_count=24, start_back=8, lag=4):
    """Replay the sort-plan policy (csrc/sort_policy.h) on the CPU against a per-step `required` stage; returns
    (stage chosen per step, single stand-by launch in the stream per step).  See fs_selftest_sort_policy."""
    lib = load_library()
    req = np.ascontiguousarray(required, dtype=np.uint32)
    stage = np.zeros(req.shape[0], dtype=np.uint32)
    single = np.zeros(req.shape[0], dtype=np.uint32)
    U = C.POINTER(C.c_uint32)
    _check(lib, lib.fs_selftest_sort_policy(int(log2_count), int(start_back), int(lag), req.ctypes.data_as(U), req.shape[0],
                                            stage.ctypes.data_as(U), single.ctypes.data_as(U)))
    return stage, single


class FluidSimulation:
    """FluidSimulation (src/simulation.rs:10-37) on one MI355X, driven through the C ABI."""

    def __init__(self, settings, device=0, sort_mode=FS_SORT_BITONIC, ref_quirks=True, initial_offset=(0.0, 0.0),
                 capacity=0, math_mode=FS_MATH_IEEE, surface_tension=False, track=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.settings = settings
        opts = Options()
        self._lib.fs_options_default(C.byref(opts))
        opts.device = int(device)
        opts.sort_mode = int(sort_mode)
        opts.ref_quirks = 1 if ref_quirks else 0
        opts.math_mode = int(math_mode)
        opts.initial_offset = Vec2(float(initial_offset[0]), float(initial_offset[1]))
        opts.capacity = int(capacity)
        _check(self._lib, self._lib.fs_create_ex(C.byref(settings), C.byref(opts), C.byref(self._h)))
        if surface_tension:
            self.set_surface_tension(True)
        if track is not None:
            self.track(track)

    @classmethod
    def new(cls, settings, device=0, **kw):
        return cls(settings, device=device, **kw)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.fs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- stepping -----------------------------------------------------------
    def tick(self, tick_settings):
        _check(self._lib, self._lib.fs_step(self._h, C.byref(tick_settings)))

    def sync(self):
        _check(self._lib, self._lib.fs_sync(self._h))

    @property
    def tick_count(self):
        return int(self._lib.fs_tick_count(self._h))

    @property
    def particle_count(self):
        return int(self._lib.fs_particle_count(self._h))

    @property
    def grid_dims(self):
        w, h = C.c_uint32(), C.c_uint32()
        _check(self._lib, self._lib.fs_grid_dims(self._h, C.byref(w), C.byref(h)))
        return int(w.value), int(h.value)

    @property
    def stream_ptr(self):
        """The HIP stream the steps (and sample_device) are enqueued on, as an integer (torch.cuda.ExternalStream)."""
        return self._lib.fs_stream(self._h)

    # -- surface tension (build extension, opt-in) ---------
    def set_surface_tension(self, enable=True):
        """Colour-field surface tension from the tick's surface_tension_coefficient / _treshold, for the steps after this call."""
        _check(self._lib, self._lib.fs_set_surface_tension(self._h, 1 if enable else 0))

    @property
    def surface_tension_enabled(self):
        return bool(self._lib.fs_surface_tension_enabled(self._h))

    def surface_tension_forces(self):
        """The last step's surface-tension force per particle, (N, 2) float32 in download_particles() order."""
        out = np.empty((self.particle_count, 2), dtype=np.float32)
        _check(self._lib, self._lib.fs_download_surface_tension(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    # -- particle tracking (build extension, opt-in) --------
    def track(self, channels=0):
        """Give every particle an id (= its current slot) and `channels` float attributes (all 0) that follow it through the
        sort of every later step.  Calling it again re-initialises."""
        _check(self._lib, self._lib.fs_track_enable(self._h, int(channels)))

    def untrack(self):
        _check(self._lib, self._lib.fs_track_disable(self._h))

    @property
    def track_channels(self):
        """-1 when tracking is off, else the number of attribute channels."""
        return int(self._lib.fs_track_channels(self._h))

    def particle_ids(self):
        """uint32 id of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.uint32)
        _check(self._lib, self._lib.fs_track_download_ids(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def set_particle_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        _check(self._lib, self._lib.fs_track_upload_ids(self._h, ids.ctypes.data_as(C.c_void_p), ids.shape[0]))

    def attribute(self, channel):
        """float32 attribute `channel` of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.float32)
        _check(self._lib, self._lib.fs_track_download_attr(self._h, int(channel), out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def set_attribute(self, channel, values):
        """`values` is copied bit for bit when it already is float32 (NaN payloads survive)."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        _check(self._lib, self._lib.fs_track_upload_attr(self._h, int(channel), values.ctypes.data_as(C.c_void_p), values.shape[0]))

    def download_particles_by_id(self):
        """The records in id order: out[id] is the particle with that id (ids >= particle_count are skipped; entries that no
        id names stay zero)."""
        out = np.zeros(self.particle_count, dtype=PARTICLE_DTYPE)
        _check(self._lib, self._lib.fs_download_particles_by_id(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def particle_ids_device_ptr(self):
        p = C.c_void_p()
        _check(self._lib, self._lib.fs_track_ids_device(self._h, C.byref(p)))
        return p.value

    def attribute_device_ptr(self, channel):
        p = C.c_void_p()
        _check(self._lib, self._lib.fs_track_attr_device(self._h, int(channel), C.byref(p)))
        return p.value

    def timed_steps(self, tick_settings, steps):
        ms = C.c_double()
        _check(self._lib, self._lib.fs_timed_steps(self._h, C.byref(tick_settings), int(steps), C.byref(ms)))
        return float(ms.value)

    def profile(self, enable=True):
        _check(self._lib, self._lib.fs_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, reset=True):
        ms = (C.c_double * len(PASS_NAMES))()
        steps = C.c_uint64()
        _check(self._lib, self._lib.fs_profile_read(self._h, ms, C.byref(steps), 1 if reset else 0))
        return dict(zip(PASS_NAMES, [float(x) for x in ms])), int(steps.value)

    def sort_plan(self):
        """Diagnostics of the sort's late-stage plan (fs_sort_plan_read): dict of counts since create.  Blocking."""
        info = _abi.SortPlanInfo()
        _check(self._lib, self._lib.fs_sort_plan_read(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _abi.SortPlanInfo._fields_}

    # -- data ---------------------------------------------------------------
    def uniform(self):
        u = Uniform()
        _check(self._lib, self._lib.fs_get_uniform(self._h, C.byref(u)))
        return u

    def download_particles(self):
        out = np.empty(self.particle_count, dtype=PARTICLE_DTYPE)
        _check(self._lib, self._lib.fs_download_particles(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def upload_particles(self, arr):
        arr = np.ascontiguousarray(arr, dtype=PARTICLE_DTYPE)
        _check(self._lib, self._lib.fs_upload_particles(self._h, arr.ctypes.data_as(C.c_void_p), arr.shape[0]))

    def download_start_indices(self):
        w, h = self.grid_dims
        out = np.empty(w * h, dtype=np.uint32)
        _check(self._lib, self._lib.fs_download_start_indices(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def upload_start_indices(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        _check(self._lib, self._lib.fs_upload_start_indices(self._h, arr.ctypes.data_as(C.c_void_p), arr.shape[0]))

    def upload_force_field(self, field):
        field = np.ascontiguousarray(field, dtype=np.float32)
        h, w = field.shape[0], field.shape[1]
        _check(self._lib, self._lib.fs_upload_force_field(self._h, field.ctypes.data_as(C.c_void_p), w, h))

    def set_obstacle_image(self, image, want_field=False):
        """Obstacle mask (u8 [h, w], > 128 = obstacle) -> push-out field written into the simulation
        (generate_smooth_gradient_field + the renderer's write_buffer: src/main.rs:403-515, renderer.rs:497-502)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        out = np.empty((h, w, 2), dtype=np.float32) if want_field else None
        _check(self._lib, self._lib.fs_generate_force_field(self._h, 0, image.ctypes.data_as(C.c_void_p), w, h,
                                                            out.ctypes.data_as(C.c_void_p) if want_field else None))
        return out

    def render_density(self, width, height, world_min=None, world_max=None):
        """Headless density-splat image (fluid_shader.wgsl:27-102): float32 [height, width, 4] RGBA.
        Default view = the reference camera: the whole domain, +y down (src/renderer.rs:558-561)."""
        sx, sy = self.settings.size.x, self.settings.size.y
        wmin = world_min if world_min is not None else (-sx / 2, -sy / 2)
        wmax = world_max if world_max is not None else (sx / 2, sy / 2)
        view = _abi.View(Vec2(float(wmin[0]), float(wmin[1])), Vec2(float(wmax[0]), float(wmax[1])), int(width), int(height))
        out = np.empty((int(height), int(width), 4), dtype=np.float32)
        _check(self._lib, self._lib.fs_render_density(self._h, C.byref(view), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- field sampling (build extension) ---------------------
    def _sample_attr(self, attributes, n):
        if not attributes:
            return None
        ch = self.track_channels
        if ch <= 0:
            raise FluidSimError(_abi.FS_ERR_INVALID, "sample(attributes=True) needs track(channels >= 1)")
        return np.empty((ch, n), dtype=np.float32)

    def sample(self, points, attributes=False, normalise=False):
        """Density, Shepard weight, velocity sum, neighbour count and cell of the fluid at `points` ((n, 2) float32, any
        place): a SAMPLE_DTYPE array, and with attributes=True also the (channels, n) float32 channel sums.  The sums are the
        un-normalised SPH interpolants (include/fluidsim.h); normalise=True divides velocity and channels by `weight` where it
        is non-zero.  Needs a step since create / the last upload.  Points in a coherent order (sorted by cell, a grid, slot
        order) are sampled several times faster than shuffled ones."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.zeros(n, dtype=SAMPLE_DTYPE)
        attr = self._sample_attr(attributes, n)
        _check(self._lib, self._lib.fs_sample_points(self._h, pts.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                                                     attr.ctypes.data_as(C.c_void_p) if attr is not None else None))
        if normalise:
            _normalise_samples(out, attr)
        return (out, attr) if attributes else out

    def sample_grid(self, width, height, world_min=None, world_max=None, attributes=False):
        """sample() at the pixel centres of render_density()'s view (same defaults): a [height, width] SAMPLE_DTYPE array, and
        with attributes=True also the (channels, height, width) float32 channel sums.  Bit-identical to sample() on those points."""
        sx, sy = self.settings.size.x, self.settings.size.y
        wmin = world_min if world_min is not None else (-sx / 2, -sy / 2)
        wmax = world_max if world_max is not None else (sx / 2, sy / 2)
        width, height = int(width), int(height)
        view = _abi.View(Vec2(float(wmin[0]), float(wmin[1])), Vec2(float(wmax[0]), float(wmax[1])), width, height)
        out = np.zeros((height, width), dtype=SAMPLE_DTYPE)
        attr = self._sample_attr(attributes, width * height)
        _check(self._lib, self._lib.fs_sample_grid(self._h, C.byref(view), out.ctypes.data_as(C.c_void_p),
                                                   attr.ctypes.data_as(C.c_void_p) if attr is not None else None))
        return (out, attr.reshape(-1, height, width)) if attributes else out

    def sample_device(self, points_ptr, n, out_ptr, attr_ptr=None):
        """fs_sample_points_device: device pointers (n fs_vec2 in, n 24-byte fs_sample out, channels * n floats out), enqueued
        on the simulation's stream after the steps in flight; non-blocking."""
        _check(self._lib, self._lib.fs_sample_points_device(self._h, C.c_void_p(points_ptr), int(n), C.c_void_p(out_ptr),
                                                            C.c_void_p(attr_ptr) if attr_ptr else None))

    def export_handle(self, which=_abi.FS_EXPORT_PARTICLES):
        """fs_export_handle: interprocess handle of the AoS particle view (switches on the live view) or of start_indices."""
        h = _abi.MemHandle()
        _check(self._lib, self._lib.fs_export_handle(self._h, int(which), C.byref(h)))
        return h

    def particles_device_ptr(self):
        p = C.c_void_p()
        _check(self._lib, self._lib.fs_particles_device(self._h, C.byref(p)))
        return p.value

    def start_indices_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(self._lib, self._lib.fs_start_indices_device(self._h, C.byref(p), C.byref(n)))
        return p.value, int(n.value)


def _normalise_samples(out, attr):
    """Shepard normalisation in place: velocity and channel sums divided by the weight, where that is non-zero."""
    w = out["weight"]
    ok = w != 0
    out["velocity"][ok] /= w[ok, None]
    if attr is not None:
        attr[:, ok] /= w[ok]


def dam_break_3d(n):
    """3D benchmark scene (SURVEY.md §8d `dam_break_3d`; build-defined, no reference counterpart):
    side^3 cube lattice, s = 0.1, h = 0.2, box (2L, 1.25L, L + 2s), block one spacing off the -x wall
    and the +y floor, centred in z; reference tick defaults with gravity (0, 9.81, 0)."""
    f = np.float32
    side = int(round(n ** (1.0 / 3.0)))
    if side ** 3 != n:
        raise ValueError("dam_break_3d expects a cube particle count")
    s, h = f(0.1), f(0.2)
    L = f(side) * s
    size = (f(2.0) * L, f(1.25) * L, L + f(2.0) * s)
    off = (-size[0] / f(2) + L / f(2) + s / f(2), size[1] / f(2) - L / f(2) - s / f(2), f(0.0))
    st = Settings3(int(n), float(s), float(h), Vec3(float(size[0]), float(size[1]), float(size[2])))
    tick = TickSettings3(float(f(1.0) / f(120.0)), Vec3(0.0, 9.81, 0.0), 1.0, 50.0, 0.0, 0.1, 25.0)
    return st, (float(off[0]), float(off[1]), float(off[2])), tick


class FluidSimulation3D:
    """3D extension (include/fluidsim.h fs3_*); not in the reference."""

    def __init__(self, settings, device=0, initial_offset=(0.0, 0.0, 0.0), math_mode=FS_MATH_IEEE, track=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.settings = settings
        off = Vec3(*[float(x) for x in initial_offset])
        _check(self._lib, self._lib.fs3_create_ex(C.byref(settings), int(device), off, int(math_mode), C.byref(self._h)))
        if track is not None:
            self.track(track)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.fs3_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tick(self, t):
        _check(self._lib, self._lib.fs3_step(self._h, C.byref(t)))

    def sync(self):
        _check(self._lib, self._lib.fs3_sync(self._h))

    @property
    def tick_count(self):
        return int(self._lib.fs3_tick_count(self._h))

    @property
    def particle_count(self):
        return int(self._lib.fs3_particle_count(self._h))

    @property
    def grid_dims(self):
        w, h, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self._lib, self._lib.fs3_grid_dims(self._h, C.byref(w), C.byref(h), C.byref(d)))
        return int(w.value), int(h.value), int(d.value)

    def download_particles(self):
        out = np.empty(self.particle_count, dtype=PARTICLE3_DTYPE)
        _check(self._lib, self._lib.fs3_download_particles(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def upload_particles(self, arr):
        arr = np.ascontiguousarray(arr, dtype=PARTICLE3_DTYPE)
        _check(self._lib, self._lib.fs3_upload_particles(self._h, arr.ctypes.data_as(C.c_void_p), arr.shape[0]))

    def timed_steps(self, t, steps):
        ms = C.c_double()
        _check(self._lib, self._lib.fs3_timed_steps(self._h, C.byref(t), int(steps), C.byref(ms)))
        return float(ms.value)

    def profile(self, enable=True):
        _check(self._lib, self._lib.fs3_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, reset=True):
        ms = (C.c_double * len(PASS_NAMES))()
        steps = C.c_uint64()
        _check(self._lib, self._lib.fs3_profile_read(self._h, ms, C.byref(steps), 1 if reset else 0))
        return dict(zip(PASS_NAMES, [float(x) for x in ms])), int(steps.value)

    @property
    def stream_ptr(self):
        """hipStream_t of the simulation as an integer (torch.cuda.ExternalStream / RCCL on the same stream)."""
        return int(self._lib.fs3_stream(self._h) or 0)

    # -- 3D surface tension (build extension) -----------------
    def set_surface_tension(self, coefficient, threshold=0.0):
        """Colour-field surface tension (include/fluidsim.h "3D surface tension") for the steps enqueued after this call:
        force -coefficient * laplace(c) * n / |n| where the colour gradient |n| exceeds `threshold`."""
        _check(self._lib, self._lib.fs3_set_surface_tension(self._h, 1, float(coefficient), float(threshold)))

    def clear_surface_tension(self):
        """Back to the plain step, for the steps enqueued after this call."""
        _check(self._lib, self._lib.fs3_set_surface_tension(self._h, 0, 0.0, 0.0))

    @property
    def surface_tension_enabled(self):
        return bool(self._lib.fs3_surface_tension_enabled(self._h))

    @property
    def surface_tension_params(self):
        """(coefficient, threshold) in use, or None when the feature is off."""
        if not self.surface_tension_enabled:
            return None
        c, t = C.c_float(), C.c_float()
        _check(self._lib, self._lib.fs3_surface_tension_params(self._h, C.byref(c), C.byref(t)))
        return float(c.value), float(t.value)

    def surface_tension_forces(self):
        """The last step's surface-tension force per particle, (N, 3) float32 in download_particles() order."""
        out = np.empty((self.particle_count, 3), dtype=np.float32)
        _check(self._lib, self._lib.fs3_download_surface_tension(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    # -- 3D particle tracking (build extension, opt-in) -------
    def track(self, channels=0):
        """Give every particle an id (= its current slot) and `channels` float attributes (all 0) that follow it through the
        sort of every later step.  Calling it again re-initialises."""
        _check(self._lib, self._lib.fs3_track_enable(self._h, int(channels)))

    def untrack(self):
        _check(self._lib, self._lib.fs3_track_disable(self._h))

    @property
    def track_channels(self):
        """-1 when tracking is off, else the number of attribute channels."""
        return int(self._lib.fs3_track_channels(self._h))

    def particle_ids(self):
        """uint32 id of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.uint32)
        _check(self._lib, self._lib.fs3_track_download_ids(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def set_particle_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        _check(self._lib, self._lib.fs3_track_upload_ids(self._h, ids.ctypes.data_as(C.c_void_p), ids.shape[0]))

    def attribute(self, channel):
        """float32 attribute `channel` of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.float32)
        _check(self._lib, self._lib.fs3_track_download_attr(self._h, int(channel), out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def set_attribute(self, channel, values):
        """`values` is copied bit for bit when it already is float32 (NaN payloads survive)."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        _check(self._lib, self._lib.fs3_track_upload_attr(self._h, int(channel), values.ctypes.data_as(C.c_void_p), values.shape[0]))

    def download_particles_by_id(self):
        """The records in id order: out[id] is the particle with that id (ids >= particle_count are skipped; entries that no
        id names stay zero)."""
        out = np.zeros(self.particle_count, dtype=PARTICLE3_DTYPE)
        _check(self._lib, self._lib.fs3_download_particles_by_id(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    def particle_ids_device_ptr(self):
        p = C.c_void_p()
        _check(self._lib, self._lib.fs3_track_ids_device(self._h, C.byref(p)))
        return p.value

    def attribute_device_ptr(self, channel):
        p = C.c_void_p()
        _check(self._lib, self._lib.fs3_track_attr_device(self._h, int(channel), C.byref(p)))
        return p.value

    # -- 3D particle count (build extension) ------------------
    @property
    def capacity(self):
        """Slots of the handle: particle_count can grow to this (reserve() raises it)."""
        return int(self._lib.fs3_capacity(self._h))

    def reserve(self, capacity):
        """Room for `capacity` particles (grow-only, blocking); the state and everything observable are preserved."""
        _check(self._lib, self._lib.fs3_reserve(self._h, int(capacity)))

    def emit(self, records):
        """Append PARTICLE3_DTYPE records behind the live particles, all fields as given; particle_count + len <= capacity."""
        arr = np.ascontiguousarray(records, dtype=PARTICLE3_DTYPE)
        _check(self._lib, self._lib.fs3_emit_particles(self._h, arr.ctypes.data_as(C.c_void_p), arr.shape[0]))

    def emit_nozzle(self, origin, u, v, velocity, nu, nv):
        """Append a layer of nu x nv particles generated on the device: centred on `origin`, spaced by the vectors u and v,
        all with `velocity` (include/fluidsim.h "3D particle count")."""
        vec = lambda a: Vec3(float(a[0]), float(a[1]), float(a[2]))
        z = Nozzle3(vec(origin), vec(u), vec(v), vec(velocity), int(nu), int(nv))
        _check(self._lib, self._lib.fs3_emit_nozzle(self._h, C.byref(z)))

    def remove_box(self, lo, hi):
        """Remove every particle with lo <= position <= hi on every axis (blocking, stable); returns how many went."""
        a, b, n = Vec3(*[float(x) for x in lo]), Vec3(*[float(x) for x in hi]), C.c_uint32()
        _check(self._lib, self._lib.fs3_remove_in_box(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return int(n.value)

    def remove(self, flags):
        """Remove the particles whose entry of `flags` (one per particle, download_particles() order) is non-zero (blocking,
        stable); returns how many went."""
        f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
        n = C.c_uint32()
        _check(self._lib, self._lib.fs3_remove_flagged(self._h, f.ctypes.data_as(C.c_void_p), f.shape[0], C.byref(n)))
        return int(n.value)

    @property
    def next_id(self):
        """The id the next emitted particle gets while tracking is on (0 when it is off)."""
        return int(self._lib.fs3_track_next_id(self._h))

    # -- 3D field sampling (build extension; DESIGN.md §14, the channels: §20) ----
    def _sample_attr(self, n):
        ch = self.track_channels
        if ch <= 0:
            raise FluidSimError(_abi.FS_ERR_INVALID, "sample(attributes=True) needs track(channels >= 1)")
        return np.zeros((ch, n), dtype=np.float32)

    def sample(self, points, attributes=False, normalise=False):
        """Density, Shepard weight, velocity sum, density gradient, neighbour count and cell of the fluid at `points`
        ((n, 3) float32, any place): a SAMPLE3_DTYPE array, and with attributes=True also the (channels, n) float32 sums of
        the tracking channels.  Velocity and channels are the un-normalised SPH interpolants (include/fluidsim.h);
        normalise=True divides them by `weight` where that is non-zero.  -gradient is the outward normal of an iso-surface.
        Needs a step since create / the last upload.  Points in a coherent order (sorted by cell, a grid, slot order) are
        sampled several times faster than shuffled ones."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        out = np.zeros(n, dtype=SAMPLE3_DTYPE)
        attr = self._sample_attr(n) if attributes else None
        _check(self._lib, self._lib.fs3_sample_points(self._h, pts.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
        if attributes:
            _check(self._lib, self._lib.fs3_sample_attr_points(self._h, pts.ctypes.data_as(C.c_void_p), n, None,
                                                               attr.ctypes.data_as(C.c_void_p)))
        if normalise:
            _normalise_samples(out, attr)
        return (out, attr) if attributes else out

    def sample_grid(self, width, height, depth=1, world_min=None, world_max=None, attributes=False):
        """sample() at the voxel centres of a box (default: the whole domain): a [depth, height, width] SAMPLE3_DTYPE array,
        and with attributes=True also the (channels, depth, height, width) float32 channel sums; bit-identical to sample() on
        those points.  A slice is depth == 1 with world_min[2] == world_max[2]."""
        view = self._view3(width, height, depth, world_min, world_max)
        width, height, depth = int(width), int(height), int(depth)
        out = np.zeros((depth, height, width), dtype=SAMPLE3_DTYPE)
        attr = self._sample_attr(width * height * depth) if attributes else None
        _check(self._lib, self._lib.fs3_sample_grid(self._h, C.byref(view), out.ctypes.data_as(C.c_void_p)))
        if attributes:
            _check(self._lib, self._lib.fs3_sample_attr_grid(self._h, C.byref(view), None, attr.ctypes.data_as(C.c_void_p)))
        return (out, attr.reshape(-1, depth, height, width)) if attributes else out

    def sample_device(self, points_ptr, n, out_ptr):
        """fs3_sample_points_device: device pointers (n fs_vec3 in, n 40-byte fs3_sample out), enqueued on the simulation's
        stream after the steps in flight; non-blocking."""
        _check(self._lib, self._lib.fs3_sample_points_device(self._h, C.c_void_p(points_ptr), int(n), C.c_void_p(out_ptr)))

    def sample_attr(self, points, weights=False):
        """The channel sums alone at `points`: (channels, n) float32, with weights=True (weight[n], sums)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        attr = self._sample_attr(n)
        w = np.zeros(n, dtype=np.float32) if weights else None
        _check(self._lib, self._lib.fs3_sample_attr_points(self._h, pts.ctypes.data_as(C.c_void_p), n,
                                                           w.ctypes.data_as(C.c_void_p) if weights else None,
                                                           attr.ctypes.data_as(C.c_void_p)))
        return (w, attr) if weights else attr

    def sample_attr_device(self, points_ptr, n, weight_ptr, attr_ptr):
        """fs3_sample_attr_points_device: device pointers (n fs_vec3 in, n floats out or 0 / None, channels * n floats out),
        enqueued on the simulation's stream after the steps in flight; non-blocking."""
        _check(self._lib, self._lib.fs3_sample_attr_points_device(self._h, C.c_void_p(points_ptr), int(n),
                                                                  C.c_void_p(weight_ptr) if weight_ptr else None,
                                                                  C.c_void_p(attr_ptr) if attr_ptr else None))

    # -- 3D surface rendering (build extension) ---------------
    def render_surface(self, camera, params, out=None):
        """Ray-march the iso-surface of the density into a G-buffer: a [height, width] SURFACE_HIT_DTYPE array (ray parameter,
        density, outward normal, Shepard velocity, march index, hit kind) for a Camera3 (look_at_camera) and SurfaceParams3.
        Blocking; needs a step since create / the last upload.  `out`: a device pointer (int) instead: fs3_render_surface_device,
        enqueued on the simulation's stream after the steps in flight, non-blocking, returns None."""
        if out is not None:
            _check(self._lib, self._lib.fs3_render_surface_device(self._h, C.byref(camera), C.byref(params), C.c_void_p(int(out))))
            return None
        hits = np.zeros((int(camera.height), int(camera.width)), dtype=SURFACE_HIT_DTYPE)
        _check(self._lib, self._lib.fs3_render_surface(self._h, C.byref(camera), C.byref(params), hits.ctypes.data_as(C.c_void_p)))
        return hits

    # -- 3D surface extraction (build extension) --------------
    def _view3(self, width, height, depth, world_min, world_max):
        sz = self.settings.size
        wmin = world_min if world_min is not None else (-sz.x / 2, -sz.y / 2, -sz.z / 2)
        wmax = world_max if world_max is not None else (sz.x / 2, sz.y / 2, sz.z / 2)
        return _abi.View3(Vec3(*[float(v) for v in wmin]), Vec3(*[float(v) for v in wmax]), int(width), int(height), int(depth))

    def extract_surface(self, width, height, depth, iso, world_min=None, world_max=None):
        """The iso-surface of the density as an indexed triangle mesh (surface nets over width x height x depth lattice NODES,
        the voxel centres of sample_grid on the same box; default: the whole domain): (vertices[V] MESH_VERTEX_DTYPE,
        triangles[T, 3] uint32), outward winding, open where the surface leaves the box.  Blocking; needs a step since create /
        the last upload.  Two ABI calls at most: the counts, then the arrays at exact size."""
        view = self._view3(width, height, depth, world_min, world_max)
        counts = (C.c_uint32 * 2)()
        _check(self._lib, self._lib.fs3_extract_surface(self._h, C.byref(view), float(iso), None, 0, None, 0, counts))
        verts = np.zeros(int(counts[0]), dtype=MESH_VERTEX_DTYPE)
        tris = np.zeros((int(counts[1]), 3), dtype=np.uint32)
        if verts.shape[0] or tris.shape[0]:
            _check(self._lib, self._lib.fs3_extract_surface(
                self._h, C.byref(view), float(iso), verts.ctypes.data_as(C.c_void_p) if verts.shape[0] else None, verts.shape[0],
                tris.ctypes.data_as(C.c_void_p) if tris.shape[0] else None, tris.shape[0], counts))
            assert (int(counts[0]), int(counts[1])) == (verts.shape[0], tris.shape[0])
        return verts, tris

    def extract_surface_device(self, width, height, depth, iso, verts_ptr, vert_cap, tris_ptr, tri_cap, counts_ptr,
                               world_min=None, world_max=None):
        """fs3_extract_surface_device: device pointers (vert_cap 40-byte fs3_mesh_vertex, 3 * tri_cap uint32, 2 uint32 counts),
        enqueued on the simulation's stream after the steps in flight; no host read.  The counts are always the full ones:
        compare them with the capacities once the stream has passed the call."""
        view = self._view3(width, height, depth, world_min, world_max)
        _check(self._lib, self._lib.fs3_extract_surface_device(
            self._h, C.byref(view), float(iso), C.c_void_p(int(verts_ptr)) if verts_ptr else None, int(vert_cap),
            C.c_void_p(int(tris_ptr)) if tris_ptr else None, int(tri_cap), C.c_void_p(int(counts_ptr)) if counts_ptr else None))

    # -- 3D colliders (build extension) -----------------------
    def set_collider(self, field):
        """Static obstacles: a float32 [D, H, W, 3] voxel field of push vectors in world units over the whole domain, zero = free
        space (include/fluidsim.h "3D colliders").  Blocking; holds for the steps enqueued afterwards; replaces an earlier one."""
        f = np.ascontiguousarray(field, dtype=np.float32)
        if f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("set_collider expects a [D, H, W, 3] float32 array")
        d, h, w = f.shape[:3]
        _check(self._lib, self._lib.fs3_collider_upload(self._h, f.ctypes.data_as(C.c_void_p), int(w), int(h), int(d)))

    def set_collider_mask(self, mask, want_field=False):
        """The collider of a uint8 [D, H, W] voxel mask (> 128: solid): every solid voxel pushes to its nearest free voxel (exact
        distance transform in index space, made on the GPU).  want_field=True returns the [D, H, W, 3] field."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != 3:
            raise ValueError("set_collider_mask expects a [D, H, W] uint8 array")
        d, h, w = m.shape
        out = np.zeros((d, h, w, 3), dtype=np.float32) if want_field else None
        _check(self._lib, self._lib.fs3_collider_from_mask(self._h, m.ctypes.data_as(C.c_void_p), int(w), int(h), int(d),
                                                          out.ctypes.data_as(C.c_void_p) if want_field else None))
        return out

    def clear_collider(self):
        _check(self._lib, self._lib.fs3_collider_clear(self._h))

    @property
    def collider_dims(self):
        """(W, H, D) of the collider, (0, 0, 0) when none is set."""
        w, h, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self._lib, self._lib.fs3_collider_dims(self._h, C.byref(w), C.byref(h), C.byref(d)))
        return int(w.value), int(h.value), int(d.value)

    def collider(self):
        """The collider in use as a float32 [D, H, W, 3] array, or None when none is set."""
        w, h, d = self.collider_dims
        if w == 0:
            return None
        out = np.zeros((d, h, w, 3), dtype=np.float32)
        _check(self._lib, self._lib.fs3_collider_download(self._h, out.ctypes.data_as(C.c_void_p), w * h * d))
        return out


def box_mask3d(size, shape, world_min, world_max):
    """A box given in world coordinates rasterised to a collider mask for FluidSimulation3D.set_collider_mask: uint8 [D, H, W] for
    shape = (W, H, D) over the domain [-size/2, size/2], 255 where the voxel's centre lies inside the box, else 0."""
    axes = []
    for a, n in enumerate(shape):
        c = (np.arange(int(n)) + 0.5) / int(n) * float(size[a]) - float(size[a]) / 2
        axes.append((c >= float(world_min[a])) & (c <= float(world_max[a])))
    inside = axes[2][:, None, None] & axes[1][None, :, None] & axes[0][None, None, :]
    return np.where(inside, 255, 0).astype(np.uint8)


def write_obj(path, vertices, triangles):
    """A mesh of extract_surface as a Wavefront OBJ: one `v` and one `vn` line per vertex, one `f a//a b//b c//c` line per
    triangle, indices 1-based.  Floats are written with nine significant digits (float32 round-trips)."""
    with open(path, "w") as fh:
        for p in vertices["position"]:
            fh.write("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]))
        for n in vertices["normal"]:
            fh.write("vn %.9g %.9g %.9g\n" % (n[0], n[1], n[2]))
        for t in np.asarray(triangles, dtype=np.int64).reshape(-1, 3) + 1:
            fh.write("f %d//%d %d//%d %d//%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2]))


def look_at_camera(eye, target, up, fov_y_or_extent, width, height, orthographic=False):
    """A Camera3 at `eye` looking at `target`.  Perspective: `fov_y_or_extent` is the vertical field of view in radians;
    orthographic: the world height of the image.  `right` and `up` of the record span the whole image (width / height gives the
    aspect), so pixel row 0 is the image's BOTTOM edge along `up`: flip the rows for a top-down image file."""
    e, t, u = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fwd = t - e
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, u)
    right = right / np.linalg.norm(right)
    upv = np.cross(right, fwd)
    span_y = float(fov_y_or_extent) if orthographic else 2.0 * np.tan(0.5 * float(fov_y_or_extent))
    span_x = span_y * float(width) / float(height)
    vec = lambda a: Vec3(*[float(np.float32(x)) for x in a])      # noqa: E731
    return Camera3(vec(e), vec(fwd), vec(right * span_x), vec(upv * span_y), int(width), int(height), 1 if orthographic else 0, 0)


def surface_hit_points(camera, hits):
    """World positions of a render_surface G-buffer's hits, float32 of the hits' shape + (3,), from the camera and the records' `t`
    (include/fluidsim.h: x(t) = o + t * d; numpy, for shading only).  Pixels without a hit get the ray origin."""
    v3 = lambda a: np.float32([a.x, a.y, a.z])      # noqa: E731
    h, w = hits.shape
    u = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w) - np.float32(0.5))[None, :, None]
    v = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h) - np.float32(0.5))[:, None, None]
    span = u * v3(camera.right) + v * v3(camera.up)
    if camera.orthographic:
        o, d = v3(camera.eye) + span, np.broadcast_to(v3(camera.forward), (h, w, 3))
    else:
        o, d = np.broadcast_to(v3(camera.eye), (h, w, 3)), v3(camera.forward) + span
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True))
    return (o + hits["t"][..., None] * d).astype(np.float32)


def shade_surface(hits, light=(0.4, -0.8, -0.45), max_speed=None):
    """Lambert shading of a render_surface G-buffer (numpy only): straight-alpha RGBA float32 of the hits' shape, for write_png.
    `light` points from the surface towards the light.  Water blue, tinted towards white by speed (relative to `max_speed`,
    default: the fastest hit); a hit whose first sample was already inside the fluid (hit == 2) is drawn flat and darker."""
    l = np.asarray(light, dtype=np.float32)
    l = l / np.linalg.norm(l)
    lambert = np.clip((hits["normal"] * l).sum(axis=-1), 0.0, 1.0)
    speed = np.sqrt((hits["velocity"].astype(np.float32) ** 2).sum(axis=-1))
    top = float(max_speed) if max_speed else float(speed.max())
    tint = np.clip(speed / top, 0.0, 1.0)[..., None] if top > 0 else np.zeros(hits.shape + (1,), dtype=np.float32)
    base = np.float32([0.10, 0.35, 0.85]) * (1.0 - tint) + np.float32([0.95, 0.97, 1.0]) * tint
    shade = np.where(hits["hit"] == 2, 0.35, 0.25 + 0.75 * lambert)[..., None]
    rgba = np.zeros(hits.shape + (4,), dtype=np.float32)
    rgba[..., 3] = (hits["hit"] != 0).astype(np.float32)
    rgba[..., :3] = base * shade * rgba[..., 3:4]
    return rgba


def reference_lattice_3d(settings, offset=(0.0, 0.0, 0.0)):
    lib = load_library()
    out = np.zeros(settings.particle_count, dtype=PARTICLE3_DTYPE)
    _check(lib, lib.fs3_reference_lattice(C.byref(settings), Vec3(*[float(x) for x in offset]),
                                          out.ctypes.data_as(C.c_void_p), out.shape[0]))
    return out


class SlabSimulation:
    """One rank of the multi-GPU slab decomposition (include/fluidsim.h fs_slab_*).

    Owns the global cell columns [own_lo, own_hi).  A step is pack() -> exchange the two
    messages with the slab neighbours -> step(); see multi.py for the driver.
    """

    def __init__(self, settings, own_lo, own_hi, has_left, has_right, capacity, recv_capacity, max_cols, device=0,
                 sort_mode=None, serial=False, strips=False, rowmajor=False):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.settings = settings
        mode = (0 if sort_mode is None else 1 + int(sort_mode)) | (FS_SLAB_SERIAL if serial else 0) | (FS_SLAB_STRIPS if strips else 0)
        mode |= FS_SLAB_ROWMAJOR if rowmajor else 0        # row-major cell ids even where a slab edge has a neighbour
        self.cfg = SlabConfig(int(own_lo), int(own_hi), int(bool(has_left)), int(bool(has_right)), int(capacity),
                              int(recv_capacity), int(max_cols), mode)
        _check(self._lib, self._lib.fs_slab_create(C.byref(settings), int(device), C.byref(self.cfg), C.byref(self._h)))
        self.capacity = int(capacity)
        self.device_index = int(device)
        self.message_bytes = int(self._lib.fs_slab_message_bytes(self._h))
        # 0 serial step; 1 edge-first (default): step() advances the edge columns, builds the NEXT step's messages and only
        # then advances the interior — the exchange runs beside that on comm_stream_ptr; 2 strips: pack() also enqueues the
        # interior columns' whole step, step() the boundary strips (include/fluidsim.h)
        self.step_mode = int(self._lib.fs_slab_overlapped(self._h))
        self.overlapped = self.step_mode != 0

    def set_boundary_cols(self, cols):
        _check(self._lib, self._lib.fs_slab_set_boundary_cols(self._h, int(cols)))

    @property
    def boundary_cols(self):
        return int(self._lib.fs_slab_boundary_cols(self._h))

    @property
    def comm_stream_ptr(self):
        return self._lib.fs_slab_comm_stream(self._h)

    def comm_begin(self):
        _check(self._lib, self._lib.fs_slab_comm_begin(self._h))

    def comm_end(self):
        _check(self._lib, self._lib.fs_slab_comm_end(self._h))

    def wait_packed(self):
        """Block the host until the outgoing messages of the current pack() are complete."""
        _check(self._lib, self._lib.fs_slab_wait_packed(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.fs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_owned(self, arr):
        arr = np.ascontiguousarray(arr, dtype=PARTICLE_DTYPE)
        _check(self._lib, self._lib.fs_slab_upload_owned(self._h, arr.ctypes.data_as(C.c_void_p), arr.shape[0]))

    def upload_force_field(self, field):
        """As FluidSimulation.upload_force_field: f32 [texture_size.y, texture_size.x, 2]."""
        field = np.ascontiguousarray(field, dtype=np.float32)
        h, w = field.shape[0], field.shape[1]
        _check(self._lib, self._lib.fs_upload_force_field(self._h, field.ctypes.data_as(C.c_void_p), w, h))

    def set_window(self, own_lo, own_hi):
        _check(self._lib, self._lib.fs_slab_set_window(self._h, int(own_lo), int(own_hi)))
        self.cfg.own_lo, self.cfg.own_hi = int(own_lo), int(own_hi)

    def pack(self, tick_settings, send_left_ptr, send_right_ptr):
        _check(self._lib, self._lib.fs_slab_pack(self._h, C.byref(tick_settings), send_left_ptr, send_right_ptr))

    def step(self, recv_left_ptr, recv_right_ptr):
        _check(self._lib, self._lib.fs_slab_step(self._h, recv_left_ptr, recv_right_ptr))

    def sync(self):
        _check(self._lib, self._lib.fs_sync(self._h))

    @property
    def stream_ptr(self):
        return self._lib.fs_stream(self._h)

    @property
    def tick_count(self):
        return int(self._lib.fs_tick_count(self._h))

    def counters(self):
        c = SlabCounters()
        _check(self._lib, self._lib.fs_slab_counters_read(self._h, C.byref(c)))
        return {"n_live": c.n_live, "lost": c.lost, "overflow": c.overflow, "far_halo": c.far_halo}

    def download(self):
        """(records with GLOBAL cell keys, owned mask) of the live slots."""
        out = np.empty(self.capacity, dtype=PARTICLE_DTYPE)
        owned = np.zeros(self.capacity, dtype=np.uint8)
        n = C.c_uint32()
        _check(self._lib, self._lib.fs_slab_download(self._h, out.ctypes.data_as(C.c_void_p),
                                                     owned.ctypes.data_as(C.c_void_p), self.capacity, C.byref(n)))
        return out[: n.value], owned[: n.value].astype(bool)

    def column_histogram(self, grid_w_global):
        h = np.zeros(int(grid_w_global), dtype=np.uint32)
        _check(self._lib, self._lib.fs_slab_column_histogram(self._h, h.ctypes.data_as(C.c_void_p), h.shape[0]))
        return h

    def max_speed(self):
        v = C.c_float()
        _check(self._lib, self._lib.fs_slab_max_speed(self._h, C.byref(v)))
        return float(v.value)

    def rebalance_stats(self, stats_dev_ptr, hist_dev_ptr, grid_w_global):
        """Enqueue the re-balancing inputs into two DEVICE buffers (4 x u32 stats, grid_w x u32 histogram); no read-back."""
        _check(self._lib, self._lib.fs_slab_rebalance_stats(self._h, stats_dev_ptr, hist_dev_ptr, int(grid_w_global)))

    def profile(self, enable=True):
        _check(self._lib, self._lib.fs_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, reset=True):
        ms = (C.c_double * len(PASS_NAMES))()
        steps = C.c_uint64()
        _check(self._lib, self._lib.fs_profile_read(self._h, ms, C.byref(steps), 1 if reset else 0))
        return dict(zip(PASS_NAMES, [float(x) for x in ms])), int(steps.value)


class ResizableBuffer:
    """ResizableBuffer<T> (src/buffer.rs:17-88) over HIP device memory."""

    def __init__(self, name, dtype, length, device=0):
        self._lib = load_library()
        self.dtype = np.dtype(dtype)
        self._h = C.c_void_p()
        st = self._lib.fs_buffer_create(int(device), self.dtype.itemsize, int(length), name.encode(), C.byref(self._h))
        _check(self._lib, st)

    def __len__(self):
        return int(self._lib.fs_buffer_len(self._h))

    def resize(self, new_cap):
        r = C.c_int()
        _check(self._lib, self._lib.fs_buffer_resize(self._h, int(new_cap), C.byref(r)))
        return bool(r.value)

    def write(self, offset, data):
        data = np.ascontiguousarray(data, dtype=self.dtype)
        _check(self._lib, self._lib.fs_buffer_write(self._h, int(offset), data.ctypes.data_as(C.c_void_p), data.shape[0]))

    def read(self, offset=0, count=None):
        count = len(self) - offset if count is None else count
        out = np.zeros(max(count, 0), dtype=self.dtype)
        _check(self._lib, self._lib.fs_buffer_read(self._h, int(offset), out.ctypes.data_as(C.c_void_p), out.shape[0]))
        return out

    @property
    def device_ptr(self):
        return self._lib.fs_buffer_device_ptr(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.fs_buffer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImportedBuffer:
    """Consumer side of fs_export_handle in another process: maps the exported device range (fs_import_open)."""

    def __init__(self, handle_bytes, device=0):
        self._lib = load_library()
        self.handle = _abi.MemHandle.from_buffer_copy(handle_bytes)
        self._p = C.c_void_p()
        _check(self._lib, self._lib.fs_import_open(C.byref(self.handle), int(device), C.byref(self._p)))

    def read(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        count = int(self.handle.bytes // dtype.itemsize) if count is None else int(count)
        out = np.empty(count, dtype=dtype)
        _check(self._lib, self._lib.fs_import_read(self._p, int(offset), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def close(self):
        if self._p.value:
            _check(self._lib, self._lib.fs_import_close(self._p))
            self._p = C.c_void_p()


def generate_force_field(image, device=0):
    """Standalone generate_smooth_gradient_field (src/main.rs:403-515) on the GPU: u8 [h, w] -> f32 [h, w, 2]."""
    lib = load_library()
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = image.shape
    out = np.empty((h, w, 2), dtype=np.float32)
    _check(lib, lib.fs_generate_force_field(None, int(device), image.ctypes.data_as(C.c_void_p), w, h,
                                            out.ctypes.data_as(C.c_void_p)))
    return out


def write_png(path, rgba, background=(0.0, 0.0, 0.0)):
    """Minimal PNG writer (zlib only): composites straight-alpha RGBA f32 over `background`, 8-bit RGB."""
    import struct
    import zlib
    a = np.clip(rgba[..., 3:4], 0.0, 1.0)
    rgb = np.clip(rgba[..., :3], 0.0, 1.0) * a + np.asarray(background, dtype=np.float32) * (1.0 - a)
    img = (np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def reference_lattice(settings, offset=(0.0, 0.0)):
    lib = load_library()
    out = np.zeros(settings.particle_count, dtype=PARTICLE_DTYPE)
    _check(lib, lib.fs_reference_lattice(C.byref(settings), Vec2(float(offset[0]), float(offset[1])),
                                         out.ctypes.data_as(C.c_void_p), out.shape[0]))
    return out


def sort_schedule(particle_count):
    lib = load_library()
    n = lib.fs_sort_schedule(int(particle_count), None, 0)
    arr = (SortStep * max(n, 1))()
    lib.fs_sort_schedule(int(particle_count), arr, n)
    return [(a.group_width, a.group_height, a.step_index, a.num_values) for a in arr[:n]]


def build_uniform(settings, tick_settings, tick_count):
    lib = load_library()
    u = Uniform()
    _check(lib, lib.fs_build_uniform(C.byref(settings), C.byref(tick_settings), int(tick_count), C.byref(u)))
    return u

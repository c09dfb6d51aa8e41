"""The 2D simulation (include/fluidsim.h fs_*): its handle, its settings and scenes, and the stateless 2D calls."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (FS_MATH_IEEE, FS_SORT_BITONIC, PARTICLE_DTYPE, SAMPLE_DTYPE, BodyLoad, BodyMotion, Nozzle, Options, Settings, SortStep, TickSettings,
                   Uniform, UVec2, Vec2, load_library)
from ._handle import _Bodies, _check, _Count, _Diffusion, _normalise_samples, _ptr, _Simulation, _Stats, _SurfaceTension, _Tracking, _vec2
from .stats import Stats


def SimulationSettings(particle_count=100_000, particle_spacing=0.1, smoothing_radius=0.2, size=(53.0, 53.0),
                       texture_size=(1024, 1024)):
    """Defaults: src/main.rs:48-54, src/renderer.rs:16."""
    return Settings(int(particle_count), float(particle_spacing), float(smoothing_radius),
                    _vec2(size), UVec2(int(texture_size[0]), int(texture_size[1])))


def default_tick_settings(**over):
    """Defaults: src/renderer.rs:374-388."""
    t = TickSettings(
        delta=np.float32(1.0) / np.float32(120.0), gravity=Vec2(0.0, 0.0), mass=1.0, pressure_constant=50.0,
        rest_density=0.0, damping_factor=0.1, viscosity_coefficient=25.0, surface_tension_treshold=0.1,
        surface_tension_coefficient=35.0, mouse_force_radius=5.0, mouse_force_power=150.0,
        mouse_pos=Vec2(0.0, 0.0), mouse_state=0)
    for k, v in over.items():
        if k in ("gravity", "mouse_pos"):
            v = _vec2(v)
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


class FluidSimulation(_Count, _Tracking, _SurfaceTension, _Diffusion, _Bodies, _Stats, _Simulation):
    """FluidSimulation (src/simulation.rs:10-37) on one MI355X, driven through the C ABI."""
    _prefix = "fs_"
    _destroy = "fs_destroy"
    _record = PARTICLE_DTYPE
    _dim = 2
    _nozzle = Nozzle         # the particle count that changes at run time: _Count
    _stats = Stats           # the fluid diagnostics: _Stats

    def __init__(self, settings, device=0, sort_mode=FS_SORT_BITONIC, ref_quirks=True, initial_offset=(0.0, 0.0),
                 capacity=0, math_mode=FS_MATH_IEEE, surface_tension=False, track=None):
        super().__init__()
        self.settings = settings
        opts = Options()
        self._lib.fs_options_default(C.byref(opts))
        opts.device = int(device)
        opts.sort_mode = int(sort_mode)
        opts.ref_quirks = 1 if ref_quirks else 0
        opts.math_mode = int(math_mode)
        opts.initial_offset = _vec2(initial_offset)
        opts.capacity = int(capacity)
        _check(self._lib, self._lib.fs_create_ex(C.byref(settings), C.byref(opts), C.byref(self._h)))
        if surface_tension:
            self.set_surface_tension(True)
        if track is not None:
            self.track(track)

    @classmethod
    def new(cls, settings, device=0, **kw):
        return cls(settings, device=device, **kw)

    @property
    def grid_dims(self):
        w, h = C.c_uint32(), C.c_uint32()
        self._call("grid_dims", C.byref(w), C.byref(h))
        return int(w.value), int(h.value)

    # -- surface tension (build extension, opt-in) ---------
    def set_surface_tension(self, enable=True):
        """Colour-field surface tension from the tick's surface_tension_coefficient / _treshold, for the steps after this call."""
        self._call("set_surface_tension", 1 if enable else 0)

    # -- channel diffusion and buoyancy (build extension, opt-in): _Diffusion, and the limit ---------
    @staticmethod
    def diffusion_limit(settings, tick, rest_density):
        """rho0 h^2 / (16 delta): the largest conductivity at which the explicit update of a uniform fluid at density rho0 is a
        convex combination of the neighbours' values.  The engine does not enforce it."""
        h = float(settings.smoothing_radius)
        return float(rest_density) * h * h / (16.0 * float(tick.delta))

    def sort_plan(self):
        """Diagnostics of the sort's late-stage plan (fs_sort_plan_read): dict of counts since create.  Blocking."""
        info = _abi.SortPlanInfo()
        self._call("sort_plan_read", C.byref(info))
        return {k: int(getattr(info, k)) for k, _ in _abi.SortPlanInfo._fields_}

    # -- data ---------------------------------------------------------------
    def uniform(self):
        u = Uniform()
        self._call("get_uniform", C.byref(u))
        return u

    def download_start_indices(self):
        w, h = self.grid_dims
        out = np.empty(w * h, dtype=np.uint32)
        self._call("download_start_indices", _ptr(out), out.shape[0])
        return out

    def upload_start_indices(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        self._call("upload_start_indices", _ptr(arr), arr.shape[0])

    def upload_force_field(self, field):
        field = np.ascontiguousarray(field, dtype=np.float32)
        h, w = field.shape[0], field.shape[1]
        self._call("upload_force_field", _ptr(field), w, h)

    def set_obstacle_image(self, image, want_field=False):
        """Obstacle mask (u8 [h, w], > 128 = obstacle) -> push-out field written into the simulation
        (generate_smooth_gradient_field + the renderer's write_buffer: src/main.rs:403-515, renderer.rs:497-502)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        out = np.empty((h, w, 2), dtype=np.float32) if want_field else None
        self._call("generate_force_field", 0, _ptr(image), w, h, _ptr(out) if want_field else None)
        return out

    def _view(self, width, height, world_min, world_max):
        """The view of render_density and sample_grid; default = the reference camera: the whole domain."""
        sx, sy = self.settings.size.x, self.settings.size.y
        wmin = world_min if world_min is not None else (-sx / 2, -sy / 2)
        wmax = world_max if world_max is not None else (sx / 2, sy / 2)
        return _abi.View(_vec2(wmin), _vec2(wmax), int(width), int(height))

    def render_density(self, width, height, world_min=None, world_max=None):
        """Headless density-splat image (fluid_shader.wgsl:27-102): float32 [height, width, 4] RGBA.
        Default view = the reference camera: the whole domain, +y down (src/renderer.rs:558-561)."""
        view = self._view(width, height, world_min, world_max)
        out = np.empty((int(height), int(width), 4), dtype=np.float32)
        self._call("render_density", C.byref(view), _ptr(out))
        return out

    # -- field sampling (build extension) ---------------------
    def sample(self, points, attributes=False, normalise=False):
        """Density, Shepard weight, velocity sum, neighbour count and cell of the fluid at `points` ((n, 2) float32, any
        place): a SAMPLE_DTYPE array, and with attributes=True also the (channels, n) float32 channel sums.  The sums are the
        un-normalised SPH interpolants (include/fluidsim.h); normalise=True divides velocity and channels by `weight` where it
        is non-zero.  Needs a step since create / the last upload.  Points in a coherent order (sorted by cell, a grid, slot
        order) are sampled several times faster than shuffled ones."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.zeros(n, dtype=SAMPLE_DTYPE)
        attr = self._sample_attr(n) if attributes else None
        self._call("sample_points", _ptr(pts), n, _ptr(out), _ptr(attr) if attributes else None)
        if normalise:
            _normalise_samples(out, attr)
        return (out, attr) if attributes else out

    def sample_grid(self, width, height, world_min=None, world_max=None, attributes=False):
        """sample() at the pixel centres of render_density()'s view (same defaults): a [height, width] SAMPLE_DTYPE array, and
        with attributes=True also the (channels, height, width) float32 channel sums.  Bit-identical to sample() on those points."""
        view = self._view(width, height, world_min, world_max)
        width, height = int(width), int(height)
        out = np.zeros((height, width), dtype=SAMPLE_DTYPE)
        attr = self._sample_attr(width * height) if attributes else None
        self._call("sample_grid", C.byref(view), _ptr(out), _ptr(attr) if attributes else None)
        return (out, attr.reshape(-1, height, width)) if attributes else out

    def sample_device(self, points_ptr, n, out_ptr, attr_ptr=None):
        """fs_sample_points_device: device pointers (n fs_vec2 in, n 24-byte fs_sample out, channels * n floats out), enqueued
        on the simulation's stream after the steps in flight; non-blocking."""
        self._call("sample_points_device", C.c_void_p(points_ptr), int(n), C.c_void_p(out_ptr),
                   C.c_void_p(attr_ptr) if attr_ptr else None)

    # -- 2D moving bodies (build extension): _Bodies, and the motion ---
    def set_body_motion(self, body, centre, rot=None, velocity=(0.0, 0.0), angular_velocity=0.0):
        """Pose and velocity of a body for the steps enqueued after this call; host memory only, no copy, no sync.  `rot`: four
        floats, row-major R with world = R * local (None: the identity).  The engine does not advance the pose: set it before
        every step of a moving body (rigid_motion2d computes one)."""
        r = np.eye(2, dtype=np.float32) if rot is None else np.asarray(rot, dtype=np.float32)
        m = BodyMotion(_vec2(centre), (C.c_float * 4)(*[float(x) for x in r.reshape(4)]), _vec2(velocity), float(angular_velocity))
        self._call("body_set_motion", int(body), C.byref(m))

    def body_motion(self, body):
        """(centre[2], rot[2, 2], velocity[2], angular_velocity) of a body: float32 arrays and a float32 scalar."""
        m = BodyMotion()
        self._call("body_get_motion", int(body), C.byref(m))
        v = lambda a: np.array([a.x, a.y], dtype=np.float32)      # noqa: E731
        return v(m.centre), np.array(list(m.rot), dtype=np.float32).reshape(2, 2), v(m.velocity), np.float32(m.angular_velocity)

    # -- 2D body loads (build extension): enable, enabled and the device pointer are _Bodies' ---
    def body_loads(self, body, reset=False):
        """What the fluid handed body `body` since its words were last zeroed: a BodyLoads record.  Blocking (one sync);
        reset=True zeroes the slot's words behind the read."""
        out = BodyLoad()
        self._call("body_loads", int(body), C.byref(out), 1 if reset else 0)
        return BodyLoads((int(out.impulse_q[0]), int(out.impulse_q[1])), int(out.angular_q), int(out.hits), int(out.dropped),
                         int(out.steps))

    def export_handle(self, which=_abi.FS_EXPORT_PARTICLES):
        """fs_export_handle: interprocess handle of the AoS particle view (switches on the live view) or of start_indices."""
        h = _abi.MemHandle()
        self._call("export_handle", int(which), C.byref(h))
        return h

    def particles_device_ptr(self):
        p = C.c_void_p()
        self._call("particles_device", C.byref(p))
        return p.value

    def start_indices_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._call("start_indices_device", C.byref(p), C.byref(n))
        return p.value, int(n.value)


class BodyLoads:
    """One body's load words (include/fluidsim.h "2D body loads"): the raw integers impulse_q (x, y) and angular_q in units of
    2^-20 velocity (and velocity * length) per unit particle mass, `hits`, `dropped`, and `steps`, the steps they were summed
    over.  The float64 views multiply by 2^-20 and the mass of one particle."""
    SCALE = 2.0 ** -_abi.FS_BODY_LOAD_SHIFT

    def __init__(self, impulse_q, angular_q, hits, dropped, steps):
        self.impulse_q, self.angular_q, self.hits, self.dropped, self.steps = tuple(impulse_q), angular_q, hits, dropped, steps

    def words(self):
        """the five device words as Python ints modulo 2^64, in the device's order"""
        m = (1 << 64) - 1
        return [self.impulse_q[0] & m, self.impulse_q[1] & m, self.angular_q & m, self.hits, self.dropped]

    def impulse(self, mass):
        """momentum handed to the body, float64 [2]"""
        return np.array([q * self.SCALE * float(mass) for q in self.impulse_q], dtype=np.float64)

    def angular_impulse(self, mass):
        """angular momentum about the body's centre handed to the body, counter-clockwise positive"""
        return self.angular_q * self.SCALE * float(mass)

    def mean_force(self, mass, dt):
        """the impulse divided by steps * dt (zero steps: zero)"""
        return self.impulse(mass) / (self.steps * float(dt)) if self.steps else np.zeros(2)

    def mean_torque(self, mass, dt):
        return self.angular_impulse(mass) / (self.steps * float(dt)) if self.steps else 0.0

    def __repr__(self):
        return (f"BodyLoads(impulse_q={self.impulse_q}, angular_q={self.angular_q}, hits={self.hits}, dropped={self.dropped}, "
                f"steps={self.steps})")


def rigid_motion2d(centre0, velocity, rate, t):
    """The pose of a body that started at `centre0` with the identity rotation, moves with `velocity` and turns counter-clockwise
    at `rate` rad/s, at time t: (centre[2], rot[4]) — in float64, cast to float32 once; the four floats are what
    FluidSimulation.set_body_motion takes as `rot`.  The matching angular velocity is `rate`."""
    c = np.asarray(centre0, dtype=np.float64) + np.asarray(velocity, dtype=np.float64) * float(t)
    th = float(rate) * float(t)
    rot = np.array([np.cos(th), -np.sin(th), np.sin(th), np.cos(th)], dtype=np.float64)
    return c.astype(np.float32), rot.astype(np.float32)


def generate_force_field(image, device=0):
    """Standalone generate_smooth_gradient_field (src/main.rs:403-515) on the GPU: u8 [h, w] -> f32 [h, w, 2]."""
    lib = load_library()
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = image.shape
    out = np.empty((h, w, 2), dtype=np.float32)
    _check(lib, lib.fs_generate_force_field(None, int(device), _ptr(image), w, h, _ptr(out)))
    return out


def reference_lattice(settings, offset=(0.0, 0.0)):
    lib = load_library()
    out = np.zeros(settings.particle_count, dtype=PARTICLE_DTYPE)
    _check(lib, lib.fs_reference_lattice(C.byref(settings), _vec2(offset), _ptr(out), out.shape[0]))
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

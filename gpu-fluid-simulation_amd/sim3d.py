"""The 3D simulation (include/fluidsim.h fs3_*; a build extension, not in the reference): its handle, its scene, the collider
mask, the motion of a rigid body and the camera of its surface renderer."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (FS_MATH_IEEE, MESH_VERTEX_DTYPE, PARTICLE3_DTYPE, SAMPLE3_DTYPE, SURFACE_HIT_DTYPE, Body3Load, BodyMotion3, Camera3,
                   Nozzle3, Settings3, TickSettings3, Vec3, load_library)
from ._handle import _Bodies, _check, _Count, _Diffusion, _normalise_samples, _ptr, _Simulation, _Stats, _SurfaceTension, _Tracking, _vec3
from .stats import Stats3D


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
    st = Settings3(int(n), float(s), float(h), _vec3(size))
    tick = TickSettings3(float(f(1.0) / f(120.0)), Vec3(0.0, 9.81, 0.0), 1.0, 50.0, 0.0, 0.1, 25.0)
    return st, (float(off[0]), float(off[1]), float(off[2])), tick


class FluidSimulation3D(_Count, _Tracking, _SurfaceTension, _Diffusion, _Bodies, _Stats, _Simulation):
    """3D extension (include/fluidsim.h fs3_*); not in the reference."""
    _prefix = "fs3_"
    _destroy = "fs3_destroy"
    _record = PARTICLE3_DTYPE
    _dim = 3
    _nozzle = Nozzle3        # the particle count that changes at run time: _Count
    _stats = Stats3D         # the fluid diagnostics: _Stats

    def __init__(self, settings, device=0, initial_offset=(0.0, 0.0, 0.0), math_mode=FS_MATH_IEEE, track=None):
        super().__init__()
        self.settings = settings
        _check(self._lib, self._lib.fs3_create_ex(C.byref(settings), int(device), _vec3(initial_offset), int(math_mode),
                                                  C.byref(self._h)))
        if track is not None:
            self.track(track)

    @property
    def grid_dims(self):
        w, h, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._call("grid_dims", C.byref(w), C.byref(h), C.byref(d))
        return int(w.value), int(h.value), int(d.value)

    @property
    def stream_ptr(self):
        """hipStream_t of the simulation as an integer (torch.cuda.ExternalStream / RCCL on the same stream)."""
        return int(self._fn("stream")(self._h) or 0)

    # -- 3D surface tension (build extension) -----------------
    def set_surface_tension(self, coefficient, threshold=0.0):
        """Colour-field surface tension (include/fluidsim.h "3D surface tension") for the steps enqueued after this call:
        force -coefficient * laplace(c) * n / |n| where the colour gradient |n| exceeds `threshold`."""
        self._call("set_surface_tension", 1, float(coefficient), float(threshold))

    def clear_surface_tension(self):
        """Back to the plain step, for the steps enqueued after this call."""
        self._call("set_surface_tension", 0, 0.0, 0.0)

    @property
    def surface_tension_params(self):
        """(coefficient, threshold) in use, or None when the feature is off."""
        if not self.surface_tension_enabled:
            return None
        c, t = C.c_float(), C.c_float()
        self._call("surface_tension_params", C.byref(c), C.byref(t))
        return float(c.value), float(t.value)

    # -- 3D channel diffusion and buoyancy (build extension): _Diffusion, and the limit ----
    @staticmethod
    def diffusion_limit(settings, tick, rest_density):
        """rho0 h^2 / (18 delta): the largest conductivity at which the explicit update of a uniform fluid at density rho0 is a
        convex combination of the neighbours' values.  The engine does not enforce it."""
        h = float(settings.smoothing_radius)
        return float(rest_density) * h * h / (18.0 * float(tick.delta))

    # -- 3D field sampling (build extension; DESIGN.md §14, the channels: §20) ----
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
        self._call("sample_points", _ptr(pts), n, _ptr(out))
        if attributes:
            self._call("sample_attr_points", _ptr(pts), n, None, _ptr(attr))
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
        self._call("sample_grid", C.byref(view), _ptr(out))
        if attributes:
            self._call("sample_attr_grid", C.byref(view), None, _ptr(attr))
        return (out, attr.reshape(-1, depth, height, width)) if attributes else out

    def sample_device(self, points_ptr, n, out_ptr):
        """fs3_sample_points_device: device pointers (n fs_vec3 in, n 40-byte fs3_sample out), enqueued on the simulation's
        stream after the steps in flight; non-blocking."""
        self._call("sample_points_device", C.c_void_p(points_ptr), int(n), C.c_void_p(out_ptr))

    def sample_attr(self, points, weights=False):
        """The channel sums alone at `points`: (channels, n) float32, with weights=True (weight[n], sums)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        attr = self._sample_attr(n)
        w = np.zeros(n, dtype=np.float32) if weights else None
        self._call("sample_attr_points", _ptr(pts), n, _ptr(w) if weights else None, _ptr(attr))
        return (w, attr) if weights else attr

    def sample_attr_device(self, points_ptr, n, weight_ptr, attr_ptr):
        """fs3_sample_attr_points_device: device pointers (n fs_vec3 in, n floats out or 0 / None, channels * n floats out),
        enqueued on the simulation's stream after the steps in flight; non-blocking."""
        self._call("sample_attr_points_device", C.c_void_p(points_ptr), int(n),
                   C.c_void_p(weight_ptr) if weight_ptr else None, C.c_void_p(attr_ptr) if attr_ptr else None)

    # -- 3D surface rendering (build extension) ---------------
    def render_surface(self, camera, params, out=None):
        """Ray-march the iso-surface of the density into a G-buffer: a [height, width] SURFACE_HIT_DTYPE array (ray parameter,
        density, outward normal, Shepard velocity, march index, hit kind) for a Camera3 (look_at_camera) and SurfaceParams3.
        Blocking; needs a step since create / the last upload.  `out`: a device pointer (int) instead: fs3_render_surface_device,
        enqueued on the simulation's stream after the steps in flight, non-blocking, returns None."""
        if out is not None:
            self._call("render_surface_device", C.byref(camera), C.byref(params), C.c_void_p(int(out)))
            return None
        hits = np.zeros((int(camera.height), int(camera.width)), dtype=SURFACE_HIT_DTYPE)
        self._call("render_surface", C.byref(camera), C.byref(params), _ptr(hits))
        return hits

    # -- 3D surface extraction (build extension) --------------
    def _view3(self, width, height, depth, world_min, world_max):
        sz = self.settings.size
        wmin = world_min if world_min is not None else (-sz.x / 2, -sz.y / 2, -sz.z / 2)
        wmax = world_max if world_max is not None else (sz.x / 2, sz.y / 2, sz.z / 2)
        return _abi.View3(_vec3(wmin), _vec3(wmax), int(width), int(height), int(depth))

    def extract_surface(self, width, height, depth, iso, world_min=None, world_max=None):
        """The iso-surface of the density as an indexed triangle mesh (surface nets over width x height x depth lattice NODES,
        the voxel centres of sample_grid on the same box; default: the whole domain): (vertices[V] MESH_VERTEX_DTYPE,
        triangles[T, 3] uint32), outward winding, open where the surface leaves the box.  Blocking; needs a step since create /
        the last upload.  Two ABI calls at most: the counts, then the arrays at exact size."""
        view = self._view3(width, height, depth, world_min, world_max)
        counts = (C.c_uint32 * 2)()
        self._call("extract_surface", C.byref(view), float(iso), None, 0, None, 0, counts)
        verts = np.zeros(int(counts[0]), dtype=MESH_VERTEX_DTYPE)
        tris = np.zeros((int(counts[1]), 3), dtype=np.uint32)
        if verts.shape[0] or tris.shape[0]:
            self._call("extract_surface", C.byref(view), float(iso), _ptr(verts) if verts.shape[0] else None, verts.shape[0],
                       _ptr(tris) if tris.shape[0] else None, tris.shape[0], counts)
            assert (int(counts[0]), int(counts[1])) == (verts.shape[0], tris.shape[0])
        return verts, tris

    def extract_surface_device(self, width, height, depth, iso, verts_ptr, vert_cap, tris_ptr, tri_cap, counts_ptr,
                               world_min=None, world_max=None):
        """fs3_extract_surface_device: device pointers (vert_cap 40-byte fs3_mesh_vertex, 3 * tri_cap uint32, 2 uint32 counts),
        enqueued on the simulation's stream after the steps in flight; no host read.  The counts are always the full ones:
        compare them with the capacities once the stream has passed the call."""
        view = self._view3(width, height, depth, world_min, world_max)
        self._call("extract_surface_device", C.byref(view), float(iso), C.c_void_p(int(verts_ptr)) if verts_ptr else None,
                   int(vert_cap), C.c_void_p(int(tris_ptr)) if tris_ptr else None, int(tri_cap),
                   C.c_void_p(int(counts_ptr)) if counts_ptr else None)

    # -- 3D colliders (build extension) -----------------------
    def set_collider(self, field):
        """Static obstacles: a float32 [D, H, W, 3] voxel field of push vectors in world units over the whole domain, zero = free
        space (include/fluidsim.h "3D colliders").  Blocking; holds for the steps enqueued afterwards; replaces an earlier one."""
        f = np.ascontiguousarray(field, dtype=np.float32)
        if f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("set_collider expects a [D, H, W, 3] float32 array")
        d, h, w = f.shape[:3]
        self._call("collider_upload", _ptr(f), int(w), int(h), int(d))

    def set_collider_mask(self, mask, want_field=False):
        """The collider of a uint8 [D, H, W] voxel mask (> 128: solid): every solid voxel pushes to its nearest free voxel (exact
        distance transform in index space, made on the GPU).  want_field=True returns the [D, H, W, 3] field."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != 3:
            raise ValueError("set_collider_mask expects a [D, H, W] uint8 array")
        d, h, w = m.shape
        out = np.zeros((d, h, w, 3), dtype=np.float32) if want_field else None
        self._call("collider_from_mask", _ptr(m), int(w), int(h), int(d), _ptr(out) if want_field else None)
        return out

    def clear_collider(self):
        self._call("collider_clear")

    @property
    def collider_dims(self):
        """(W, H, D) of the collider, (0, 0, 0) when none is set."""
        w, h, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._call("collider_dims", C.byref(w), C.byref(h), C.byref(d))
        return int(w.value), int(h.value), int(d.value)

    def collider(self):
        """The collider in use as a float32 [D, H, W, 3] array, or None when none is set."""
        w, h, d = self.collider_dims
        if w == 0:
            return None
        out = np.zeros((d, h, w, 3), dtype=np.float32)
        self._call("collider_download", _ptr(out), w * h * d)
        return out

    # -- 3D moving bodies (build extension): _Bodies, and the motion ---
    def set_body_motion(self, body, centre, rot=None, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0)):
        """Pose and velocity of a body for the steps enqueued after this call; host memory only, no copy, no sync.  `rot`: nine
        floats, row-major R with world = R * local (None: the identity).  The engine does not advance the pose: set it before
        every step of a moving body (rigid_motion computes one)."""
        r = np.eye(3, dtype=np.float32) if rot is None else np.asarray(rot, dtype=np.float32).reshape(9)
        m = BodyMotion3(_vec3(centre), (C.c_float * 9)(*[float(x) for x in r.reshape(9)]), _vec3(velocity), _vec3(angular_velocity))
        self._call("body_set_motion", int(body), C.byref(m))

    def body_motion(self, body):
        """(centre[3], rot[3, 3], velocity[3], angular_velocity[3]) of a body as float32 arrays."""
        m = BodyMotion3()
        self._call("body_get_motion", int(body), C.byref(m))
        v = lambda a: np.array([a.x, a.y, a.z], dtype=np.float32)      # noqa: E731
        return v(m.centre), np.array(list(m.rot), dtype=np.float32).reshape(3, 3), v(m.velocity), v(m.angular_velocity)

    # -- 3D body loads (build extension): enable, enabled and the device pointer are _Bodies' ---
    def body_loads(self, body, reset=False):
        """What the fluid handed body `body` since its words were last zeroed: a BodyLoads3D record.  Blocking (one sync);
        reset=True zeroes the slot's words behind the read."""
        out = Body3Load()
        self._call("body_loads", int(body), C.byref(out), 1 if reset else 0)
        return BodyLoads3D([int(q) for q in out.impulse_q], [int(q) for q in out.angular_q], int(out.hits), int(out.dropped),
                           int(out.steps))


class BodyLoads3D:
    """One body's load words (include/fluidsim.h "3D body loads"): the raw integers impulse_q (x, y, z) and angular_q (x, y, z,
    about the body's centre, world frame) in units of 2^-20 velocity (and velocity * length) per unit particle mass, `hits`,
    `dropped`, and `steps`, the steps they were summed over.  The float64 views multiply by 2^-20 and the mass of one particle."""
    SCALE = 2.0 ** -_abi.FS_BODY_LOAD_SHIFT

    def __init__(self, impulse_q, angular_q, hits, dropped, steps):
        self.impulse_q, self.angular_q, self.hits, self.dropped, self.steps = tuple(impulse_q), tuple(angular_q), hits, dropped, steps
        if len(self.impulse_q) != 3 or len(self.angular_q) != 3:
            raise ValueError("BodyLoads3D: impulse_q and angular_q have three components each")

    def words(self):
        """the eight device words as Python ints modulo 2^64, in the device's order"""
        m = (1 << 64) - 1
        return [q & m for q in self.impulse_q + self.angular_q] + [self.hits, self.dropped]

    def impulse(self, mass):
        """momentum handed to the body, float64 [3]"""
        return np.array([q * self.SCALE * float(mass) for q in self.impulse_q], dtype=np.float64)

    def angular_impulse(self, mass):
        """angular momentum about the body's centre handed to the body, world frame, float64 [3]"""
        return np.array([q * self.SCALE * float(mass) for q in self.angular_q], dtype=np.float64)

    def mean_force(self, mass, dt):
        """the impulse divided by steps * dt (zero steps: zero)"""
        return self.impulse(mass) / (self.steps * float(dt)) if self.steps else np.zeros(3)

    def mean_torque(self, mass, dt):
        return self.angular_impulse(mass) / (self.steps * float(dt)) if self.steps else np.zeros(3)

    def __repr__(self):
        return (f"BodyLoads3D(impulse_q={self.impulse_q}, angular_q={self.angular_q}, hits={self.hits}, dropped={self.dropped}, "
                f"steps={self.steps})")


def rigid_motion(centre0, velocity, axis, rate, t):
    """The pose of a body that started at `centre0` with the identity rotation, moves with `velocity` and turns about the unit
    vector along `axis` at `rate` rad/s, at time t: (centre[3], rot[9]) — Rodrigues' formula in float64, cast to float32 once; the
    nine floats are what FluidSimulation3D.set_body_motion takes as `rot`.  The matching angular velocity is rate * axis / |axis|."""
    c = np.asarray(centre0, dtype=np.float64) + np.asarray(velocity, dtype=np.float64) * float(t)
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = float(rate) * float(t)
    kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    rot = np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)
    return c.astype(np.float32), rot.astype(np.float32).reshape(9)


def box_mask3d(size, shape, world_min, world_max):
    """A box given in world coordinates rasterised to a collider mask for FluidSimulation3D.set_collider_mask: uint8 [D, H, W] for
    shape = (W, H, D) over the domain [-size/2, size/2], 255 where the voxel's centre lies inside the box, else 0."""
    axes = []
    for a, n in enumerate(shape):
        c = (np.arange(int(n)) + 0.5) / int(n) * float(size[a]) - float(size[a]) / 2
        axes.append((c >= float(world_min[a])) & (c <= float(world_max[a])))
    inside = axes[2][:, None, None] & axes[1][None, :, None] & axes[0][None, None, :]
    return np.where(inside, 255, 0).astype(np.uint8)


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


def reference_lattice_3d(settings, offset=(0.0, 0.0, 0.0)):
    lib = load_library()
    out = np.zeros(settings.particle_count, dtype=PARTICLE3_DTYPE)
    _check(lib, lib.fs3_reference_lattice(C.byref(settings), _vec3(offset), _ptr(out), out.shape[0]))
    return out

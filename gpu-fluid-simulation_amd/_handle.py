"""What the handles of the C ABI share: the status check, the marshalling helpers, the life cycle of a handle, the calls that
exist under both the `fs_` and the `fs3_` prefix, and the features (tracking, surface-tension read-outs, a particle count that
changes at run time, moving bodies) that are the same for 2D and 3D once the prefix, the record dtype and the vector width come from the class."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import PASS_NAMES, Vec2, Vec3, load_library


class FluidSimError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"fluidsim status {status}: {message}")
        self.status = status


def _check(lib, status):
    if status != _abi.FS_OK:
        raise FluidSimError(status, lib.fs_last_error().decode("utf-8", "replace"))


def _ptr(arr):
    """The data of a numpy array as a c_void_p."""
    return arr.ctypes.data_as(C.c_void_p)


def _vec2(a):
    return Vec2(float(a[0]), float(a[1]))


def _vec3(a):
    return Vec3(*[float(x) for x in a])


def _normalise_samples(out, attr):
    """Shepard normalisation in place: velocity and channel sums divided by the weight, where that is non-zero."""
    w = out["weight"]
    ok = w != 0
    out["velocity"][ok] /= w[ok, None]
    if attr is not None:
        attr[:, ok] /= w[ok]


class _Handle:
    """Owner of one handle of the library.  `_prefix` selects the family of calls; `_destroy` is the full name of the call
    that frees the handle, written out per class because it does not follow from the prefix (a slab is made by
    fs_slab_create and freed by fs_destroy)."""
    _prefix = "fs_"
    _destroy = None

    def __init__(self):
        self._lib = load_library()
        self._h = C.c_void_p()

    def _fn(self, stem):
        return getattr(self._lib, self._prefix + stem)

    def _call(self, stem, *args):
        """`prefix + stem` on this handle; its status is checked."""
        _check(self._lib, self._fn(stem)(self._h, *args))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
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


class _Engine(_Handle):
    """A handle that steps on a stream of its own: both simulations and the slab."""

    def sync(self):
        self._call("sync")

    @property
    def tick_count(self):
        return int(self._fn("tick_count")(self._h))

    @property
    def stream_ptr(self):
        """The HIP stream the steps (and the *_device calls) are enqueued on, as an integer (torch.cuda.ExternalStream)."""
        return self._fn("stream")(self._h)

    def profile(self, enable=True):
        self._call("profile_enable", 1 if enable else 0)

    def profile_read(self, reset=True):
        ms = (C.c_double * len(PASS_NAMES))()
        steps = C.c_uint64()
        self._call("profile_read", ms, C.byref(steps), 1 if reset else 0)
        return dict(zip(PASS_NAMES, [float(x) for x in ms])), int(steps.value)


class _Simulation(_Engine):
    """A whole simulation on one device: its records are `_record`, its vectors have `_dim` components."""
    _record = None
    _dim = None

    def _vec(self, a):
        return _vec2(a) if self._dim == 2 else _vec3(a)

    def tick(self, tick_settings):
        self._call("step", C.byref(tick_settings))

    def timed_steps(self, tick_settings, steps):
        ms = C.c_double()
        self._call("timed_steps", C.byref(tick_settings), int(steps), C.byref(ms))
        return float(ms.value)

    @property
    def particle_count(self):
        return int(self._fn("particle_count")(self._h))

    def download_particles(self):
        out = np.empty(self.particle_count, dtype=self._record)
        self._call("download_particles", _ptr(out), out.shape[0])
        return out

    def upload_particles(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self._record)
        self._call("upload_particles", _ptr(arr), arr.shape[0])


class _SurfaceTension:
    """The read-outs of the opt-in surface tension; set_surface_tension differs and stays per class."""

    @property
    def surface_tension_enabled(self):
        return bool(self._fn("surface_tension_enabled")(self._h))

    def surface_tension_forces(self):
        """The last step's surface-tension force per particle, (N, 2) float32 for the 2D simulation and (N, 3) for the 3D one,
        in download_particles() order."""
        out = np.empty((self.particle_count, self._dim), dtype=np.float32)
        self._call("download_surface_tension", _ptr(out), out.shape[0])
        return out


class _Stats:
    """Fluid diagnostics reduced on the device (build extension).  `_stats` is the class's record object
    (stats.Stats / stats.Stats3D)."""
    _stats = None

    def stats(self):
        """fs_stats_read / fs3_stats_read: momentum, energy, centre of mass, density range, bounding box, channel sums and a
        count of non-finite particles of the state behind everything enqueued so far, as exact integer words (blocking).  Works
        in every state of the handle and changes none of it."""
        raw = self._stats._ctype()
        self._call("stats_read", C.byref(raw))
        return self._stats(raw)

    def stats_device_ptr(self, ptr):
        """fs_stats_device / fs3_stats_device: the same record written to device memory at `ptr` (8-byte aligned, 208 bytes in
        2D and 232 in 3D), stream-ordered on stream_ptr and without a host read; Stats.from_bytes reads it back."""
        self._call("stats_device", C.c_void_p(int(ptr)))


class _Diffusion:
    """Opt-in diffusion and buoyancy of the tracking channels (build extension; DESIGN.md §27, 3D: §28).  diffusion_limit stays
    per class: the constant differs."""

    def set_diffusion(self, channel, conductivity):
        """Channel `channel` diffuses between neighbours with conductivity kappa >= 0 (0: not at all, the default), for the steps
        after this call.  Tracking must be on; track() and untrack() clear every conductivity and the buoyancy channel.  The
        explicit update is stable while conductivity <= diffusion_limit(...)."""
        self._call("set_diffusion", int(channel), float(conductivity))

    def diffusion(self, channel):
        k = C.c_float()
        self._call("get_diffusion", int(channel), C.byref(k))
        return float(k.value)

    def set_buoyancy(self, channel, beta, reference=0.0):
        """Channel `channel` becomes the buoyancy channel: a particle with value a gains -beta * (a - reference) * gravity * delta
        of velocity per step (Boussinesq), for the steps after this call."""
        self._call("set_buoyancy", int(channel), float(beta), float(reference))

    def clear_buoyancy(self):
        self._call("set_buoyancy", -1, 0.0, 0.0)

    @property
    def buoyancy(self):
        """(channel, beta, reference) of the buoyancy channel, or None"""
        c, b, r = C.c_int(), C.c_float(), C.c_float()
        self._call("get_buoyancy", C.byref(c), C.byref(b), C.byref(r))
        return None if c.value < 0 else (int(c.value), float(b.value), float(r.value))

    def buoyancy_forces(self):
        """What the last step with a buoyancy channel handed the force pass per particle (the buoyancy force, plus the surface
        tension's when that is on): (N, 2) float32 for the 2D simulation and (N, 3) for the 3D one, in download_particles() order."""
        out = np.empty((self.particle_count, self._dim), dtype=np.float32)
        self._call("download_buoyancy", _ptr(out), out.shape[0])
        return out


class _Count:
    """A particle count that changes at run time (build extension; DESIGN.md §22, 3D: §21).  `_nozzle` is the class's nozzle
    structure (fs_nozzle / fs3_nozzle); vectors have `_dim` components."""
    _nozzle = None

    @property
    def capacity(self):
        """Slots of the handle: particle_count can grow to this (reserve() raises it)."""
        return int(self._fn("capacity")(self._h))

    def reserve(self, capacity):
        """Room for `capacity` particles (grow-only, blocking); the state and everything observable are preserved."""
        self._call("reserve", int(capacity))

    def emit(self, records):
        """Append records (the class's particle dtype) behind the live particles, all fields as given;
        particle_count + len <= capacity."""
        arr = np.ascontiguousarray(records, dtype=self._record)
        self._call("emit_particles", _ptr(arr), arr.shape[0])

    def emit_nozzle(self, origin, u, v, velocity, nu, nv=1):
        """Append nu x nv particles generated on the device: centred on `origin`, spaced by the vectors u and v, all with
        `velocity` (include/fluidsim.h "2D particle count" / "3D particle count").  nv == 1 is a line."""
        z = self._nozzle(self._vec(origin), self._vec(u), self._vec(v), self._vec(velocity), int(nu), int(nv))
        self._call("emit_nozzle", C.byref(z))

    def remove_box(self, lo, hi):
        """Remove every particle with lo <= position <= hi on every axis (blocking, stable); returns how many went."""
        a, b, n = self._vec(lo), self._vec(hi), C.c_uint32()
        self._call("remove_in_box", C.byref(a), C.byref(b), C.byref(n))
        return int(n.value)

    def remove(self, flags):
        """Remove the particles whose entry of `flags` (one per particle, download_particles() order) is non-zero (blocking,
        stable); returns how many went."""
        f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
        n = C.c_uint32()
        self._call("remove_flagged", _ptr(f), f.shape[0], C.byref(n))
        return int(n.value)

    @property
    def next_id(self):
        """The id the next emitted particle gets while tracking is on (0 when it is off)."""
        return int(self._fn("track_next_id")(self._h))


class _Bodies:
    """Opt-in moving rigid bodies (build extension; DESIGN.md §24, 3D: §23).  A field is a float32 [H, W, 2] or [D, H, W, 3]
    array, a mask a uint8 [H, W] or [D, H, W] one: `_dim` axes, slowest first (the C calls take the extents fastest first), and
    `_dim` components.  set_body_motion and body_motion stay per class: their defaults and the angular velocity (a scalar in 2D, a
    vector in 3D) differ."""

    def _axes(self):
        return "H, W" if self._dim == 2 else "D, H, W"

    def add_body(self, field, extent):
        """A kinematic rigid body: a field of push vectors in world units (zero = free space) over the body's own box
        [-extent/2, extent/2] in the body frame (include/fluidsim.h "2D moving bodies" / "3D moving bodies").  Returns its slot, the
        lowest free one of 0 .. 7.  Blocking.  The body starts at the origin with the identity pose, at rest: set_body_motion
        places it."""
        f = np.ascontiguousarray(field, dtype=np.float32)
        if f.ndim != self._dim + 1 or f.shape[-1] != self._dim:
            raise ValueError(f"add_body expects a [{self._axes()}, {self._dim}] float32 array")
        slot = C.c_uint32()
        self._call("body_create", _ptr(f), *[int(n) for n in f.shape[-2::-1]], self._vec(extent), C.byref(slot))
        return int(slot.value)

    def add_body_mask(self, mask, extent, want_field=False):
        """The body of a mask (> 128: solid) over the box `extent`: the exact distance transform of set_collider_mask's producer
        on the body's box (in 2D: not set_obstacle_image's chamfer).  Returns the slot, with want_field=True (slot, the field)."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != self._dim:
            raise ValueError(f"add_body_mask expects a [{self._axes()}] uint8 array")
        out = np.zeros(m.shape + (self._dim,), dtype=np.float32) if want_field else None
        slot = C.c_uint32()
        self._call("body_create_from_mask", _ptr(m), *[int(n) for n in m.shape[::-1]], self._vec(extent),
                   _ptr(out) if want_field else None, C.byref(slot))
        return (int(slot.value), out) if want_field else int(slot.value)

    def body_dims(self, body):
        """((W, H), (ex, ey)) or ((W, H, D), (ex, ey, ez)) of a body: its field's extents and its box."""
        n, e = [C.c_uint32() for _ in range(self._dim)], self._vec((0.0,) * self._dim)
        self._call("body_dims", int(body), *[C.byref(k) for k in n], C.byref(e))
        return tuple(int(k.value) for k in n), tuple(float(getattr(e, a)) for a in "xyz"[:self._dim])

    def body_field(self, body):
        """A body's field as a float32 [H, W, 2] or [D, H, W, 3] array.  Blocking."""
        shape = self.body_dims(body)[0][::-1]
        out = np.zeros(shape + (self._dim,), dtype=np.float32)
        self._call("body_download", int(body), _ptr(out), int(np.prod(shape)))
        return out

    def remove_body(self, body):
        """Destroys a body and frees its slot; the other bodies keep theirs.  Blocking."""
        self._call("body_destroy", int(body))

    @property
    def body_count(self):
        return int(self._fn("body_count")(self._h))

    # -- body loads (build extension; DESIGN.md §25, 3D: §26); body_loads stays per class: the records differ
    def enable_body_loads(self, on=True):
        """Turns the per-body load sums on or off (include/fluidsim.h "2D body loads" / "3D body loads").  Enabling zeroes every
        body's words.  While off a step launches what it launched without them; while on the particles are still byte for byte
        the same."""
        self._call("body_loads_enable", 1 if on else 0)

    @property
    def body_loads_enabled(self):
        return bool(self._fn("body_loads_enabled")(self._h))

    def body_loads_device_ptr(self):
        """fs_body_loads_device / fs3_body_loads_device: the device address of the 8 x 5 (3D: 8 x 8) 64-bit words, by slot, for a
        consumer on the handle's stream."""
        p = C.c_void_p()
        self._call("body_loads_device", C.byref(p))
        return p.value


class _Tracking:
    """Opt-in particle tracking (build extension; DESIGN.md §12, 3D: §20)."""

    def track(self, channels=0):
        """Give every particle an id (= its current slot) and `channels` float attributes (all 0) that follow it through the
        sort of every later step.  Calling it again re-initialises."""
        self._call("track_enable", int(channels))

    def untrack(self):
        self._call("track_disable")

    @property
    def track_channels(self):
        """-1 when tracking is off, else the number of attribute channels."""
        return int(self._fn("track_channels")(self._h))

    def particle_ids(self):
        """uint32 id of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.uint32)
        self._call("track_download_ids", _ptr(out), out.shape[0])
        return out

    def set_particle_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self._call("track_upload_ids", _ptr(ids), ids.shape[0])

    def attribute(self, channel):
        """float32 attribute `channel` of the particle in every slot, in download_particles() order."""
        out = np.empty(self.particle_count, dtype=np.float32)
        self._call("track_download_attr", int(channel), _ptr(out), out.shape[0])
        return out

    def set_attribute(self, channel, values):
        """`values` is copied bit for bit when it already is float32 (NaN payloads survive)."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        self._call("track_upload_attr", int(channel), _ptr(values), values.shape[0])

    def download_particles_by_id(self):
        """The records in id order: out[id] is the particle with that id (ids >= particle_count are skipped; entries that no
        id names stay zero)."""
        out = np.zeros(self.particle_count, dtype=self._record)
        self._call("download_particles_by_id", _ptr(out), out.shape[0])
        return out

    def particle_ids_device_ptr(self):
        p = C.c_void_p()
        self._call("track_ids_device", C.byref(p))
        return p.value

    def attribute_device_ptr(self, channel):
        p = C.c_void_p()
        self._call("track_attr_device", int(channel), C.byref(p))
        return p.value

    def _sample_attr(self, n):
        """The zeroed (channels, n) array that a sampling call fills with the channel sums."""
        ch = self.track_channels
        if ch <= 0:
            raise FluidSimError(_abi.FS_ERR_INVALID, "sample(attributes=True) needs track(channels >= 1)")
        return np.zeros((ch, n), dtype=np.float32)

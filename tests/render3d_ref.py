"""ctypes loader of the 3D surface-rendering checker (tests/render3d_checker.cpp on top of tests/sample3d_checker.cpp and
oracle/sph_oracle3d.cpp, both included unchanged).  TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by
tests/checker_lib.py: the oracle's flags, a per-user cache outside the tree, keyed by the sources' contents.  Also here: the
cameras and the iso rule that the CPU and the GPU tests share."""
import ctypes as C

import numpy as np

from tests import checker_lib as CL
from tests import sample3d_ref as S3

P = C.c_void_p
SOURCES = [CL.here("render3d_checker.cpp")] + S3.SOURCES
OWN = {"smp3_load": S3.OWN["smp3_load"], "smp3_sample": S3.OWN["smp3_sample"],
       "rnd3_render": (None, [P, P, P, P]), "rnd3_ray": (None, [P, C.c_uint32, C.c_uint32, P])}

SURFACE_HIT_DTYPE = np.dtype([("t", "<f4"), ("density", "<f4"), ("normal", "<f4", (3,)), ("velocity", "<f4", (3,)),
                              ("steps", "<u4"), ("hit", "<u4")])
assert SURFACE_HIT_DTYPE.itemsize == 40
f = np.float32


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Camera3(C.Structure):
    _fields_ = [("eye", Vec3), ("forward", Vec3), ("right", Vec3), ("up", Vec3), ("width", C.c_uint32), ("height", C.c_uint32),
                ("orthographic", C.c_int32), ("reserved", C.c_uint32)]


class SurfaceParams3(C.Structure):
    _fields_ = [("iso", C.c_float), ("t_near", C.c_float), ("ds", C.c_float), ("max_steps", C.c_uint32), ("refine", C.c_uint32)]


assert C.sizeof(Camera3) == 64 and C.sizeof(SurfaceParams3) == 20


def lib():
    return CL.load("render3d_checker", SOURCES, "orc3_", OWN)


def as_camera(cam):
    """Any camera record of the 64-byte layout (the product's Camera3 included) as this module's."""
    return Camera3.from_buffer_copy(bytes(cam))


def as_params(sp):
    return SurfaceParams3.from_buffer_copy(bytes(sp))


class Render3Checker(S3.Sample3Checker):
    """The sampling checker with the ray-marcher of DESIGN.md §16 on the loaded state."""

    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0)):
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc3_create(C.addressof(settings), *[float(x) for x in initial_offset])
        if not self.h:
            raise ValueError("checker: invalid settings")
        self.n = int(self.L.orc3_count(self.h))

    def render(self, cam, sp):
        cam, sp = as_camera(cam), as_params(sp)
        out = np.zeros((cam.height, cam.width), dtype=SURFACE_HIT_DTYPE)
        self.L.rnd3_render(self.h, C.addressof(cam), C.addressof(sp), out.ctypes.data)
        return out


def params(iso, t_near, ds, max_steps, refine):
    return SurfaceParams3(float(iso), float(t_near), float(ds), int(max_steps), int(refine))


def camera(eye, forward, right, up, width, height, orthographic):
    v = lambda a: Vec3(*[float(f(x)) for x in a])       # noqa: E731
    return Camera3(v(eye), v(forward), v(right), v(up), int(width), int(height), 1 if orthographic else 0, 0)


def rays(cam):
    """numpy-f32 restatement of the statement's rays: (o, d), each [height, width, 3] float32."""
    w, h = cam.width, cam.height
    u = ((np.arange(w, dtype=f) + f(0.5)) / f(w) - f(0.5))[None, :, None]
    v = ((np.arange(h, dtype=f) + f(0.5)) / f(h) - f(0.5))[:, None, None]
    vec = lambda q: f([q.x, q.y, q.z])                  # noqa: E731
    eye, fw, ri, up = vec(cam.eye), vec(cam.forward), vec(cam.right), vec(cam.up)
    if cam.orthographic:
        o = ((eye + u * ri) + v * up).astype(f)
        D = np.broadcast_to(fw, o.shape).astype(f)
    else:
        D = ((fw + u * ri) + v * up).astype(f)
        o = np.broadcast_to(eye, D.shape).astype(f)
    ln = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]).astype(f)
    return o, (D / ln[..., None]).astype(f)


def points_at(cam, t):
    """x(t) of every pixel for a [height, width] float32 array of ray parameters, in numpy f32."""
    o, d = rays(cam)
    return (o + np.asarray(t, dtype=f)[..., None] * d).astype(f)


def iso_of(particles, fraction=0.5):
    """The threshold of the tests: a fraction of the median stored density of the state."""
    return float(f(fraction) * f(np.median(particles["density"])))


def fluid_box(particles):
    p = particles["predicted_position"]
    return p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)


def scene_cameras(settings, particles, width, height):
    """Named cameras around the state's fluid: {name: (Camera3, t_near)}.  The march of the tests is 64 steps of h / 2 = 32 h."""
    h = float(settings.smoothing_radius)
    lo, hi = fluid_box(particles)
    c, ext = 0.5 * (lo + hi), hi - lo
    size = np.float64([settings.size.x, settings.size.y, settings.size.z])
    aspect = width / height
    span = 1.6 * max(ext[0] / max(aspect, 1e-9), ext[1])          # the block with a margin: hits in the middle, misses around
    out = {}
    # outside the box on -z, looking in along +z: parallel rays, wider than the fluid
    out["ortho_front"] = (camera(c - [0, 0, 0.5 * ext[2] + 6 * h], [0, 0, 1], [span * aspect, 0, 0], [0, -span, 0], width, height, True), 0.0)
    # perspective from outside the domain, oblique: no axis-aligned component
    eye = c + np.float64([-0.9 * ext[0] - 5 * h, -0.7 * ext[1] - 4 * h, -0.8 * ext[2] - 6 * h])
    fw = (c - eye) / np.linalg.norm(c - eye)
    ri = np.cross(fw, [0, -1, 0]); ri /= np.linalg.norm(ri)
    up = np.cross(ri, fw)
    out["persp_oblique"] = (camera(eye, fw, ri * 1.4 * aspect, up * 1.4, width, height, False), 2.0 * h)
    # the eye inside the fluid, at its densest particle: every ray starts inside (hit == 2)
    deep = particles["predicted_position"][np.argmax(particles["density"])].astype(np.float64)
    out["persp_inside"] = (camera(deep, [0.3, 0.2, 1], [6.0, 0, 0], [0, 6.0, 0], width, height, False), 0.0)
    # ... and just outside it, looking through it with a wide fan: hits, misses, and rays that leave the domain on every side
    out["persp_fan"] = (camera(c - [0, 0, 0.5 * ext[2] + 1.5 * h], [0.1, -0.05, 1], [8.0, 0, 0], [0, 8.0, 0], width, height, False), 0.0)
    # looking away from the fluid, out of the domain
    out["persp_away"] = (camera(c - [0, 0, 0.5 * ext[2] + 2 * h], [0, 0, -1], [aspect, 0, 0], [0, 1, 0], width, height, False), 0.0)
    # parallel rays over four times the domain, starting outside it: wrapped cell coordinates and the X >= grid_w skips on every side
    out["ortho_overhang"] = (camera([0, 0, -0.5 * size[2] - 3 * h], [0, 0, 1], [4 * size[0], 0, 0], [0, 4 * size[1], 0], width, height, True), 0.0)
    # ... and so far out that u32_sat saturates and the + 1 wraps the cell coordinate to 0 (only the centre rays are near the domain)
    out["ortho_huge"] = (camera([0, 0, -0.5 * size[2] - 3 * h], [0, 0, 1], [4e10, 0, 0], [0, 4e10, 0], width, height, True), 0.0)
    return out

"""ctypes binding of the 3D field-sampling checker (tests/sample3d_checker.cpp, which includes oracle/sph_oracle3d.cpp
unchanged).  TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by tests/checker_lib.py: the oracle's flags, a per-user
cache outside the tree, keyed by the sources' contents."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL

P = C.c_void_p
SOURCES = [CL.here("sample3d_checker.cpp")] + CL.ORACLE_3D
OWN = {"smp3_load": (C.c_int, [P, P, C.c_size_t, C.c_float]), "smp3_sample": (None, [P, P, C.c_size_t, P]),
       "smp3_grid_points": (None, [P, P]), "smp3_sample_grid": (None, [P, P, P])}

SAMPLE3_DTYPE = np.dtype([("density", "<f4"), ("weight", "<f4"), ("velocity", "<f4", (3,)), ("gradient", "<f4", (3,)),
                          ("neighbours", "<u4"), ("cell", "<u4")])
assert SAMPLE3_DTYPE.itemsize == 40


class View3(C.Structure):
    _fields_ = [("world_min", C.c_float * 3), ("world_max", C.c_float * 3), ("width", C.c_uint32), ("height", C.c_uint32),
                ("depth", C.c_uint32)]


def lib():
    return CL.load("sample3d_checker", SOURCES, "orc3_", OWN)


def _view(width, height, depth, world_min, world_max):
    f3 = C.c_float * 3
    return View3(f3(*[float(v) for v in world_min]), f3(*[float(v) for v in world_max]), int(width), int(height), int(depth))


def grid_points(width, height, depth, world_min, world_max):
    """The voxel centres of a view in the header's expression: (depth * height * width, 3) float32, x fastest."""
    v = _view(width, height, depth, world_min, world_max)
    pts = np.empty((int(width) * int(height) * int(depth), 3), dtype=np.float32)
    lib().smp3_grid_points(C.addressof(v), pts.ctypes.data)
    return pts


class Sample3Checker(O.OracleSim3D):
    """The 3D oracle with the sampler of DESIGN.md §14 on a loaded state: the records after a step and that step's mass."""

    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0)):
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc3_create(C.addressof(settings), *[float(x) for x in initial_offset])
        if not self.h:
            raise ValueError("checker: invalid settings")
        self.n = int(self.L.orc3_count(self.h))

    def load(self, particles, mass):
        """fs3_download_particles of a handle after a step (or the 3D oracle's records) and the mass of that step's tick."""
        p = np.ascontiguousarray(particles, dtype=O.PARTICLE3_DTYPE)
        r = self.L.smp3_load(self.h, p.ctypes.data, p.shape[0], float(mass))
        assert r != 1, "checker: the state does not fit the settings"
        assert r != 2, "checker: the records are not sorted by grid"
        assert r == 0
        return self

    def sample(self, points):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(pts.shape[0], dtype=SAMPLE3_DTYPE)
        self.L.smp3_sample(self.h, pts.ctypes.data, pts.shape[0], out.ctypes.data)
        return out

    def sample_grid(self, width, height, depth, world_min, world_max):
        v = _view(width, height, depth, world_min, world_max)
        out = np.zeros((int(depth), int(height), int(width)), dtype=SAMPLE3_DTYPE)
        self.L.smp3_sample_grid(self.h, C.addressof(v), out.ctypes.data)
        return out


# ---- query sets shared by the CPU and the GPU tests -----------------------------------------------------------------------
def uniform_points(settings, count, seed, scale=1.2):
    """`count` points uniform over `scale` x the domain (so that some lie outside it)."""
    rng = np.random.default_rng(seed)
    half = np.float32([settings.size.x, settings.size.y, settings.size.z]) * np.float32(0.5 * scale)
    return rng.uniform(-half, half, size=(count, 3)).astype(np.float32)


def boundary_points(settings, particles, count, seed):
    """Points on faces of the cells next to particles (a coordinate exactly on a cell boundary, where floor() decides), and the
    corners and edge mid-points of the domain, on it and just outside."""
    f = np.float32
    rng = np.random.default_rng(seed)
    h = f(settings.smoothing_radius)
    half = f([settings.size.x, settings.size.y, settings.size.z]) * f(0.5)
    pick = particles["predicted_position"][rng.choice(particles.shape[0], count, replace=False)].astype(np.float32)
    faces = pick.copy()
    axis = rng.integers(0, 3, size=count)
    side = rng.integers(0, 2, size=count)
    for k in range(count):
        a = axis[k]
        c = np.floor((faces[k, a] + half[a]) / h) + f(side[k])      # the lower or the upper face of the particle's cell
        faces[k, a] = c * h - half[a]
    corners = np.array([[sx, sy, sz] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)], dtype=np.float32)
    on = corners * half
    out = corners * (half + f(0.5) * h)
    return np.concatenate([faces, on, out]).astype(np.float32)

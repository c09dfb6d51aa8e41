"""ctypes loader of the field-sampling checker (tests/sample_checker.cpp, which includes oracle/sph_oracle.cpp unchanged).
TEST INFRASTRUCTURE ONLY.  Built on first use with the oracle's flags into a per-user cache directory outside the tree
(the checkout may be read-only), keyed by the sources' contents."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "sample_checker.cpp"), os.path.join(ROOT, "oracle", "sph_oracle.cpp"),
           os.path.join(ROOT, "include", "fluidsim.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-shared"]   # oracle/Makefile

SAMPLE_DTYPE = np.dtype([("density", "<f4"), ("weight", "<f4"), ("velocity", "<f4", (2,)), ("neighbours", "<u4"), ("cell", "<u4")])
assert SAMPLE_DTYPE.itemsize == 24

_lib = None


def build():
    h = hashlib.sha256()
    for s in SOURCES:
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    d = os.path.join(tempfile.gettempdir(), f"fs_sample_checker_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, f"libsample_checker_{h.hexdigest()[:16]}.so")
    if not os.path.exists(out):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + ["-o", tmp, SOURCES[0]])
        os.replace(tmp, out)
    return out


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        for name, f in O.lib().__dict__.items():        # the oracle's entry points, same prototypes
            if name.startswith("orc_") and not name.startswith("orc3_"):
                g = getattr(L, name)
                g.argtypes, g.restype = f.argtypes, f.restype
        P = C.c_void_p
        L.smp_load.argtypes = [P, P, C.c_size_t, P, C.c_size_t, P]
        L.smp_load.restype = C.c_int
        L.smp_sample.argtypes = [P, P, C.c_size_t, C.c_int, P, P, P]
        L.smp_sample.restype = None
        L.smp_grid_points.argtypes = [C.c_float] * 4 + [C.c_uint32, C.c_uint32, P]
        L.smp_grid_points.restype = None
        L.smp_sample_grid.argtypes = [P] + [C.c_float] * 4 + [C.c_uint32, C.c_uint32, C.c_int, P, P, P]
        L.smp_sample_grid.restype = None
        L.orc_set_threads(1)
        _lib = L
    return _lib


def set_threads(n):
    lib().orc_set_threads(int(n))


def grid_points(width, height, world_min, world_max):
    """The pixel centres of a view in orc_render's expression: (height * width, 2) float32, row-major."""
    pts = np.empty((int(width) * int(height), 2), dtype=np.float32)
    lib().smp_grid_points(float(world_min[0]), float(world_min[1]), float(world_max[0]), float(world_max[1]),
                          int(width), int(height), pts.ctypes.data)
    return pts


class SampleChecker(O.OracleSim):
    """The oracle with the sampler of DESIGN.md §13 on its current state (after a step), or on a loaded one."""

    def __init__(self, settings, initial_offset=(0.0, 0.0), ref_quirks=True):
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc_create(C.addressof(settings), float(initial_offset[0]), float(initial_offset[1]),
                                   1 if ref_quirks else 0)
        if not self.h:
            raise ValueError("checker: invalid settings (particle_count <= 1)")
        self.n = int(self.L.orc_count(self.h))

    def load(self, particles, start_indices, uniform):
        """A downloaded state: fs_download_particles, fs_download_start_indices and fs_get_uniform of one handle."""
        p = np.ascontiguousarray(particles, dtype=O.PARTICLE_DTYPE)
        s = np.ascontiguousarray(start_indices, dtype=np.uint32)
        r = self.L.smp_load(self.h, p.ctypes.data, p.shape[0], s.ctypes.data, s.shape[0], C.addressof(uniform))
        assert r == 0, "checker: the state does not fit the settings"

    def _attr(self, attr):
        if attr is None:
            return 0, None
        attr = np.ascontiguousarray(attr, dtype=np.float32)
        assert attr.ndim == 2 and attr.shape[1] == self.n and 1 <= attr.shape[0] <= 4
        return attr.shape[0], attr

    def sample(self, points, attr=None):
        """-> (SAMPLE_DTYPE[n], float32 (C, n) or None)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n = pts.shape[0]
        ch, attr = self._attr(attr)
        out = np.zeros(n, dtype=SAMPLE_DTYPE)
        aout = np.zeros((ch, n), dtype=np.float32) if ch else None
        self.L.smp_sample(self.h, pts.ctypes.data, n, ch, attr.ctypes.data if ch else None, out.ctypes.data,
                          aout.ctypes.data if ch else None)
        return out, aout

    def sample_grid(self, width, height, world_min, world_max, attr=None):
        n = int(width) * int(height)
        ch, attr = self._attr(attr)
        out = np.zeros(n, dtype=SAMPLE_DTYPE)
        aout = np.zeros((ch, n), dtype=np.float32) if ch else None
        self.L.smp_sample_grid(self.h, float(world_min[0]), float(world_min[1]), float(world_max[0]), float(world_max[1]),
                               int(width), int(height), ch, attr.ctypes.data if ch else None, out.ctypes.data,
                               aout.ctypes.data if ch else None)
        return out, aout

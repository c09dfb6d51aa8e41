"""ctypes binding of the field-sampling checker (tests/sample_checker.cpp, which includes oracle/sph_oracle.cpp unchanged).
TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by tests/checker_lib.py: the oracle's flags, a per-user cache outside
the tree, keyed by the sources' contents."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL

P = C.c_void_p
SOURCES = [CL.here("sample_checker.cpp")] + CL.ORACLE_2D
OWN = {"smp_load": (C.c_int, [P, P, C.c_size_t, P, C.c_size_t, P]),
       "smp_sample": (None, [P, P, C.c_size_t, C.c_int, P, P, P]),
       "smp_grid_points": (None, [C.c_float] * 4 + [C.c_uint32, C.c_uint32, P]),
       "smp_sample_grid": (None, [P] + [C.c_float] * 4 + [C.c_uint32, C.c_uint32, C.c_int, P, P, P])}

SAMPLE_DTYPE = np.dtype([("density", "<f4"), ("weight", "<f4"), ("velocity", "<f4", (2,)), ("neighbours", "<u4"), ("cell", "<u4")])
assert SAMPLE_DTYPE.itemsize == 24


def lib():
    return CL.load("sample_checker", SOURCES, "orc_", OWN)


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

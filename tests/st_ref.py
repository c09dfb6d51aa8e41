"""ctypes binding of the surface-tension checker (tests/st_checker.cpp, which includes oracle/sph_oracle.cpp unchanged).
TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by tests/checker_lib.py: the oracle's flags, a per-user cache outside
the tree, keyed by the sources' contents."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL

P = C.c_void_p
SOURCES = [CL.here("st_checker.cpp")] + CL.ORACLE_2D
OWN = {"stc_surface_tension": (None, [P, P, P]), "stc_move": (None, [P, P]), "stc_step": (None, [P, P, C.c_int, P])}


def lib():
    return CL.load("st_checker", SOURCES, "orc_", OWN)


def set_threads(n):
    lib().orc_set_threads(int(n))


class STChecker(O.OracleSim):
    """The oracle with the opt-in surface-tension pass.  `st` holds the last ST step's forces."""

    def __init__(self, settings, initial_offset=(0.0, 0.0), ref_quirks=True):
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc_create(C.addressof(settings), float(initial_offset[0]), float(initial_offset[1]),
                                   1 if ref_quirks else 0)
        if not self.h:
            raise ValueError("checker: invalid settings (particle_count <= 1)")
        self.n = int(self.L.orc_count(self.h))
        self.st = None

    def step(self, tick, stable_sort=False, surface_tension=True):
        if surface_tension:
            st = np.zeros((self.n, 2), dtype=np.float32)
            self.L.stc_step(self.h, C.addressof(tick), 1 if stable_sort else 0, st.ctypes.data)
            self.st = st
        else:
            self.L.stc_step(self.h, C.addressof(tick), 1 if stable_sort else 0, None)

    def sort_stable(self):
        """the stable sort of step(stable_sort=True), as a pass of its own (beside OracleSim.sort)"""
        self.L.orc_sort_stable(self.h)

    def surface_tension_pass(self):
        """The ST pass on the current state (after density()): (st (N, 2) f32, {n.x, n.y, L} (N, 3) f32)."""
        st = np.zeros((self.n, 2), dtype=np.float32)
        nl = np.zeros((self.n, 3), dtype=np.float32)
        self.L.stc_surface_tension(self.h, st.ctypes.data, nl.ctypes.data)
        return st, nl

    def move_st(self, st=None):
        if st is None:
            self.L.stc_move(self.h, None)
        else:
            st = np.ascontiguousarray(st, dtype=np.float32)
            self.L.stc_move(self.h, st.ctypes.data)

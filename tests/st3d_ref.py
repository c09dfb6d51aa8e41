"""ctypes binding of the 3D surface-tension checker (tests/st3d_checker.cpp, which includes oracle/sph_oracle3d.cpp unchanged).
TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by tests/checker_lib.py: the oracle's flags, a per-user cache outside
the tree, keyed by the sources' contents."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL

P = C.c_void_p
SOURCES = [CL.here("st3d_checker.cpp")] + CL.ORACLE_3D
OWN = {"st3_step": (None, [P, P, C.c_int, C.c_float, C.c_float, P, P]), "st3_pass": (None, [P, C.c_float, C.c_float, P, P, P])}


def lib():
    return CL.load("st3d_checker", SOURCES, "orc3_", OWN)


class ST3Checker(O.OracleSim3D):
    """The 3D oracle with the opt-in surface-tension pass.  `st` holds the last ST step's forces, (N, 3) f32
    in particles() order."""

    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0)):
        self.L = lib()
        self.h = self.L.orc3_create(C.addressof(settings), *[float(x) for x in initial_offset])
        if not self.h:
            raise ValueError("checker: invalid settings")
        self.n = int(self.L.orc3_count(self.h))
        self.st = None

    def step(self, tick, surface_tension=None, want_acc=False):
        """surface_tension: None (the oracle's step) or (sigma, tau).  want_acc: returns the step's `acc`, (N, 3) f32."""
        acc = np.zeros((self.n, 3), dtype=np.float32) if want_acc else None
        accp = acc.ctypes.data if want_acc else None
        if surface_tension is None:
            self.L.st3_step(self.h, C.addressof(tick), 0, 0.0, 0.0, None, accp)
            return acc
        st = np.zeros((self.n, 3), dtype=np.float32)
        self.L.st3_step(self.h, C.addressof(tick), 1, float(surface_tension[0]), float(surface_tension[1]), st.ctypes.data, accp)
        self.st = st
        return acc

    def surface_tension_pass(self, sigma, tau):
        """The pass alone on the state the last step left: (n (N, 3), L (N,), st (N, 3)), all f32."""
        n = np.zeros((self.n, 3), dtype=np.float32)
        L = np.zeros(self.n, dtype=np.float32)
        st = np.zeros((self.n, 3), dtype=np.float32)
        self.L.st3_pass(self.h, float(sigma), float(tau), n.ctypes.data, L.ctypes.data, st.ctypes.data)
        return n, L, st

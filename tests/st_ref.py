"""ctypes loader of the surface-tension checker (tests/st_checker.cpp, which includes oracle/sph_oracle.cpp unchanged).
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
SOURCES = [os.path.join(HERE, "st_checker.cpp"), os.path.join(ROOT, "oracle", "sph_oracle.cpp"),
           os.path.join(ROOT, "include", "fluidsim.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-shared"]   # oracle/Makefile

_lib = None


def build():
    h = hashlib.sha256()
    for s in SOURCES:
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    d = os.path.join(tempfile.gettempdir(), f"fs_st_checker_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, f"libst_checker_{h.hexdigest()[:16]}.so")
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
        L.stc_surface_tension.argtypes = [P, P, P]
        L.stc_surface_tension.restype = None
        L.stc_move.argtypes = [P, P]
        L.stc_move.restype = None
        L.stc_step.argtypes = [P, P, C.c_int, P]
        L.stc_step.restype = None
        L.orc_sort_stable.argtypes = [P]
        L.orc_sort_stable.restype = None
        L.orc_set_threads(1)
        _lib = L
    return _lib


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

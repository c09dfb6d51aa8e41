"""ctypes loader of the 3D surface-tension checker (tests/st3d_checker.cpp, which includes oracle/sph_oracle3d.cpp unchanged).
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
SOURCES = [os.path.join(HERE, "st3d_checker.cpp"), os.path.join(ROOT, "oracle", "sph_oracle3d.cpp"),
           os.path.join(ROOT, "include", "fluidsim.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-shared"]   # oracle/Makefile

_lib = None


def build():
    h = hashlib.sha256()
    for s in SOURCES:
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    d = os.path.join(tempfile.gettempdir(), f"fs_st3d_checker_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, f"libst3d_checker_{h.hexdigest()[:16]}.so")
    if not os.path.exists(out):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + ["-o", tmp, SOURCES[0]])
        os.replace(tmp, out)
    return out


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        for name, fn in O.lib().__dict__.items():       # the 3D oracle's entry points, same prototypes
            if name.startswith("orc3_"):
                g = getattr(L, name)
                g.argtypes, g.restype = fn.argtypes, fn.restype
        P = C.c_void_p
        L.st3_step.argtypes = [P, P, C.c_int, C.c_float, C.c_float, P, P]
        L.st3_step.restype = None
        L.st3_pass.argtypes = [P, C.c_float, C.c_float, P, P, P]
        L.st3_pass.restype = None
        _lib = L
    return _lib


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

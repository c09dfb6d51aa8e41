"""ctypes loader of the diffusion / buoyancy checker (tests/diffuse_checker.cpp, which includes tests/st_checker.cpp and through
it oracle/sph_oracle.cpp, both unchanged).  TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by tests/checker_lib.py:
the oracle's flags, a per-user cache outside the tree, keyed by the sources' contents.

DiffuseChecker steps the oracle pass by pass.  Between spatial_lookup and the sort it reads the keys and derives the permutation
the sort is about to apply, exactly as tests/track_ref.TrackChecker does (oracle.bitonic_keys for the reference network,
np.argsort(kind="stable") for the stable sort); ids and channels follow it (the carry), then the C side finishes the step:
cell starts -> density -> optional surface tension -> diffusion / buoyancy -> the move with what the pass hands on."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL
from tests import st_ref

P = C.c_void_p
SOURCES = [CL.here("diffuse_checker.cpp")] + st_ref.SOURCES
OWN = {"stc_surface_tension": st_ref.OWN["stc_surface_tension"], "stc_move": st_ref.OWN["stc_move"],
       "dfc_diffuse": (None, [P] * 8), "dfc_finish_step": (None, [P] * 8)}
MAX_CHANNELS = 4


class Settings(C.Structure):
    _fields_ = [("channels", C.c_int), ("kappa", C.c_float * 4), ("buoy", C.c_int), ("beta", C.c_float), ("reference", C.c_float)]


def lib():
    return CL.load("diffuse_checker", SOURCES, "orc_", OWN)


def set_threads(n):
    lib().orc_set_threads(int(n))


class DiffuseChecker(O.OracleSim):
    """The oracle with tracking's carry, the opt-in surface tension and the diffusion / buoyancy pass (§27).
    ids (N) and attr (C, N) are in slot order; after a step: st (the ST forces, or None), fb (what the pass handed the move,
    or None without a buoyancy channel), R (float64, N) and acc (f32, C x N) of the pass, attr_in (what the pass read)."""

    def __init__(self, settings, initial_offset=(0.0, 0.0), ref_quirks=True, channels=1):
        assert 0 <= channels <= MAX_CHANNELS
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc_create(C.addressof(settings), float(initial_offset[0]), float(initial_offset[1]), 1 if ref_quirks else 0)
        if not self.h:
            raise ValueError("checker: invalid settings (particle_count <= 1)")
        self.n = int(self.L.orc_count(self.h))
        self.initial_offset, self.ref_quirks = initial_offset, ref_quirks
        self.surface_tension = False
        self.reset(channels)

    def reset(self, channels=None):
        """fs_track_enable: id = current slot, every channel +0.0, every conductivity and the buoyancy channel cleared"""
        if channels is not None:
            self.channels = channels
        self.ids = np.arange(self.n, dtype=np.uint32)
        self.attr = np.zeros((self.channels, self.n), dtype=np.float32)
        self.kappa = [0.0] * MAX_CHANNELS
        self.buoyancy = None                # (channel, beta, reference)
        self.st = self.fb = self.R = self.acc = self.attr_in = self.last_perm = None

    def _settings(self):
        S = Settings()
        S.channels = self.channels
        for c in range(MAX_CHANNELS):
            S.kappa[c] = float(self.kappa[c]) if c < self.channels else 0.0
        b = self.buoyancy
        S.buoy, S.beta, S.reference = (int(b[0]), float(b[1]), float(b[2])) if b is not None else (-1, 0.0, 0.0)
        return S

    def diffuse_pass(self, st=None):
        """the pass alone on the current state (after density()) and self.attr: (attr', fb or None, R, acc); changes nothing"""
        S = self._settings()
        attr = np.ascontiguousarray(self.attr, dtype=np.float32)
        out = np.empty_like(attr)
        fb = np.zeros((self.n, 2), dtype=np.float32) if S.buoy >= 0 else None
        R = np.zeros(self.n, dtype=np.float64)
        acc = np.zeros_like(attr)
        if st is not None:
            st = np.ascontiguousarray(st, dtype=np.float32)
        self.L.dfc_diffuse(self.h, C.addressof(S), attr.ctypes.data, out.ctypes.data, st.ctypes.data if st is not None else None,
                           fb.ctypes.data if fb is not None else None, R.ctypes.data, acc.ctypes.data)
        return out, fb, R, acc

    def sorted_state(self, tick, stable_sort=False):
        """a step up to its sort, the carry included: returns the permutation"""
        self.begin_tick(tick); self.predict(); self.spatial_lookup()
        keys = self.particles()["grid"]
        if stable_sort:
            perm = np.argsort(keys, kind="stable").astype(np.uint32)
            self.L.orc_sort_stable(self.h)
        else:
            perm = O.bitonic_keys(keys)[1]
            self.sort()
        self.ids = self.ids[perm]
        self.attr = np.ascontiguousarray(self.attr[:, perm])
        self.last_perm = perm
        return perm

    def step(self, tick, stable_sort=False):
        perm = self.sorted_state(tick, stable_sort)
        S = self._settings()
        attr = self.attr
        out = np.empty_like(attr)
        st = np.zeros((self.n, 2), dtype=np.float32) if self.surface_tension else None
        fb = np.zeros((self.n, 2), dtype=np.float32) if S.buoy >= 0 else None
        R = np.zeros(self.n, dtype=np.float64)
        acc = np.zeros_like(attr)
        self.L.dfc_finish_step(self.h, C.addressof(S), attr.ctypes.data, out.ctypes.data, st.ctypes.data if st is not None else None,
                               fb.ctypes.data if fb is not None else None, R.ctypes.data, acc.ctypes.data)
        self.attr_in, self.attr, self.st, self.fb, self.R, self.acc = attr, out, st, fb, R, acc
        return perm

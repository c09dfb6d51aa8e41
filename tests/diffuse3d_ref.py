"""ctypes binding of the 3D diffusion / buoyancy checker (tests/diffuse3d_checker.cpp, which includes tests/st3d_checker.cpp and
through it oracle/sph_oracle3d.cpp, both unchanged).  TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by
tests/checker_lib.py: the oracle's flags, a per-user cache outside the tree, keyed by the sources' contents.

Diffuse3Checker steps in one call, so it derives the permutation of a step from the records before it, exactly as
tests/track3d_ref.Track3Checker does (predict_keys in numpy f32, then oracle.bitonic_keys, the network the 3D oracle sorts with);
ids and channels follow it (the carry), then the C side runs the whole step on the carried channels:
sort -> starts -> density -> optional surface tension -> diffusion / buoyancy -> integrate with what the pass hands on."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import checker_lib as CL
from tests import st3d_ref
from tests import track3d_ref as TR

P = C.c_void_p
SOURCES = [CL.here("diffuse3d_checker.cpp")] + st3d_ref.SOURCES
OWN = dict(st3d_ref.OWN)
OWN.update({"df3_step": (None, [P, P, C.c_int, C.c_float, C.c_float] + [P] * 7),
            "df3_set_tick": (None, [P, C.c_uint32]), "df3_tick": (C.c_uint32, [P])})
MAX_CHANNELS = 4
f32 = np.float32


class Settings(C.Structure):
    _fields_ = [("channels", C.c_int), ("kappa", C.c_float * 4), ("buoy", C.c_int), ("beta", C.c_float), ("reference", C.c_float)]


def lib():
    return CL.load("diffuse3d_checker", SOURCES, "orc3_", OWN)


def _p(a):
    return a.ctypes.data if a is not None else None


class Diffuse3Checker(O.OracleSim3D):
    """The 3D oracle with tracking's carry, the opt-in surface tension and the diffusion / buoyancy pass (§28).
    ids (N) and attr (C, N) are in slot order; after a step: st (the ST forces, (N, 3), or None), fb (what the pass handed the
    integrate step, (N, 3), or None without a buoyancy channel), R (float64, N) and acc (f32, C x N) of the pass, attr_in (what the
    pass read)."""

    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0), channels=1, tick_count=0):
        assert 0 <= channels <= MAX_CHANNELS
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc3_create(C.addressof(settings), *[float(x) for x in initial_offset])
        if not self.h:
            raise ValueError("checker: invalid settings")
        self.n = int(self.L.orc3_count(self.h))
        self.surface_tension = None         # (sigma, tau)
        if tick_count:
            self.L.df3_set_tick(self.h, int(tick_count))
        self.reset(channels)

    def reset(self, channels=None):
        """fs3_track_enable: id = current slot, every channel +0.0, every conductivity and the buoyancy channel cleared"""
        if channels is not None:
            self.channels = channels
        self.ids = np.arange(self.n, dtype=np.uint32)
        self.attr = np.zeros((self.channels, self.n), dtype=np.float32)
        self.kappa = [0.0] * MAX_CHANNELS
        self.buoyancy = None                # (channel, beta, reference)
        self.st = self.fb = self.R = self.acc = self.attr_in = self.last_perm = None

    @property
    def tick_count(self):
        return int(self.L.df3_tick(self.h))

    def _settings(self):
        S = Settings()
        S.channels = self.channels
        for c in range(MAX_CHANNELS):
            S.kappa[c] = float(self.kappa[c]) if c < self.channels else 0.0
        b = self.buoyancy
        S.buoy, S.beta, S.reference = (int(b[0]), float(b[1]), float(b[2])) if b is not None else (-1, 0.0, 0.0)
        return S

    def _outputs(self, S):
        out = np.empty_like(self.attr)
        fb = np.zeros((self.n, 3), dtype=np.float32) if S.buoy >= 0 else None
        return out, fb, np.zeros(self.n, dtype=np.float64), np.zeros_like(self.attr)

    def step(self, tick):
        _, keys = TR.predict_keys(self.settings, self.grid_dims, self.particles_view(), tick.delta)
        perm = O.bitonic_keys(keys)[1]
        self.ids = self.ids[perm]
        attr = self.attr = np.ascontiguousarray(self.attr[:, perm], dtype=np.float32)
        S = self._settings()
        out, fb, R, acc = self._outputs(S)
        cfg = self.surface_tension
        st = np.zeros((self.n, 3), dtype=np.float32) if cfg is not None else None
        with np.errstate(all="ignore"):
            self.L.df3_step(self.h, C.addressof(tick), 1 if cfg is not None else 0, float(cfg[0]) if cfg else 0.0,
                            float(cfg[1]) if cfg else 0.0, C.addressof(S), _p(attr), _p(out), _p(st), _p(fb), _p(R), _p(acc))
        self.attr_in, self.attr, self.st, self.fb, self.R, self.acc, self.last_perm = attr, out, st, fb, R, acc, perm
        return perm


def tick_of(fs, tick, **over):
    kw = dict(delta=tick.delta, gravity=(tick.gravity.x, tick.gravity.y, tick.gravity.z), mass=tick.mass,
              pressure_constant=tick.pressure_constant, rest_density=tick.rest_density, damping_factor=tick.damping_factor,
              viscosity_coefficient=tick.viscosity_coefficient)
    kw.update(over)
    return fs.TickSettings3(kw["delta"], fs.Vec3(*kw["gravity"]), kw["mass"], kw["pressure_constant"], kw["rest_density"],
                            kw["damping_factor"], kw["viscosity_coefficient"])

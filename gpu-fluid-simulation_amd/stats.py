"""The record of the fluid diagnostics (include/fluidsim.h "fluid diagnostics") as a Python object: the raw words of
fs_stats / fs3_stats, and what a host derives from them.  Everything here is plain host arithmetic on one record; nothing in the
engine reads it back."""
import math

import numpy as np

from . import _abi

SCALE = 2.0 ** -_abi.FS_STATS_SHIFT


class Stats:
    """One fs_stats record.  The fields of the C struct are attributes: count, nonfinite, dropped, momentum_q, energy_q,
    position_q, density_q (Python ints, the sums of Q(x) = rint(x * 2^20)), speed2_max, density_min, density_max, pos_min, pos_max
    (numpy float32, bit for bit), tick, channels, attr_q, attr_dropped, attr_min, attr_max."""
    dim = 2
    _ctype = _abi.Stats

    def __init__(self, raw):
        self.raw = raw
        ax = "xyz"[:self.dim]
        self.count, self.nonfinite, self.dropped = int(raw.count), int(raw.nonfinite), int(raw.dropped)
        self.momentum_q = tuple(int(x) for x in raw.momentum_q)
        self.position_q = tuple(int(x) for x in raw.position_q)
        self.energy_q, self.density_q = int(raw.energy_q), int(raw.density_q)
        self.speed2_max, self.density_min, self.density_max = (np.float32(x) for x in (raw.speed2_max, raw.density_min, raw.density_max))
        self.pos_min = np.array([getattr(raw.pos_min, a) for a in ax], dtype=np.float32)
        self.pos_max = np.array([getattr(raw.pos_max, a) for a in ax], dtype=np.float32)
        self.tick, self.channels = int(raw.tick), int(raw.channels)
        self.attr_q = tuple(int(x) for x in raw.attr_q)
        self.attr_dropped = tuple(int(x) for x in raw.attr_dropped)
        self.attr_min = np.array(list(raw.attr_min), dtype=np.float32)
        self.attr_max = np.array(list(raw.attr_max), dtype=np.float32)

    @classmethod
    def from_bytes(cls, data):
        """A record from the bytes fs_stats_device left in device memory (e.g. a torch buffer copied to the host)."""
        return cls(cls._ctype.from_buffer_copy(bytes(data)))

    def to_bytes(self):
        return bytes(self.raw)

    # ---- what the words mean
    @property
    def summed(self):
        """The number of records in every sum: the one denominator of every mean."""
        return self.count - self.nonfinite - self.dropped

    @property
    def healthy(self):
        return self.nonfinite == 0

    def momentum(self, mass):
        return tuple(mass * q * SCALE for q in self.momentum_q)

    def kinetic_energy(self, mass):
        return 0.5 * mass * self.energy_q * SCALE

    def potential_energy(self, mass, gravity):
        """-mass * (gravity . sum of positions); gravity has one component per axis"""
        return -mass * sum(float(g) * q for g, q in zip(gravity, self.position_q)) * SCALE

    def centre_of_mass(self):
        """None when no record is in the sums"""
        return tuple(q * SCALE / self.summed for q in self.position_q) if self.summed else None

    def mean_density(self):
        return self.density_q * SCALE / self.summed if self.summed else None

    def max_speed(self):
        """sqrtf(speed2_max) in float32; 0.0 when no finite record contributed"""
        if self.speed2_max == -np.inf:
            return 0.0
        return float(np.sqrt(self.speed2_max, dtype=np.float32))

    def bounding_box(self):
        """(pos_min, pos_max) over the finite records: (+inf, -inf) per axis when there is none"""
        return self.pos_min.copy(), self.pos_max.copy()

    def channel_sum(self, c):
        self._channel(c)
        return self.attr_q[c] * SCALE

    def channel_range(self, c):
        self._channel(c)
        return float(self.attr_min[c]), float(self.attr_max[c])

    def _channel(self, c):
        if not 0 <= c < self.channels:
            raise IndexError(f"channel {c} of {self.channels}")

    def cfl_delta(self, h, courant=0.4, floor=None, ceil=None):
        """A CFL time step from the largest speed: courant * h / max_speed(), clamped to [floor, ceil] where given.  Plain host
        arithmetic on this record: the caller passes the result as the next tick's `delta`; nothing in the engine changes it.
        Returns `ceil` when the largest speed is 0 or no record contributed, and raises ValueError if that happens and no
        `ceil` was given."""
        speed = self.max_speed()
        if speed == 0.0:
            if ceil is None:
                raise ValueError("cfl_delta: the largest speed is 0 (or nothing contributed) and no ceil was given")
            return float(ceil)
        delta = 0.0 if math.isinf(speed) else courant * h / speed
        if ceil is not None:
            delta = min(delta, float(ceil))
        if floor is not None:
            delta = max(delta, float(floor))
        return delta

    def __repr__(self):
        return (f"{type(self).__name__}(count={self.count}, nonfinite={self.nonfinite}, dropped={self.dropped}, tick={self.tick}, "
                f"max_speed={self.max_speed():.6g}, channels={self.channels})")


class Stats3D(Stats):
    """One fs3_stats record: Stats with three components."""
    dim = 3
    _ctype = _abi.Stats3

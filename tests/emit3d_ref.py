"""CPU checker of a 3D particle count that changes at run time (include/fluidsim.h "3D particle count").
TEST INFRASTRUCTURE ONLY: numpy on the unchanged 3D oracle.

The checker holds the records and the tick count.  A step is the 3D oracle at the current count: orc3_create takes any count > 1,
so a count change makes a new oracle with particle_count = count.  The oracle has no tick setter and seeds its coincident-pair
PRNG with the tick, so a fresh oracle is first advanced by the ticks taken so far on its own lattice, then loaded with the
records.  Emission is np.concatenate, the nozzle the header's formula in np.float32 with one operation per line, removal
rec[~kill].  With surface tension the oracle is tests/st3d_ref.ST3Checker at the current count, with a collider every step ends in
tests/collide3d_ref.apply_collider, with tracking the ids and channels follow tests/track3d_ref's permutation of each step, are
appended to on emission (id = next_id++, +0.0 per channel) and compacted on removal."""
import numpy as np

from oracle import oracle as O
from tests import collide3d_ref as CR
from tests import track3d_ref as TR

f32 = np.float32
DTYPE = O.PARTICLE3_DTYPE


def nozzle_records(origin, u, v, velocity, nu, nv):
    """The nu * nv records of fs3_emit_nozzle, in emission order."""
    origin, u, v, velocity = (np.asarray(a, dtype=f32) for a in (origin, u, v, velocity))
    q = np.arange(int(nu) * int(nv), dtype=np.uint32)
    a = q % np.uint32(nu)
    b = q // np.uint32(nu)
    sa = a.astype(f32) + f32(0.5)
    sa = sa - f32(0.5) * f32(nu)
    sb = b.astype(f32) + f32(0.5)
    sb = sb - f32(0.5) * f32(nv)
    rec = np.zeros(q.shape[0], dtype=DTYPE)
    for c in range(3):
        t = sa * u[c]
        t = origin[c] + t
        w = sb * v[c]
        rec["position"][:, c] = t + w
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = velocity
    return rec


def nozzle_positions_f64(origin, u, v, nu, nv):
    """The same positions evaluated in float64 from the f32 inputs (what the f32 formula approximates)."""
    origin, u, v = (np.asarray(a, dtype=f32).astype(np.float64) for a in (origin, u, v))
    q = np.arange(int(nu) * int(nv))
    sa = (q % nu + 0.5) - 0.5 * nu
    sb = (q // nu + 0.5) - 0.5 * nv
    return origin[None, :] + sa[:, None] * u[None, :] + sb[:, None] * v[None, :]


def kill_box(rec, lo, hi):
    """fs3_remove_in_box: lo.a <= position.a <= hi.a on every axis, edges inclusive; a NaN coordinate is never removed."""
    lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    p = rec["position"]
    with np.errstate(invalid="ignore"):
        return np.all((lo[None, :] <= p) & (p <= hi[None, :]), axis=1)


def jittered_scene(fs, n, seed=3, **kw):
    """(checker, tick, settings, offset) of dam_break_3d(n) with jittered velocities."""
    st, off, tick = fs.dam_break_3d(n)
    chk = Emit3Checker(fs, st, off, **kw)
    chk.set_particles(TR.jitter_velocities3(chk.rec, seed))
    return chk, tick, st, off


def random_records(settings, m, seed, vmax=3.0):
    """m records uniform over the inner 90 % of the box, velocities up to vmax per axis."""
    rng = np.random.default_rng(seed)
    half = f32([settings.size.x, settings.size.y, settings.size.z]) * f32(0.45)
    rec = np.zeros(m, dtype=DTYPE)
    rec["position"] = rng.uniform(-half, half, size=(m, 3)).astype(f32)
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = rng.uniform(-vmax, vmax, size=(m, 3)).astype(f32)
    return rec


# The hard places of an emission (tests/test_emit3d_gpu.py: the engine against the checker; tests/test_emit3d.py: each case does
# what it says, on the checker alone).  `rec`: the state the records are emitted into, `settings`: its box.
HARD_CASES = ["coincident", "outside", "on_plus_b", "nan_velocity", "extreme_cells"]


def hard_scene(fs, name):
    """jittered_scene(12^3) for a hard case.  The dam break's block reaches cell (1, 1, 1), the lowest there is; for the case that
    wants a particle alone in the lowest occupied cell the block starts one cell further from the -x wall."""
    chk, tick, st, off = jittered_scene(fs, 12 ** 3)
    if name == "extreme_cells":
        rec = chk.rec.copy()
        rec["position"][:, 0] += f32(st.smoothing_radius)
        rec["predicted_position"] = rec["position"]
        chk.set_particles(rec)
    return chk, tick, st, off


def hard_records(name, rec, settings):
    half = f32([settings.size.x, settings.size.y, settings.size.z]) * f32(0.5)
    if name == "coincident":                  # exactly on an existing particle, with its velocity: the pair's distance stays 0
        out = rec[[rec.shape[0] // 2]].copy()
        out["density"], out["grid"] = 0, 0
        return out
    out = np.zeros(3 if name == "outside" else 2 if name == "extreme_cells" else 1, dtype=DTYPE)
    if name == "outside":                     # beyond the wall on each axis in turn
        out["position"] = np.diag([half[0] + f32(1.0), -half[1] - f32(0.5), half[2] + f32(2.0)]).astype(f32)
        out["velocity"] = f32([[0.5, 0.0, 0.0], [0.0, -0.25, 0.0], [0.0, 0.0, 1.0]])
    elif name == "on_plus_b":
        out["position"] = half
    elif name == "nan_velocity":
        out["position"] = f32([0.05, -0.1, 0.02])
        out["velocity"] = f32([1.0, np.nan, -1.0])
    elif name == "extreme_cells":             # the corners no particle of the dam break comes near: the last and the first cell
        out["position"][0] = half - f32(0.01)
        out["position"][1] = -half + f32(0.01)
    out["predicted_position"] = out["position"]
    return out


class Emit3Checker:
    """records + tick count (+ ids / channels, surface tension, collider).  `st` after a step with surface tension: its forces."""

    def __init__(self, fs, settings, offset=(0.0, 0.0, 0.0), channels=None, surface_tension=None, field=None):
        self.fs, self.base, self.offset = fs, settings, offset
        self.size = (settings.size.x, settings.size.y, settings.size.z)
        self.ticks = 0
        self.cfg, self.field, self.st = surface_tension, field, None
        self._sim = None
        first = O.OracleSim3D(settings, offset)
        self.rec = first.particles()
        self.grid_dims = first.grid_dims
        first.close()
        self.channels = channels
        if channels is not None:
            self.track(channels)

    @property
    def n(self):
        return self.rec.shape[0]

    def settings(self, n):
        b = self.base
        return self.fs.Settings3(int(n), b.particle_spacing, b.smoothing_radius, self.fs.Vec3(b.size.x, b.size.y, b.size.z))

    # ---- tracking --------------------------------------------------------------------------------------------------------
    def track(self, channels):
        self.channels = channels
        self.ids = np.arange(self.n, dtype=np.uint32)
        self.attr = np.zeros((channels, self.n), dtype=f32)
        self.next_id = self.n

    # ---- the count ---------------------------------------------------------------------------------------------------------
    def set_particles(self, rec):
        self.rec = np.ascontiguousarray(rec, dtype=DTYPE).copy()
        self._drop()

    def emit(self, rec):
        rec = np.ascontiguousarray(rec, dtype=DTYPE)
        m = rec.shape[0]
        self.rec = np.concatenate([self.rec, rec])
        if self.channels is not None:
            new = (np.uint64(self.next_id) + np.arange(m, dtype=np.uint64)).astype(np.uint32)      # wraps
            self.ids = np.concatenate([self.ids, new])
            self.attr = np.concatenate([self.attr, np.zeros((self.channels, m), dtype=f32)], axis=1)
            self.next_id = int((self.next_id + m) & 0xFFFFFFFF)
        self._drop()

    def emit_nozzle(self, origin, u, v, velocity, nu, nv):
        self.emit(nozzle_records(origin, u, v, velocity, nu, nv))

    def remove(self, kill):
        kill = np.asarray(kill).astype(bool)
        assert kill.shape[0] == self.n and (~kill).sum() >= 2
        self.rec = self.rec[~kill]
        if self.channels is not None:
            self.ids = self.ids[~kill]
            self.attr = self.attr[:, ~kill]
        self._drop()
        return int(kill.sum())

    def remove_box(self, lo, hi):
        return self.remove(kill_box(self.rec, lo, hi))

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def _drop(self):
        if self._sim is not None:
            self._sim.close()
            self._sim = None

    def _oracle(self, tick):
        """An oracle at the current count whose tick counter is self.ticks, holding self.rec."""
        if self._sim is None:
            st = self.settings(self.n)
            if self.cfg is None:
                sim = O.OracleSim3D(st, self.offset)
            else:
                from tests import st3d_ref
                sim = st3d_ref.ST3Checker(st, self.offset)
            with np.errstate(all="ignore"):
                for _ in range(self.ticks):                 # the tick alignment, on the fresh oracle's own lattice
                    sim.step(tick)
            self._sim = sim
        self._sim.set_particles(self.rec)
        return self._sim

    def step(self, tick):
        sim = self._oracle(tick)
        if self.channels is not None:
            _, keys = TR.predict_keys(self.base, self.grid_dims, self.rec, tick.delta)
            perm = O.bitonic_keys(keys)[1]
            self.ids = self.ids[perm]
            self.attr = self.attr[:, perm]
        with np.errstate(all="ignore"):
            if self.cfg is None:
                sim.step(tick)
            else:
                sim.step(tick, self.cfg)
                self.st = sim.st.copy()
            rec = sim.particles()
            if self.field is not None:
                rec = CR.apply_collider(rec, self.field, self.size, tick.damping_factor)[0]
        self.rec = rec
        self.ticks += 1
        return rec

    def close(self):
        self._drop()

"""CPU checker of a 2D particle count that changes at run time (include/fluidsim.h "2D particle count").
TEST INFRASTRUCTURE ONLY: numpy on the unchanged 2D oracle, in the pattern of tests/emit3d_ref.py.

The checker holds the records, the start_indices table and the tick count.  A step is the 2D oracle at the current count:
orc_create takes any count > 1, so a count change makes a new oracle with particle_count = count, the same quirk flag and the
same sort flavour (stable_sort=True is the counting mode's arrangement).  The oracle has no tick setter and seeds its
coincident-pair PRNG with the tick, so a fresh oracle is first advanced by the ticks taken so far on its own lattice, then
loaded with the records and — the 2D-specific part — with the carried start_indices table: the table is persistent and sized
by the grid, the engine never clears it, and with ref_quirks the stale start of a cell decides which candidates a walk sees.
Emission is np.concatenate, the nozzle the header's formula in np.float32 with one operation per line, removal rec[~kill].
With surface tension the oracle is tests/st_ref.STChecker at the current count; with tracking the step runs pass by pass as
tests/track_ref.TrackChecker does and the ids and channels follow its permutation, are appended to on emission
(id = next_id++, +0.0 per channel) and compacted on removal."""
import numpy as np

from oracle import oracle as O
from tests import track_ref as TR

f32 = np.float32
DTYPE = O.PARTICLE_DTYPE
SORTS = ("bitonic", "counting")


def nozzle_records(origin, u, v, velocity, nu, nv=1):
    """The nu * nv records of fs_emit_nozzle, in emission order."""
    origin, u, v, velocity = (np.asarray(a, dtype=f32) for a in (origin, u, v, velocity))
    q = np.arange(int(nu) * int(nv), dtype=np.uint32)
    a = q % np.uint32(nu)
    b = q // np.uint32(nu)
    sa = a.astype(f32) + f32(0.5)
    sa = sa - f32(0.5) * f32(nu)
    sb = b.astype(f32) + f32(0.5)
    sb = sb - f32(0.5) * f32(nv)
    rec = np.zeros(q.shape[0], dtype=DTYPE)
    for c in range(2):
        t = sa * u[c]
        t = origin[c] + t
        w = sb * v[c]
        rec["position"][:, c] = t + w
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = velocity
    return rec


def nozzle_positions_f64(origin, u, v, nu, nv=1):
    """The same positions evaluated in float64 from the f32 inputs (what the f32 formula approximates)."""
    origin, u, v = (np.asarray(a, dtype=f32).astype(np.float64) for a in (origin, u, v))
    q = np.arange(int(nu) * int(nv))
    sa = (q % nu + 0.5) - 0.5 * nu
    sb = (q // nu + 0.5) - 0.5 * nv
    return origin[None, :] + sa[:, None] * u[None, :] + sb[:, None] * v[None, :]


def kill_box(rec, lo, hi):
    """fs_remove_in_box: lo.a <= position.a <= hi.a on both axes, edges inclusive; a NaN coordinate is never removed."""
    lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    p = rec["position"]
    with np.errstate(invalid="ignore"):
        return np.all((lo[None, :] <= p) & (p <= hi[None, :]), axis=1)


def jittered_scene(fs, n, seed=3, **kw):
    """(checker, tick, settings, offset) of dam_break_2d(n) with jittered velocities; any n > 1."""
    st, off, tick = fs.dam_break_2d(n)
    chk = Emit2Checker(fs, st, off, **kw)
    chk.set_particles(TR.jitter_velocities(chk.rec, seed))
    return chk, tick, st, off


def random_records(settings, m, seed, vmax=3.0):
    """m records uniform over the inner 90 % of the box, velocities up to vmax per axis."""
    rng = np.random.default_rng(seed)
    half = f32([settings.size.x, settings.size.y]) * f32(0.45)
    rec = np.zeros(m, dtype=DTYPE)
    rec["position"] = rng.uniform(-half, half, size=(m, 2)).astype(f32)
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = rng.uniform(-vmax, vmax, size=(m, 2)).astype(f32)
    return rec


# The hard places of an emission (tests/test_emit2d_gpu.py: the engine against the checker; tests/test_emit2d.py: each case does
# what it says, on the checker alone).  tests/hard_states2d.py builds whole scenes for a fixed count; what fits here are single
# records appended to a running scene, so these are written out.  `rec`: the state the records are emitted into.
HARD_CASES = ["coincident", "outside", "on_plus_b", "nan_velocity", "extreme_cells"]


def hard_records(name, rec, settings):
    half = f32([settings.size.x, settings.size.y]) * f32(0.5)
    if name == "coincident":                  # exactly on an existing particle, with its velocity: the pair's distance stays 0
        out = rec[[rec.shape[0] // 2]].copy()
        out["density"], out["grid"] = 0, 0
        return out
    out = np.zeros(2 if name in ("outside", "extreme_cells") else 1, dtype=DTYPE)
    if name == "outside":                     # beyond the wall on each axis in turn
        out["position"] = np.diag([half[0] + f32(1.0), -half[1] - f32(0.5)]).astype(f32)
        out["velocity"] = f32([[0.5, 0.0], [0.0, -0.25]])
    elif name == "on_plus_b":
        out["position"] = half
    elif name == "nan_velocity":
        out["position"] = f32([0.05, -0.1])
        out["velocity"] = f32([1.0, np.nan])
    elif name == "extreme_cells":             # the corners the dam break's block (at -x, +y) leaves empty: the first and the last cell
        out["position"][0] = -half + f32(0.01)
        out["position"][1] = half - f32(0.01)
    out["predicted_position"] = out["position"]
    return out


def step_passes(sim, tick, stable):
    """One oracle step pass by pass, exactly as orc_step / orc_step_stable (tests/track_ref.py); returns the sort's permutation."""
    sim.begin_tick(tick)
    sim.predict()
    sim.spatial_lookup()
    keys = sim.particles()["grid"]
    if stable:
        perm = np.argsort(keys, kind="stable").astype(np.uint32)
        sim.L.orc_sort_stable(sim.h)
    else:
        perm = O.bitonic_keys(keys)[1]
        sim.sort()
    sim.cell_starts()
    sim.density(1)
    sim.move()
    return perm


class Emit2Checker:
    """records + start_indices + tick count (+ ids / channels, surface tension, force field).  `st` after a step with surface
    tension: its forces."""

    def __init__(self, fs, settings, offset=(0.0, 0.0), sort="bitonic", ref_quirks=True, channels=None, surface_tension=False,
                 field=None):
        assert sort in SORTS
        self.fs, self.base, self.offset = fs, settings, offset
        self.sort, self.quirks, self.surface_tension, self.field = sort, ref_quirks, surface_tension, field
        self.ticks = 0
        self.st = None
        self._sim = None
        first = O.OracleSim(settings, offset, ref_quirks=ref_quirks)
        self.rec = first.particles()
        self.start = first.start_indices()
        self.grid_dims = first.grid_dims
        first.close()
        self.channels = None
        if channels is not None:
            self.track(channels)

    @property
    def n(self):
        return self.rec.shape[0]

    def settings(self, n):
        b = self.base
        return self.fs.SimulationSettings(int(n), b.particle_spacing, b.smoothing_radius, (b.size.x, b.size.y),
                                          (b.texture_size.x, b.texture_size.y))

    # ---- tracking --------------------------------------------------------------------------------------------------------
    def track(self, channels):
        assert not self.surface_tension, "the checker steps surface tension in one call: no permutation to follow"
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

    def emit_nozzle(self, origin, u, v, velocity, nu, nv=1):
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
        """An oracle at the current count whose tick counter is self.ticks, holding self.rec and the carried table."""
        if self._sim is None:
            st = self.settings(self.n)
            if self.surface_tension:
                from tests import st_ref
                sim = st_ref.STChecker(st, self.offset, ref_quirks=self.quirks)
            else:
                sim = O.OracleSim(st, self.offset, ref_quirks=self.quirks)
            with np.errstate(all="ignore"):
                for _ in range(self.ticks):                 # the tick alignment, on the fresh oracle's own lattice
                    sim.step(tick, stable_sort=self.sort == "counting")
            assert sim.tick_count == self.ticks
            self._sim = sim
        self._sim.set_particles(self.rec)
        self._sim.start_indices_view()[:] = self.start
        if self.field is not None:
            self._sim.texture_view()[:] = self.field
        return self._sim

    def step(self, tick):
        sim = self._oracle(tick)
        stable = self.sort == "counting"
        with np.errstate(all="ignore"):
            if self.channels is not None:
                perm = step_passes(sim, tick, stable)
                self.ids = self.ids[perm]
                self.attr = self.attr[:, perm]
            elif self.surface_tension:
                sim.step(tick, stable_sort=stable, surface_tension=True)
                self.st = sim.st.copy()
            else:
                sim.step(tick, stable_sort=stable)
        self.rec = sim.particles()
        self.start = sim.start_indices()
        self.ticks += 1
        return self.rec

    def close(self):
        self._drop()

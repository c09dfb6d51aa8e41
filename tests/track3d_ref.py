"""CPU checker of the opt-in 3D particle tracking.  TEST INFRASTRUCTURE ONLY, pure Python on the unchanged
3D oracle.

oracle.OracleSim3D steps in one call, so Track3Checker derives the permutation of a step itself.  From the records before the
step it computes, in numpy f32 (one rounding per operation, as oracle/sph_oracle3d.cpp step3 does):
    pred = position + velocity * delta, clamped to +-size/2 (size/2 * sign where |pred| exceeds it)
    c    = u32_sat(floor((pred + size/2) / h)) + 1 per axis (true division),  key = (cz * grid_h + cy) * grid_w + cx
and takes perm = oracle.bitonic_keys(keys)[1] — the same network template the 3D oracle sorts its records with.  Then
ids = ids[perm], attr = attr[:, perm]: the statement of include/fluidsim.h.  `verify=True` also checks, at every step, that
the oracle's sorted keys are keys[perm] and its predicted positions pred[perm] byte for byte: with all predicted positions
distinct (asserted), the derived permutation is the one the oracle applied."""
import numpy as np

from oracle import oracle as O

MAX_CHANNELS = 4
f = np.float32


def scene3(fs, side, box, spacing=0.1, h=0.2):
    """(settings, offset, tick): a side^3 lattice centred in a box^3 domain, the 3D benchmark scene's tick."""
    st = fs.Settings3(int(side) ** 3, float(spacing), float(h), fs.Vec3(float(box), float(box), float(box)))
    tick = fs.TickSettings3(float(f(1.0) / f(120.0)), fs.Vec3(0.0, 9.81, 0.0), 1.0, 50.0, 0.0, 0.1, 25.0)
    return st, (0.0, 0.0, 0.0), tick


# side -> (box, spacing, velocity range): every scene moves most of its slots in every step (the 2^3 lattice needs the wide
# spacing and the fast particles: at spacing 0.1 it does not move at all)
SCENES = {2: (4.0, 0.5, 30.0), 3: (4.0, 0.1, 3.0), 16: (6.0, 0.1, 3.0), 17: (6.0, 0.1, 3.0), 40: (6.0, 0.1, 3.0),
          64: (8.0, 0.1, 3.0)}


def jitter_velocities3(p, seed, vmax=3.0):
    rng = np.random.default_rng(seed)
    p = p.copy()
    p["velocity"] = rng.uniform(-vmax, vmax, size=p["velocity"].shape).astype(np.float32)
    return p


def u32_sat(x):
    """f32 -> u32, saturating; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    big = x >= f(4294967296.0)
    small = ~(x > f(0.0))
    return np.where(big, np.uint32(0xFFFFFFFF), np.where(big | small, f(0.0), x).astype(np.uint32)).astype(np.uint32)


def cell_xyz(settings, pts):
    """(n, 3) uint32 cell coordinates of (n, 3) f32 points: the oracle's cell_xyz."""
    half = f([settings.size.x, settings.size.y, settings.size.z]) * f(0.5)
    q = (np.asarray(pts, dtype=np.float32) + half) / f(settings.smoothing_radius)
    return u32_sat(np.floor(q)) + np.uint32(1)


def predict_keys(settings, grid_dims, p, delta):
    """(pred[n, 3] f32, keys[n] u32) of a step over the records p with this delta."""
    half = f([settings.size.x, settings.size.y, settings.size.z]) * f(0.5)
    pred = p["position"] + p["velocity"] * f(delta)
    pred = np.where(np.abs(pred) > half, half * np.sign(pred), pred).astype(np.float32)
    c = cell_xyz(settings, pred)
    gw, gh = np.uint32(grid_dims[0]), np.uint32(grid_dims[1])
    with np.errstate(over="ignore"):
        keys = (c[:, 2] * gh + c[:, 1]) * gw + c[:, 0]
    return pred, keys.astype(np.uint32)


class Track3Checker:
    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0), channels=0, verify=False):
        assert 0 <= channels <= MAX_CHANNELS
        self.settings = settings
        self.sim = O.OracleSim3D(settings, initial_offset)
        self.n = self.sim.n
        self.verify = verify
        self.last_perm = None
        self.reset(channels)

    def reset(self, channels=None):
        """fs3_track_enable: id = current slot, every channel +0.0."""
        if channels is not None:
            self.channels = channels
        self.ids = np.arange(self.n, dtype=np.uint32)
        self.attr = np.zeros((self.channels, self.n), dtype=np.float32)

    def particles(self): return self.sim.particles()
    def particles_view(self): return self.sim.particles_view()
    def set_particles(self, p): self.sim.set_particles(p)      # like fs3_upload_particles: ids and channels stay with the slot

    def step(self, tick):
        before = self.sim.particles()
        pred, keys = predict_keys(self.settings, self.sim.grid_dims, before, tick.delta)
        perm = O.bitonic_keys(keys)[1]
        self.sim.step(tick)
        if self.verify:
            after = self.sim.particles_view()
            assert np.unique(pred, axis=0).shape[0] == self.n, "predicted positions repeat: the verification is ambiguous"
            assert np.array_equal(after["grid"], keys[perm]), "the derived keys are not the oracle's"
            assert after["predicted_position"].tobytes() == pred[perm].tobytes(), \
                "the derived permutation is not the one the oracle's sort applied"
        self.ids = self.ids[perm]
        self.attr = self.attr[:, perm]
        self.last_perm = perm
        return perm

    def close(self):
        self.sim.close()


def make_checker3(fs, side, seed, **kw):
    """(checker, tick) of SCENES[side] with its jittered velocities."""
    box, spacing, vmax = SCENES[side]
    st, off, tick = scene3(fs, side, box, spacing)
    chk = Track3Checker(st, off, **kw)
    chk.set_particles(jitter_velocities3(chk.particles(), seed, vmax))
    return chk, tick


def wide_grid_scene(fs, orc, seed=5):
    """(settings, offset, tick, records): 17^3 particles at spacing 1.35 in a 24^3 box (122^3 = 1 815 848 cells), jittered and in a
    random order, so that every 4096-slot tile of the first sort kernel spans more than 2^20 keys (the wide-key hand-over)."""
    st, off, tick = scene3(fs, 17, 24.0, 1.35)
    ref = orc.OracleSim3D(st, off)
    p = jitter_velocities3(ref.particles(), seed)
    ref.close()
    return st, off, tick, p[np.random.default_rng(seed).permutation(p.shape[0])]

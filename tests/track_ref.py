"""CPU checker of the opt-in particle tracking.  TEST INFRASTRUCTURE ONLY, pure Python on the unchanged oracle.

TrackChecker steps oracle.OracleSim pass by pass, exactly as orc_step / orc_step_stable do (begin_tick, predict,
spatial_lookup, the sort, cell_starts, density(1), move).  Between spatial_lookup and the sort it reads the keys and derives
the permutation the sort is about to apply to the records:
  * reference sort: oracle.bitonic_keys(keys)[1], which runs the same bitonic_network template as orc_sort;
  * stable sort:    np.argsort(keys, kind="stable"), the order of std::stable_sort (orc_sort_stable).
Then ids = ids[perm], attr = attr[:, perm]: the statement of include/fluidsim.h.  `verify=True` also checks, at every step,
that before[perm] IS the oracle's sorted array byte for byte, i.e. that the derived permutation is the one the oracle applied."""
import numpy as np

from oracle import oracle as O

MAX_CHANNELS = 4


def jitter_velocities(p, seed):
    """The scene of the tracking tests: velocities drawn uniformly from [-3, 3], so that most slots change occupant every step."""
    rng = np.random.default_rng(seed)
    p = p.copy()
    p["velocity"] = rng.uniform(-3.0, 3.0, size=p["velocity"].shape).astype(np.float32)
    return p


class TrackChecker:
    def __init__(self, settings, initial_offset=(0.0, 0.0), ref_quirks=True, channels=0, verify=False):
        assert 0 <= channels <= MAX_CHANNELS
        self.sim = O.OracleSim(settings, initial_offset, ref_quirks=ref_quirks)
        self.n = self.sim.n
        self.verify = verify
        self.last_perm = None
        self.reset(channels)

    def reset(self, channels=None):
        """fs_track_enable: id = current slot, every channel +0.0."""
        if channels is not None:
            self.channels = channels
        self.ids = np.arange(self.n, dtype=np.uint32)
        self.attr = np.zeros((self.channels, self.n), dtype=np.float32)

    # the oracle's state
    def particles(self): return self.sim.particles()
    def particles_view(self): return self.sim.particles_view()
    def set_particles(self, p): self.sim.set_particles(p)      # like fs_upload_particles: ids and channels stay with the slot
    def start_indices_view(self): return self.sim.start_indices_view()

    def step(self, tick, stable_sort=False):
        s = self.sim
        s.begin_tick(tick)
        s.predict()
        s.spatial_lookup()
        before = s.particles()
        keys = before["grid"]
        if stable_sort:
            perm = np.argsort(keys, kind="stable").astype(np.uint32)
            s.L.orc_sort_stable(s.h)
        else:
            perm = O.bitonic_keys(keys)[1]
            s.sort()
        if self.verify:
            after = s.particles_view()
            assert before[perm].tobytes() == after.tobytes(), "the derived permutation is not the one the oracle's sort applied"
        s.cell_starts()
        s.density(1)
        s.move()
        self.ids = self.ids[perm]
        self.attr = self.attr[:, perm]
        self.last_perm = perm
        return perm

    def close(self):
        self.sim.close()

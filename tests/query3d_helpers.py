"""What the GPU tests of the three 3D queries (sampling, surface extraction, surface rendering) share: the handle they query and
the checker loaded with that handle's own state.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def make_sim(fs, n, mode, seed=7):
    from tests.track_ref import jitter_velocities
    st, off, tick = fs.dam_break_3d(n)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
    sim.upload_particles(jitter_velocities(sim.download_particles(), seed))
    return sim, st, off, tick


def checker_of(checker_class, sim, st, off, mass):
    """-> (a checker of the class loaded with the handle's state, that state), the state asserted finite."""
    p = sim.download_particles()
    for fld in ("position", "predicted_position", "velocity", "density"):
        assert np.isfinite(p[fld]).all(), f"non-finite {fld}"
    chk = checker_class(st, off).load(p, mass)
    assert chk.grid_dims == sim.grid_dims
    return chk, p

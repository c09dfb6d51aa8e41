"""The dense 2D scene shared by the GPU tests of the force pass."""
import numpy as np


def dense_scene(fs, n=8192, seed=17):
    """8192 particles, 3000 of them thrown into about 3 x 3 cells, 64 of those on top of 64 others.  The smallest scene that
    reaches every path of the force pass in one step: the lean mask sweep, the staged and the unstaged chunk sweep (rows
    longer than 32 candidates, tiles that do not fit the LDS stage), both deferred-wave lists, and the coincident pair's
    serial random direction (compute.wgsl:211)."""
    st = fs.SimulationSettings(n, 0.1, 0.2, (40.0, 30.0))
    tick = fs.default_tick_settings(gravity=(0.0, 9.81))
    rng = np.random.default_rng(seed)
    p = fs.reference_lattice(st, (0.0, 0.0))
    idx = rng.choice(n, 3000, replace=False)
    p["position"][idx] = rng.uniform(-0.3, 0.3, size=(3000, 2)).astype(np.float32) + np.float32([5.0, -4.0])
    p["position"][idx[:64]] = p["position"][idx[64:128]]          # coincident pairs
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-0.5, 0.5, size=(n, 2)).astype(np.float32)
    return st, tick, p

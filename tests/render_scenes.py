"""The scenes and views of the renderer's tests (tests/test_render.py on the CPU, tests/test_render_gpu.py on the GPU), and the
tolerances both use.  TEST INFRASTRUCTURE ONLY.  A scene is built the same way on the oracle and on a GPU handle: create,
`prepare(records)` uploaded on both sides (or nothing), `steps` steps of `tick`."""
import numpy as np

import gpu_fluid_simulation_amd as g

EPS23 = 2.0 ** -23

# D_scene: max abs deviation, over all channels, pixels and views of the scene, of the f32 oracle (orc_render) from the float64
# restatement (tests/render_ref.py), as tests/test_render.py measures and prints it; rounded up to two digits.  DESIGN.md §15
# holds the same table.  The GPU tests derive their kernel-vs-oracle bound from these and from nothing the GPU computed.
D_SCENE = {"dam": 1.3e-6, "random": 1.5e-6, "stale": 2.0e-6, "outside": 3.7e-6}


def oracle_bound(scene):
    """Kernel vs oracle: both are in-order f32 sums over the same candidates that differ in expf / logf only (device 1-2 ulp,
    glibc < 1 ulp; sqrt and the divisions are correctly rounded on both sides), so a few times the oracle's own f32 error."""
    return max(4.0 * D_SCENE[scene], 16.0 * EPS23)


class Scene:
    def __init__(self, name, settings, offset, tick, steps, prepare=None, views=()):
        self.name, self.settings, self.offset, self.tick, self.steps, self.prepare = name, settings, offset, tick, steps, prepare
        self.views = dict(views)              # name -> (width, height, world_min, world_max)


def dam(steps=40):
    st, off, tick = g.dam_break_2d(4096)
    sx, sy = float(st.size.x), float(st.size.y)
    views = {"domain": (160, 100, (-sx / 2, -sy / 2), (sx / 2, sy / 2)),
             "zoom": (64, 64, (-6.4, 2.0), (-4.4, 4.0)),
             "129x65": (129, 65, (-sx / 2, -sy / 2), (0.0, sy / 2)),
             "1x300": (1, 300, (-4.0, -sy / 2), (-3.9, sy / 2)),
             "257x1": (257, 1, (-sx / 2, 2.1), (sx / 2, 2.15)),
             "1x1": (1, 1, (-3.3, 1.0), (-3.2, 1.2))}
    return Scene("dam", st, off, tick, steps, None, views)


def _random_records(st, seed):
    """5000 particles over the whole box and past its walls (predict clamps those onto the wall: the last cell column and row are
    occupied), thinning out towards +x so that the image sweeps the whole colour ramp; speeds up to ~4."""
    def prepare(p):
        rng = np.random.default_rng(seed)
        n = p.shape[0]
        sx, sy = float(st.size.x), float(st.size.y)
        p = p.copy()
        x = (rng.uniform(0.0, 1.0, n) ** 2.0 * 1.1 - 0.55) * sx
        y = rng.uniform(-0.55, 0.55, n) * sy
        p["position"] = np.stack([x, y], axis=1).astype(np.float32)
        p["predicted_position"] = p["position"]
        p["velocity"] = rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32)
        return p
    return prepare


def _random_settings():
    st = g.SimulationSettings(5000, 0.1, 0.2, (9.0, 7.0))
    tick = g.default_tick_settings(gravity=(6.0, 9.81))      # towards the +x and +y walls: the last column and row stay occupied
    tick.mass = 1.5
    return st, tick


def random(steps=3):
    st, tick = _random_settings()
    sx, sy = float(st.size.x), float(st.size.y)
    views = {"domain": (160, 100, (-sx / 2, -sy / 2), (sx / 2, sy / 2)),
             "129x65": (129, 65, (-1.0, -sy / 2), (sx / 2, sy / 2))}
    return Scene("random", st, (0.0, 0.0), tick, steps, _random_records(st, 31), views)


def outside(steps=1):
    """The random scene after ONE step (the particles uploaded past the walls sit exactly on them, in the last cell column and row;
    later they bounce back inside) under views that leave the domain."""
    st, tick = _random_settings()
    sx, sy, h = float(st.size.x), float(st.size.y), float(st.smoothing_radius)
    o = 3 * h
    views = {"overhang": (129, 65, (-sx / 2 - o, -sy / 2 - o), (sx / 2 + o, sy / 2 + o)),          # all four sides by 3 cells
             "left": (65, 33, (-sx / 2 - o, -sy / 4), (-sx / 2 + o, sy / 4)),
             "right": (65, 33, (sx / 2 - o, -sy / 4), (sx / 2 + o, sy / 4)),
             "above": (65, 33, (-sx / 4, -sy / 2 - o), (sx / 4, -sy / 2 + o)),
             "below": (65, 33, (-sx / 4, sy / 2 - o), (sx / 4, sy / 2 + o)),
             "beyond": (33, 17, (sx / 2 + 2.0, sy / 2 + 2.0), (sx / 2 + 5.0, sy / 2 + 4.0)),       # entirely outside: all zero
             "far": (160, 100, (-5 * sx, -5 * sy), (5 * sx, 5 * sy)),                               # 10 x the domain
             "flipped": (129, 65, (sx / 2 + o, sy / 2 + o), (-sx / 2 - o, -sy / 2 - o)),
             "point": (9, 7, (-sx / 2 + 0.31, 0.17), (-sx / 2 + 0.31, 0.17))}                       # world_min == world_max
    return Scene("outside", st, (0.0, 0.0), tick, steps, _random_records(st, 31), views)


def stale_prepare(p, seed=9, vel=1.0, jitter=0.025):
    """The jittered dam break of tests/test_parity_gpu.py make_pair(seed=9) (test_poisoned_stale_start)."""
    rng = np.random.default_rng(seed)
    n = p.shape[0]
    p = p.copy()
    p["position"] += rng.uniform(-jitter, jitter, size=(n, 2)).astype(np.float32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-vel, vel, size=(n, 2)).astype(np.float32)
    return p


def stale():
    """One step, then start_indices[first sorted cell] = POISON on both sides, then one more step.  Views: see stale_views()."""
    st, off, tick = g.dam_break_2d(4096)
    return Scene("stale", st, off, tick, 1, stale_prepare, {})


STALE_POISON = (2, 1000)          # hides two particles of the cell; hides the whole cell (min(v, cnt) = cnt)


def stale_views(settings, first_cell, grid_w):
    """A zoomed view centred on the first sorted cell (its 5x5 window and a margin) and the whole domain."""
    sx, sy, h = float(settings.size.x), float(settings.size.y), float(settings.smoothing_radius)
    cx, cy = int(first_cell) % int(grid_w), int(first_cell) // int(grid_w)
    mx, my = (cx - 1 + 0.5) * h - sx / 2, (cy - 1 + 0.5) * h - sy / 2
    return {"zoom": (64, 64, (mx - 0.8, my - 0.8), (mx + 0.8, my + 0.8)),
            "domain": (160, 100, (-sx / 2, -sy / 2), (sx / 2, sy / 2))}


def build_oracle(orc, scene, quirks=True, stable_sort=False):
    ref = orc.OracleSim(scene.settings, scene.offset, ref_quirks=quirks)
    if scene.prepare is not None:
        ref.set_particles(scene.prepare(ref.particles()))
    for _ in range(scene.steps):
        ref.step(scene.tick, stable_sort=stable_sort)
    return ref


def poison(ref, value, sim=None):
    """-> the first sorted cell.  The oracle's table and, if given, the handle's get `value` there."""
    c0 = int(ref.particles()["grid"][0])
    si = ref.start_indices()
    si[c0] = value
    ref.start_indices_view()[:] = si
    if sim is not None:
        sim.upload_start_indices(si)
    return c0

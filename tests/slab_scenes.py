"""Scenes that put the slab step (csrc/engine_slab.hip, kernels_slab.hip, kernels_strip.hip and the n_live / adv_lo / adv_hi /
transposed branches of the density and force kernels) on the inputs the single-domain force pass was pinned on — TEST
INFRASTRUCTURE, plain numpy and the CPU oracle, no GPU.

Every fixed scene is SimulationSettings(8192, 0.1, 0.2, (40, 30)): a 202 x 152 cell grid, the reference lattice centred on the
origin (x, y in +-4.55), random velocities in +-0.5, gravity (0, 9.81).  The column boundaries are explicit (BOUNDS), so the
seams lie at known x: two ranks meet at x = 0 (column 101), three ranks at x = -4 and x = 0 (columns 81 and 101; the middle
rank has two neighbours and 20 columns).  Global column c holds x in [(c - 1) * 0.2 - 20, c * 0.2 - 20).

  cluster_on_seam          3000 particles thrown into +-0.3 around the seam at x = 0 (columns 99 .. 102: both ranks' edge and ghost
                           columns) and 700 into +-0.15 around (-2.1, 2.0) — columns 89 .. 91, interior of the rank left of the seam —
                           so that both launches of an overlapped step have waves k_density pre-registers;
  cluster_with_coincident  the same plus 64 coincident pairs (their random direction is seeded by the slot index, so only runs
                           that share the slot order may be compared);
  late_list_on_both_sides  pairs one ulp of x apart (r2 between 5.6e-15 and 2.3e-13 < 2^-40: the guard that sends a wave to
                           FS_LIST_LATE) with tiny velocities, at three heights in the last edge-zone column, the first interior
                           column next to it (each side of each seam) and a column deep in every rank's interior;
  mouse_and_field_on_seam  mouse_state = 1 on the seam with a radius that covers both ranks, a non-zero force field over a band
                           across the seam (FIELD_BAND);
  obstacle_on_seam         the same particles and mouse with the push-out field of an obstacle image instead (obstacle_image: a bar
                           across the seam), which the GPU tests produce with generate_force_field; two ranks;
  walls_and_bad_values     particles beyond all four walls, a NaN velocity in an edge-zone column and one in the interior of rank 0
                           (a NaN predicted position has cell (1, 1), which rank 0 owns), one velocity of 5000 along y;
  random_settings(case)    test_random_configurations' generator, restricted to grids of at least 24 columns, three ranks.

scene(name, world) returns (settings, tick, particles, bounds, boundary_cols); random_settings(case) the same with world = 3.
boundary_cols is multi.boundary_columns for the largest speed the ORACLE reaches in the STEPS steps the GPU tests run
(tests/test_slab_scenes.py measures it again and compares).

Tolerances.  A slab run differs from the oracle by the order of summation inside a cell and across cells.  That spread is
measured on the oracle alone (test_slab_scenes.py: the input permuted; the x <-> y mirrored problem mirrored back) and must stay
within a quarter of match_and_compare's defaults at steps 1 and 2; a scene that does not fit is listed in TOLERANCES with four
times its measured spread (none does).  The figures measured when the scenes were made are in MEASURED_SPREAD."""
import functools

import numpy as np

import gpu_fluid_simulation_amd as g
from gpu_fluid_simulation_amd import multi

f32 = np.float32
N, SPACING, H, BOX = 8192, 0.1, 0.2, (40.0, 30.0)
GRID = (202, 152)
BLOCK = 256
NBF_TILE = 544                       # csrc/fs_neighbours.h
STEPS = 8                            # steps the GPU tests run; steps 1 and 2 are compared with the oracle
COMPARED = (1, 2)
BOUNDS = {1: [0, 202], 2: [0, 101, 202], 3: [0, 81, 101, 202]}
CLOSE_R2 = 2.0 ** -40
FIXED = ("cluster_on_seam", "late_list_on_both_sides", "mouse_and_field_on_seam", "walls_and_bad_values")
PAIR_HEIGHTS = (-4.217, 0.033, 4.217)


def col_x(c, frac=0.35):
    """x at `frac` of the way through global column c."""
    return (c - 1 + frac) * H - BOX[0] / 2


def zones(bounds, rank, z):
    """(adv_lo, adv_hi) of a rank: its interior columns; the edge zone is the owned columns outside (engine_slab.hip plan_overlap)."""
    lo, hi = bounds[rank], bounds[rank + 1]
    zl, zr = (z if rank > 0 else 0), (z if rank < len(bounds) - 2 else 0)
    if zl + zr >= hi - lo:
        return lo, lo
    return lo + zl, hi - zr


def _base(seed):
    from oracle import oracle as O
    st = g.SimulationSettings(N, SPACING, H, BOX)
    tick = g.default_tick_settings(gravity=(0.0, 9.81))
    ref = O.OracleSim(st, (0.0, 0.0))
    p = ref.particles()
    ref.close()
    # the reference lattice of 8192 particles wraps: 46 of its sites hold two particles.  Coincident pairs draw their direction
    # from the slot index, so the second particle of each goes half a spacing up and to the right
    _, first = np.unique(np.ascontiguousarray(p["position"]).view(np.uint64).reshape(-1), return_index=True)
    dup = np.setdiff1d(np.arange(N), first)
    p["position"][dup] += f32(SPACING / 2)
    rng = np.random.default_rng(seed)
    p["velocity"] = rng.uniform(-0.5, 0.5, size=(N, 2)).astype(f32)
    return st, tick, p, rng


def _finish(p, st):
    bs = f32([st.size.x, st.size.y]) * f32(0.5)
    p["predicted_position"] = np.clip(p["position"], -bs, bs)          # (every step predicts again: nothing reads this)
    p["density"] = 0
    p["grid"] = 0
    return p


def _clusters(p, rng, coincident):
    idx = rng.choice(N, 3700, replace=False)
    p["position"][idx[:3000]] = rng.uniform(-0.3, 0.3, size=(3000, 2)).astype(f32) + f32([0.0, -1.0])
    p["position"][idx[3000:]] = rng.uniform(-0.15, 0.15, size=(700, 2)).astype(f32) + f32([-2.1, 2.0])
    if coincident:
        p["position"][idx[:64]] = p["position"][idx[64:128]]
    return p


# boundary_cols per (scene, world): multi.boundary_columns(vmax, |g|, dt, h, 1) for the oracle's largest speed over STEPS steps
BOUNDARY_COLS = {
    ("cluster_on_seam", 2): 5, ("cluster_on_seam", 3): 5, ("cluster_with_coincident", 2): 5, ("cluster_with_coincident", 3): 5,
    ("late_list_on_both_sides", 2): 4, ("late_list_on_both_sides", 3): 4,
    ("mouse_and_field_on_seam", 2): 4, ("mouse_and_field_on_seam", 3): 4,
    ("walls_and_bad_values", 2): 24, ("walls_and_bad_values", 3): 24, ("obstacle_on_seam", 2): 4,
}
MOUSE_POWER = 4.0                    # the default 150 takes the oracle to 105 units/s at step 2: 4.4 columns per step
FIELD_BAND = (slice(440, 600), slice(480, 545))         # texture rows (y in -2.1 .. 2.6), columns (x in -1.25 .. 1.3)
FIELD_VALUE = (0.35, -0.6)


@functools.lru_cache(maxsize=None)
def band_field():
    field = np.zeros((1024, 1024, 2), dtype=f32)
    field[FIELD_BAND] = FIELD_VALUE
    return field


OBSTACLE_BAR = (slice(500, 600), slice(510, 514))       # texture rows (y in -0.35 .. 2.6), columns: two texels on either side of x = 0


@functools.lru_cache(maxsize=None)
def obstacle_image():
    """u8 [1024, 1024]: 255 but for a bar of zeros four texels wide across the seam at x = 0.  Its push-out field
    (generate_smooth_gradient_field) is non-zero inside the bar only, at most two texels long: 0.16 units, 0.8 columns."""
    img = np.full((1024, 1024), 255, dtype=np.uint8)
    img[OBSTACLE_BAR] = 0
    return img


@functools.lru_cache(maxsize=None)
def obstacle_field():
    from oracle import oracle as O
    return O.gradient_field(obstacle_image())


def pair_columns(world, z):
    """Global columns of the close pairs: per rank the last edge-zone column and the first interior column on each side that has a
    neighbour, and one column deep in the interior."""
    b = BOUNDS[world]
    cols = []
    for r in range(world):
        lo, hi = zones(b, r, z)
        if r > 0:
            cols += [lo - 1, lo]
        if r < world - 1:
            cols += [hi - 1, hi]
        cols.append({(2, 0): 85, (2, 1): 115, (3, 0): 70, (3, 1): 90, (3, 2): 115}[(world, r)])
    return cols


@functools.lru_cache(maxsize=None)
def scene(name, world):
    b = BOUNDS[world]
    z = BOUNDARY_COLS[(name, world)]
    st, tick, p, rng = _base({"cluster_on_seam": 17, "cluster_with_coincident": 17, "late_list_on_both_sides": 23,
                              "mouse_and_field_on_seam": 29, "obstacle_on_seam": 29, "walls_and_bad_values": 31}[name])
    if name in ("cluster_on_seam", "cluster_with_coincident"):
        _clusters(p, rng, name == "cluster_with_coincident")
    elif name == "late_list_on_both_sides":
        cols = pair_columns(world, z)
        pool = iter(rng.choice(N, 2 * 3 * len(cols), replace=False))
        tiny = ((1e-30, -2e-38), (3e-30, 1e-45))
        for c in cols:
            for y in PAIR_HEIGHTS:
                i, j = next(pool), next(pool)
                x = f32(col_x(c))
                p["position"][i] = (x, y)
                p["position"][j] = (np.nextafter(x, f32(np.inf)), y)
                p["velocity"][i], p["velocity"][j] = tiny
    elif name in ("mouse_and_field_on_seam", "obstacle_on_seam"):
        tick = g.default_tick_settings(gravity=(0.0, 9.81), mouse_state=1, mouse_pos=(0.0, 0.5), mouse_force_radius=3.0,
                                       mouse_force_power=MOUSE_POWER)
    elif name == "walls_and_bad_values":
        k = rng.choice(N, 16, replace=False)
        # beyond the four walls (not near the corner cell (1, 1), where the NaN particles' predicted positions are keyed)
        p["position"][k[0]] = (25.0, 3.0); p["position"][k[1]] = (-25.0, 2.0); p["position"][k[2]] = (1.0, 19.0)
        p["position"][k[3]] = (-1.5, -19.0); p["position"][k[4]] = (21.0, -16.0); p["position"][k[5]] = (3.0e9, 0.5)
        # rank 0 owns column 1, the column of a NaN predicted position: one NaN in its edge zone, one in its interior
        lo, hi = zones(b, 0, z)
        # (not in the two halo columns: the particle is keyed to column 1 in step 1 and to its own column in step 2 — a jump no edge
        # zone covers, which an edge-first rank counts in far_halo like any other: DESIGN.md §5)
        p["position"][k[6]] = (col_x(b[1] - 10), 0.51); p["velocity"][k[6]] = (np.nan, 0.25)
        p["position"][k[7]] = (col_x(hi - 6), -0.77); p["velocity"][k[7]] = (np.nan, np.nan)
        # far above the speed clamp, along y: in the first column right of the seam at x = 0
        p["position"][k[8]] = (col_x(101), -2.03); p["velocity"][k[8]] = (0.0, 5000.0)
    else:
        raise KeyError(name)
    return st, tick, _finish(p, st), list(b), z


# ---- random settings -------------------------------------------------------------------------------------------------------
RANDOM_CASES = 6
# seeds of test_random_configurations' generator (1000 + k) whose grid is at least 24 columns wide and whose oracle run keeps
# the travel condition over STEPS steps; boundary_cols per seed as for the fixed scenes
RANDOM_SEEDS = (1002, 1006, 1008, 1011, 1015, 1016)
RANDOM_BOUNDARY_COLS = {1002: 4, 1006: 4, 1008: 4, 1011: 4, 1015: 4, 1016: 4}


def random_config(seed):
    """(settings, tick, offset, field or None, rng): test_random_configurations' draws, in its order.  The velocities and the
    mouse power are scaled to the cell size (a quarter column per step at most to begin with): the halo is two columns."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 6000))
    h = float(rng.choice([0.05, 0.1, 0.2, 0.33, 0.5, 1.0]))
    spacing = float(h * rng.uniform(0.3, 0.9))
    side = np.sqrt(n) * spacing
    size = (float(side * rng.uniform(1.2, 3.0) + 4 * h), float(side * rng.uniform(1.2, 3.0) + 4 * h))
    tex = (int(rng.choice([64, 256, 1024])), int(rng.choice([64, 128, 1024])))
    st = g.SimulationSettings(n, spacing, h, size, tex)
    dt = float(rng.choice([1 / 240, 1 / 120, 1 / 60]))
    radius = float(rng.uniform(0.5, 5))
    tick = g.default_tick_settings(
        delta=dt, gravity=(float(rng.uniform(-5, 5)), float(rng.uniform(-10, 10))),
        mass=float(rng.uniform(0.5, 2.0)), pressure_constant=float(rng.uniform(5, 100)),
        rest_density=float(rng.choice([0.0, 1.0, 20.0])), damping_factor=float(rng.uniform(0.0, 0.9)),
        viscosity_coefficient=float(rng.choice([0.0, 5.0, 25.0])), mouse_state=int(rng.choice([0, 0, 1, -1])),
        mouse_pos=(float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))), mouse_force_radius=radius,
        mouse_force_power=0.02 * h / dt * radius)
    off = (float(rng.uniform(-0.2, 0.2) * size[0]), float(rng.uniform(-0.2, 0.2) * size[1]))
    return st, tick, off, tex, rng


def grid_width(st):
    return int(np.ceil(f32(st.size.x) / f32(st.smoothing_radius))) + 2


@functools.lru_cache(maxsize=None)
def random_settings(case):
    """-> (settings, tick, particles, bounds, field or None, boundary_cols); three ranks of equal particle counts."""
    seed = RANDOM_SEEDS[case]
    return random_scene(seed, case % 2 == 0) + (RANDOM_BOUNDARY_COLS[seed],)


def random_scene(seed, with_field):
    from oracle import oracle as O
    st, tick, off, tex, rng = random_config(seed)
    n, h, dt = st.particle_count, st.smoothing_radius, tick.delta
    ref = O.OracleSim(st, off)
    p = ref.particles()
    ref.close()
    p["position"] += rng.uniform(-0.3, 0.3, size=(n, 2)).astype(f32) * f32(st.particle_spacing)
    p["velocity"] = (rng.standard_normal((n, 2)) * min(2.0, 0.08 * h / dt)).astype(f32)
    field = None
    if with_field:
        field = np.zeros((tex[1], tex[0], 2), dtype=f32)
        field[tex[1] // 3: tex[1] // 2, tex[0] // 4: tex[0] // 2] = (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)))
    gw = grid_width(st)
    cols = multi.global_columns(p["position"][:, 0], st.size.x, h)
    bounds = multi.partition_columns(np.bincount(cols, minlength=gw)[:gw], 3)
    return st, tick, _finish(p, st), bounds, field


def scene_field(name):
    """The force field a fixed scene uploads (None: the zero field)."""
    return band_field() if name == "mouse_and_field_on_seam" else obstacle_field() if name == "obstacle_on_seam" else None


# ---- what the CPU proof and the GPU tests share ------------------------------------------------------------------------------
def predicted_columns(st, tick, p):
    from tests.slab_oracle import predicted_columns as pc
    with np.errstate(invalid="ignore"):
        px = p["position"][:, 0] + p["velocity"][:, 0] * f32(tick.delta)
        col = pc(np.nan_to_num(p["position"], nan=0.0), np.nan_to_num(p["velocity"], nan=0.0), st, tick.delta)
    return np.where(np.isnan(px), 1, col)          # f32 -> u32 of a NaN is 0 (fs_device.h f32_to_u32_sat): column 1


def distinct_positions(p):
    return np.unique(np.ascontiguousarray(p["position"]).view(np.uint64).reshape(-1), return_counts=True)[1]


def step_oracle(st, tick, p, steps, field=None):
    """The oracle's states after 1 .. steps steps (stable sort, quirks off), from `p`."""
    from oracle import oracle as O
    ref = O.OracleSim(st, ref_quirks=False)
    ref.set_particles(p)
    if field is not None:
        ref.texture_view()[:] = field
    out = []
    with np.errstate(all="ignore"):
        for _ in range(steps):
            ref.step(tick, stable_sort=True)
            out.append(ref.particles())
    ref.close()
    return out


def local_order(st, tick, p, bounds, rank, column_major):
    """The local live set of `rank` at the first step, in the rank's cell order: the records whose predicted column is within 2
    of its window (owned, ghosts, near-leavers), sorted stably by the local cell id — u = y, v = local column for a rank with
    column-major ids, the reference layout otherwise.  -> (indices into p in sorted order, keys, (grid_u, grid_v), global columns
    in sorted order)."""
    lo, hi = bounds[rank], bounds[rank + 1]
    col = predicted_columns(st, tick, p)
    with np.errstate(invalid="ignore"):
        py = p["position"][:, 1] + p["velocity"][:, 1] * f32(tick.delta)
        bs = f32(st.size.y) * f32(0.5)
        py = np.where(np.abs(py) > bs, bs * np.sign(py), py).astype(f32)
    row = np.where(np.isnan(py), 1, multi.global_columns(np.nan_to_num(py, nan=0.0), st.size.y, st.smoothing_radius))
    live = np.nonzero((col >= lo - 2) & (col < hi + 2))[0]
    gh = int(np.ceil(f32(st.size.y) / f32(st.smoothing_radius))) + 2
    W = hi - lo + 6
    lc = col[live] - (lo - 3)
    keys = lc * gh + row[live] if column_major else row[live] * W + lc
    order = np.argsort(keys, kind="stable")
    return live[order], keys[order], ((gh, W) if column_major else (W, gh)), col[live][order]


# the tolerances of match_and_compare a scene needs beyond the defaults (rtol 1e-4, atol_vel 1e-3, atol_pos 1e-4 h): none does
TOLERANCES = {}

# Order spread of the oracle at step 2 (step 1 is 5 to 20 times smaller), the larger of the permuted and the mirrored run, as
# (density rel, velocity abs, position abs); a quarter of the defaults is (2.5e-5, 2.5e-4 + 2.5e-5 |v|, 2.5e-5 h).  Cell keys
# identical and the matching a bijection in every run.  tests/test_slab_scenes.py measures them again and prints them.
MEASURED_SPREAD = {
    "cluster_on_seam": (7.5e-6, 7.0e-5, 9.5e-7), "late_list_on_both_sides": (3.1e-6, 2.7e-5, 9.5e-7),
    "mouse_and_field_on_seam": (4.2e-6, 3.9e-5, 9.5e-7), "obstacle_on_seam": (4.2e-6, 3.9e-5, 9.5e-7), "walls_and_bad_values": (3.1e-6, 3.3e-5, 9.5e-7),
    "random 0": (2.6e-6, 1.8e-5, 9.5e-7), "random 1": (1.8e-6, 1.5e-5, 4.8e-7), "random 2": (2.7e-6, 6.7e-6, 2.4e-7),
    "random 3": (1.2e-6, 3.7e-6, 1.2e-7), "random 4": (2.3e-6, 1.4e-5, 4.8e-7), "random 5": (2.0e-6, 1.1e-5, 2.4e-7),
}


def tolerances(name):
    return dict(TOLERANCES.get(name, {}))

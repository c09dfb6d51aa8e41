"""CPU model of the path choice of the 3D density / force kernels (csrc/fs_sweep3.h, kernels_density3d.hip, kernels_force3d.hip), and the scenes built to reach
every path.  Pure numpy.  The model restates, from the SORTED KEYS of a state alone:

  row3_key           id_lo = key + (oz*gh + oy)*gw - 1 (u32 wrap), no row when id_lo >= ncell, id_hi = min(id_lo + 3, ncell),
                     [lo, hi) = [cs[id_lo], cs[id_hi]) with cs[c] = index of the first sorted particle whose key is >= c
  block_tile_bounds  per 256-particle block and sweep row: the first has-lane's lo and the last has-lane's hi of every wave,
                     min / max over the block's waves; the plane fits when all three extents are <= TILE3
  plane_class        per wave: the longest of a lane's three rows, wave-wide: <= 64 / <= 128 / longer

and names the sweep each (wave, plane) takes: mask64, mask128, chunks_staged, chunks_unstaged.  It is always fed the
ORACLE's state (the keys the step sorted), never the engine's: the parity tests assert from it that the scene they compare
really runs the path they are named after.  The constants are compared with the kernel sources in test_3d_paths.py."""
import os

import numpy as np

B3F = 256              # particles per workgroup of k3_density / k3_force
WAVE = 64
TILE3 = 400            # staged candidates per sweep row (B3F == 256)
MASK64, MASK128 = 64, 128
FS_PRED_SLACK = 64     # elements behind the sorted predicted positions the unstaged sweep may read ahead into

PATHS = ("mask64", "mask128", "chunks_staged", "chunks_unstaged")
P_MASK64, P_MASK128, P_STAGED, P_UNSTAGED = range(4)


def row_ranges(keys, dims):
    """[lo, hi) of the nine sweep rows of every particle: two (n, 9) arrays; rows without candidates are (0, 0)."""
    gw, gh, gd = (int(x) for x in dims)
    ncell = gw * gh * gd
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    assert np.all(keys[:-1] <= keys[1:]), "the model wants the sorted keys of a stepped state"
    kc = np.minimum(keys, ncell)                       # k3_reorder: ids past the table count as `ncell`
    lo = np.zeros((keys.shape[0], 9), dtype=np.int64)
    hi = np.zeros_like(lo)
    for j in range(9):
        off = ((j // 3 - 1) * gh + (j % 3 - 1)) * gw - 1
        id_lo = (keys + off) & 0xFFFFFFFF              # u32 arithmetic: a row below the grid wraps to >= ncell
        ok = id_lo < ncell
        id_lo = np.where(ok, id_lo, 0)
        id_hi = np.minimum(id_lo + 3, ncell)
        a = np.searchsorted(kc, id_lo, side="left")
        b = np.searchsorted(kc, id_hi, side="left")
        ok &= a < b
        lo[:, j] = np.where(ok, a, 0)
        hi[:, j] = np.where(ok, b, 0)
    return lo, hi


class PathModel:
    """path[w, p]: which sweep wave w takes in z-plane p (index into PATHS); longest[w, p]: the wave's longest row there;
    lane_longest[i, p]: particle i's longest row; extent[b, p]: the block's largest row extent; live[w]: wave holds particles."""

    def __init__(self, keys, dims, tile=None):
        tile = TILE3 if tile is None else tile
        n = int(np.asarray(keys).shape[0])
        lo, hi = row_ranges(keys, dims)
        nb = (n + B3F - 1) // B3F
        pad = nb * B3F - n
        lo = np.concatenate([lo, np.zeros((pad, 9), np.int64)]).reshape(nb, B3F // WAVE, WAVE, 3, 3)   # block, wave, lane, plane, row
        hi = np.concatenate([hi, np.zeros((pad, 9), np.int64)]).reshape(nb, B3F // WAVE, WAVE, 3, 3)
        has = lo < hi
        big = np.int64(0xFFFFFFFF)
        first = np.argmax(has, axis=2)                                  # first / last has-lane of every wave and row
        last = WAVE - 1 - np.argmax(has[:, :, ::-1], axis=2)
        anyh = has.any(axis=2)
        wmn = np.where(anyh, np.take_along_axis(lo, first[:, :, None], axis=2)[:, :, 0], big)
        wmx = np.where(anyh, np.take_along_axis(hi, last[:, :, None], axis=2)[:, :, 0], 0)
        mn, mx = wmn.min(axis=1), wmx.max(axis=1)                       # (block, plane, row)
        ext = np.where(mx <= mn, 0, mx - mn)
        self.row_extent = ext                                           # (block, plane, row)
        self.extent = ext.max(axis=2)                                   # (block, plane)
        fit = (ext <= tile).all(axis=2)
        lane = (hi - lo).max(axis=4)                                    # (block, wave, lane, plane)
        wave = lane.max(axis=2)                                         # (block, wave, plane)
        path = np.where(wave <= MASK64, P_MASK64, np.where(wave <= MASK128, P_MASK128, P_STAGED))
        path = np.where(fit[:, None, :], path, P_UNSTAGED)
        self.n = n
        self.path = path.reshape(-1, 3)
        self.longest = wave.reshape(-1, 3)
        self.lane_longest = lane.reshape(-1, 3)[:n]
        self.live = np.arange(self.path.shape[0]) * WAVE < n
        self.lo, self.hi = lo.reshape(-1, 9)[:n], hi.reshape(-1, 9)[:n]

    def count(self, name):
        """wave-planes that take `name` and have at least one candidate (a wave of empty rows sweeps nothing)."""
        p = PATHS.index(name)
        return int(((self.path == p) & (self.longest > 0) & self.live[:, None]).sum())

    def waves(self, name):
        p = PATHS.index(name)
        return np.argwhere((self.path == p) & (self.longest > 0) & self.live[:, None])

    def summary(self):
        return {name: self.count(name) for name in PATHS}


# ---------------------------------------------------------------------------------------------------------------------
# Scenes.  Every scene is a hand-placed state of side^3 particles in a roomy box: a FEATURE (over-full cells, strips of
# cells) in an empty part of the domain, and a sparse background of single particles, one per cell at most, in z-planes far
# below / above it, whose count below the feature fixes where the feature starts in the sorted array.  Stiffness, time step
# and velocities are small, so every particle stays in its cell for the compared steps and the asserted row lengths / block
# extents hold after every step (checked on the oracle alone in test_3d_paths.py, and again in the GPU test).
H = 0.25                                         # exactly representable: cell faces are exact, 2^-19 <= h, h*spiky < 2^19
GRID = (40, 24, 24)                              # interior cells; the box is GRID * H


class Scene:
    def __init__(self, name, side, expect, steps=2):
        self.name, self.side, self.n, self.steps = name, side, side ** 3, steps
        self.expect = expect                     # list of checks: callables PathModel -> None (assert inside)
        self.cells = []                          # (cx, cy, cz, count, coincident) in the order given; cell coords are 1-based
        self.tick_over = {}

    def add(self, cx, cy, cz, count, coincident=0):
        self.cells.append((cx, cy, cz, count, coincident))
        return self


def _settings(fs, n):
    size = fs.Vec3(GRID[0] * H, GRID[1] * H, GRID[2] * H)
    return fs.Settings3(int(n), 0.1, H, size)


def scene_tick(fs, **over):
    f = np.float32
    kw = dict(delta=float(f(1) / f(480)), gravity=(0.05, 0.2, -0.03), mass=1.0, pressure_constant=0.02, rest_density=3.0,
              damping_factor=0.4, viscosity_coefficient=2.0)
    kw.update(over)
    return fs.TickSettings3(kw["delta"], fs.Vec3(*kw["gravity"]), kw["mass"], kw["pressure_constant"], kw["rest_density"],
                            kw["damping_factor"], kw["viscosity_coefficient"])


def build_state(fs, scene, seed=0):
    """(settings, tick, particles): the feature cells filled with random points kept 0.2 h off the cell faces, the rest of
    the particles as background singles; velocities small and random; `coincident` particles of a cell share one point."""
    rng = np.random.default_rng(seed)
    st = _settings(fs, scene.n)
    f = np.float32
    half = np.array(GRID, dtype=np.float64) * H / 2
    pos = []
    used = set()
    for cx, cy, cz, count, coin in scene.cells:
        corner = (np.array([cx, cy, cz], dtype=np.float64) - 1) * H - half
        pts = corner + rng.uniform(0.2, 0.8, size=(count, 3)) * H
        if coin:
            pts[1:coin] = pts[0]
        pos.append(pts)
        used.add((cx, cy, cz))
    placed = sum(p.shape[0] for p in pos)
    assert placed <= scene.n, f"{scene.name}: {placed} feature particles, {scene.n} in all"
    zs = sorted({c[2] for c in scene.cells}) or [GRID[2] // 2]
    below = getattr(scene, "below", None)
    rest = scene.n - placed
    below = rest // 2 if below is None else below
    assert below <= rest
    # background singles: every other cell of z-planes at least three cells away from the feature
    def singles(count, planes):
        out = []
        for z in planes:
            for y in range(2, GRID[1], 2):
                for x in range(2, GRID[0], 2):
                    if len(out) == count:
                        return out
                    corner = (np.array([x, y, z], dtype=np.float64) - 1) * H - half
                    out.append(corner + rng.uniform(0.3, 0.7, size=3) * H)
        assert len(out) == count, f"{scene.name}: no room for {count} background particles"
        return out
    lo_planes = [z for z in range(1, zs[0] - 2)]
    hi_planes = [z for z in range(zs[-1] + 3, GRID[2] + 1)]
    if getattr(scene, "feature_last", False):
        assert below == rest
    bg = singles(below, lo_planes) + singles(rest - below, hi_planes)
    if bg:
        pos.append(np.array(bg))
    p = np.zeros(scene.n, dtype=fs.PARTICLE3_DTYPE)
    p["position"] = np.concatenate(pos).astype(f)[rng.permutation(scene.n)]
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-0.02, 0.02, size=(scene.n, 3)).astype(f)
    return st, scene_tick(fs, **scene.tick_over), p


def _has(name, at_least=1, longest=None):
    def check(m):
        w = m.waves(name)
        assert w.shape[0] >= at_least, f"{name}: {w.shape[0]} wave-planes, wanted >= {at_least}; {m.summary()}"
        if longest is not None:
            got = sorted({int(m.longest[a, b]) for a, b in w})
            assert longest in got, f"{name}: no wave whose longest row is {longest} (have {got})"
    return check


def _none(name):
    def check(m):
        assert m.count(name) == 0, f"{name} must not run here; {m.summary()}"
    return check


def _extent(value, path):
    def check(m):
        b, p = np.nonzero(m.extent == value)
        assert b.shape[0], f"no block-plane of extent {value}: {sorted(set(m.extent.ravel().tolist()))[-5:]}"
        ok = False
        for bb, pp in zip(b, p):
            w = m.path[bb * 4:(bb + 1) * 4, pp]
            ok |= bool((w == PATHS.index("chunks_unstaged")).all()) if path == "chunks_unstaged" else \
                bool((w != PATHS.index("chunks_unstaged")).all())
        assert ok, f"the block of extent {value} does not take the {path} side"
    return check


def _mixed_wave(m):
    """a wave whose lanes are of all three classes in one plane: it takes the chunked sweep as a whole"""
    lane = np.concatenate([m.lane_longest, np.zeros((m.path.shape[0] * WAVE - m.n, 3), np.int64)]).reshape(-1, WAVE, 3)
    small = ((lane > 0) & (lane <= MASK64)).any(axis=1)
    mid = ((lane > MASK64) & (lane <= MASK128)).any(axis=1)
    long_ = (lane > MASK128).any(axis=1)
    mixed = small & mid & long_
    assert mixed.any(), "no wave mixes lanes of all three classes"
    assert (m.path[mixed] >= P_STAGED).all()


def _self_bit_words(lo_word, hi_word):
    """lanes whose own particle is candidate d of its own row with d < 64 / d >= 64, in a wave of the two-word path"""
    def check(m):
        d = np.arange(m.n) - m.lo[:, 4]                                  # row 1 of the middle plane
        wave_path = np.repeat(m.path[:, 1], WAVE)[:m.n]
        two = wave_path == P_MASK128
        assert (not hi_word) or (two & (d < 64)).any(), "no own bit in the hi word"
        assert (not lo_word) or (two & (d >= 64)).any(), "no own bit in the lo word"
    return check


def _cluster_rows(rows):
    """the over-full row is row r of a plane for some lane of a two-word wave, for every r in `rows` (r of 0..8)"""
    def check(m):
        length = m.hi - m.lo
        wave_path = np.repeat(m.path, WAVE, axis=0)[:m.n]
        for j in rows:
            ok = (length[:, j] > MASK64) & (wave_path[:, j // 3] == P_MASK128)
            assert ok.any(), f"no lane of a two-word wave has the over-full row as its row {j}"
    return check


def scenes():
    """name -> Scene.  One generator for the oracle-only coverage check and the GPU parity test."""
    out = {}
    cx, cy, cz = 20, 12, 12

    def reg(s):
        out[s.name] = s
        return s
    # ---- row-length edges: one cell of m particles, neighbours in x empty: every lane of the cell has a row of exactly m
    for m, path in ((63, "mask64"), (64, "mask64"), (65, "mask128"), (127, "mask128"), (128, "mask128"), (129, "chunks_staged")):
        checks = [_has(path, longest=m)]
        if path == "mask64":
            checks += [_none("mask128"), _none("chunks_staged"), _none("chunks_unstaged")]
        if path == "mask128":
            checks += [_none("chunks_staged"), _none("chunks_unstaged"), _self_bit_words(m > 64, True)]
        s = reg(Scene(f"row{m}", 8, checks)).add(cx, cy, cz, m)
        s.below = 256 - 30                       # the cell straddles a block boundary: its lanes sit in two workgroups
    # ---- the over-full row seen as row 0, 1, 2 of each plane: probes in the eight (y, z) neighbour cells of the cluster
    for m in (65, 100, 128):
        s = reg(Scene(f"probes{m}", 8, [_has("mask128", longest=m), _cluster_rows(range(9)), _self_bit_words(True, True),
                                        _none("chunks_staged"), _none("chunks_unstaged")]))
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                s.add(cx, cy + dy, cz + dz, m if (dy, dz) == (0, 0) else 3)
        s.below = 100
    # ---- coincident groups: the PRNG stream of a lane must be consumed in candidate order on every path
    reg(Scene("coincident_two_word", 8, [_has("mask128", longest=110), _none("chunks_staged")])).add(cx, cy, cz, 110, coincident=5) \
        .add(cx, cy + 1, cz, 4, coincident=2).below = 70
    reg(Scene("coincident_chunked", 8, [_has("chunks_staged", longest=200)])).add(cx, cy, cz, 200, coincident=6) \
        .add(cx, cy, cz + 1, 4, coincident=3).below = 64
    reg(Scene("coincident_unstaged", 10, [_has("chunks_unstaged")])).add(cx, cy, cz, 450, coincident=7).below = 128
    # ---- block extent: a strip of 32 cells x 8 particles = one whole block, 72 particles in the cell before it, R behind it
    for ext, path in ((399, "staged"), (400, "staged"), (401, "chunks_unstaged")):
        checks = [_extent(ext, path)]
        checks += [_has("chunks_unstaged", at_least=4)] if path == "chunks_unstaged" else \
            [_none("chunks_unstaged"), _has("mask128"), _has("mask64")]
        s = reg(Scene(f"extent{ext}", 10, checks))
        s.add(4, cy, cz, 72)
        for k in range(32):
            s.add(5 + k, cy, cz, 8)
        s.add(37, cy, cz, ext - 72 - 256)
        s.below = 256 - 72                       # the strip starts exactly at a block boundary
    # ---- far above the tile, in the last (partial) block of the array: the read-ahead runs into the slack behind the array
    s = reg(Scene("unstaged_last_block", 10, [_has("chunks_unstaged", at_least=3), lambda m: _last_block_unstaged(m)]))
    s.add(GRID[0], GRID[1], GRID[2], 600)        # the highest cell of the domain: sorted last
    s.feature_last = True
    s.below = 400
    # ---- a wave that mixes lanes of all classes
    s = reg(Scene("mixed_wave", 8, [_mixed_wave, _has("chunks_staged")]))
    for k, c in enumerate((4, 4, 4, 20, 80, 50, 4)):
        s.add(10 + k, cy, cz, c)
    s.below = 128
    return out


def _last_block_unstaged(m):
    assert m.n % B3F != 0, "the scene wants a partial last block"
    last = m.path[-4:][m.live[-4:]]
    assert (last[:, 1] == P_UNSTAGED).all(), "the last block of the array does not take the unstaged sweep"


def oracle_states(fs, orc, scene, seed=0):
    """(settings, tick, start state, [oracle state after step 1, 2, ...])"""
    st, tick, p = build_state(fs, scene, seed)
    ref = orc.OracleSim3D(st)
    ref.set_particles(p)
    after = []
    for _ in range(scene.steps):
        ref.step(tick)
        after.append(ref.particles())
    dims = ref.grid_dims
    ref.close()
    return st, tick, p, after, dims


def check_scene(scene, after, dims):
    for s, state in enumerate(after):
        m = PathModel(state["grid"], dims)
        for chk in scene.expect:
            try:
                chk(m)
            except AssertionError as e:
                raise AssertionError(f"scene {scene.name}, step {s + 1}: {e}") from None


# ---------------------------------------------------------------------------------------------------------------------
# Random configurations (tests and tools/fuzz_parity.py share this generator)
def random_case(fs, case, squeeze=None, vel=None):
    """Seeded random 3D configuration: (settings, offset, tick, mutate(particles) -> particles, description).
    `squeeze`, `vel`: replace the drawn squeeze factor / velocity scale (every other draw stays as it is)."""
    rng = np.random.default_rng(7000 + case)
    side = int(rng.integers(2, 25))
    n = side ** 3
    h = float(rng.choice([0.05, 0.1, 0.2, 0.33, 0.5, 1.0]))
    spacing = float(h * rng.uniform(0.3, 0.9))
    ext = side * spacing
    size = [float(ext * rng.uniform(1.2, 3.0) + 4 * h) for _ in range(3)]
    shape = case % 4
    if shape == 1:                               # a side shorter than h: the grid is three cells thick there
        size[int(rng.integers(0, 3))] = float(h * rng.uniform(0.3, 0.95))
    elif shape == 2:                             # sides that are exact multiples of h (cell gw - 1 exists only for +b)
        size = [float(np.float32(h) * np.float32(np.ceil(s / h))) for s in size]
    elif shape == 3:
        size[int(rng.integers(0, 3))] = float(h * rng.uniform(1.05, 2.5))
    st = fs.Settings3(n, spacing, h, fs.Vec3(*size))
    tick = fs.TickSettings3(float(rng.choice([1 / 240, 1 / 120, 1 / 60])),
                            fs.Vec3(float(rng.uniform(-5, 5)), float(rng.uniform(-10, 10)), float(rng.uniform(-5, 5))),
                            float(rng.uniform(0.5, 2.0)), float(rng.choice([0.0, 5.0, 50.0, 500.0])),
                            float(rng.choice([0.0, 1.0, 20.0, 1000.0])), float(rng.uniform(0.0, 0.9)),
                            float(rng.choice([0.0, 5.0, 25.0])))
    off = tuple(float(rng.uniform(-0.2, 0.2) * s) for s in size)
    drawn = float(rng.choice([1.0, 1.0, 0.5, 0.25]))
    squeeze = drawn if squeeze is None else float(squeeze)
    drawn_vel = float(rng.choice([0.0, 1e-6, 2.0, 100.0]))
    vel = drawn_vel if vel is None else float(vel)

    def mutate(p):
        f = np.float32
        centre = p["position"].mean(axis=0)
        p["position"] = ((p["position"] - centre) * f(squeeze) + centre).astype(f)
        p["position"] += rng.uniform(-0.3, 0.3, size=(n, 3)).astype(f) * f(spacing)
        if case % 4 == 0 and n > 20:
            p["position"][1:int(rng.integers(3, 7))] = p["position"][0]
        p["predicted_position"] = p["position"]
        p["velocity"] = (rng.standard_normal((n, 3)) * vel).astype(f)
        return p
    desc = f"case {case}: side {side}, h {h}, spacing/h {spacing / h:.2f}, size {size}, squeeze {squeeze}, vel {vel}"
    return st, off, tick, mutate, desc


def parse_define(text, name):
    """value of `#define NAME value` (first match) in a source text"""
    import re
    m = re.search(r"^\s*#\s*define\s+" + re.escape(name) + r"\s+([0-9A-Za-z_.+\-]+)", text, re.M)
    assert m, f"#define {name} not found"
    return m.group(1)


def source_text(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "gpu-fluid-simulation_amd", "csrc", name)) as fh:
        return fh.read()


# ---------------------------------------------------------------------------------------------------------------------
# State builders of tests/test_3d_paths_gpu.py (operand guards, walls, grid edges), kept here so that the feature tests run
# the same states: they need the oracle for the initial lattice and no GPU.
f32 = np.float32


def pair3_state(fs, orc, side, h=0.2, spacing=0.1, seed=21, vel=1.0, jitter=0.25, room=2.0, **tick_over):
    """centred lattice (even side: the origin lies inside the fluid) in a roomy box, jittered, with velocities:
    (oracle, settings, tick, particles)"""
    n = side ** 3
    ext = side * spacing
    st = fs.Settings3(n, float(spacing), float(h), fs.Vec3(*[float(ext * room + 4 * h)] * 3))
    kw = dict(delta=float(f32(1) / f32(120)), gravity=(0.3, 9.81, -0.2), mass=1.0, pressure_constant=50.0, rest_density=0.0,
              damping_factor=0.1, viscosity_coefficient=25.0)
    kw.update(tick_over)
    tick = fs.TickSettings3(kw["delta"], fs.Vec3(*kw["gravity"]), kw["mass"], kw["pressure_constant"], kw["rest_density"],
                            kw["damping_factor"], kw["viscosity_coefficient"])
    ref = orc.OracleSim3D(st)
    p = ref.particles()
    if seed is not None:
        rng = np.random.default_rng(seed)
        p["position"] += rng.uniform(-jitter, jitter, size=(n, 3)).astype(f32) * f32(spacing)
        p["velocity"] = rng.uniform(-vel, vel, size=(n, 3)).astype(f32)
    p["predicted_position"] = p["position"]
    return ref, st, tick, p


GUARD_CASES = ["tiny_offsets", "tiny_velocities", "huge_velocities", "inf_velocity", "zero_aligned", "huge_pressure",
               "near_zero_coordinates", "small_operands_on_the_fast_path", "density_across_2p20", "pressure_across_2p39",
               "distance_across_2m20", "unsafe_next_to_safe"]


def guard_overrides(case):
    """tick settings a guard case replaces"""
    over = {}
    if case == "huge_pressure":
        over = dict(pressure_constant=3.0e33)
    elif case == "density_across_2p20":            # interior ~1.5e6 > 2^20 > surface and corner densities
        over = dict(mass=1500.0)
    elif case == "pressure_across_2p39":           # |k rho| from ~1e11 at the corners to ~1e12 inside: 2^39 = 5.5e11 between
        over = dict(pressure_constant=1.0e9)
    return over


def guard_state(orc, st, p, case):
    """the particles of pair3_state(side 12) with the operands of one guard case put in"""
    n = p.shape[0]
    near = np.argsort(np.abs(p["position"]).max(axis=1))[:16]            # the particles around the origin
    if case == "tiny_offsets":                     # |o| from 2^-149 to ~2^-20 around the origin (r2 below 2^-40 too)
        p["position"][near[0]] = 0
        for k, d in enumerate([1e-45, 1e-40, 1e-30, 1e-19, 3e-13, 1e-7]):
            p["position"][near[1 + k]] = f32(d) * np.array([1, 0 if k % 2 else 1, 0 if k % 3 else -1], f32)
    elif case == "tiny_velocities":                # differences far below 2^-76 and denormal
        p["velocity"][:] = 0
        p["velocity"][::3] = (1e-30, -2e-38, 3e-31)
        p["velocity"][1::3] = (3e-30, 1e-45, -1e-44)
    elif case == "huge_velocities":                # differences above 2^60 (clamped only after the force pass)
        p["velocity"][50] = (3e30, -3e30, 1e29)
        p["velocity"][51] = (-2e25, 1e19, 7e18)     # 2^59 = 5.8e17 < 7e18
        p["velocity"][52] = (5e17, -5.7e17, 5.9e17)  # around 2^59 itself
    elif case == "inf_velocity":
        p["velocity"][60] = (np.inf, 0.0, 1.0)
        p["velocity"][61] = (-np.inf, np.nan, 0.0)
        p["velocity"][62] = (0.0, 1.0, np.inf)
    elif case == "zero_aligned":                   # exact zeros in every numerator: the lattice, equal velocities
        p["position"] = orc.OracleSim3D(st).particles()["position"]
        p["velocity"][:] = (0.25, -0.5, 0.125)
    elif case == "small_operands_on_the_fast_path":     # numerators between 2^-76 and 2^-60: exact quotients by reciprocal
        tiny = f32(2.0 ** -53)
        j = np.arange(n, dtype=f32) % 7
        p["velocity"][:, 0] = tiny * (f32(1) + j * f32(2.0 ** -22))
        p["velocity"][:, 1] = tiny * (f32(3) - j * f32(2.0 ** -21))
        p["velocity"][:, 2] = tiny * (f32(2) + j * f32(2.0 ** -20))
        col = np.nonzero(np.abs(p["position"][:, 2]) < 0.1)[0][:40]      # a slab moved onto z ~ 2^-53
        p["position"][col, 2] = tiny * (f32(1) + (np.arange(len(col)) % 5).astype(f32) * f32(2.0 ** -22))
    elif case == "near_zero_coordinates":
        rng = np.random.default_rng(5)
        p["position"][near] = (rng.standard_normal((16, 3)) * 1e-22).astype(f32)
    elif case == "distance_across_2m20":           # pair distances 2^-21 .. 2^-19, r2 on both sides of 2^-40 and at it
        e = f32(2.0 ** -20)
        p["position"][near[0]] = 0
        for k, d in enumerate([e / 2, np.nextafter(e, f32(0)), e, np.nextafter(e, f32(1)), e * 2]):
            q = np.zeros(3, f32); q[k % 3] = d if k % 2 else -d
            p["position"][near[1 + k]] = q
        p["position"][near[6]] = (e * f32(0.6), e * f32(0.8), 0)         # |o|^2 rounds next to 2^-40 off the axes
    elif case == "unsafe_next_to_safe":            # the sign of vel_s.w is per particle, the decision per pair
        p["velocity"][near[0]] = (1e-30, 0.5, -0.5)                      # one unsafe component, safe neighbours all round
        p["velocity"][near[3]] = (0.5, 2e-17, 0.5)                       # just below 2^-53 = 1.1e-16
        p["velocity"][near[5]] = (0.5, 0.5, 1.2e-16)                     # just above it: safe
        p["position"][near[7], 1] = 3e-20                                # an unsafe coordinate
        p["velocity"][near[9]] = (np.nan, 0.0, 0.0)
    return p


RADII = [0.05, 0.1, 0.2, 0.33, 0.5, 1.0]


def radius_state(fs, orc, h):
    """the state of test_3d_smoothing_radii_with_the_shared_path_on_and_off: (oracle, settings, tick, particles)"""
    return pair3_state(fs, orc, 12, h=h, spacing=h / 2, seed=int(h * 100), rest_density=1.0)


def box_settings(fs, n, size, h=0.2):
    return fs.Settings3(n, 0.1, h, fs.Vec3(*[float(s) for s in size]))


def box_tick(fs, **over):
    kw = dict(delta=float(f32(1) / f32(120)), gravity=(0.3, 9.81, -0.2), mass=1.0, pressure_constant=50.0, rest_density=1.0,
              damping_factor=0.3, viscosity_coefficient=5.0)
    kw.update(over)
    return fs.TickSettings3(kw["delta"], fs.Vec3(*kw["gravity"]), kw["mass"], kw["pressure_constant"], kw["rest_density"],
                            kw["damping_factor"], kw["viscosity_coefficient"])


def faces_state(fs, orc, exact_multiple):
    """uploads exactly at +b and -b: 6 faces, 12 edges, 8 corners (26 sign patterns), far outside the box, and the rest of
    the particles near them: (settings, tick, particles)"""
    size = (2.0, 1.5, 1.25) if exact_multiple else (2.1, 1.55, 1.27)      # h = 0.25: 8 x 6 x 5 cells exactly
    n = 8 ** 3
    st = box_settings(fs, n, size, h=0.25)
    tick = box_tick(fs)
    ref = orc.OracleSim3D(st)
    b = np.array([f32(s) * f32(0.5) for s in size], dtype=f32)
    rng = np.random.default_rng(11)
    p = ref.particles()
    ref.close()
    signs = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    k = 0
    for rep in range(4):                           # each pattern: on the wall; twice near it (neighbours); far outside
        for sg in signs:
            s = np.array(sg, dtype=f32)
            inner = rng.uniform(-0.5, 0.5, size=3).astype(f32) * b
            on = np.where(s != 0, s * b, inner).astype(f32)
            if rep == 0:
                p["position"][k] = on
            elif rep == 3:
                p["position"][k] = np.where(s != 0, s * b * f32(1e3 if k % 2 else 1.0001), inner)
            else:
                p["position"][k] = np.where(s != 0, s * (b - f32(0.07) * rng.uniform(0, 1, 3).astype(f32)), inner)
            k += 1
    p["velocity"] = rng.uniform(-1, 1, size=(n, 3)).astype(f32)
    for j, sg in enumerate(signs):                 # the particles on the walls move outwards: predicted exactly at +-b
        s = np.array(sg, dtype=f32)
        p["velocity"][j] = np.where(s != 0, s * np.abs(p["velocity"][j]), p["velocity"][j])
    p["predicted_position"] = p["position"]
    return st, tick, p


WALLS = [(a, s) for a in range(3) for s in (-1, 1)]


def wall_state(fs, orc, axis, sign):
    """gravity and initial velocity towards one wall: (oracle, settings, tick, particles)"""
    g = [0.0, 0.0, 0.0]; g[axis] = 60.0 * sign
    ref, st, tick, p = pair3_state(fs, orc, 8, seed=axis * 2 + (sign > 0), room=1.3, gravity=tuple(g), rest_density=1.0,
                                   damping_factor=0.5)
    p["velocity"][:, axis] += f32(25.0 * sign)
    p["predicted_position"] = p["position"]
    return ref, st, tick, p


THIN_SIZES = [(0.15, 0.15, 0.15), (0.15, 2.0, 1.0), (1.0, 0.1, 2.0), (2.0, 1.0, 0.19), (0.2, 0.2, 3.0)]


def thin_state(fs, orc, size):
    """a 3 x 3 x 3 grid (the whole domain one cell) and grids three cells thick along one axis: (settings, tick, particles)"""
    n = 6 ** 3
    st = box_settings(fs, n, size)
    tick = box_tick(fs, pressure_constant=5.0)
    ref = orc.OracleSim3D(st)
    rng = np.random.default_rng(int(sum(size) * 100))
    p = ref.particles()
    ref.close()
    half = np.array(size, dtype=f32) * f32(0.5)
    p["position"] = (rng.uniform(-1, 1, size=(n, 3)) * half).astype(f32)
    p["velocity"] = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(f32)
    p["predicted_position"] = p["position"]
    return st, tick, p

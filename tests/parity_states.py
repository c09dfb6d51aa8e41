"""The states of the plain 2D parity tests (tests/test_parity_gpu.py) that other files run as well — TEST INFRASTRUCTURE, plain
numpy, no GPU.  One definition of each: tests/test_parity_gpu.py runs them against the oracle, tests/features2d.py runs them
with the opt-in surface-tension pass against its checker.  Every builder returns fresh arrays."""
import numpy as np

f32 = np.float32
GUARD_CASES = ["tiny_offsets", "tiny_velocities", "huge_velocities", "inf_velocity", "zero_aligned", "huge_pressure",
               "near_zero_coordinates", "small_operands_on_the_fast_path"]
RANDOM_CASES = 16
RADII = [0.05, 0.1, 0.2, 0.33, 0.5, 1.0]
RAGGED_DAM_N = [2, 3, 5, 257, 5000, 4097]
RAGGED_BOX = (9.0, 7.0)


def pair_settings(fs, n, size=None, off=None, **tick_over):
    """(settings, offset, tick) of make_pair: the dam break of n particles, or n particles in a `size` box under gravity"""
    if size is None:
        st, off_, tick = fs.dam_break_2d(n)
        off = off_ if off is None else off
    else:
        st = fs.SimulationSettings(n, 0.1, 0.2, size)
        tick = fs.default_tick_settings(gravity=(0.0, 9.81))
        off = off or (0.0, 0.0)
    for k, v in tick_over.items():
        if k in ("gravity", "mouse_pos"):
            v = fs.Vec2(*v)
        setattr(tick, k, v)
    return st, off, tick


def jitter(p, seed, vel=1.0, jitter=0.025):
    """the lattice `p` moved by up to `jitter` per coordinate, velocities up to `vel` (in place; returns p)"""
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    p["position"] += rng.uniform(-jitter, jitter, size=(n, 2)).astype(np.float32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-vel, vel, size=(n, 2)).astype(np.float32)
    return p


def lattice(orc, st, off):
    ref = orc.OracleSim(st, off)
    p = ref.particles()
    ref.close()
    return p


def jittered_dam_break(fs, orc, n, seed, **kw):
    """(settings, offset, tick, records): make_pair(fs, orc, n, seed=seed)'s state"""
    st, off, tick = pair_settings(fs, n, **kw)
    return st, off, tick, jitter(lattice(orc, st, off), seed)


# ---- test_force_quotient_guards ---------------------------------------------------------------------------------------------
GUARD_SEED = 21


def guard_overrides(case):
    if case == "huge_pressure":
        return dict(pressure_constant=3.0e33)              # dx*kern*shared beyond 2^60, some overflow to inf
    return {}


def guard_state(orc, st, p, case):
    """operands at and beyond the guards of the shared-denominator quotients: `p` is the jittered 4096 dam break"""
    n = p.shape[0]
    base = p["position"][100].copy()
    if case == "tiny_offsets":                             # |ox|, |oy| from 2^-149 up to ~2^-20 (r2 below 2^-40 too)
        for k, d in enumerate([1e-45, 1e-40, 1e-30, 1e-19, 3e-13, 1e-7]):
            p["position"][101 + k] = base + np.float32(d) * np.array([1, 0 if k % 2 else 1], np.float32)
        p["position"][100:108] -= base                     # around the origin, where such offsets are representable
    elif case == "tiny_velocities":                        # velocity differences far below 2^-60 and denormal
        p["velocity"][:] = 0
        p["velocity"][::3] = (1e-30, -2e-38)
        p["velocity"][1::3] = (3e-30, 1e-45)
    elif case == "huge_velocities":                        # differences above 2^60 (clamped only after the force pass)
        p["velocity"][50] = (3e30, -3e30)
        p["velocity"][51] = (-2e25, 1e19)
    elif case == "inf_velocity":
        p["velocity"][60] = (np.inf, 0.0)
        p["velocity"][61] = (-np.inf, np.nan)
    elif case == "zero_aligned":                           # exact zeros in every numerator: lattice, equal velocities
        q = orc.OracleSim(st, (0.0, 0.0)).particles()
        p["position"] = q["position"]
        p["velocity"][:] = (0.25, -0.5)
    elif case == "small_operands_on_the_fast_path":        # numerators between 2^-76 and 2^-60: exact quotients by reciprocal
        f = np.float32
        tiny = f(2.0 ** -53)
        j = np.arange(n, dtype=np.float32) % 7
        p["velocity"][:, 0] = tiny * (f(1) + j * f(2.0 ** -22))      # differences are multiples of 2^-75
        p["velocity"][:, 1] = tiny * (f(3) - j * f(2.0 ** -21))
        col = np.isclose(p["position"][:, 0], p["position"][np.argmin(np.abs(p["position"][:, 0])), 0])
        k = np.nonzero(col)[0][:40]                        # one lattice column moved onto x ~ 2^-53: offsets of 2^-75 .. 2^-73
        p["position"][k, 0] = tiny * (f(1) + (np.arange(len(k)) % 5).astype(np.float32) * f(2.0 ** -22))
    elif case == "near_zero_coordinates":                  # positions within 1e-20 of the origin: tiny but nonzero offsets
        rng = np.random.default_rng(5)
        idx = np.arange(200, 232)
        p["position"][idx] = (rng.standard_normal((32, 2)) * 1e-22).astype(np.float32)
    p["predicted_position"] = p["position"]
    return p


# ---- test_nan_reset_speed_clamp_and_walls, test_coincident_particles_prng_path, test_mouse_and_force_field -------------------
NAN_CLAMP = dict(seed=6, vel=40.0)
COINCIDENT = dict(seed=4)
MOUSE_FIELD = dict(seed=3, mouse_state=-1, mouse_pos=(-3.0, 2.5))


def nan_clamp_state(p):
    p["velocity"][7] = (np.nan, 1.0)
    p["velocity"][11] = (9000.0, -9000.0)
    p["position"][13] = (1e6, -1e6)        # outside the box: clamps in predict and at the walls
    p["predicted_position"][13] = p["position"][13]
    return p


def coincident_state(p):
    p["position"][1:6] = p["position"][0]
    p["predicted_position"][1:6] = p["position"][0]
    p["velocity"][:6] = 0
    return p


def mouse_field():
    field = np.zeros((1024, 1024, 2), dtype=np.float32)
    field[500:900, 0:600] = (0.25, -0.75)
    return field


# ---- test_random_configurations ---------------------------------------------------------------------------------------------
def random_configuration(fs, orc, case):
    """Seeded random settings (smoothing radius, spacing, domain aspect, dt, mass, stiffness, rest density, damping, viscosity,
    gravity sign, texture size, mouse) and particle counts.  Returns (settings, offset, tick, runs); runs = one
    (sort name, records, field or None) per sort mode, drawn in that order from the case's one random stream."""
    rng = np.random.default_rng(1000 + case)
    n = int(rng.integers(2, 6000))
    h = float(rng.choice([0.05, 0.1, 0.2, 0.33, 0.5, 1.0]))
    spacing = float(h * rng.uniform(0.3, 0.9))
    side = np.sqrt(n) * spacing
    size = (float(side * rng.uniform(1.2, 3.0) + 4 * h), float(side * rng.uniform(1.2, 3.0) + 4 * h))
    tex = (int(rng.choice([64, 256, 1024])), int(rng.choice([64, 128, 1024])))
    st = fs.SimulationSettings(n, spacing, h, size, tex)
    tick = fs.default_tick_settings(
        delta=float(rng.choice([1 / 240, 1 / 120, 1 / 60])), gravity=(float(rng.uniform(-5, 5)), float(rng.uniform(-10, 10))),
        mass=float(rng.uniform(0.5, 2.0)), pressure_constant=float(rng.uniform(5, 100)),
        rest_density=float(rng.choice([0.0, 1.0, 20.0])), damping_factor=float(rng.uniform(0.0, 0.9)),
        viscosity_coefficient=float(rng.choice([0.0, 5.0, 25.0])), mouse_state=int(rng.choice([0, 0, 1, -1])),
        mouse_pos=(float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))), mouse_force_radius=float(rng.uniform(0.5, 5)))
    off = (float(rng.uniform(-0.2, 0.2) * size[0]), float(rng.uniform(-0.2, 0.2) * size[1]))
    runs = []
    for sort in ("bitonic", "counting"):
        p = lattice(orc, st, off)
        p["position"] += rng.uniform(-0.3, 0.3, size=(n, 2)).astype(np.float32) * np.float32(spacing)
        p["predicted_position"] = p["position"]
        p["velocity"] = (rng.standard_normal((n, 2)) * 2.0).astype(np.float32)
        field = None
        if case % 3 == 0:
            field = np.zeros((tex[1], tex[0], 2), dtype=np.float32)
            field[tex[1] // 3: tex[1] // 2, tex[0] // 4: tex[0] // 2] = (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)))
        runs.append((sort, p, field))
    return st, off, tick, runs


# ---- tests/test_surface_tension_gpu.py::test_other_math_modes_within_contract ------------------------------------------------
def disordered_dam_break(fs, n=16384, seed=11):
    """the dam break of n particles, jittered by 0.02 with velocities up to 1: (settings, offset, tick, records)"""
    from oracle import oracle as O
    st, off, tick = fs.dam_break_2d(n)
    p = lattice(O, st, off)
    rng = np.random.default_rng(seed)
    p["position"] += rng.uniform(-0.02, 0.02, size=p["position"].shape).astype(np.float32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-1, 1, size=p["velocity"].shape).astype(np.float32)
    return st, off, tick, p

"""Scenes for the loops of the 2D force walk, its scan and the density row loop (csrc/fs_force_sweep.h, kernels_force_quad.inc,
fs_force_pair.h force_terms_shared, kernels_density.hip DensityTerms::row) — TEST INFRASTRUCTURE, plain numpy, n <= 4096.

  rim(h)            a square lattice at rest with spacing h along both axes: axis neighbours sit ON the rim of the kernel support
                    (r2 == sqr_radius: admitted by the scan, dst == h, kern == -0; or one ulp outside), diagonals outside.  For a
                    power-of-two h every spacing is exact; for the default h = 0.2f the products k * h round, so the spacings are
                    h and its neighbours one ulp either side.  No velocity and no gravity in step 1, so that step sees the lattice.
  exit_rows()       lanes whose sweep rows hold 0, 1, 3, 4, 5, 31 and 32 candidates: every trip count of the four-wide scan.
  exit_waves()      wave 0: one lane with >= 20 in-radius neighbours, its other 63 lanes none; wave 1: no neighbour at all.
  dam(n)            the jittered dam break of n = 64, 65, 255, 256, 257 particles: one wave, one lane more, one block, one more.
  density_trips()   lanes whose rows hold 0 ... 9 candidates in each of the three sweep rows (the own row at least the lane itself):
                    every residue of the density pass's four-wide row loop and of its tail.
  guard_tiny_dst()  a pair a little more than 2^-20 apart: the lower end of the shared-reciprocal path's proven range.
  guard_coincident() coincident particles: the PRNG direction, which only the general kernel evaluates.

Every builder returns (settings, ticks, records): one tick-settings object per step (STEPS of them).  `row_lengths` and `pair_r2`
are the models tests/test_walk_diet_scenes.py applies to the ORACLE's state to prove the scenes are what they are named."""
import functools

import numpy as np

import gpu_fluid_simulation_amd as g
from tests import csort_scenes as CS
from tests import parity_states as PS
from tests import prologue_scenes as S

f32 = np.float32
STEPS = 3
H = CS.H
WIDE_BOX = (112.0, 12.0)             # 562 x 62 cells of 0.2
RIM_SIDE = 64                        # 64 x 64 = 4096 particles
RIM_H = {"pow2": 0.25, "default": 0.2}
EXIT_LENGTHS = (0, 1, 3, 4, 5, 31, 32)
TRIP_LENGTHS = tuple(range(10))
DAM_N = (64, 65, 255, 256, 257)
BUSY_NEIGHBOURS = 24


def _ticks(first=None):
    t = [g.default_tick_settings(gravity=(0.0, 9.81)) for _ in range(STEPS)]
    if first is not None:
        t[0] = first
    return t


def _place(p, k, st, cell, frac):
    """particle k at the fraction `frac` (per axis, of the cell size) inside cell (cx, cy)"""
    p["position"][k] = (CS.cell_origin(st, *cell) + H * np.asarray(frac, dtype=np.float64)).astype(f32)


def _finish(p, vel=0.0, seed=0):
    n = p.shape[0]
    p["predicted_position"] = p["position"]
    p["velocity"] = np.random.default_rng(seed).uniform(-vel, vel, size=(n, 2)).astype(f32) if vel else 0
    return p


# ---- rim pairs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rim(kind):
    h = f32(RIM_H[kind])
    n = RIM_SIDE * RIM_SIDE
    side = float(h) * (RIM_SIDE + 8)
    st = g.SimulationSettings(n, float(h), float(h), (side, side))
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    k = np.arange(n)
    # (index - 32) * h in f32: exact for h = 0.25; for h = 0.2f the products round and neighbouring ones differ by h or by h +- 1 ulp
    p["position"][:, 0] = (k % RIM_SIDE - RIM_SIDE // 2).astype(f32) * h
    p["position"][:, 1] = (k // RIM_SIDE - RIM_SIDE // 2).astype(f32) * h
    return st, _ticks(first=g.default_tick_settings(gravity=(0.0, 0.0))), _finish(p)


# ---- loop exits ---------------------------------------------------------------------------------------------------------------
def _probes(lengths_low, lengths_own, lengths_up, seed):
    """One probe lane per entry: alone in its cell (column 6 + 6 j of row 30) but for lengths_own[j] - 1 companions in the cell, with
    lengths_low[j] / lengths_up[j] particles in the three cells below / above it.  Probes are six columns apart: nothing else is
    in their rows.  -> (settings, records, probe indices)"""
    rng = np.random.default_rng(seed)
    cells, probes = [], []
    for j, (lo, own, up) in enumerate(zip(lengths_low, lengths_own, lengths_up)):
        cx, cy = 6 + 6 * j, 30
        probes.append(len(cells))
        cells += [(cx, cy)] * max(own, 1)
        cells += [(cx - 1 + int(t), cy - 1) for t in rng.integers(0, 3, lo)]
        cells += [(cx - 1 + int(t), cy + 1) for t in rng.integers(0, 3, up)]
    n = len(cells)
    st = g.SimulationSettings(n, 0.1, H, WIDE_BOX)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    CS.fill(p, np.arange(n), st, cells, rng)
    return st, CS.finish(st, p, rng, vel=0.0), np.array(probes)


@functools.lru_cache(maxsize=None)
def exit_rows():
    L = EXIT_LENGTHS
    st, p, probes = _probes(L, [max(x, 1) for x in L], L[::-1], seed=41)
    return st, _ticks(), p


@functools.lru_cache(maxsize=None)
def density_trips():
    L = TRIP_LENGTHS
    st, p, probes = _probes(L, [max(x, 1) for x in L], L[::-1], seed=43)
    return st, _ticks(), p


@functools.lru_cache(maxsize=None)
def exit_waves():
    """Row 2 (the lowest keys: sorted slots 0 .. 127 = waves 0 and 1 of block 0): one particle in every third cell, 128 of them.
    Above lane 5 of wave 0, BUSY_NEIGHBOURS particles within its radius; nothing else anywhere near row 2."""
    n = 128 + BUSY_NEIGHBOURS
    st = g.SimulationSettings(n, 0.1, H, WIDE_BOX)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    rng = np.random.default_rng(47)
    for k in range(128):
        _place(p, k, st, (3 + 3 * k, 2), (0.5, 0.9))
    busy = (3 + 3 * 5, 2)
    for j in range(BUSY_NEIGHBOURS):          # in the cell above, within 0.35 h of the busy lane
        _place(p, 128 + j, st, (busy[0], busy[1] + 1), (0.5 + rng.uniform(-0.2, 0.2), 0.02 + 0.2 * rng.uniform()))
    p = p[rng.permutation(n)]
    return st, _ticks(), _finish(p)


@functools.lru_cache(maxsize=None)
def dam(n):
    from oracle import oracle as O
    st, off, tick, p = PS.jittered_dam_break(g, O, n, seed=100 + n)
    return st, _ticks(), p


# ---- the paths beside B and C ---------------------------------------------------------------------------------------------------
TINY_PAIR = (100, 101)


@functools.lru_cache(maxsize=None)
def guard_tiny_dst():
    from oracle import oracle as O
    st, off, tick, p = PS.jittered_dam_break(g, O, 4096, seed=PS.GUARD_SEED)
    a, b = TINY_PAIR
    p["velocity"][[a, b]] = 0
    # the first point of the positions' own grid past 2^-20 along x: the smallest distance above the range's lower end there
    x = p["position"][a, 0]
    ulp = np.spacing(np.abs(x))
    p["position"][b] = (x + (np.floor(f32(2.0 ** -20) / ulp) + 1) * ulp, p["position"][a, 1])
    p["predicted_position"] = p["position"]
    return st, _ticks(), p


@functools.lru_cache(maxsize=None)
def guard_coincident():
    from oracle import oracle as O
    st, off, tick, p = PS.jittered_dam_break(g, O, 4096, seed=PS.COINCIDENT["seed"])
    return st, _ticks(), PS.coincident_state(p)


SCENES = {"rim_pow2": lambda: rim("pow2"), "rim_default": lambda: rim("default"), "exit_rows": exit_rows, "exit_waves": exit_waves,
          "density_trips": density_trips, "guard_tiny_dst": guard_tiny_dst, "guard_coincident": guard_coincident}
SCENES.update({f"dam_{n}": (lambda n=n: dam(n)) for n in DAM_N})
NAMES = tuple(SCENES)


def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle_states(name):
    """The oracle's state after each of the STEPS steps: [(records, start_indices)], computed once per scene and left unchanged."""
    from oracle import oracle as O
    st, ticks, p = scene(name)
    ref = O.OracleSim(st)
    ref.set_particles(p)
    out = []
    for t in ticks:
        ref.step(t)
        a, s = ref.particles().copy(), ref.start_indices().copy()
        a.setflags(write=False); s.setflags(write=False)
        out.append((a, s))
    grid = tuple(ref.grid_dims)
    ref.close()
    return out, grid


# ---- models --------------------------------------------------------------------------------------------------------------------
def row_lengths(keys, grid):
    """per sorted particle, the number of candidates in its three sweep rows (prologue_scenes.block_rows)"""
    return S.block_rows(keys, grid)[1]


def pair_r2(pred):
    """r2 of every ordered pair (i, j) as the scan forms it in f32: ox = q.x - me.x, oy = q.y - me.y, ox * ox + oy * oy; the
    diagonal is set to infinity (k != i)"""
    x, y = pred[:, 0].astype(f32), pred[:, 1].astype(f32)
    ox, oy = x[None, :] - x[:, None], y[None, :] - y[:, None]
    r2 = ox * ox + oy * oy
    np.fill_diagonal(r2, np.inf)
    return r2

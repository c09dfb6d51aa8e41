"""Scenes that put the prologue of the 2D density / force / surface-tension passes on its edges — TEST INFRASTRUCTURE, plain numpy.

The prologue (csrc/fs_neighbours.h: lane_row_ranges, stage_rows_load / stage_rows_store; force_block for the force pass, the driver
walk_lane / walk_bounds / walk_rows for the density, surface-tension and diffusion passes) looks up
the lane's three row ranges in the dense cell table and stages the block-wide ranges of a workgroup's 256 consecutive sorted
particles in LDS, in up to three trips of 256 candidates per row.  The scenes choose cell keys through crafted positions
(tests/csort_scenes.py's placement rules: h = 0.2, a point 0.01 .. 0.19 inside its cell, no motion in the predict step) so that

  corners()        clusters sit in the four corner cells a particle can be in, which puts row ranges on the table's ends;
  ragged(n)        the last workgroup holds one live lane (n = 257, 4097: the dam break, jittered);
  one_cell()       a block's rows are all staged in one trip (256 particles in one cell);
  strip(step, extra)  block 0 is one grid row's 256 particles, `step` cells apart, under a row that holds one particle per cell plus
                   `extra`: the block-wide length of that row is 255 * step + 3 + extra, chosen on either side of 256, 512, NBF_TILE = 544
                   and NB_TILE = 640.

Which cells can hold a particle: predict_pos clamps every coordinate to [-size/2, +size/2] and the cell coordinate is
u32sat(floor((x + size/2) / h)) + 1, so on a single-domain handle cx is 1 .. floor(size_x / h) + 1 and never 0; the grid has
ceil(size_x / h) + 2 columns, so the last column grid_w - 1 is reached exactly when size_x / h is a whole number in f32 and x is ON
the wall.  corners() therefore uses h = 0.25 and a 10 x 7.5 box (42 x 32 cells), and its corner cells are (1, 1), (41, 1), (1, 31)
and (41, 31) = (grid_w - 1, grid_h - 1); the cluster of (41, 31) is coincident (both coordinates on the walls), the ones of (41, 1)
and (1, 31) share one coordinate.  Column 0 and row 0 (and with them the wrapped cy - 1, the wrapped cx - 1 on row 0 and an id_lo
past the table) cannot be reached from a single-domain handle at all: what the scenes reach of lane_row_ranges is the empty column 0
and row 0 as NEIGHBOURS (id_lo = y * grid_w + 0), cy + 1 == grid_v, id_hi clamped to ncell, cx + 1 == grid_w (the range runs into
the next row's column 0) and, in every scene, the cell of sorted index 0 (a == 0 -> lo_fix from the first step).  The inputs no
scene can reach are swept on the CPU instead: tests/row_ranges_checker.hip compares lane_row_ranges with three row_range calls
for every (cx, cy) of small grids, 0 and wrapped coordinates included (tests/test_row_ranges_host.py).

`block_rows(keys, grid)` is the model the CPU test (tests/test_prologue_scenes.py) applies to the ORACLE's sorted keys: the dense cell
table and, per workgroup and sweep row, the block-wide candidate range the kernels reduce."""
import functools

import numpy as np

import gpu_fluid_simulation_amd as g
from tests import csort_scenes as CS

f32 = np.float32
H = CS.H
BLOCK = 256
NBF_TILE, NB_TILE = 544, 640          # csrc/fs_neighbours.h
STRIP_BOX = (112.0, 6.0)              # 562 x 32 cells: a row longer than 514 cells
STRIP_X0, STRIP_ROW = 20, 10          # first cell of block 0's particles, their grid row


def tick_settings():
    return g.default_tick_settings(gravity=(0.0, 9.81))


def block_rows(keys, grid):
    """(cs, lane_len, lo, hi): the dense cell table of the sorted keys, cs[c] = index of the first particle whose key is >= c
    (ncell + 1 entries); per particle and sweep row the length of its candidate range; per workgroup b and sweep row r the
    block-wide candidate range [lo[b, r], hi[b, r]) — min lo / max hi over the lanes that have candidates in the row, (0, 0) when
    none has (fs_device.h block_tile_bounds).  The stale-start rule is left out: it only moves the lo of ranges that begin at
    index 0 to lo_fix <= the first cell's count."""
    gw, gh = grid
    ncell = gw * gh
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.shape[0]
    cs = np.searchsorted(keys, np.arange(ncell + 1), side="left")
    cx, cy = keys % gw, keys // gw
    nb = -(-n // BLOCK)
    lo = np.zeros((nb, 3), dtype=np.int64)
    hi = np.zeros((nb, 3), dtype=np.int64)
    lane_len = np.zeros((n, 3), dtype=np.int64)
    for r in range(3):
        y = cy + r - 1
        id_lo = y * gw + cx - 1
        ok = (y >= 0) & (y < gh) & (id_lo >= 0) & (id_lo < ncell)
        id_hi = np.minimum(id_lo + 3, ncell)
        a = np.where(ok, cs[np.where(ok, id_lo, 0)], 0)
        b = np.where(ok, cs[np.where(ok, id_hi, 0)], 0)
        has = a < b
        lane_len[:, r] = np.where(has, b - a, 0)
        for blk in range(nb):
            s = slice(blk * BLOCK, min((blk + 1) * BLOCK, n))
            if has[s].any():
                lo[blk, r], hi[blk, r] = a[s][has[s]].min(), b[s][has[s]].max()
    return cs, lane_len, lo, hi


def _particles(n):
    return np.zeros(n, dtype=g.PARTICLE_DTYPE)


# ---- corners ----------------------------------------------------------------------------------------------------------------
CORNER_H, CORNER_BOX, CORNER_GRID = 0.25, (10.0, 7.5), (42, 32)
CORNER_CELLS = ((1, 1), (41, 1), (1, 31), (41, 31))
CORNER_CLUSTER = 4


@functools.lru_cache(maxsize=None)
def corners(seed=5):
    """Four clusters of CORNER_CLUSTER particles in the corner cells, 284 particles scattered over the middle of the box (three to a
    cell at most): 300 particles, two workgroups.  No velocity, so the predicted positions are the uploaded ones."""
    n = 300
    st, tick = g.SimulationSettings(n, 0.1, CORNER_H, CORNER_BOX), tick_settings()
    rng = np.random.default_rng(seed)
    p = _particles(n)
    bs = np.array(CORNER_BOX) / 2
    pos = np.empty((n, 2))
    k = 0
    for (cx, cy) in CORNER_CELLS:
        for j in range(CORNER_CLUSTER):
            # inside the cell where the cell has an inside; ON the wall (beyond it: predict_pos clamps) in the last column / row
            x = bs[0] + 1.0 if cx == CORNER_GRID[0] - 1 else (cx - 1) * CORNER_H - bs[0] + 0.02 + 0.05 * j
            y = bs[1] + 1.0 if cy == CORNER_GRID[1] - 1 else (cy - 1) * CORNER_H - bs[1] + 0.03 + 0.04 * j
            pos[k] = (x, y)
            k += 1
    cells = CS.sparse_cells(rng, n - k, (8, 34), (6, 26))
    pos[k:] = (cells - 1) * CORNER_H - bs + rng.uniform(0.01, 0.24, size=(n - k, 2))
    p["position"] = pos[rng.permutation(n)].astype(f32)
    p["predicted_position"] = p["position"]
    return st, tick, p


# ---- ragged counts ----------------------------------------------------------------------------------------------------------
RAGGED_N = (257, 4097)


@functools.lru_cache(maxsize=None)
def ragged(n):
    """The dam break of n particles, jittered and with random velocities: n = 1 (mod 256), one live lane in the last workgroup."""
    from oracle import oracle as O
    st, off, tick = g.dam_break_2d(n)
    ref = O.OracleSim(st, off)
    p = ref.particles()
    ref.close()
    rng = np.random.default_rng(n)
    p["position"] += rng.uniform(-0.025, 0.025, size=p["position"].shape).astype(f32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-1.0, 1.0, size=p["velocity"].shape).astype(f32)
    return st, tick, p


# ---- staging depth ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_cell(seed=6, cell=(100, CS.BIG_ROW)):
    """256 particles in one cell: one workgroup, its own row 256 candidates long (one staging trip), the other rows empty."""
    n = BLOCK
    st, tick = g.SimulationSettings(n, 0.1, H, CS.BOX), tick_settings()
    rng = np.random.default_rng(seed)
    p = _particles(n)
    CS.fill(p, np.arange(n), st, [tuple(cell)] * n, rng)
    return st, tick, CS.finish(st, p, rng, vel=0.0)


#            name        step extra  length of block 0's longest row       density   force
STRIP_CASES = (("trips2", 1, 0),     # 258: in (256, 512]                   staged    staged, two trips
               ("trips3", 2, 0),     # 513: in (512, 544]                   staged    staged, three trips
               ("force_unstaged", 2, 60),    # 573: in (544, 640]           staged    unstaged: the general kernel
               ("both_unstaged", 2, 200))    # 713: > 640                   unstaged  unstaged
STRIP = {name: (step, extra) for name, step, extra in STRIP_CASES}


def strip_length(step, extra):
    return (BLOCK - 1) * step + 3 + extra


@functools.lru_cache(maxsize=None)
def strip(step, extra, seed=7):
    """Row STRIP_ROW: 256 particles, one in every `step`-th cell from column STRIP_X0 — the lowest keys, so they are workgroup 0.
    Row STRIP_ROW + 1: one particle per cell over the columns those 256 sweep (one more on either side), and a second one in the
    first `extra` of them.  Block 0's rows are then 0, 256 and strip_length(step, extra) candidates long."""
    span = (BLOCK - 1) * step + 1
    above = span + 2 + extra
    n = BLOCK + above
    st, tick = g.SimulationSettings(n, 0.1, H, STRIP_BOX), tick_settings()
    rng = np.random.default_rng(seed + 1000 * step + extra)
    p = _particles(n)
    src = rng.permutation(n)
    own = [(STRIP_X0 + j * step, STRIP_ROW) for j in range(BLOCK)]
    cols = list(range(STRIP_X0 - 1, STRIP_X0 + span + 1))
    up = [(c, STRIP_ROW + 1) for c in cols + cols[:extra]]
    CS.fill(p, src[:BLOCK], st, own, rng)
    CS.fill(p, src[BLOCK:], st, up, rng)
    return st, tick, CS.finish(st, p, rng, vel=0.0)


STAGING_SCENES = ("one_cell",) + tuple(name for name, _, _ in STRIP_CASES)


def staging_scene(name):
    return one_cell() if name == "one_cell" else strip(*STRIP[name])

"""CPU-side proof that the scenes of tests/prologue_scenes.py reach the edges of the density / force prologue they are named
after.  Every scene is stepped once by the ORACLE; numpy on its sorted keys (prologue_scenes.block_rows: the dense cell table, the
per-lane and the block-wide row ranges the kernels reduce) then says which corner cells are occupied, which ends of the table the
row ranges touch, how many lanes of the last workgroup are live and how long block 0's rows are against the staging trips (256,
512) and the two tiles (NBF_TILE = 544, NB_TILE = 640).  tests/test_prologue_edges_gpu.py runs the same scenes on the engine.
No GPU."""
import glob
import os

import numpy as np
import pytest

from tests import prologue_scenes as S


def sorted_keys(orc, scene, quirks=True):
    st, tick, p = scene
    ref = orc.OracleSim(st, ref_quirks=quirks)
    ref.set_particles(p)
    ref.step(tick, stable_sort=True)
    keys, grid, start = ref.particles()["grid"].copy(), tuple(ref.grid_dims), ref.start_indices()
    ref.close()
    assert np.all(keys[:-1] <= keys[1:])
    return keys, grid, start


def assert_reachable_cells_only(keys, grid):
    """On a single-domain handle no particle is in column 0 or row 0 (prologue_scenes.py, "Which cells can hold a particle")."""
    gw, gh = grid
    assert (keys % gw).min() >= 1 and (keys // gw).min() >= 1 and (keys // gw).max() <= gh - 1


def test_corner_clusters_sit_in_the_corner_cells_and_touch_the_table_ends(fs, orc):
    keys, grid, start = sorted_keys(orc, S.corners())
    gw, gh = grid
    assert grid == S.CORNER_GRID and keys.shape[0] == 300          # two workgroups
    assert_reachable_cells_only(keys, grid)
    for (cx, cy) in S.CORNER_CELLS:
        assert int((keys == cy * gw + cx).sum()) == S.CORNER_CLUSTER >= 3, (cx, cy)
    assert S.CORNER_CELLS[-1] == (gw - 1, gh - 1)
    ncell = gw * gh
    kx, ky = keys.astype(np.int64) % gw, keys.astype(np.int64) // gw
    # the cell of sorted index 0 is the (1, 1) cluster's: every range that begins there starts at cs == 0 (a == 0 -> lo_fix)
    assert keys[0] == 1 * gw + 1 and np.all(keys[:S.CORNER_CLUSTER] == keys[0])
    # row ranges on the table's ends, among the lanes' three rows y = cy - 1 .. cy + 1:
    assert np.any(ky + 1 == gh)                                    # cy + 1 == grid_v: a row past the grid
    id_lo = ky * gw + kx - 1
    assert np.any(id_lo + 3 > ncell)                               # id_hi clamped to ncell (own row of the last cell)
    assert np.any((ky - 1 == 0) & (kx - 1 == 0))                   # row 0 and column 0 as neighbours: id_lo == 0
    assert np.any((kx + 1 == gw) & (ky + 1 < gh))                  # cx + 1 == grid_w: the range runs into the next row's column 0
    cs, lane_len, lo, hi = S.block_rows(keys, grid)
    assert cs[ncell] == 300 and lo.shape[0] == 2
    assert np.all(hi - lo <= S.NBF_TILE)                           # both workgroups stage
    # the sort left the quirk's input as the reference does: the minimum cell's start is never written
    assert start[keys[0]] == 0


@pytest.mark.parametrize("quirks", [True, False])
def test_corner_scene_second_step_still_starts_in_the_first_corner_cell(fs, orc, quirks):
    """The GPU cases run two steps: after the first one the cell of sorted index 0 is still the (1, 1) cluster's, so the second
    step's ranges begin at cs == 0 again, now with a start entry the first step left behind."""
    st, tick, p = S.corners()
    ref = orc.OracleSim(st, ref_quirks=quirks)
    ref.set_particles(p)
    ref.step(tick, stable_sort=True)
    ref.step(tick, stable_sort=True)
    keys, (gw, gh) = ref.particles()["grid"], ref.grid_dims
    ref.close()
    assert_reachable_cells_only(keys, (gw, gh))
    assert keys[0] == 1 * gw + 1


@pytest.mark.parametrize("n", S.RAGGED_N)
def test_ragged_counts_leave_one_live_lane_in_the_last_workgroup(fs, orc, n):
    keys, grid, _ = sorted_keys(orc, S.ragged(n))
    assert keys.shape[0] == n and n % S.BLOCK == 1
    assert_reachable_cells_only(keys, grid)
    cs, lane_len, lo, hi = S.block_rows(keys, grid)
    assert lo.shape[0] == n // S.BLOCK + 1
    assert lane_len[-1, 1] >= 1                                    # the last lane has candidates (itself at least)
    assert np.all(hi - lo <= S.NBF_TILE)


def test_one_cell_block_is_staged_in_one_trip(fs, orc):
    keys, grid, _ = sorted_keys(orc, S.one_cell())
    cs, lane_len, lo, hi = S.block_rows(keys, grid)
    assert keys.shape[0] == S.BLOCK and np.unique(keys).size == 1
    assert (hi - lo).tolist() == [[0, 256, 0]]
    assert np.all(lane_len[:, 1] == 256)                           # longer than 32: the force pass's chunked sweep, staged


@pytest.mark.parametrize("name,step,extra", S.STRIP_CASES)
def test_strip_block_zero_has_the_row_length_it_is_named_after(fs, orc, name, step, extra):
    keys, grid, _ = sorted_keys(orc, S.strip(step, extra))
    assert_reachable_cells_only(keys, grid)
    cs, lane_len, lo, hi = S.block_rows(keys, grid)
    length = S.strip_length(step, extra)
    assert (hi[0] - lo[0]).tolist() == [0, 256, length]
    lo_bound, hi_bound = {"trips2": (256, 512), "trips3": (512, S.NBF_TILE), "force_unstaged": (S.NBF_TILE, S.NB_TILE),
                          "both_unstaged": (S.NB_TILE, 1 << 30)}[name]
    assert lo_bound < length <= hi_bound
    # every lane's own ranges are short: a staged block takes the force pass's mask sweep, not the chunked one
    assert lane_len[:S.BLOCK].max() <= 32
    # block 0 is exactly the lower row's particles
    gw = grid[0]
    assert np.all(keys[:S.BLOCK] // gw == S.STRIP_ROW) and np.all(keys[S.BLOCK:] // gw == S.STRIP_ROW + 1)
    # the other workgroups (the upper row's particles) stage in both passes
    assert np.all(hi[1:] - lo[1:] <= S.NBF_TILE)


def test_the_strip_cases_cover_every_interval(fs):
    lengths = sorted(S.strip_length(step, extra) for _, step, extra in S.STRIP_CASES)
    assert [sum(a < x <= b for x in lengths) for a, b in ((256, 512), (512, 544), (544, 640), (640, 1 << 30))] == [1, 1, 1, 1]


def test_the_three_term_passes_share_one_walk():
    """The prologue, the stage-and-barrier and the two row loops of k_density / k_density_edge, k_surface_tension and k_diffuse exist
    once, as the driver of csrc/fs_neighbours.h (walk_lane, walk_bounds, walk_rows): the passes hold their terms and call it."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-fluid-simulation_amd", "csrc")
    text = {}
    for path in glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.inc")):
        with open(path) as fh:
            text[os.path.basename(path)] = fh.read()
    for name in ("kernels_density.hip", "kernels_diffuse.hip"):
        for own in ("lane_row_ranges(", "stage_rows_load(", "stage_rows_store(", "block_tile_bounds(", "recorded_tile_bounds("):
            assert own not in text[name], (name, own)
    for name, fn in (("kernels_density.hip", "void density_block("), ("kernels_density.hip", "void k_surface_tension("),
                     ("kernels_diffuse.hip", "void k_diffuse(")):
        body = text[name][text[name].index(fn):]
        body = body[:body.index("\n}\n")]
        assert body.count("walk_rows<") == 1 and body.count("walk_bounds<") == 1, fn
        assert body.count("walk_lane(") + body.count("walk_lane_particle(") == 1, fn
    driver = text["fs_neighbours.h"]
    walk = driver[driver.index("void walk_rows("):]
    walk = walk[:walk.index("\n}\n")]
    assert walk.count("stage_rows_load(") == 1 and walk.count("stage_rows_store(") == 1 and walk.count("__syncthreads()") == 1
    assert driver.count("lane_row_ranges(P, cs, L.lo_fix") == 1
    for name, t in text.items():
        assert "df_weight_" not in t and "st_weight_" not in t, name

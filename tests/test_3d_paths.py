"""The CPU model of the 3D kernels' path choice (tests/paths3d.py): known answers on hand-built key arrays, the constants it
mirrors compared with the kernel sources, and every path scene of test_3d_paths_gpu.py run on the oracle alone — the
asserted coverage (which sweep carries which scene, at every compared step) holds without a GPU."""
import re

import numpy as np
import pytest

import paths3d
from paths3d import PathModel

DIMS = (42, 26, 26)                                    # gw, gh, gd


def _key(x, y, z, dims=DIMS):
    return (z * dims[1] + y) * dims[0] + x


def _singles(count, z0, dz):
    """keys of `count` particles alone in every other cell of the z-planes z0, z0 + 2 dz, ...: rows of one candidate"""
    return [_key(2 + 2 * (k % 19), 2 + 2 * ((k // 19) % 11), z0 + 2 * dz * (k // 209)) for k in range(count)]


def _one_cell(m, n=512, before=100, cell=(20, 12, 12)):
    """m particles in one cell; the others alone in cells of their own, far away, `before` of them sorted first"""
    lo, hi = _singles(before, 2, 1), _singles(n - m - before, 24, -1)
    return np.array(sorted(lo + [_key(*cell)] * m + hi), dtype=np.uint32)


@pytest.mark.parametrize("m,path,n,before", [(1, "mask64", 512, 100), (63, "mask64", 512, 100), (64, "mask64", 512, 100),
                                             (65, "mask128", 512, 100), (128, "mask128", 512, 100),
                                             (129, "chunks_staged", 512, 100), (400, "chunks_staged", 400, 0),
                                             (401, "chunks_unstaged", 401, 0)])
def test_one_cell_of_m_particles(m, path, n, before):
    """the sorted neighbours of the cell count towards its blocks' extents (first has-lane's lo, last has-lane's hi), so the
    cases at the tile's edge are arrays that hold the cell alone"""
    mod = PathModel(_one_cell(m, n, before), DIMS)
    want = paths3d.PATHS.index(path)
    lanes = np.arange(before, before + m)
    waves = np.unique(lanes // 64)
    assert (mod.path[waves, 1] == want).all(), mod.summary()
    assert (mod.longest[waves, 1] == m).all()
    assert (mod.lane_longest[lanes, 1] == m).all() and (mod.lane_longest[lanes][:, [0, 2]] == 0).all()
    others = np.setdiff1d(np.arange(mod.path.shape[0]), waves)
    if path != "chunks_unstaged":                      # the background: rows of one candidate
        assert (mod.path[others] == paths3d.P_MASK64).all() and mod.longest[others].max() <= 1
    else:                                              # the block decides: every wave of a block that does not fit
        blocks = np.unique(waves // 4)
        for b in blocks:
            assert (mod.path[b * 4:(b + 1) * 4, 1] == want).all()
    assert mod.count(path) >= len(waves)


@pytest.mark.parametrize("extent,path", [(400, "staged"), (401, "chunks_unstaged")])
def test_block_extent_decides_staging(extent, path):
    """block 1 = 32 cells x 8 particles; 72 in the cell before it, extent - 328 in the cell behind it"""
    keys = sorted(_singles(184, 2, 1)) + [_key(4, 12, 12)] * 72
    for k in range(32):
        keys += [_key(5 + k, 12, 12)] * 8
    keys += [_key(37, 12, 12)] * (extent - 328)
    keys += sorted(_singles(1000 - len(keys), 24, -1))
    keys = np.array(keys, dtype=np.uint32)
    assert np.all(keys[:-1] <= keys[1:])
    mod = PathModel(keys, DIMS)
    assert mod.extent[1, 1] == extent and mod.extent[1, 0] == 0 and mod.extent[1, 2] == 0
    if path == "chunks_unstaged":
        assert (mod.path[4:8, 1] == paths3d.P_UNSTAGED).all()
    else:
        assert list(mod.path[4:8, 1]) == [paths3d.P_MASK128, paths3d.P_MASK64, paths3d.P_MASK64, paths3d.P_MASK128]
        assert list(mod.longest[4:8, 1]) == [88, 24, 24, 8 + 8 + extent - 328]
    # the model's tile is the only thing that separates the two: a retuned TILE3 moves the edge
    assert (PathModel(keys, DIMS, tile=extent).path[4:8, 1] != paths3d.P_UNSTAGED).all()
    assert (PathModel(keys, DIMS, tile=extent - 1).path[4:8, 1] == paths3d.P_UNSTAGED).all()


def test_rows_below_above_and_past_the_grid():
    gw, gh, gd = dims = (5, 4, 3)                      # 60 cells
    ncell = gw * gh * gd
    # a particle in the lowest reachable cell (1, 1, 1), one in the highest (gw-1, gh-1, gd-1), one in the last cell of a row
    keys = np.array(sorted([_key(1, 1, 1, dims), _key(4, 1, 1, dims), _key(4, 3, 2, dims), _key(4, 3, 2, dims)]), dtype=np.uint32)
    lo, hi = paths3d.row_ranges(keys, dims)
    ln = hi - lo
    # (1,1,1): rows at z = 0 and y = 0 exist (padding cells) and are empty; its own row holds itself only: x + 1 = 2 is empty
    assert ln[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    # (4,1,1): last cell of its row — the three ids run into cell 0 of the next row, which is padding and empty
    assert ln[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    # (4,3,2), the last cell of the table: ids past the table are cut off (id_hi = ncell), rows above the grid do not exist
    assert _key(4, 3, 2, dims) == ncell - 1
    assert ln[2].tolist() == [0, 0, 0, 0, 2, 0, 0, 0, 0] and ln[3].tolist() == ln[2].tolist()
    assert hi[2, 4] == 4 and lo[2, 4] == 2
    # neighbours across rows and planes: (2,2,1) sees (1,1,1) in row 3 (oz 0, oy -1) and, from plane z = 0, nothing
    keys = np.array(sorted([_key(1, 1, 1, dims), _key(2, 2, 1, dims), _key(2, 2, 2, dims)]), dtype=np.uint32)
    lo, hi = paths3d.row_ranges(keys, dims)
    ln = hi - lo
    assert ln[1].tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 0]           # (2,2,1): row 3 = (1,1,1), row 4 = itself, row 7 = (2,2,2)
    assert ln[2].tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 0]           # (2,2,2): row 0 = (1,1,1), row 1 = (2,2,1), row 4 = itself
    # a key past the table (never produced by a step; an uploaded record may carry one) has no rows at all and breaks nothing
    keys = np.array([_key(1, 1, 1, dims), ncell + 7], dtype=np.uint32)
    lo, hi = paths3d.row_ranges(keys, dims)
    assert (hi - lo)[1].sum() == 0 and (hi - lo)[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_first_and_last_has_lane_give_the_block_bounds():
    """lanes without candidates in a row (lo = hi = 0) must not pull the block's lower bound to 0"""
    keys = np.array(sorted(_one_cell(70, 509, 130).tolist() + [_key(20, 13, 12)] * 3), dtype=np.uint32)
    mod = PathModel(keys, DIMS)                        # the cell: lanes 130 .. 199; three probes in the cell above it: 200 .. 202
    assert (mod.lo[200:203, 3] == 130).all() and (mod.hi[200:203, 3] == 200).all()
    assert mod.row_extent[0, 1].tolist() == [70, 256, 3]          # row 0: the probes' lanes only; row 1: every lane, itself
    assert mod.extent[0, 0] == 0 and mod.extent[0, 2] == 0
    assert mod.path[2, 1] == paths3d.P_MASK128 and mod.path[3, 1] == paths3d.P_MASK128 and mod.path[1, 1] == paths3d.P_MASK64


def test_model_constants_match_the_kernel_sources():
    sweep = paths3d.source_text("fs_sweep3.h")          # what the sweep passes share; the passes themselves, and the rest of the step:
    passes = {name: paths3d.source_text(name) for name in ("kernels_density3d.hip", "kernels_force3d.hip", "kernels_3d.hip")}
    k3d = sweep + "".join(passes.values())
    kern = paths3d.source_text("fs_kernels.h")
    assert int(paths3d.parse_define(kern, "FS_PRED_SLACK")) == paths3d.FS_PRED_SLACK
    assert int(paths3d.parse_define(sweep, "B3F")) == paths3d.B3F
    assert int(paths3d.parse_define(sweep, "TILE3")) == paths3d.TILE3
    assert k3d.count("#define B3F ") == 1 and k3d.count("#define TILE3 ") == 1
    assert "#ifndef B3F" not in k3d and "#ifndef TILE3" not in k3d            # plain constants: no other value is ever built
    body = sweep[sweep.index("int plane_class("):]
    body = body[:body.index("\n}")]
    assert "mx > 64u" in body and "mx > 128u" in body and "if (!fit) return 0;" in body
    assert paths3d.MASK64 == 64 and paths3d.MASK128 == 128
    # every pass takes its block bounds and its plane class from ONE call each, with one tile: the plane driver's (fs_sweep3.h
    # sweep3_planes), which k3_density, k3_surface_tension and force3_body call with their work as a force-inlined callable.  The
    # nine looked-up ranges stay locals of the driver, which also indexes them: a helper around "rows of plane p -> RowRanges,
    # block_tile_bounds" that gets them by pointer makes the compiler keep them in scratch (96 B in every kernel; k3_density
    # 72 -> 54 VGPRs, k3_force 128 -> 107 / 109), which the driver does not (profiles/3d_sweep_split_resource_usage.txt)
    assert k3d.count("block_tile_bounds<W3F>(") == 1 and sweep.count("block_tile_bounds<W3F>(R, s_red, blo, bhi, TILE3)") == 1
    assert k3d.count("int plane_class(") == 1 and k3d.count("plane_class(R, fit)") == 1 and sweep.count("plane_class(R, fit)") == 1
    driver = sweep[sweep.index("void sweep3_planes("):]
    driver = driver[:driver.index("\n}")]
    assert "block_tile_bounds<W3F>(R, s_red, blo, bhi, TILE3)" in driver and "plane_class(R, fit)" in driver
    assert "xcd_block3(" in sweep[sweep.index("bool sweep3_lane("):sweep.index("void sweep3_planes(")] and "rows3_lookup(" in driver
    for name, fn in (("kernels_density3d.hip", "void k3_density("), ("kernels_density3d.hip", "void k3_surface_tension("),
                     ("kernels_force3d.hip", "void force3_body(")):
        text = passes[name][passes[name].index(fn):]
        text = text[:text.index("\n}\n")]
        assert text.count("sweep3_lane(") == 1 and text.count("sweep3_planes(") == 1, fn
    assert sum(t.count("sweep3_planes(") for t in passes.values()) == 3
    # the 128-bit masks are no longer a switch: rows <= 128 are class 2 unconditionally
    # (the name is spelt in two halves so that a search of the tree for the removed switch finds nothing, this test included)
    assert "FS3_" + "MASK128" not in k3d and "return !__any(mx > 128u) ? 2 : 0;" in body
    # the unstaged sweep reads at most three candidates past a row's end (chunks are scanned four at a time)
    assert paths3d.FS_PRED_SLACK >= 3


@pytest.mark.parametrize("name", sorted(paths3d.scenes()))
def test_scene_reaches_its_path_on_the_oracle(fs, orc, name):
    scene = paths3d.scenes()[name]
    assert scene.n <= 24 ** 3
    st, tick, p, after, dims = paths3d.oracle_states(fs, orc, scene)
    assert dims == (paths3d.GRID[0] + 2, paths3d.GRID[1] + 2, paths3d.GRID[2] + 2)
    paths3d.check_scene(scene, after, dims)
    for state in after:
        assert np.isfinite(state["position"]).all() and np.isfinite(state["velocity"]).all()


def test_scenes_cover_every_path(fs, orc):
    seen = {name: 0 for name in paths3d.PATHS}
    for scene in paths3d.scenes().values():
        st, tick, p, after, dims = paths3d.oracle_states(fs, orc, scene)
        for state in after:
            for k, v in PathModel(state["grid"], dims).summary().items():
                seen[k] += v
    assert all(v > 0 for v in seen.values()), seen


def test_changed_tile_in_the_model_is_noticed(fs, orc):
    """the extent scenes sit on the edge: with another TILE3 in the model alone their assertions fail"""
    sc = paths3d.scenes()
    for name, tile in (("extent400", 399), ("extent401", 401)):
        st, tick, p, after, dims = paths3d.oracle_states(fs, orc, sc[name])
        m = PathModel(after[0]["grid"], dims, tile=tile)
        with pytest.raises(AssertionError):
            for chk in sc[name].expect:
                chk(m)

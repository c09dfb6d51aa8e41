"""The prologue of the 2D density, surface-tension and force passes on its edges (csrc/fs_neighbours.h: lane_row_ranges,
stage_rows_load / stage_rows_store; the driver walk_lane / walk_bounds / walk_rows under density_block and k_surface_tension;
force_block): the scenes of tests/prologue_scenes.py, whose
edges tests/test_prologue_scenes.py proves on the CPU from the oracle's sorted keys, run on the engine for two steps and compared
with the oracle bit for bit — every field of every particle and start_indices — in both sort modes.

Edge                                                                    test
corner cells, row ranges on the ends of the cell table, quirks on/off   test_corner_clusters
one live lane in the last workgroup (n = 257, 4097)                     test_ragged_counts
block-wide row length <= 256, (256, 512], (512, 544], (544, 640], > 640 test_staging_depth
the same with surface tension, against tests/st_checker.cpp             test_staging_depth_with_surface_tension"""
import numpy as np
import pytest

from tests import prologue_scenes as S
from tests.test_parity_gpu import assert_particles_equal

pytestmark = pytest.mark.gpu
STEPS = 2
SORTS = ("bitonic", "counting")


def sort_mode(fs, sort):
    return fs.FS_SORT_BITONIC if sort == "bitonic" else fs.FS_SORT_COUNTING


def run_against_oracle(fs, orc, scene, sort, quirks=True, ctx=""):
    st, tick, p = scene
    sim = fs.FluidSimulation(st, device=0, ref_quirks=quirks, sort_mode=sort_mode(fs, sort))
    ref = orc.OracleSim(st, ref_quirks=quirks)
    sim.upload_particles(p); ref.set_particles(p)
    for s in range(STEPS):
        sim.tick(tick)
        ref.step(tick, stable_sort=sort == "counting")
        assert_particles_equal(sim.download_particles(), ref.particles(), f"{ctx} {sort} step {s}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices()), f"{ctx} {sort} step {s}: start_indices"
    sim.close(); ref.close()


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("quirks", [True, False])
def test_corner_clusters(fs, orc, quirks, sort):
    """Clusters in the four corner cells a particle can be in — (1, 1), (grid_w - 1, 1), (1, grid_h - 1), (grid_w - 1, grid_h - 1):
    row 0 and column 0 as neighbours, cy + 1 == grid_v, id_hi clamped to ncell, and the cell of sorted index 0 (a == 0 -> lo_fix)
    from the first step.  Column 0 and row 0 themselves hold no particle on a single-domain handle (prologue_scenes.py); those
    inputs of lane_row_ranges are swept on the CPU (tests/test_row_ranges_host.py)."""
    run_against_oracle(fs, orc, S.corners(), sort, quirks=quirks, ctx=f"corners quirks={quirks}")


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("n", S.RAGGED_N)
def test_ragged_counts(fs, orc, n, sort):
    run_against_oracle(fs, orc, S.ragged(n), sort, ctx=f"ragged {n}")


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", S.STAGING_SCENES)
def test_staging_depth(fs, orc, name, sort):
    """One, two and three staging trips; a block the force pass cannot stage (k_force_general's unstaged sweep) while the density
    pass can; a block neither stages."""
    run_against_oracle(fs, orc, S.staging_scene(name), sort, ctx=name)


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", S.STAGING_SCENES)
def test_staging_depth_with_surface_tension(fs, name, sort):
    """k_surface_tension stages the same rows (position and weight operand) and the ST force kernels read its output: state,
    start_indices and the st buffer against the CPU checker, bit for bit."""
    from tests.st_ref import STChecker
    from tests.test_surface_tension_gpu import assert_state_equal
    st, tick, p = S.staging_scene(name)
    sim = fs.FluidSimulation(st, device=0, sort_mode=sort_mode(fs, sort), surface_tension=True)
    chk = STChecker(st)
    sim.upload_particles(p); chk.set_particles(p)
    for s in range(STEPS):
        sim.tick(tick)
        chk.step(tick, stable_sort=sort == "counting")
        assert_state_equal(sim, chk, f"{name} {sort} step {s}")
    assert np.any(chk.st != 0.0), f"{name}: no particle felt surface tension"
    sim.close(); chk.close()

"""FS_SORT_COUNTING on its own edges (csrc/kernels_csort.hip, csrc/fs_scan.h): the scenes of tests/csort_scenes.py, whose `facts`
tests/test_csort_scenes.py proves on the CPU, run on the engine with tracking on, so that particle_ids() is the permutation
the sort applied.  Every step is checked twice: the ARRANGEMENT against a plain numpy stable argsort of the keys (no oracle
involved), and the whole state — records, cell starts — bit for bit against the oracle stepped with std::stable_sort.

Edge                                                         test
rank bound 2047 / 2048 / 2049, network sizes 4095 .. 8193    test_rank_bound_and_network_sizes
lo % 256 in {0, 1, 255}, hi == n (n = 0, 1 mod 256)          test_segment_placement_among_the_workgroups
two big cells back to back in one workgroup, 2048 | 2049     test_big_cells_back_to_back
the whole population in one cell                             test_whole_population_in_one_cell
n = 2 .. 4097 around 64, 256, 1024                           test_small_and_ragged_counts
ncell + 1 around 16 and 16384, 66 and 131 tiles              test_scan_table_edges
key runs over the lanes of a wave, ragged last wave          test_histogram_run_aggregation
big cells in slab handles (DEAD slots, n_dev, edge chain)    test_slab_handles_sort_big_cells"""
import inspect
import time

import numpy as np
import pytest

from tests import csort_scenes as S
from tests.test_parity_gpu import assert_particles_equal

pytestmark = pytest.mark.gpu


def assert_stable_step(fs, orc, scene, steps=2):
    st, tick, p, facts = scene
    n = facts["n"]
    sim = fs.FluidSimulation(st, device=0, sort_mode=fs.FS_SORT_COUNTING, track=0)
    assert sim.grid_dims == facts["grid"]
    ref = orc.OracleSim(st)
    assert ref.grid_dims == facts["grid"]
    ref.set_particles(p); sim.upload_particles(p)
    prev = np.arange(n, dtype=np.uint32)
    assert np.array_equal(sim.particle_ids(), prev)
    for s in range(steps):
        sim.tick(tick)
        ref.step(tick, stable_sort=True)
        got, ids = sim.download_particles(), sim.particle_ids()
        grid = got["grid"]
        assert np.all(grid[:-1] <= grid[1:]), f"step {s}: keys not sorted"
        assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32)), f"step {s}: a particle was lost or duplicated"
        # the slot every particle came from in this step's input order, and that slot's key: the arrangement must be the stable
        # argsort of those keys, exactly
        where = np.empty(n, dtype=np.uint32)
        where[prev] = np.arange(n, dtype=np.uint32)
        src = where[ids]
        key_src = np.empty(n, dtype=np.uint32)
        key_src[src] = grid
        want_src = np.argsort(key_src, kind="stable")
        bad = np.nonzero(src != want_src)[0]
        assert bad.size == 0, (f"step {s}: not the stable arrangement in {bad.size} slots, first {bad[0]} "
                               f"(key {grid[bad[0]]}): source {src[bad[0]]}, stable sort says {want_src[bad[0]]}")
        if s == 0:
            assert np.array_equal(key_src, facts["keys"]), "step 0: keys differ from the CPU keys of the scene"
            assert np.array_equal(ids, facts["perm"])
        assert np.array_equal(sim.download_start_indices(), ref.start_indices()), f"step {s}: start_indices"
        assert_particles_equal(got, ref.particles(), f"step {s}")
        prev = ids
    sim.close(); ref.close()


@pytest.mark.parametrize("m,before,after", S.RANK_CASES)
def test_rank_bound_and_network_sizes(fs, orc, m, before, after):
    """`hi - lo > CS_RANK_MAX` chooses between the serial rank loop (2047, 2048) and cs_sort_segment (2049 ...); the network runs
    with p2 == m (4096: no guarded partner), p2 = 8192 for 4095 (one) and 4097 (nearly half of them guarded by b < m), and
    p2 = 16384 for 8193.  A wrong guard moves the slots after the segment, which belong to the next cells: the arrangement of
    the WHOLE array is compared."""
    assert_stable_step(fs, orc, S.one_cell(m, before, after))


@pytest.mark.parametrize("m,before,after,lo_mod,ends", S.PLACEMENT_CASES)
def test_segment_placement_among_the_workgroups(fs, orc, m, before, after, lo_mod, ends):
    """`p == lo` picks the sorting workgroup: lo first, second and last slot of its workgroup; a segment that ends at the last
    slot of the array, with a full and with a one-slot last workgroup."""
    assert_stable_step(fs, orc, S.one_cell(m, before, after))


@pytest.mark.parametrize("m_a,m_b,before,lo_b_mod", S.TWO_CASES)
def test_big_cells_back_to_back(fs, orc, m_a, m_b, before, lo_b_mod):
    """One workgroup holds the tail of cell A and the first slot of cell B: its threads must sort B before they wait on A.  Also a
    sorted cell directly followed by a rank-loop cell at the bound, and the other way round."""
    assert_stable_step(fs, orc, S.two_cells(m_a, m_b, before))


@pytest.mark.parametrize("n", S.ALL_CASES)
def test_whole_population_in_one_cell(fs, orc, n):
    """Every workgroup but the first only waits for the flag; the table has one non-zero entry."""
    assert_stable_step(fs, orc, S.all_in_one(n))


@pytest.mark.parametrize("n", S.LATTICE_N)
def test_small_and_ragged_counts(fs, orc, n):
    """k_cs_hist presets (n + 63) / 64 safe words, k_cs_scatter works in 1024-slot blocks, k_cs_fixreorder in 256-slot blocks:
    n below, on and above each, down to 2."""
    assert_stable_step(fs, orc, S.lattice(n), steps=3)


@pytest.mark.parametrize("gw,gh,count,tiles", S.TABLE_CASES)
def test_scan_table_edges(fs, orc, gw, gh, count, tiles):
    """k_scan_lookback: count = ncell + 1 around the 16 items of a thread (vector path / guarded path) and the 16384 of a tile
    (a last tile of one item; cs[ncell] written by the thread that owns item count - 1), the table's first reachable and very
    last cell occupied; 66 and 131 tiles for the look-back's second and third 64-tile trip.  Three steps: epochs of earlier
    launches sit in the state array."""
    t0 = time.perf_counter()
    assert_stable_step(fs, orc, S.table(gw, gh), steps=3)
    print(f"table {gw} x {gh}: {tiles} tiles, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("pattern", S.RUN_PATTERNS)
def test_histogram_run_aggregation(fs, orc, pattern):
    """wave_run / cell_ticket: one atomic per run of equal keys in adjacent lanes.  A wrong length or offset gives two particles
    the same slot: one is lost, one duplicated — ids stop being a permutation."""
    assert_stable_step(fs, orc, S.runs(pattern))


# ---- slab handles ------------------------------------------------------------------------------------------------------------
def match_bits(got, want, ctx):
    """tests/slab_oracle.py match_and_compare with its tolerances on position, velocity and key replaced by bit equality (the
    scene's force terms vanish exactly); density keeps match_and_compare's own rtol, the project's number for summation order."""
    from scipy.spatial import cKDTree
    from tests.slab_oracle import match_and_compare
    rtol = inspect.signature(match_and_compare).parameters["rtol"].default
    assert got.shape[0] == want.shape[0], (ctx, got.shape, want.shape)
    d, idx = cKDTree(want["predicted_position"].astype(np.float64)).query(got["predicted_position"].astype(np.float64))
    assert np.unique(idx).shape[0] == got.shape[0], f"{ctx}: matching is not a bijection"
    w = want[idx]
    worst = {f: float(np.abs(got[f].astype(np.float64) - w[f].astype(np.float64)).max())
             for f in ("predicted_position", "position", "velocity")}
    print(f"{ctx}: largest differences {worst}, density rel "
          f"{float(np.abs(got['density'] / w['density'].astype(np.float64) - 1).max()):.3g}")
    for f in ("predicted_position", "position", "velocity"):
        assert np.array_equal(got[f].view(np.uint32), w[f].view(np.uint32)), f"{ctx}: {f} not bit-equal, largest difference {worst[f]:g}"
    assert np.array_equal(got["grid"], w["grid"]), f"{ctx}: cell keys differ"
    np.testing.assert_allclose(got["density"], w["density"], rtol=rtol)


@pytest.mark.parametrize("mode", ["edge", "strips", "serial"])
def test_slab_handles_sort_big_cells(fs, mode):
    """k_cs_fixreorder<true> with cells above CS_RANK_MAX: DEAD slots behind the live ones, the device-side slot count of the
    strips, the edge-first chain.  Two cells of 2500 particles, one deep inside rank 0 and one in rank 0's last column, which
    rank 1 receives as halo and sorts as well.  Pressure and viscosity constants are 0, so positions and velocities do not
    depend on any order (tests/test_csort_scenes.py shows it on the oracle) and must be bit-equal to the single-GPU counting
    engine's; density to match_and_compare's rtol."""
    from tests.test_multi_gpu import InProcessSlabs
    st, tick, p, facts = S.slab_two_big_cells()
    n = facts["n"]
    slabs = InProcessSlabs(fs, st, (0.0, 0.0), 2, cap=n + 2 * 4096, recv=4096, serial=mode == "serial", strips=mode == "strips",
                           particles=p)
    assert slabs.bounds == facts["bounds"]
    single = fs.FluidSimulation(st, device=0, sort_mode=fs.FS_SORT_COUNTING, ref_quirks=False)
    single.upload_particles(p)
    assert slabs.owned().shape[0] == n
    for s in range(2):
        slabs.step(tick)
        single.tick(tick)
        slabs.assert_clean()
        owned = slabs.owned()
        assert owned.shape[0] == n, f"step {s}: {owned.shape[0]} owned particles of {n}"
        want = single.download_particles()
        assert np.unique(want["grid"], return_counts=True)[1].max() >= 2400
        if s == 0:                                                       # both ranks held cell B: rank 1 as halo
            for r, sim in enumerate(slabs.sims):
                rec, own = sim.download()
                cnt = np.unique(rec["grid"], return_counts=True)[1]
                assert cnt.max() >= 2500 and (~own).sum() >= (2500 if r == 1 else 1), (r, cnt.max(), int((~own).sum()))
                assert rec.shape[0] < sim.capacity                       # DEAD slots behind the live ones
        match_bits(owned, want, f"{mode} step {s}")
    for sim in slabs.sims:
        sim.close()
    single.close()

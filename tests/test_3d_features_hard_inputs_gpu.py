"""The 3D step's two opt-in passes — static colliders and colour-field surface tension (§19) — at the inputs at
which tests/test_3d_paths_gpu.py holds the plain step: operand guards, six smoothing radii, random configurations, faces, edges
and corners, walls, one-cell and thin grids, every sweep path in tolerance mode, and the host paths (timed and profiled steps,
partial and shuffled uploads).  Every case runs one state on the engine and on the checker of tests/features3d.py:
C(ST3Checker.step(state)), set back each step.  The states are those of the plain tests (tests/paths3d.py); the feature settings
of a case (sigma, tau, the field) are chosen from the checker alone in tests/features3d.py, and the CPU companions in
tests/test_surface_tension3d.py and tests/test_collide3d.py assert without a GPU that every case takes both threshold branches,
pushes and re-clamps.  FS_MATH_IEEE: byte equality of all five record fields and of surface_tension_forces(); a float that is a NaN
on the checker must be a NaN on the engine (payload and sign of a NaN are not compared: host and device default NaNs differ).
FS_MATH_TOLERANCE: the stated contract, _assert_tolerance of tests/test_3d_paths_gpu.py unchanged."""
import numpy as np
import pytest

import paths3d
from tests import features3d as F
from tests.bitcmp import assert_records_equal
from tests.test_3d_paths_gpu import _assert_tolerance

pytestmark = pytest.mark.gpu
f32 = np.float32


def _same_words(got, want, ctx):
    """word for word, except that a NaN of `want` is met by any NaN"""
    a = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(want.shape[0], -1)
    ok = a == b
    if got.dtype == np.float32:
        ok |= (np.isnan(np.ascontiguousarray(want)) & np.isnan(np.ascontiguousarray(got))).reshape(ok.shape)
    if not ok.all():
        rows = np.nonzero(~ok.all(axis=1))[0]
        raise AssertionError(f"{ctx}: differs in {rows.shape[0]} particles, first {int(rows[0])}: {got[rows[0]]} / {want[rows[0]]}")


def assert_same(got, want, got_st, want_st, ctx):
    """all five record fields, and the surface-tension forces where the pass is on"""
    assert_records_equal(got, want, ctx, nan_any=True)
    if want_st is not None:
        _same_words(got_st, want_st, f"{ctx}: st")


def _engine(fs, case, **kw):
    sim = fs.FluidSimulation3D(case.st, device=0, initial_offset=case.off, **kw)
    sim.upload_particles(case.start)
    if case.field is not None:
        sim.set_collider(case.field)
    if case.cfg is not None:
        sim.set_surface_tension(*case.cfg)
    return sim


def run_case(fs, case):
    """every step of the case: the engine equals the checker"""
    ref = case.run()
    print(F.describe(case))
    sim = _engine(fs, case)
    for s, (want, want_st) in enumerate(ref):
        sim.tick(case.tick)
        got_st = sim.surface_tension_forces() if want_st is not None else None
        assert_same(sim.download_particles(), want, got_st, want_st, f"{case.name} step {s}")
    sim.close()


# ---- a. operand guards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", F.FEATURES)
@pytest.mark.parametrize("name", F.GUARDS)
def test_operand_guards(fs, orc, name, features):
    """the twelve guard cases of the plain step and three of this file (mass_tiny: every density at the 0.1 floor;
    positions_on_plus_b: (p + b) / size == 1 in the collider's look-up; nan_next_to_everyone: a one-cell box in which one NaN
    predicted coordinate is every particle's candidate, so density and tension admit a NaN r2 on every sweep), 3 steps.  NaN and
    infinite velocities become NaN positions after a step: the look-up's NaN -> voxel 0 and the pass's NaN radius test run on steps 2 and 3."""
    run_case(fs, F.guard_case(fs, orc, name, features))


# ---- b. smoothing radii -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", paths3d.RADII)
def test_smoothing_radii(fs, orc, h):
    """6 poly6 and 3 h^2 change with h; at h = 0.05 the shared-reciprocal path of the force pass is off"""
    run_case(fs, F.radius_case(fs, orc, h))


# ---- c. random configurations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(F.RANDOM_CASES))
def test_random_configurations(fs, orc, k):
    """masses 0.5 to 2, three time steps, boxes one cell thick, coincident particles; both features, 4 steps"""
    run_case(fs, F.random_case(fs, orc, k))


# ---- d. grid edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.EDGE_CASES)
def test_grid_edges(fs, orc, name):
    """particles on every face, edge and corner; one-cell and thin grids (with a (7, 5, 3) and a one-voxel field); the block
    driven into each wall, where the collider's re-clamp follows the step's clamp"""
    run_case(fs, F.edge_case(fs, orc, name))


# ---- e. tolerance mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.TOL_CASES)
def test_tolerance_mode(fs, orc, name):
    """every path scene with SCENE_ST, one FS_MATH_TOLERANCE step from the uploaded state, under the mode's stated contract; and
    the longest row scene with a collider as well (k3_force_st<2, true>), where the particles whose position on the checker lies
    within the position contract (1e-4 h) of a voxel face are left out of the float comparison: their voxel may differ.
    SCENE_ST moves velocities by no more than 1e-4 m/s here, five times the contract's atol, so the record comparison sees little
    of the pass: surface_tension_forces() is therefore compared with the checker's st under features3d.tolerance_force_bound,
    which follows from the mode's density contract (below 1e-3 of |st| in every scene), and a zero force stays zero.
    The measured errors are printed per case before they are asserted."""
    case = F.tolerance_case(fs, orc, name)
    want, want_st = case.run()[0]
    print(F.describe(case))
    if case.figures["lowered"]:
        print(f"[features3d] {case.name}: ill-conditioned on the checker, sigma lowered to {case.sigma}")
    paths3d.check_scene(paths3d.scenes()[name.split("+")[0]], [want], F.R.ST3Checker(case.st).grid_dims)
    sim = _engine(fs, case, math_mode=fs.FS_MATH_TOLERANCE)
    sim.tick(case.tick)
    got = sim.download_particles()
    got_st = sim.surface_tension_forces()
    sim.close()
    bound, _ = F.tolerance_force_bound(case, want)
    err = np.abs(got_st.astype(np.float64) - want_st).max(axis=1)
    mag = np.linalg.norm(want_st.astype(np.float64), axis=1)
    on = mag > 0
    print(f"[tolerance] {case.name}: st error up to {float((err[on] / mag[on]).max()):.3g} of |st| "
          f"(bound there up to {float((bound[on] / mag[on]).max()):.3g}), worst share of the bound {float((err[on] / bound[on]).max()):.3g}")
    assert not got_st[~on].any(), "a particle without a force on the checker has one in tolerance mode"
    assert (err[on] <= bound[on]).all(), f"{case.name}: st outside the bound in {int((err[on] > bound[on]).sum())} particles"
    if case.field is not None:
        chk = case.checker()
        _, pre, _, _, _ = case.checker_step(chk)
        chk.close()
        keep = F.face_distance(pre, case.field, case.size) > F.CONTRACT_POS * case.h
        print(f"[features3d] {case.name}: {int((~keep).sum())} of {keep.shape[0]} particles left out (near a voxel face)")
        assert (~keep).sum() <= 0.01 * keep.shape[0]
        assert np.array_equal(got["grid"], want["grid"])
        got, want = got[keep], want[keep]
    _assert_tolerance(got, want, case.h, case.name)


# ---- f. host paths with the features on ---------------------------------------------------------------------------------------
def test_timed_and_profiled_steps_give_the_same_bits(fs):
    """6 steps by tick(), by fs3_timed_steps and with the profile enabled: the same bytes, the same forces, equal to the checker"""
    case = F.host_case(fs)
    want, want_st = case.run()[-1]
    print(F.describe(case))
    plain, prof, timed = _engine(fs, case), _engine(fs, case), _engine(fs, case)
    prof.profile(True)
    for _ in range(case.steps):
        plain.tick(case.tick); prof.tick(case.tick)
    assert timed.timed_steps(case.tick, case.steps) > 0.0
    for ctx, sim in (("tick", plain), ("profiled", prof), ("timed", timed)):
        assert_same(sim.download_particles(), want, sim.surface_tension_forces(), want_st, f"host {ctx}")
    ms, steps = prof.profile_read()
    total = sum(ms.values())
    assert steps == case.steps and np.isfinite(total) and total >= 0.0 and all(v >= 0.0 for v in ms.values()), ms
    assert plain.tick_count == prof.tick_count == timed.tick_count == case.steps
    for sim in (plain, prof, timed):
        sim.close()


def test_partial_upload_then_step(fs):
    """3 steps, half of the records uploaded anew, 2 steps: the engine equals the checker fed the same merged state, and the
    forces are those of the last step"""
    case = F.host_case(fs)
    sim, chk = _engine(fs, case), case.checker()
    for _ in range(3):
        sim.tick(case.tick)
        state = case.checker_step(chk)[0]
    k = state.shape[0] // 2
    rng = np.random.default_rng(8)
    head = state[:k].copy()
    head["position"] += rng.uniform(-0.02, 0.02, size=(k, 3)).astype(f32)
    head["velocity"] = rng.uniform(-1, 1, size=(k, 3)).astype(f32)
    sim.upload_particles(head)
    state = state.copy()
    state[:k] = head
    chk.set_particles(state)
    assert_same(sim.download_particles(), state, None, None, "the merged state")
    for s in range(2):
        sim.tick(case.tick)
        want = case.checker_step(chk)[0]
        assert_same(sim.download_particles(), want, sim.surface_tension_forces(), chk.st, f"after a partial upload, step {s}")
    sim.close(); chk.close()


def test_shuffled_upload_then_step(fs):
    """a permuted upload, then 2 steps: the engine equals the checker.  (A 3D handle has no sort-plan read-out, and 16^3 particles
    are one 4096-element tile on a grid of far fewer than 2^20 cells: no wide tile exists here to be counted; the wide-tile path
    itself is run by test_3d.py at 200^3.)"""
    case = F.host_case(fs)
    start = case.start[np.random.default_rng(6).permutation(case.start.shape[0])]
    sim, chk = _engine(fs, case), case.checker()
    sim.upload_particles(start); chk.set_particles(start)
    for s in range(2):
        sim.tick(case.tick)
        want = case.checker_step(chk)[0]
        assert_same(sim.download_particles(), want, sim.surface_tension_forces(), chk.st, f"after a shuffled upload, step {s}")
    sim.close(); chk.close()

"""The 2D step's opt-in surface tension (k_surface_tension<MASS1> and the ST instantiations of k_force,
k_force_general and k_force_quad) at the inputs at which tests/test_parity_gpu.py and tests/test_prologue_edges_gpu.py hold the
plain step: operand guards (NaN, infinite and unsafe operands, densities at the floor, isolated particles, tau exactly on a
particle's |n|, sigma < 0, sigma = inf, tau = NaN), six smoothing radii, the sixteen random configurations in both sort modes,
corner cells and ragged counts, mouse impulse and obstacle field, the other two math modes on every force path, the host paths
(timed and profiled steps, partial and shuffled uploads, enabling the pass mid-run) and the process-wide A/B switches.

Every case runs one state on the engine and on the checker (tests/st_checker.cpp through tests/st_ref.py).  The states are those
of the plain tests (tests/parity_states.py, tests/prologue_scenes.py); sigma and tau of a case are chosen from the checker alone
in tests/features2d.py, and the CPU companion in tests/test_surface_tension.py asserts without a GPU that every case takes both
branches of the threshold (or, where that is the point, exactly one).  FS_MATH_IEEE: cell keys and start_indices equal, the four
float fields and surface_tension_forces() word for word; a float that is a NaN on the checker must be a NaN on the engine
(payload and sign of a NaN are not compared: host and device default NaNs differ).  The other modes: their stated per-step
contract for the records, and for the force the bound that follows from the density contract (features2d.tolerance_force_bound)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import features2d as F
from tests.test_3d_features_hard_inputs_gpu import _same_words

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_same(got, got_start, got_st, step, ctx):
    """keys, the four float fields and start_indices, and the forces where `got_st` is given, against one checker step"""
    assert np.array_equal(got["grid"], step.rec["grid"]), f"{ctx}: cell keys differ"
    for name in F.FLOAT_FIELDS:
        _same_words(got[name], step.rec[name], f"{ctx}: {name}")
    assert np.array_equal(got_start, step.start), f"{ctx}: start_indices"
    if got_st is not None:
        _same_words(got_st, step.st, f"{ctx}: st")


def assert_engine(sim, step, ctx, st=True):
    assert_same(sim.download_particles(), sim.download_start_indices(), sim.surface_tension_forces() if st else None, step, ctx)


def _engine(fs, case, surface_tension=True, **kw):
    sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, ref_quirks=case.quirks,
                             sort_mode=fs.FS_SORT_COUNTING if case.stable else fs.FS_SORT_BITONIC, surface_tension=surface_tension, **kw)
    sim.upload_particles(case.start)
    if case.start_indices is not None:
        sim.upload_start_indices(case.start_indices)
    if case.field is not None:
        sim.upload_force_field(case.field)
    return sim


def run_case(fs, case):
    """every step of the case: the engine equals the checker"""
    ref = case.run()
    print(F.describe(case))
    sim = _engine(fs, case)
    for s, step in enumerate(ref):
        sim.tick(case.tick)
        assert_engine(sim, step, f"{case.name} step {s}")
    sim.close()


# ---- a. to e. in FS_MATH_IEEE -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_hard_inputs(fs, orc, cid):
    """guard/*: the eight scenes of test_force_quotient_guards, tiny_offsets_at_rest (offsets of 2^-149 .. 1e-7 between predicted
    positions, which tiny_offsets loses to rounding), the NaN / speed-clamp / outside-the-box scene, coincident
    particles, mass_tiny (every density at the 0.1 floor), nan_next_to_everyone (a NaN r2 for every particle of a one-cell block:
    admitted by `!(r2 > h2)`), isolated particles with tau = 0 and tau = -1 (only `nl > 0` keeps them from 0 / 0), tau_exact (tau
    is one particle's f32 |n|: `>` and not `>=`), sigma = -35, sigma = inf, tau = NaN.  radius/*: h from 0.05 to 1.  random/*: the
    sixteen configurations in both sort modes, quirks by parity.  edge/*: corner cells, ragged counts, 2, 3 and 5 particles.
    mouse_field: the impulse and the obstacle field after `ax + st.x`."""
    run_case(fs, F.case_by_id(fs, orc, cid))


# ---- the other math modes -------------------------------------------------------------------------------------------------------
def _math_mode(fs, mode):
    return fs.FS_MATH_TOLERANCE if mode == "tolerance" else fs.FS_MATH_WGSL_ULP


def assert_contract(got, got_start, step, h, ctx):
    """the modes' per-step contract against the IEEE statement (tests/test_surface_tension_gpu.py)"""
    want = step.rec
    assert np.array_equal(got["grid"], want["grid"]), f"{ctx}: cell keys"
    assert np.array_equal(got_start, step.start), f"{ctx}: start_indices"
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32)), f"{ctx}: predicted"
    for name, rtol, atol in (("density", 1e-5, 0.0), ("velocity", 1e-5, 2e-5), ("position", 0.0, 1e-4 * h)):
        err = np.abs(got[name].astype(np.float64) - want[name]) / (atol + rtol * np.abs(want[name].astype(np.float64)))
        print(f"[contract] {ctx}: {name} error up to {float(err.max()):.3g} of the contract")
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5, err_msg=ctx)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5, err_msg=ctx)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h, err_msg=ctx)


def assert_force(fs, case, got, got_st, step, mode, ctx):
    """surface_tension_forces() of a step in another math mode against the checker's st.  FS_MATH_WGSL_ULP runs the IEEE density
    pass and the IEEE surface-tension pass: where its densities equal the checker's bit for bit the force must too.  Otherwise
    (FS_MATH_TOLERANCE) the force lies within features2d.tolerance_force_bound, and a particle without a force on the checker has
    none on the engine.  Returns the worst error as a share of the bound (0.0 for a bit-equal force)."""
    want_st = step.st
    if mode == "ulp":
        exact = np.array_equal(got["density"].view(np.uint32), step.rec["density"].view(np.uint32))
        print(f"[force] {ctx}: densities {'bit-equal' if exact else 'differ'} in FS_MATH_WGSL_ULP")
        if exact:
            _same_words(got_st, want_st, f"{ctx}: st")
            return 0.0
    cg = fs.build_uniform(case.st, case.tick, 1).poly6_kernel_derivative
    bound, K, _, _ = F.tolerance_force_bound(case, step.rec, cg)
    err = np.abs(got_st.astype(np.float64) - want_st).max(axis=1)
    mag = np.linalg.norm(want_st.astype(np.float64), axis=1)
    on = mag > 0
    share = float((err[on] / bound[on]).max())
    print(f"[force] {ctx}: st error up to {float((err[on] / mag[on]).max()):.3g} of |st| (bound there up to "
          f"{float((bound[on] / mag[on]).max()):.3g}), worst share of the bound {share:.3g}, K up to {int(K.max())}")
    assert not got_st[~on].any(), f"{ctx}: a particle without a force on the checker has one"
    assert (err[on] <= bound[on]).all(), f"{ctx}: st outside the bound in {int((err[on] > bound[on]).sum())} particles"
    return share


def _one_step(fs, case, mode, export=False):
    sim = _engine(fs, case, math_mode=_math_mode(fs, mode))
    if export:
        sim.export_handle(fs._abi.FS_EXPORT_PARTICLES)
    sim.tick(case.tick)
    out = sim.download_particles(), sim.download_start_indices(), sim.surface_tension_forces()
    sim.close()
    return out


@pytest.mark.parametrize("mode", ["ulp", "tolerance"])
@pytest.mark.parametrize("path", ["general", "quad", "aos"])
def test_force_paths_in_the_other_math_modes(fs, orc, monkeypatch, path, mode):
    """dense_scene (rows longer than the tiles: k_force_general and the unstaged sweeps) with the registry's sigma and tau, one step
    from the uploaded state through `general`, `quad` (FS_FORCE_QUAD_ALWAYS=1) and `aos` (a registered export handle) in
    FS_MATH_WGSL_ULP and FS_MATH_TOLERANCE: the per-step contract for the records, assert_force for the force.  k_force_quad has
    no tolerance instantiation and launch_force never hands it that mode (`mode != 2`): with FS_FORCE_QUAD_ALWAYS=1 a tolerance
    step runs the general kernel, so its records and forces are byte for byte those of the `general` row; in FS_MATH_WGSL_ULP the
    quad kernel must leave every bit where the general kernel leaves it."""
    case = F.tolerance_case(fs, orc, "dense")
    step = case.run()[0]
    print(F.describe(case))
    if path == "quad":
        monkeypatch.setenv("FS_FORCE_QUAD_ALWAYS", "1")
    got, got_start, got_st = _one_step(fs, case, mode, export=path == "aos")
    monkeypatch.delenv("FS_FORCE_QUAD_ALWAYS", raising=False)
    ctx = f"{path}/{mode}"
    assert_force(fs, case, got, got_st, step, mode, ctx)
    assert_contract(got, got_start, step, case.h, ctx)
    if path == "quad":
        plain, plain_start, plain_st = _one_step(fs, case, mode)
        assert got.tobytes() == plain.tobytes() and got_st.tobytes() == plain_st.tobytes(), f"{ctx}: not the general kernel's bytes"


@pytest.mark.parametrize("mode", ["ulp", "tolerance"])
@pytest.mark.parametrize("name", ["dam16384/mass1", "dam16384/mass1.25"])
def test_force_outside_ieee(fs, orc, name, mode):
    """One step from a checker state (records and start_indices of the disordered 16384 dam break after three checker steps), at
    mass 1 and 1.25.  FS_MATH_TOLERANCE runs k_surface_tension<false> with the separate density array and a true division per
    candidate, whatever the mass; its force lies within the bound that follows from the density contract, and a zero force stays
    zero.  Measured on the MI355X: the worst error is 0.0096 (mass 1) and 0.0108 (mass 1.25) of the bound, 0.0089 in dense_scene
    (DESIGN.md §11).  FS_MATH_WGSL_ULP: the observed case is the first one — the densities were bit-equal to the checker's in
    both scenes and on every force path of test_force_paths_in_the_other_math_modes, so the force was asserted bit-equal."""
    case = F.tolerance_case(fs, orc, name)
    step = case.run()[0]
    print(F.describe(case))
    got, got_start, got_st = _one_step(fs, case, mode)
    ctx = f"{name}/{mode}"
    assert_force(fs, case, got, got_st, step, mode, ctx)
    assert_contract(got, got_start, step, case.h, ctx)


# ---- host paths with the pass on ------------------------------------------------------------------------------------------------
def test_timed_and_profiled_steps_give_the_same_bits(fs, orc):
    """6 steps by tick(), by fs_timed_steps and with the profile enabled: the same bytes, the same forces, equal to the checker"""
    case = F.host_case(fs, orc)
    last = case.run()[-1]
    print(F.describe(case))
    plain, prof, timed = _engine(fs, case), _engine(fs, case), _engine(fs, case)
    prof.profile(True)
    for _ in range(case.steps):
        plain.tick(case.tick); prof.tick(case.tick)
    assert timed.timed_steps(case.tick, case.steps) > 0.0
    for ctx, sim in (("tick", plain), ("profiled", prof), ("timed", timed)):
        assert_engine(sim, last, f"host {ctx}")
    ms, steps = prof.profile_read()
    total = sum(ms.values())
    assert steps == case.steps and np.isfinite(total) and total >= 0.0 and all(v >= 0.0 for v in ms.values()), ms
    assert plain.tick_count == prof.tick_count == timed.tick_count == case.steps
    a, b, c = plain.download_particles().tobytes(), prof.download_particles().tobytes(), timed.download_particles().tobytes()
    assert a == b == c
    assert plain.surface_tension_forces().tobytes() == prof.surface_tension_forces().tobytes() == timed.surface_tension_forces().tobytes()
    for sim in (plain, prof, timed):
        sim.close()


def test_counting_sort_without_quirks(fs, orc):
    """the host case under FS_SORT_COUNTING with ref_quirks off, every one of its 6 steps"""
    run_case(fs, F.host_case(fs, orc, "counting", False))


def _checker_step(case, chk):
    with np.errstate(all="ignore"):
        nl = F.checker_step(chk, case.tick, case.stable)
    return F.Step(chk.particles(), chk.start_indices(), chk.st.copy(), nl)


def test_partial_upload_then_step(fs, orc):
    """3 steps, half of the records uploaded anew, 2 steps: the engine equals the checker fed the same merged state.  The forces
    are indexed by sorted slot: after the upload the engine still holds the last step's, and the next step's are the checker's."""
    case = F.host_case(fs, orc)
    sim, chk = _engine(fs, case), case.checker()
    for _ in range(3):
        sim.tick(case.tick)
        step = _checker_step(case, chk)
    assert_engine(sim, step, "before the upload")
    state = step.rec.copy()
    k = state.shape[0] // 2
    rng = np.random.default_rng(8)
    head = state[:k].copy()
    head["position"] += rng.uniform(-0.02, 0.02, size=(k, 2)).astype(f32)
    head["velocity"] = rng.uniform(-1, 1, size=(k, 2)).astype(f32)
    sim.upload_particles(head)
    state[:k] = head
    chk.set_particles(state)
    assert sim.download_particles().tobytes() == state.tobytes(), "the merged state"
    _same_words(sim.surface_tension_forces(), step.st, "the forces after the upload")
    for s in range(2):
        sim.tick(case.tick)
        assert_engine(sim, _checker_step(case, chk), f"after a partial upload, step {s}")
    sim.close(); chk.close()


def test_shuffled_upload_then_step(fs, orc):
    """a permuted upload, then 2 steps: the engine equals the checker, the forces in the new sorted order"""
    case = F.host_case(fs, orc)
    start = case.start[np.random.default_rng(6).permutation(case.start.shape[0])]
    sim, chk = _engine(fs, case), case.checker()
    sim.upload_particles(start); chk.set_particles(start)
    for s in range(2):
        sim.tick(case.tick)
        assert_engine(sim, _checker_step(case, chk), f"after a shuffled upload, step {s}")
    sim.close(); chk.close()


def test_enabling_the_pass_mid_run(fs, orc):
    """3 plain steps, then fs_set_surface_tension: the very first step with the pass — forces and records — equals the checker
    fed the downloaded state and start_indices"""
    case = F.host_case(fs, orc)
    sim = _engine(fs, case, surface_tension=False)
    for _ in range(3):
        sim.tick(case.tick)
    state, start = sim.download_particles(), sim.download_start_indices()
    sim.set_surface_tension(True)
    sim.tick(case.tick)
    chk = case.checker()
    chk.set_particles(state)
    chk.start_indices_view()[:] = start
    step = _checker_step(case, chk)
    assert step.st.any()
    assert_engine(sim, step, "the first step after enabling")
    sim.close(); chk.close()


# ---- process-wide A/B switches ----------------------------------------------------------------------------------------------------
SWITCH_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gpu_fluid_simulation_amd as fs
from oracle import oracle as orc
from tests import features2d as F
from tests.st_ref import STChecker
for case in F.switch_cases(fs, orc):
    for on in (False, True):
        sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, surface_tension=on)
        CHECK
        ref = STChecker(case.st, case.off) if on else orc.OracleSim(case.st, case.off)
        sim.upload_particles(case.start); ref.set_particles(case.start)
        for s in range(case.steps):
            sim.tick(case.tick); ref.step(case.tick)
            assert sim.download_particles().tobytes() == ref.particles().tobytes(), (case.name, on, s)
            assert np.array_equal(sim.download_start_indices(), ref.start_indices()), (case.name, on, s)
            if on:
                assert sim.surface_tension_forces().tobytes() == ref.st.tobytes() and ref.st.any(), (case.name, on, s)
        sim.close(); ref.close()
print("ok")
'''
SWITCHES = [("FS_NO_BLOCK_BOUNDS", "1", "pass"), ("FS_NO_MASS1", "1", "pass"),
            ("FS_NO_CONSTDIV", "1", 'assert fs.load_library().fs_constdiv_status(sim._h) & 19 == 0, "constant divisions should be off"'),
            ("FS_SIDE_STREAM", "1", "pass"), ("FS_XCD_CHUNK_LOG2", "0", "pass"), ("FS_XCD_CHUNK_LOG2", "8", "pass")]


@pytest.mark.parametrize("var,value,check", SWITCHES, ids=[f"{v}={x}" for v, x, _ in SWITCHES])
def test_ab_switch(var, value, check):
    """The switches are read once per process into `static const`, so each runs in a child with the variable in its environment
    only: block_tile_bounds in the density, surface-tension and force passes (FS_NO_BLOCK_BOUNDS), the general density form at
    mass 1 (FS_NO_MASS1), true divisions by 2h^3, h^2 and h (FS_NO_CONSTDIV), the fork/join launch of the pre-registered general
    work, which takes st_in too (FS_SIDE_STREAM), and xcd_block with one block and with 256 blocks per chunk (FS_XCD_CHUNK_LOG2).
    Two scenes, 3 steps each — the jittered 5000-particle dam break and dense_scene, whose long rows give the general kernel and
    so the side stream work — once plain against the oracle and once with the pass against the checker, byte for byte."""
    env = dict(os.environ)
    env[var] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", SWITCH_CHILD.replace("CHECK", check)], cwd=root, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr

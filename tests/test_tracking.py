"""CPU-side checks of the opt-in particle tracking: the checker of tests/track_ref.py is sound (its permutation
is the one the oracle's sort applies, for both sorts), ids stay a permutation, every host binding names every new call, and the
calls refuse a NULL handle without touching a device.  Last, the registry of the plain step's hard inputs
(tests/hard_states2d.py) on the checker alone: every case moves most slots, the tie cases have ties the two sorts arrange
differently.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

TRACK_CALLS = ("fs_track_enable", "fs_track_disable", "fs_track_channels", "fs_track_download_ids", "fs_track_upload_ids",
               "fs_track_download_attr", "fs_track_upload_attr", "fs_track_ids_device", "fs_track_attr_device",
               "fs_download_particles_by_id")


def make_checker(fs, n, seed, **kw):
    from tests.track_ref import TrackChecker, jitter_velocities
    st, off, tick = fs.dam_break_2d(n)
    chk = TrackChecker(st, off, **kw)
    chk.set_particles(jitter_velocities(chk.particles(), seed))
    return chk, tick


@pytest.mark.parametrize("n,stable", [(4096, False), (4096, True), (5000, False), (5000, True)])
def test_checker_permutation_reproduces_the_oracles_sort(fs, orc, n, stable):
    """before[perm] is byte-equal to the oracle's sorted records at every step (verify=True asserts it inside step()), the
    checker's state stays the plain oracle's, and the scene is not vacuous: most slots change occupant."""
    chk, tick = make_checker(fs, n, seed=n, verify=True)
    st, off, _ = fs.dam_break_2d(n)
    ref = orc.OracleSim(st, off)
    ref.set_particles(chk.particles())
    moved = []
    for _ in range(8):
        perm = chk.step(tick, stable_sort=stable)
        ref.step(tick, stable_sort=stable)
        assert chk.particles_view().tobytes() == ref.particles_view().tobytes()
        assert np.array_equal(chk.start_indices_view(), ref.start_indices_view())
        moved.append(float((perm != np.arange(n)).mean()))
    assert sum(m > 0.5 for m in moved) >= 6, moved
    assert (chk.ids != np.arange(n)).mean() > 0.5


@pytest.mark.parametrize("stable", [False, True])
def test_ids_stay_a_permutation_and_compose(fs, orc, stable):
    """ids are a permutation of 0..N-1 after every step, and composing the per-step permutations equals tracking the ids;
    a channel initialised to float(id) still equals the ids."""
    n = 5000
    chk, tick = make_checker(fs, n, seed=11, channels=2)
    chk.attr[0] = np.arange(n, dtype=np.float32)
    composed = np.arange(n, dtype=np.uint32)
    for _ in range(8):
        perm = chk.step(tick, stable_sort=stable)
        composed = composed[perm]
        assert np.array_equal(np.sort(chk.ids), np.arange(n, dtype=np.uint32))
        assert np.array_equal(chk.ids, composed)
    assert np.array_equal(chk.attr[0], chk.ids.astype(np.float32))
    assert not chk.attr[1].any()
    assert (chk.ids != np.arange(n)).mean() > 0.5


def test_reset_restarts_the_ids_at_the_current_slots(fs, orc):
    chk, tick = make_checker(fs, 4096, seed=3, channels=1)
    for _ in range(3):
        chk.step(tick)
    chk.reset(channels=3)
    assert np.array_equal(chk.ids, np.arange(4096, dtype=np.uint32)) and chk.attr.shape == (3, 4096)
    perm = chk.step(tick)
    assert np.array_equal(chk.ids, perm)


def test_every_layer_names_every_tracking_call(fs):
    from tests.layers import assert_every_layer_names, header_text
    assert_every_layer_names(fs, TRACK_CALLS, fs.FluidSimulation, (
        "track", "untrack", "track_channels", "particle_ids", "set_particle_ids", "attribute", "set_attribute",
        "download_particles_by_id", "particle_ids_device_ptr", "attribute_device_ptr"))
    assert re.search(r"#define\s+FS_TRACK_MAX_CHANNELS\s+4\b", header_text())


def test_null_handle_is_invalid_without_a_device(fs):
    lib = fs.load_library()
    inv = fs._abi.FS_ERR_INVALID
    buf = (C.c_uint32 * 4)()
    out = C.c_void_p()
    assert lib.fs_track_enable(None, 0) == inv
    assert lib.fs_track_disable(None) == inv
    assert lib.fs_track_channels(None) == -1
    assert lib.fs_track_download_ids(None, buf, 4) == inv
    assert lib.fs_track_upload_ids(None, buf, 4) == inv
    assert lib.fs_track_download_attr(None, 0, buf, 4) == inv
    assert lib.fs_track_upload_attr(None, 0, buf, 4) == inv
    assert lib.fs_track_ids_device(None, C.byref(out)) == inv
    assert lib.fs_track_attr_device(None, 0, C.byref(out)) == inv
    assert lib.fs_download_particles_by_id(None, buf, 4) == inv
    assert b"null" in lib.fs_last_error()


# ---- the registry of hard inputs (tests/hard_states2d.py): its cases test what they say ---------------------------------------
from tests import hard_states2d as H  # noqa: E402


@pytest.mark.parametrize("cid", H.CASE_IDS)
def test_hard_input_cases_are_not_vacuous(fs, orc, cid):
    """Every case of the registry on TrackChecker(verify=True) — the derived permutation IS the one the oracle's sort applied, at
    every step, also where records are NaN or infinite and where hundreds of keys tie — and the figures the GPU tests rest on: a
    case of at least 64 particles has a step in which more than half of the slots change occupant; a tie case run with the
    reference network has a step with slots where the network's arrangement differs from the stable one (so an id that followed
    the stable order would show); the ids stay a permutation.  tests/test_tracking_hard_inputs_gpu.py runs the same cases on
    the engine."""
    case = H.case_by_id(fs, orc, cid)
    run = case.run()                                   # verify=True inside
    print(case.describe())
    assert len(run) == case.steps >= H.MIN_STEPS
    moved, ties, finite = case.moved(), case.tie_slots(), case.finite_after()
    assert len(moved) == len(ties) == len(finite) == case.steps
    if case.n >= H.MOVED_MIN_N:
        assert max(moved) > 0.5, moved
    if case.tie_case and not case.stable:
        assert max(ties) > 0, ties
    for s, ids in enumerate(case.ids()):
        assert np.array_equal(np.sort(ids), np.arange(case.n, dtype=np.uint32)), f"step {s}"
    for s, step in enumerate(run):                     # the keys kept per step are the sorted records' keys, un-permuted
        assert np.array_equal(step.keys[step.perm], step.rec["grid"]) and np.all(step.rec["grid"][:-1] <= step.rec["grid"][1:])


def test_hard_input_registry_names_its_tie_cases_and_sorts(fs, orc):
    """coincident, one_cell, corners, dense_scene and the four strips are tie cases and run with the reference network (the
    strips, one_cell, corners and dense_scene with the counting sort as well); both sort modes and both quirk settings occur;
    the cases that do not stay finite are the two the sampler's file names."""
    tie = set(H.TIE_CASE_IDS)
    for want in ("coincident", "one_cell/bitonic", "corners/quirks/bitonic", "corners/noquirks/bitonic", "dense_scene/bitonic",
                 "strip/trips2/bitonic", "strip/trips3/bitonic", "strip/force_unstaged/bitonic", "strip/both_unstaged/bitonic"):
        assert want in tie, want
    assert len(H.CASE_IDS) == len(set(H.CASE_IDS))
    cases = [H.case_by_id(fs, orc, cid) for cid in H.CASE_IDS]
    assert {c.sort for c in cases} == set(H.SORTS) and {c.quirks for c in cases} == {True, False}
    assert {c.n for c in cases} >= {2, 3, 5, 257, 4097, 5000}
    assert sorted(c.name for c in cases if not c.stays_finite) == ["guard/inf_velocity", "nan_clamp"]

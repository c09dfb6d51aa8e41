"""GPU tests of a 3D particle count that changes at run time (include/fluidsim.h "3D particle count"):
fs3_reserve, fs3_emit_particles, fs3_emit_nozzle, fs3_remove_in_box and fs3_remove_flagged against the CPU checker of
tests/emit3d_ref.py — the unchanged 3D oracle at the current count, np.concatenate and rec[~kill].  Byte-equal in FS_MATH_IEEE
everywhere; the one tolerance-mode test uses the mode's stated contract.  Scenes are dam_break_3d(12^3) or (16^3) with jittered
velocities unless a test names a size; counts are chosen at the boundaries the kernels have (the 256-lane block, the sort's padded
size and tile, the size where the sort policy's plan starts)."""
import ctypes as C

import numpy as np
import pytest

from tests.bitcmp import assert_records_equal, assert_track_equal, bits, set_channels
from tests.bitcmp import expect_invalid as invalid

pytestmark = pytest.mark.gpu

f32 = np.float32
FIELDS = ("position", "predicted_position", "velocity", "density")


def assert_state(sim, chk, ctx):
    got, want = sim.download_particles(), chk.rec
    assert got.shape[0] == want.shape[0] == sim.particle_count, f"{ctx}: count {got.shape[0]} / {want.shape[0]}"
    assert_records_equal(got, want, ctx)


def assert_track(sim, chk, ctx):
    assert_track_equal(sim, chk, ctx)
    assert sim.next_id == chk.next_id, ctx


def steps(sim, chk, tick, k, ctx):
    for s in range(k):
        sim.tick(tick)
        chk.step(tick)
        assert_state(sim, chk, f"{ctx}, step {s + 1}")


def make(fs, n, seed=3, mode=None, track=None, **kw):
    from tests.emit3d_ref import jittered_scene
    chk, tick, st, off = jittered_scene(fs, n, seed, channels=track, **kw)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_IEEE if mode is None else mode, track=track)
    sim.upload_particles(chk.rec)
    return sim, chk, tick, st


def emit_to(sim, chk, st, count, seed):
    from tests.emit3d_ref import random_records
    rec = random_records(st, count - sim.particle_count, seed)
    sim.emit(rec)
    chk.emit(rec)
    assert sim.particle_count == count == chk.n


# ---- 1. reserve ----------------------------------------------------------------------------------------------------------
def test_reserve_preserves_everything(fs):
    sim, chk, tick, st = make(fs, 12 ** 3, track=4)
    set_channels(sim, chk, 11)
    steps(sim, chk, tick, 1, "before reserve")
    assert sim.capacity == sim.particle_count == 1728
    before = sim.download_particles()
    pts = before["predicted_position"].copy()
    sampled = sim.sample(pts)
    sim.reserve(5000)
    assert sim.capacity == 5000 and sim.particle_count == 1728 and sim.tick_count == 1
    assert sim.download_particles().tobytes() == before.tobytes()
    assert_track(sim, chk, "after reserve")
    assert sim.sample(pts).tobytes() == sampled.tobytes(), "the queries stay valid, on the same state"
    sim.reserve(3000)                                    # below the capacity: a no-op
    assert sim.capacity == 5000
    steps(sim, chk, tick, 2, "after reserve")
    assert_track(sim, chk, "two steps after reserve")
    invalid(fs, lambda: sim.reserve((1 << 28) + 1))
    assert sim.capacity == 5000
    sim.close(); chk.close()


def test_reserve_keeps_surface_tension_forces_and_the_collider(fs):
    from tests.collide3d_ref import random_field
    field = random_field((7, 5, 3), 5, mag=0.2)
    sim, chk, tick, st = make(fs, 12 ** 3, surface_tension=(0.02, 0.5), field=field)
    sim.set_surface_tension(0.02, 0.5)
    sim.set_collider(field)
    steps(sim, chk, tick, 1, "before reserve")
    forces = sim.surface_tension_forces()
    assert np.array_equal(bits(forces), bits(chk.st))
    sim.reserve(1800)
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(forces))
    assert np.array_equal(bits(sim.collider()), bits(field))
    steps(sim, chk, tick, 2, "after reserve")
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    sim.close(); chk.close()


# ---- 2. counts at every boundary the kernels have ------------------------------------------------------------------------
def test_counts_around_the_block_and_the_padded_size(fs):
    """1728 -> 1791, 1792, 1793 (the 256-lane block) -> 2047, 2048, 2049 (the sort's padded size: the plan words move at 2049)
    -> back to 2047 by removal; two steps against the checker after every change."""
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.reserve(2100)
    for k, count in enumerate([1791, 1792, 1793, 2047, 2048, 2049]):
        emit_to(sim, chk, st, count, 100 + k)
        assert_state(sim, chk, f"emitted to {count}")
        steps(sim, chk, tick, 2, f"count {count}")
    kill = np.zeros(2049, dtype=np.uint8)
    kill[[5, 1500]] = 1
    assert sim.remove(kill) == 2 == chk.remove(kill)
    assert sim.particle_count == 2047
    assert_state(sim, chk, "removed to 2047")
    steps(sim, chk, tick, 2, "count 2047 again")
    sim.sync()
    sim.close(); chk.close()


def test_counts_around_the_sort_tile(fs):
    sim, chk, tick, st = make(fs, 16 ** 3)
    sim.reserve(4100)
    steps(sim, chk, tick, 1, "4096")
    kill = np.zeros(4096, dtype=np.uint8)
    kill[2222] = 1
    assert sim.remove(kill) == 1 == chk.remove(kill)
    steps(sim, chk, tick, 2, "count 4095")
    emit_to(sim, chk, st, 4097, 7)
    steps(sim, chk, tick, 2, "count 4097")
    sim.sync()
    sim.close(); chk.close()


def test_counts_around_the_start_of_the_sort_policy(fs):
    """32^3 = 2^15 is where the sort policy's plan (certificate, plan words, stand-by kernel) starts."""
    sim, chk, tick, st = make(fs, 32 ** 3)
    sim.reserve(32 ** 3 + 64)
    steps(sim, chk, tick, 1, "32768")
    emit_to(sim, chk, st, 32769, 9)
    steps(sim, chk, tick, 2, "count 32769")
    sim.sync()
    kill = np.zeros(32769, dtype=np.uint8)
    kill[[0, 32768]] = 1
    assert sim.remove(kill) == 2 == chk.remove(kill)
    steps(sim, chk, tick, 2, "count 32767")
    sim.sync()
    sim.close(); chk.close()


# ---- 3. emitted particles in the hard places -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coincident", "outside", "on_plus_b", "nan_velocity", "extreme_cells"])
def test_emitted_particles_in_the_hard_places(fs, name):
    """What each case is, tests/test_emit3d.py asserts on the checker alone.  One step first: the emission then meets a sorted
    state at tick 1, and the coincident pair's PRNG needs the checker's tick alignment."""
    from tests.emit3d_ref import hard_records, hard_scene
    chk, tick, st, off = hard_scene(fs, name)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(chk.rec)
    sim.reserve(1800)
    steps(sim, chk, tick, 1, name)
    rec = hard_records(name, chk.rec, st)
    sim.emit(rec)
    chk.emit(rec)
    assert_state(sim, chk, f"{name}: emitted")
    steps(sim, chk, tick, 3, name)
    sim.close(); chk.close()


# ---- 4. the capacity edge ------------------------------------------------------------------------------------------------
def test_emit_to_exactly_the_capacity(fs):
    from tests.emit3d_ref import random_records
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.emit(random_records(st, 0, 1))                   # n == 0: FS_OK, even with no room at all
    invalid(fs, lambda: sim.emit(random_records(st, 1, 1)))
    sim.reserve(1800)
    emit_to(sim, chk, st, 1800, 2)
    steps(sim, chk, tick, 1, "full")
    before = sim.download_particles().tobytes()
    invalid(fs, lambda: sim.emit(random_records(st, 1, 3)))
    invalid(fs, lambda: sim.emit_nozzle((0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (0, 0, 0), 1, 1))
    assert sim.particle_count == 1800 and sim.download_particles().tobytes() == before
    sim.emit(random_records(st, 0, 4))
    lib = fs.load_library()
    assert lib.fs3_emit_particles(sim._h, None, 0) == fs._abi.FS_OK
    assert lib.fs3_emit_particles(sim._h, None, 1) == fs._abi.FS_ERR_INVALID
    assert lib.fs3_emit_particles(None, None, 0) == fs._abi.FS_ERR_INVALID
    assert sim.sample(np.zeros((1, 3), dtype=f32)).shape[0] == 1, "nothing changed: the queries stay valid"
    steps(sim, chk, tick, 1, "after the refused calls")
    sim.close(); chk.close()


# ---- 5. the nozzle -------------------------------------------------------------------------------------------------------
NOZZLE = dict(origin=(0.13, -0.21, 0.07), u=(0.045, 0.004, -0.002), v=(-0.003, 0.002, 0.026), velocity=(0.5, 2.0, -0.25))


@pytest.mark.parametrize("nu,nv", [(1, 1), (3, 5), (17, 16), (64, 64)])
def test_nozzle_layer_equals_the_formula(fs, nu, nv):
    from tests.emit3d_ref import nozzle_records
    sim, chk, tick, st = make(fs, 16 ** 3)
    sim.reserve(4096 + nu * nv)
    steps(sim, chk, tick, 1, "before")
    sim.emit_nozzle(nu=nu, nv=nv, **NOZZLE)
    chk.emit_nozzle(nu=nu, nv=nv, **NOZZLE)
    tail = sim.download_particles()[4096:]
    assert tail.tobytes() == nozzle_records(nu=nu, nv=nv, **NOZZLE).tobytes()
    assert_state(sim, chk, "emitted")
    steps(sim, chk, tick, 2, f"nozzle {nu} x {nv}")
    sim.close(); chk.close()


def test_nozzle_refusals_leave_the_state_alone(fs):
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.reserve(1728 + 16)
    steps(sim, chk, tick, 1, "before")
    before = sim.download_particles().tobytes()
    good = dict(NOZZLE, nu=4, nv=4)
    for key in ("origin", "u", "v", "velocity"):
        for bad in (np.nan, np.inf):
            for axis in range(3):
                vec = list(good[key])
                vec[axis] = bad
                invalid(fs, lambda: sim.emit_nozzle(**dict(good, **{key: vec})))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=0)))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nv=0)))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=1 << 20, nv=1 << 9)))       # nu * nv > 2^28
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=17, nv=1)))                # one more than the room
    lib = fs.load_library()
    assert lib.fs3_emit_nozzle(sim._h, None) == fs._abi.FS_ERR_INVALID
    assert sim.particle_count == 1728 and sim.download_particles().tobytes() == before
    assert sim.sample(np.zeros((1, 3), dtype=f32)).shape[0] == 1
    sim.emit_nozzle(**good)                              # exactly the room
    chk.emit_nozzle(**good)
    steps(sim, chk, tick, 1, "after")
    sim.close(); chk.close()


# ---- 6. removal ----------------------------------------------------------------------------------------------------------
def removal_case(name, rec):
    """-> ('flags', kill) or ('box', lo, hi) on the state `rec` (4096 records)."""
    n = rec.shape[0]
    p = rec["position"]
    kill = np.zeros(n, dtype=bool)
    if name == "every_third":
        kill[::3] = True
    elif name == "first_and_last_block":
        kill[:256] = True
        kill[n - 256:] = True
    elif name == "slot_0":
        kill[0] = True
    elif name == "last_slot":
        kill[n - 1] = True
    elif name == "two_particles_coordinates":
        a, b = p[100], p[3000]
        return "box", np.minimum(a, b), np.maximum(a, b)
    return "flags", kill


@pytest.mark.parametrize("name", ["every_third", "first_and_last_block", "slot_0", "last_slot", "two_particles_coordinates"])
def test_removal_is_a_stable_compaction(fs, name):
    from tests.emit3d_ref import kill_box
    sim, chk, tick, st = make(fs, 16 ** 3)
    steps(sim, chk, tick, 1, "before")
    case = removal_case(name, chk.rec)
    if case[0] == "box":
        kill = kill_box(chk.rec, case[1], case[2])
        assert kill[100] and kill[3000], "the edges are inclusive: both particles go"
        removed = sim.remove_box(case[1], case[2])
    else:
        kill = case[1]
        removed = sim.remove(kill)
    assert removed == int(kill.sum()) == chk.remove(kill)
    assert sim.particle_count == 4096 - removed
    assert_state(sim, chk, f"{name}: compacted")
    steps(sim, chk, tick, 2, name)
    sim.close(); chk.close()


def test_removal_that_matches_nothing_or_too_much_changes_nothing(fs):
    from tests.emit3d_ref import kill_box
    sim, chk, tick, st = make(fs, 16 ** 3)
    steps(sim, chk, tick, 1, "before")
    before = sim.download_particles()
    pts = before["predicted_position"][:64].copy()
    sampled = sim.sample(pts).tobytes()
    assert sim.remove_box((50.0, 50.0, 50.0), (60.0, 60.0, 60.0)) == 0
    assert sim.remove_box((1.0, 1.0, 1.0), (-1.0, -1.0, -1.0)) == 0              # lo > hi: an empty box
    assert sim.remove(np.zeros(4096, dtype=np.uint8)) == 0
    assert sim.download_particles().tobytes() == before.tobytes()
    assert sim.sample(pts).tobytes() == sampled, "nothing matched: the queries stay valid"
    # all but one: the particle with the largest x stays outside
    x = before["position"][:, 0]
    k = int(np.argmax(x))
    big = f32(1e6)
    lo, hi = (-big, -big, -big), (np.nextafter(x[k], f32(-np.inf)), big, big)
    assert int(kill_box(before, lo, hi).sum()) == 4095
    lib = fs.load_library()
    removed = C.c_uint32(77)
    a, b = fs.Vec3(*[float(v) for v in lo]), fs.Vec3(*[float(v) for v in hi])
    assert lib.fs3_remove_in_box(sim._h, C.byref(a), C.byref(b), C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert removed.value == 0
    flags = np.ones(4096, dtype=np.uint8)
    removed = C.c_uint32(77)
    assert lib.fs3_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4096, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert removed.value == 0
    assert lib.fs3_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4095, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    for args in ((None, C.byref(a), C.byref(b), C.byref(removed)), (sim._h, None, C.byref(b), C.byref(removed)),
                 (sim._h, C.byref(a), None, C.byref(removed)), (sim._h, C.byref(a), C.byref(b), None)):
        assert lib.fs3_remove_in_box(*args) == fs._abi.FS_ERR_INVALID
    assert lib.fs3_remove_flagged(sim._h, None, 4096, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert lib.fs3_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4096, None) == fs._abi.FS_ERR_INVALID
    assert sim.particle_count == 4096 and sim.download_particles().tobytes() == before.tobytes()
    assert sim.sample(pts).tobytes() == sampled
    steps(sim, chk, tick, 1, "after the refused calls")
    sim.close(); chk.close()


def test_nan_position_inside_the_box_is_kept(fs):
    from tests.emit3d_ref import kill_box
    sim, chk, tick, st = make(fs, 16 ** 3)
    rec = chk.rec.copy()
    rec["position"][1234, 0] = np.nan                    # y and z inside the box below
    sim.upload_particles(rec)
    chk.set_particles(rec)
    big = f32(1e6)
    lo, hi = (-big, -big, -big), (rec["position"][:, 0][np.isfinite(rec["position"][:, 0])].mean(), big, big)
    kill = kill_box(rec, lo, hi)
    assert not kill[1234] and 1000 < kill.sum() < 3500
    assert sim.remove_box(lo, hi) == int(kill.sum()) == chk.remove(kill)
    assert_state(sim, chk, "compacted")
    assert np.isnan(sim.download_particles()["position"][:, 0]).sum() == 1
    steps(sim, chk, tick, 2, "with the NaN kept")
    sim.close(); chk.close()


# ---- 7. the stale tail ---------------------------------------------------------------------------------------------------
def test_nan_records_left_behind_the_live_count_touch_nothing(fs):
    """The last 100 records are all-NaN and removed by flags: the NaNs now sit in [n, n + 100) and in the slack behind pred[n - 1]."""
    from tests.sample3d_ref import Sample3Checker
    sim, chk, tick, st = make(fs, 16 ** 3)
    rec = chk.rec.copy()
    for fld in FIELDS:
        rec[fld][-100:] = np.nan
    sim.upload_particles(rec)
    chk.set_particles(rec)
    kill = np.zeros(4096, dtype=np.uint8)
    kill[-100:] = 1
    assert sim.remove(kill) == 100 == chk.remove(kill)
    steps(sim, chk, tick, 3, "stale NaN tail")
    p = sim.download_particles()
    assert np.isfinite(p["predicted_position"]).all() and np.isfinite(p["density"]).all()
    smp = Sample3Checker(chk.settings(3996), chk.offset).load(p, tick.mass)
    pts = p["predicted_position"].copy()
    assert sim.sample(pts).tobytes() == smp.sample(pts).tobytes()
    smp.close(); sim.close(); chk.close()


# ---- 8. tracking ---------------------------------------------------------------------------------------------------------
def test_ids_and_channels_follow_emission_and_removal(fs):
    from tests.emit3d_ref import random_records
    sim, chk, tick, st = make(fs, 12 ** 3, track=4)
    sim.reserve(2000)
    set_channels(sim, chk, 21)
    assert sim.next_id == 1728
    rec = random_records(st, 70, 31)
    sim.emit(rec); chk.emit(rec)
    assert_track(sim, chk, "emit")
    assert np.array_equal(sim.particle_ids()[1728:], np.arange(1728, 1798, dtype=np.uint32))
    steps(sim, chk, tick, 1, "after emit")
    assert_track(sim, chk, "emit, step")
    assert not np.array_equal(chk.ids, np.arange(chk.n)), "the checker's permutation is the identity: the test shows nothing"
    kill = np.random.default_rng(5).random(chk.n) < 0.3
    assert sim.remove(kill) == chk.remove(kill)
    assert_track(sim, chk, "remove")
    steps(sim, chk, tick, 1, "after remove")
    assert_track(sim, chk, "remove, step")
    sim.emit_nozzle(nu=5, nv=7, **NOZZLE); chk.emit_nozzle(nu=5, nv=7, **NOZZLE)
    assert_track(sim, chk, "second emit")
    assert sim.next_id == 1728 + 70 + 35
    assert np.array_equal(sim.particle_ids()[-35:], np.arange(1798, 1833, dtype=np.uint32))
    # by id: every live particle's record at its id, the removed ids' entries untouched
    by_id = sim.download_particles_by_id()
    now, ids = sim.download_particles(), sim.particle_ids()
    small = ids < now.shape[0]
    assert by_id[ids[small]].tobytes() == now[small].tobytes()
    # upload_ids leaves next_id alone
    sim.set_particle_ids(np.arange(chk.n, dtype=np.uint32)[::-1].copy())
    assert sim.next_id == chk.next_id
    sim.track(1)                                         # a new enable starts over at the live count
    assert sim.next_id == chk.n
    sim.untrack()
    assert sim.next_id == 0
    sim.close(); chk.close()


# ---- 9. features on ------------------------------------------------------------------------------------------------------
def test_collider_and_surface_tension_across_an_emit_and_a_remove(fs):
    from tests.collide3d_ref import random_field
    from tests.emit3d_ref import random_records
    field = random_field((7, 5, 3), 8, mag=0.2)
    sim, chk, tick, st = make(fs, 12 ** 3, surface_tension=(0.02, 0.5), field=field)
    sim.set_surface_tension(0.02, 0.5)
    sim.set_collider(field)
    sim.reserve(1900)
    steps(sim, chk, tick, 1, "before")
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    rec = random_records(st, 150, 41)
    sim.emit(rec); chk.emit(rec)
    invalid(fs, sim.surface_tension_forces)              # between the change and the next step
    steps(sim, chk, tick, 2, "after emit")
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    kill = np.random.default_rng(6).random(chk.n) < 0.25
    assert sim.remove(kill) == chk.remove(kill)
    invalid(fs, sim.surface_tension_forces)
    steps(sim, chk, tick, 2, "after remove")
    assert sim.surface_tension_forces().shape[0] == chk.n
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    sim.close(); chk.close()


# ---- 10. queries ---------------------------------------------------------------------------------------------------------
def test_queries_wait_for_a_step_after_a_change(fs):
    from tests.emit3d_ref import random_records
    from tests.sample3d_ref import Sample3Checker
    sim, chk, tick, st = make(fs, 12 ** 3, track=1)
    sim.reserve(1800)
    cam = fs.look_at_camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.9, 8, 8)
    sp = fs.SurfaceParams3(10.0, 0.0, 0.05, 64, 4)
    pts = np.zeros((4, 3), dtype=f32)

    def all_queries():
        return [lambda: sim.sample(pts), lambda: sim.sample_attr(pts), lambda: sim.render_surface(cam, sp),
                lambda: sim.extract_surface(4, 4, 4, 10.0)]

    def change_emit():
        rec = random_records(st, 13, 51)
        sim.emit(rec); chk.emit(rec)

    def change_nozzle():
        sim.emit_nozzle(nu=2, nv=3, **NOZZLE); chk.emit_nozzle(nu=2, nv=3, **NOZZLE)

    def change_remove():
        kill = np.zeros(chk.n, dtype=np.uint8)
        kill[::7] = 1
        assert sim.remove(kill) == chk.remove(kill)

    for change in (change_emit, change_nozzle, change_remove):
        steps(sim, chk, tick, 1, "valid again")
        for q in all_queries():
            q()
        change()
        for q in all_queries():
            invalid(fs, q)
    steps(sim, chk, tick, 1, "last")
    n = sim.particle_count
    assert round(n ** (1 / 3)) ** 3 != n, "a count that is no cube"
    p = sim.download_particles()
    smp = Sample3Checker(chk.settings(n), chk.offset).load(p, tick.mass)
    own = p["predicted_position"].copy()
    assert sim.sample(own).tobytes() == smp.sample(own).tobytes()
    smp.close(); sim.close(); chk.close()


def test_rendering_and_extraction_with_a_live_count_below_the_capacity(fs):
    """reserve, emit 150, step, remove a quarter, step: after each of the two steps the G-buffer at 37 x 23 and the meshes on
    (17, 9, 6) and (33, 33, 33) equal their checkers, both loaded from the download at the live count"""
    from tests.emit3d_ref import random_records
    from tests.mesh3d_ref import Mesh3Checker, scene_views
    from tests.render3d_ref import Render3Checker, iso_of, params, scene_cameras
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.reserve(1900)

    def check(ctx):
        n = sim.particle_count
        assert n < sim.capacity == 1900
        p = sim.download_particles()
        assert p.shape[0] == n and all(np.isfinite(p[fld]).all() for fld in FIELDS)
        live, iso = chk.settings(n), iso_of(p)
        rnd = Render3Checker(live, chk.offset).load(p, tick.mass)
        kinds = set()
        for name, (cam, t_near) in scene_cameras(live, p, 37, 23).items():
            for refine in (0, 8):
                sp = params(iso, t_near, 0.5 * st.smoothing_radius, 64, refine)
                want = rnd.render(cam, sp)
                got = sim.render_surface(fs.Camera3.from_buffer_copy(bytes(cam)), fs.SurfaceParams3.from_buffer_copy(bytes(sp)))
                assert got.tobytes() == want.tobytes(), f"{ctx}: render {name} refine {refine}"
                kinds.update(np.unique(want["hit"]).tolist())
        assert kinds == {0, 1, 2}, f"{ctx}: hit kinds {kinds}"
        rnd.close()
        msh = Mesh3Checker(live, chk.offset).load(p, tick.mass)
        most = 0
        for name, (wmin, wmax) in scene_views(live, p).items():
            for dims in ((17, 9, 6), (33, 33, 33)):
                want_v, want_t, want_c = msh.extract(dims, wmin, wmax, iso)
                got_v, got_t = sim.extract_surface(*dims, iso, wmin, wmax)
                assert (got_v.shape[0], got_t.shape[0]) == want_c, f"{ctx}: mesh {name} {dims}: counts"
                assert got_v.tobytes() == want_v.tobytes() and got_t.tobytes() == want_t.tobytes(), f"{ctx}: mesh {name} {dims}"
                most = max(most, want_c[0])
        assert most > 500, f"{ctx}: the largest mesh has {most} vertices"
        msh.close()

    rec = random_records(st, 150, 81)
    sim.emit(rec); chk.emit(rec)
    steps(sim, chk, tick, 1, "after emit")
    assert sim.particle_count == 1878
    check("1878 of 1900")
    kill = np.random.default_rng(7).random(chk.n) < 0.25
    assert sim.remove(kill) == chk.remove(kill)
    steps(sim, chk, tick, 1, "after remove")
    assert 1300 < sim.particle_count < 1500
    check(f"{sim.particle_count} of 1900")
    sim.close(); chk.close()


# ---- 11. stream order ----------------------------------------------------------------------------------------------------
def test_nozzle_between_steps_without_a_sync(fs):
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.reserve(1728 + 35)
    for _ in range(2):
        sim.tick(tick)
    sim.emit_nozzle(nu=5, nv=7, **NOZZLE)
    for _ in range(2):
        sim.tick(tick)
    for _ in range(2):
        chk.step(tick)
    chk.emit_nozzle(nu=5, nv=7, **NOZZLE)
    for _ in range(2):
        chk.step(tick)
    assert_state(sim, chk, "step, step, nozzle, step, step")
    sim.close(); chk.close()


# ---- 12. tolerance mode --------------------------------------------------------------------------------------------------
def test_tolerance_mode_keeps_its_contract_across_count_changes(fs):
    """1728 -> 2049 -> 2047, one step after each, each from the state the handle holds: cell keys and predicted positions
    bit-exact, floats within the mode's contract (rtol 1e-5, velocity atol 2e-5, position atol 1e-4 h)."""
    sim, chk, tick, st = make(fs, 12 ** 3, mode=fs.FS_MATH_TOLERANCE)
    h = st.smoothing_radius
    sim.reserve(2049)

    def one_step(ctx):
        start = sim.download_particles()
        assert_records_equal(start, chk.rec, f"{ctx}: the change itself is a bit copy")
        sim.tick(tick)
        want = chk.step(tick)
        got = sim.download_particles()
        with np.errstate(all="ignore"):
            dv = np.abs(got["velocity"].astype(np.float64) - want["velocity"]).max()
            dx = np.abs(got["position"].astype(np.float64) - want["position"]).max()
        print(f"[tolerance] {ctx}: velocity abs {dv:.3g}, position abs {dx:.3g} (atol {1e-4 * h:.3g})")
        assert np.array_equal(got["grid"], want["grid"]), f"{ctx}: cell keys must stay bit-exact in tolerance mode"
        assert np.array_equal(bits(got["predicted_position"]), bits(want["predicted_position"])), ctx
        np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5, err_msg=ctx)
        np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5, err_msg=ctx)
        np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h, err_msg=ctx)
        chk.set_particles(got)                           # the next step starts from the handle's state, as the contract says

    one_step("1728")
    emit_to(sim, chk, st, 2049, 61)
    one_step("2049")
    kill = np.zeros(2049, dtype=np.uint8)
    kill[[17, 2040]] = 1
    assert sim.remove(kill) == 2 == chk.remove(kill)
    one_step("2047")
    sim.close(); chk.close()


# ---- 13. the timing calls ------------------------------------------------------------------------------------------------
def test_timed_steps_and_the_profile_after_a_change(fs):
    sim, chk, tick, st = make(fs, 12 ** 3)
    sim.reserve(1900)
    emit_to(sim, chk, st, 1850, 71)
    assert sim.timed_steps(tick, 2) > 0.0
    for _ in range(2):
        chk.step(tick)
    assert_state(sim, chk, "two timed steps")
    sim.profile(True)
    kill = np.zeros(1850, dtype=np.uint8)
    kill[:50] = 1
    assert sim.remove(kill) == 50 == chk.remove(kill)
    steps(sim, chk, tick, 2, "profiled")
    ms, count = sim.profile_read()
    assert count == 2 and all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    sim.close(); chk.close()


# ---- 14. the feature unused ----------------------------------------------------------------------------------------------
def test_a_handle_that_never_calls_them_stays_the_oracle(fs, orc):
    from tests.track3d_ref import jitter_velocities3
    st, off, tick = fs.dam_break_3d(16 ** 3)
    ref = orc.OracleSim3D(st, off)
    p = jitter_velocities3(ref.particles(), 3)
    ref.set_particles(p)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    assert sim.capacity == sim.particle_count == 4096 and sim.next_id == 0
    for s in range(6):
        sim.tick(tick)
        ref.step(tick)
        got, want = sim.download_particles(), ref.particles_view()
        assert_records_equal(got, want, f"step {s + 1}")
    sim.close(); ref.close()

"""GPU tests of a 2D particle count that changes at run time (include/fluidsim.h "2D particle count"):
fs_reserve, fs_emit_particles, fs_emit_nozzle, fs_remove_in_box and fs_remove_flagged against the CPU checker of
tests/emit2d_ref.py — the unchanged 2D oracle at the current count with the carried start_indices table, np.concatenate and
rec[~kill].  Byte-equal in FS_MATH_IEEE everywhere, in both sort modes unless a test is about one of them; the one
tolerance-mode test uses the mode's stated contract.  Scenes are dam_break_2d(n) with jittered velocities; counts are chosen at
the boundaries the kernels have (the 256-lane block, the sort's padded size and 4096-element tile, the size where the sort
policy's plan starts).  The numbers in the section comments are those of the feature's issue."""
import ctypes as C

import numpy as np
import pytest

from tests import emit2d_ref as ER
from tests.bitcmp import assert_records_equal, assert_track_equal, bits, set_channels
from tests.bitcmp import expect_invalid as invalid

pytestmark = pytest.mark.gpu

f32 = np.float32
FIELDS = ("position", "predicted_position", "velocity", "density")
SORTS = ER.SORTS
NOZZLE = dict(origin=(0.13, -0.21), u=(0.045, 0.004), v=(-0.003, 0.026), velocity=(0.5, 2.0))


def assert_state(sim, chk, ctx):
    got, want = sim.download_particles(), chk.rec
    assert got.shape[0] == want.shape[0] == sim.particle_count, f"{ctx}: count {got.shape[0]} / {want.shape[0]}"
    assert_records_equal(got, want, ctx)
    assert np.array_equal(sim.download_start_indices(), chk.start), f"{ctx}: start_indices differ"


def assert_track(sim, chk, ctx):
    assert_track_equal(sim, chk, ctx)
    assert sim.next_id == chk.next_id, ctx


def steps(sim, chk, tick, k, ctx):
    for s in range(k):
        sim.tick(tick)
        chk.step(tick)
        assert_state(sim, chk, f"{ctx}, step {s + 1}")
        assert sim.uniform().particle_count == chk.n


def sort_mode(fs, sort):
    return fs.FS_SORT_COUNTING if sort == "counting" else fs.FS_SORT_BITONIC


def make(fs, n, sort="bitonic", seed=3, mode=None, track=None, quirks=True, capacity=0, surface_tension=False, field=None):
    chk, tick, st, off = ER.jittered_scene(fs, n, seed, sort=sort, ref_quirks=quirks, channels=track,
                                           surface_tension=surface_tension, field=field)
    sim = fs.FluidSimulation(st, device=0, sort_mode=sort_mode(fs, sort), ref_quirks=quirks, initial_offset=off, capacity=capacity,
                             math_mode=fs.FS_MATH_IEEE if mode is None else mode, surface_tension=surface_tension, track=track)
    sim.upload_particles(chk.rec)
    if field is not None:
        sim.upload_force_field(field)
    return sim, chk, tick, st


def emit_to(sim, chk, st, count, seed):
    rec = ER.random_records(st, count - sim.particle_count, seed)
    sim.emit(rec)
    chk.emit(rec)
    assert sim.particle_count == count == chk.n


def remove_slots(sim, chk, slots):
    kill = np.zeros(chk.n, dtype=np.uint8)
    kill[list(slots)] = 1
    assert sim.remove(kill) == len(slots) == chk.remove(kill)


def push_field(st, seed):
    """A sparse obstacle field: a few patches of small push vectors, zero elsewhere."""
    rng = np.random.default_rng(seed)
    w, h = st.texture_size.x, st.texture_size.y
    field = np.zeros((h, w, 2), dtype=f32)
    for _ in range(6):
        x, y = int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64))
        field[y:y + 64, x:x + 64] = rng.uniform(-0.05, 0.05, size=2).astype(f32)
    return field


# ---- 3. counting mode, many changes in a row: the scratch layout.  First in the file on purpose ------------------
def test_counting_mode_many_changes_in_a_row(fs):
    """emit 1, step, remove 1, step, emit 300, step, remove 700, step, four more steps at ~3000 particles.  With a scratch laid out
    by the live count the look-back words and the ticket would land in former sort data after the first change."""
    sim, chk, tick, st = make(fs, 3025, sort="counting")
    sim.reserve(3400)
    steps(sim, chk, tick, 1, "before")
    emit_to(sim, chk, st, 3026, 11)
    steps(sim, chk, tick, 1, "emit 1")
    remove_slots(sim, chk, [1500])
    steps(sim, chk, tick, 1, "remove 1")
    emit_to(sim, chk, st, 3325, 12)
    steps(sim, chk, tick, 1, "emit 300")
    kill = np.random.default_rng(13).permutation(3325) < 700
    assert sim.remove(kill) == 700 == chk.remove(kill)
    steps(sim, chk, tick, 5, "remove 700")
    sim.sync()
    sim.close(); chk.close()


# ---- 1. reserve ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_reserve_preserves_everything(fs, sort):
    sim, chk, tick, st = make(fs, 1764, sort=sort, track=4)
    set_channels(sim, chk, 11)
    steps(sim, chk, tick, 1, "before reserve")
    assert sim.capacity == sim.particle_count == 1764
    before, table = sim.download_particles(), sim.download_start_indices()
    grid, image = sim.sample_grid(37, 23, attributes=True), sim.render_density(37, 23)
    sim.reserve(5000)
    assert sim.capacity == 5000 and sim.particle_count == 1764 and sim.tick_count == 1
    assert sim.download_particles().tobytes() == before.tobytes()
    assert sim.download_start_indices().tobytes() == table.tobytes()
    assert_track(sim, chk, "after reserve")
    again = sim.sample_grid(37, 23, attributes=True)
    assert again[0].tobytes() == grid[0].tobytes() and again[1].tobytes() == grid[1].tobytes(), "the queries stay valid, on the same state"
    assert sim.render_density(37, 23).tobytes() == image.tobytes()
    sim.reserve(3000)                                    # below the capacity: a no-op
    assert sim.capacity == 5000
    steps(sim, chk, tick, 3, "after reserve")
    assert_track(sim, chk, "three steps after reserve")
    invalid(fs, lambda: sim.reserve((1 << 28) + 1))
    assert sim.capacity == 5000
    sim.close(); chk.close()


@pytest.mark.parametrize("sort", SORTS)
def test_reserve_keeps_surface_tension_forces_and_the_force_field(fs, sort):
    st0 = fs.dam_break_2d(1764)[0]
    field = push_field(st0, 5)
    sim, chk, tick, st = make(fs, 1764, sort=sort, surface_tension=True, field=field)
    steps(sim, chk, tick, 1, "before reserve")
    forces = sim.surface_tension_forces()
    assert np.array_equal(bits(forces), bits(chk.st))
    sim.reserve(1800)
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(forces))
    steps(sim, chk, tick, 3, "after reserve")
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    sim.close(); chk.close()


# ---- 2. counts at every boundary the kernels have ------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_counts_around_the_block_and_the_padded_size(fs, sort):
    """1764 -> 1791, 1792, 1793 (the 256-lane block) -> 2047, 2048, 2049 (the sort's padded size: the plan words move at 2049)
    -> back to 2047 by removal; two steps against the checker after every change."""
    sim, chk, tick, st = make(fs, 1764, sort=sort)
    sim.reserve(2100)
    for k, count in enumerate([1791, 1792, 1793, 2047, 2048, 2049]):
        emit_to(sim, chk, st, count, 100 + k)
        assert_state(sim, chk, f"emitted to {count}")
        steps(sim, chk, tick, 2, f"count {count}")
    remove_slots(sim, chk, [5, 1500])
    assert sim.particle_count == 2047
    assert_state(sim, chk, "removed to 2047")
    steps(sim, chk, tick, 2, "count 2047 again")
    sim.sync()
    sim.close(); chk.close()


@pytest.mark.parametrize("sort", SORTS)
def test_counts_around_the_sort_tile(fs, sort):
    sim, chk, tick, st = make(fs, 4096, sort=sort)
    sim.reserve(4100)
    steps(sim, chk, tick, 1, "4096")
    remove_slots(sim, chk, [2222])
    steps(sim, chk, tick, 2, "count 4095")
    emit_to(sim, chk, st, 4096, 6)
    steps(sim, chk, tick, 2, "count 4096")
    emit_to(sim, chk, st, 4097, 7)
    steps(sim, chk, tick, 2, "count 4097")
    sim.sync()
    sim.close(); chk.close()


@pytest.mark.parametrize("sort", SORTS)
def test_counts_around_the_start_of_the_sort_policy(fs, sort):
    """2^15 is where the bitonic sort policy's plan (certificate, plan words, stand-by kernel) starts."""
    sim, chk, tick, st = make(fs, 181 * 181, sort=sort)          # 32761
    sim.reserve(32800)
    steps(sim, chk, tick, 1, "32761")
    emit_to(sim, chk, st, 32767, 8)
    steps(sim, chk, tick, 2, "count 32767")
    emit_to(sim, chk, st, 32769, 9)
    steps(sim, chk, tick, 2, "count 32769")
    sim.sync()
    remove_slots(sim, chk, [0, 32768])
    steps(sim, chk, tick, 2, "count 32767 again")
    sim.sync()
    sim.close(); chk.close()


# ---- 4. emitted particles in the hard places -----------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", ER.HARD_CASES)
def test_emitted_particles_in_the_hard_places(fs, name, sort):
    """What each case is, tests/test_emit2d.py asserts on the checker alone.  One step first: the emission then meets a sorted
    state at tick 1, and the coincident pair's PRNG needs the checker's tick alignment."""
    sim, chk, tick, st = make(fs, 1764, sort=sort)
    sim.reserve(1800)
    steps(sim, chk, tick, 1, name)
    rec = ER.hard_records(name, chk.rec, st)
    sim.emit(rec)
    chk.emit(rec)
    assert_state(sim, chk, f"{name}: emitted")
    steps(sim, chk, tick, 3, name)
    sim.close(); chk.close()


# ---- 5. a nozzle into one cell -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_nozzle_of_300_records_into_one_cell(fs, sort):
    """20 x 15 records, 4 mm apart, centred on the centre of a cell in the middle of the block: a row of more than 32 candidates
    and a cell that spans two 256-blocks (the pre-registered list, the general force kernel, the counting sort's ranked fix-up)."""
    sim, chk, tick, st = make(fs, 2048, sort=sort)
    sim.reserve(2048 + 300)
    steps(sim, chk, tick, 1, "before")
    h = f32(st.smoothing_radius)
    half = f32([st.size.x, st.size.y]) * f32(0.5)
    mid = np.median(chk.rec["position"], axis=0).astype(f32)
    origin = (np.floor((mid + half) / h) + f32(0.5)) * h - half
    args = dict(origin=origin, u=(0.004, 0.0), v=(0.0, 0.004), velocity=(0.0, 0.0), nu=20, nv=15)
    sim.emit_nozzle(**args)
    chk.emit_nozzle(**args)
    assert_state(sim, chk, "emitted")
    steps(sim, chk, tick, 1, "nozzle, first step")
    keys, counts = np.unique(chk.rec["grid"], return_counts=True)
    assert counts.max() >= 300, "all 300 records fell into one cell"
    first = int(np.flatnonzero(chk.rec["grid"] == keys[np.argmax(counts)])[0])
    assert first // 256 != (first + int(counts.max()) - 1) // 256, "and the cell spans two 256-blocks"
    steps(sim, chk, tick, 1, "nozzle, second step")
    sim.close(); chk.close()


# ---- 6. nozzle shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("nu,nv", [(1, 1), (15, 1), (17, 16), (64, 64)])
def test_nozzle_equals_the_formula(fs, nu, nv, sort):
    sim, chk, tick, st = make(fs, 4096, sort=sort)
    sim.reserve(4096 + nu * nv)
    steps(sim, chk, tick, 1, "before")
    sim.emit_nozzle(nu=nu, nv=nv, **NOZZLE)
    chk.emit_nozzle(nu=nu, nv=nv, **NOZZLE)
    tail = sim.download_particles()[4096:]
    assert tail.tobytes() == ER.nozzle_records(nu=nu, nv=nv, **NOZZLE).tobytes()
    assert_state(sim, chk, "emitted")
    steps(sim, chk, tick, 2, f"nozzle {nu} x {nv}")
    sim.close(); chk.close()


def test_nozzle_refusals_leave_the_state_alone(fs):
    sim, chk, tick, st = make(fs, 1764)
    sim.reserve(1764 + 16)
    steps(sim, chk, tick, 1, "before")
    before = sim.download_particles().tobytes()
    good = dict(NOZZLE, nu=4, nv=4)
    for key in ("origin", "u", "v", "velocity"):
        for bad in (np.nan, np.inf):
            for axis in range(2):
                vec = list(good[key])
                vec[axis] = bad
                invalid(fs, lambda: sim.emit_nozzle(**dict(good, **{key: vec})))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=0)))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nv=0)))
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=1 << 20, nv=1 << 9)))       # nu * nv > 2^28
    invalid(fs, lambda: sim.emit_nozzle(**dict(good, nu=17, nv=1)))                # one more than the room
    lib = fs.load_library()
    assert lib.fs_emit_nozzle(sim._h, None) == fs._abi.FS_ERR_INVALID
    assert sim.particle_count == 1764 and sim.download_particles().tobytes() == before
    assert sim.sample(np.zeros((1, 2), dtype=f32)).shape[0] == 1
    sim.emit_nozzle(**good)                              # exactly the room
    chk.emit_nozzle(**good)
    steps(sim, chk, tick, 1, "after")
    sim.close(); chk.close()


# ---- 7. the capacity edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_emit_to_exactly_the_capacity(fs, sort):
    sim, chk, tick, st = make(fs, 1764, sort=sort)
    sim.emit(ER.random_records(st, 0, 1))                # n == 0: FS_OK, even with no room at all
    invalid(fs, lambda: sim.emit(ER.random_records(st, 1, 1)))
    sim.reserve(1800)
    emit_to(sim, chk, st, 1800, 2)
    steps(sim, chk, tick, 1, "full")
    before = sim.download_particles().tobytes()
    invalid(fs, lambda: sim.emit(ER.random_records(st, 1, 3)))
    invalid(fs, lambda: sim.emit_nozzle((0, 0), (0.1, 0), (0, 0.1), (0, 0), 1, 1))
    assert sim.particle_count == 1800 and sim.download_particles().tobytes() == before
    lib = fs.load_library()
    assert lib.fs_emit_particles(sim._h, None, 0) == fs._abi.FS_OK
    assert lib.fs_emit_particles(sim._h, None, 1) == fs._abi.FS_ERR_INVALID
    assert lib.fs_emit_particles(None, None, 0) == fs._abi.FS_ERR_INVALID
    assert sim.sample(np.zeros((1, 2), dtype=f32)).shape[0] == 1, "nothing changed: the queries stay valid"
    steps(sim, chk, tick, 1, "after the refused calls")
    sim.close(); chk.close()


# ---- 8. removal ----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", ["every_third", "first_and_last_block", "slot_0", "last_slot", "two_particles_coordinates"])
def test_removal_is_a_stable_compaction(fs, name, sort):
    sim, chk, tick, st = make(fs, 4096, sort=sort)
    steps(sim, chk, tick, 1, "before")
    case = removal_case(name, chk.rec)
    if case[0] == "box":
        kill = ER.kill_box(chk.rec, case[1], case[2])
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
    sim, chk, tick, st = make(fs, 4096)
    steps(sim, chk, tick, 1, "before")
    before = sim.download_particles()
    pts = before["predicted_position"][:64].copy()
    sampled, image = sim.sample(pts).tobytes(), sim.render_density(16, 16).tobytes()
    assert sim.remove_box((500.0, 500.0), (600.0, 600.0)) == 0
    assert sim.remove_box((1.0, 1.0), (-1.0, -1.0)) == 0                          # lo > hi: an empty box
    assert sim.remove(np.zeros(4096, dtype=np.uint8)) == 0
    assert sim.download_particles().tobytes() == before.tobytes()
    assert sim.sample(pts).tobytes() == sampled and sim.render_density(16, 16).tobytes() == image, "nothing matched: the queries stay valid"
    # all but one: the particle with the largest x stays outside
    x = before["position"][:, 0]
    k = int(np.argmax(x))
    assert (x == x[k]).sum() == 1
    big = f32(1e6)
    lo, hi = (-big, -big), (np.nextafter(x[k], f32(-np.inf)), big)
    assert int(ER.kill_box(before, lo, hi).sum()) == 4095
    lib = fs.load_library()
    removed = C.c_uint32(77)
    a, b = fs.Vec2(*[float(v) for v in lo]), fs.Vec2(*[float(v) for v in hi])
    assert lib.fs_remove_in_box(sim._h, C.byref(a), C.byref(b), C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert removed.value == 0
    flags = np.ones(4096, dtype=np.uint8)
    removed = C.c_uint32(77)
    assert lib.fs_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4096, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert removed.value == 0
    assert lib.fs_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4095, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    for args in ((None, C.byref(a), C.byref(b), C.byref(removed)), (sim._h, None, C.byref(b), C.byref(removed)),
                 (sim._h, C.byref(a), None, C.byref(removed)), (sim._h, C.byref(a), C.byref(b), None)):
        assert lib.fs_remove_in_box(*args) == fs._abi.FS_ERR_INVALID
    assert lib.fs_remove_flagged(sim._h, None, 4096, C.byref(removed)) == fs._abi.FS_ERR_INVALID
    assert lib.fs_remove_flagged(sim._h, flags.ctypes.data_as(C.c_void_p), 4096, None) == fs._abi.FS_ERR_INVALID
    assert sim.particle_count == 4096 and sim.download_particles().tobytes() == before.tobytes()
    assert sim.sample(pts).tobytes() == sampled
    steps(sim, chk, tick, 1, "after the refused calls")
    sim.close(); chk.close()


@pytest.mark.parametrize("sort", SORTS)
def test_nan_position_inside_the_box_is_kept(fs, sort):
    sim, chk, tick, st = make(fs, 4096, sort=sort)
    rec = chk.rec.copy()
    rec["position"][1234, 0] = np.nan                    # y inside the box below
    sim.upload_particles(rec)
    chk.set_particles(rec)
    big = f32(1e6)
    lo, hi = (-big, -big), (rec["position"][:, 0][np.isfinite(rec["position"][:, 0])].mean(), big)
    kill = ER.kill_box(rec, lo, hi)
    assert not kill[1234] and 1000 < kill.sum() < 3500
    assert sim.remove_box(lo, hi) == int(kill.sum()) == chk.remove(kill)
    assert_state(sim, chk, "compacted")
    assert np.isnan(sim.download_particles()["position"][:, 0]).sum() == 1
    steps(sim, chk, tick, 2, "with the NaN kept")
    sim.close(); chk.close()


# ---- 9. the stale tail ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_nan_records_left_behind_the_live_count_touch_nothing(fs, sort):
    """The last 100 records are all-NaN and removed by flags: the NaNs now sit in [n, n + 100) and in the slack behind
    pred[n - 1].  Then the same through a larger reserve: 200 all-NaN records emitted into the new arrays and removed again."""
    from tests.sample_ref import SampleChecker
    sim, chk, tick, st = make(fs, 4096, sort=sort)
    rec = chk.rec.copy()
    for fld in FIELDS:
        rec[fld][-100:] = np.nan
    sim.upload_particles(rec)
    chk.set_particles(rec)
    kill = np.zeros(4096, dtype=np.uint8)
    kill[-100:] = 1
    assert sim.remove(kill) == 100 == chk.remove(kill)
    steps(sim, chk, tick, 1, "stale NaN tail")
    sim.reserve(4400)
    nan = np.zeros(200, dtype=ER.DTYPE)
    for fld in FIELDS:
        nan[fld] = np.nan
    nan["grid"] = 0xFFFFFFFF
    sim.emit(nan)
    kill = np.zeros(3996 + 200, dtype=np.uint8)
    kill[3996:] = 1
    assert sim.remove(kill) == 200
    assert_state(sim, chk, "emitted and removed again")
    steps(sim, chk, tick, 3, "stale NaN tail in the new arrays")
    p = sim.download_particles()
    assert np.isfinite(p["predicted_position"]).all() and np.isfinite(p["density"]).all()
    smp = SampleChecker(chk.settings(3996), chk.offset)
    smp.load(p, sim.download_start_indices(), sim.uniform())
    pts = p["predicted_position"].copy()
    assert sim.sample(pts).tobytes() == smp.sample(pts)[0].tobytes()
    smp.close(); sim.close(); chk.close()


# ---- 10. the quirk table across a removal --------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("quirks", [True, False])
def test_start_table_across_a_removal(fs, quirks, sort):
    """tests/test_emit2d.py's case on the device: every low cell is removed, the new first cell's stale start names a slot behind
    the live count.  ref_quirks = 1 walks that cell from the stale start (clamped), ref_quirks = 0 does not read the table."""
    sim, chk, tick, st = make(fs, 1764, sort=sort, quirks=quirks)
    steps(sim, chk, tick, 1, "before")
    kill = np.arange(chk.n) < (chk.n * 6) // 10
    assert sim.remove(kill) == chk.remove(kill)
    assert_state(sim, chk, "removed every low cell")
    table = chk.start.copy()
    steps(sim, chk, tick, 1, "first step after the removal")
    if quirks:
        assert table[chk.rec["grid"][0]] >= chk.n, "the case is what it says: a stale start >= the live count"
    steps(sim, chk, tick, 2, "after the removal")
    sim.close(); chk.close()


# ---- 11. tracking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_ids_and_channels_follow_emission_and_removal(fs, sort):
    sim, chk, tick, st = make(fs, 1764, sort=sort, track=4)
    sim.reserve(2000)
    set_channels(sim, chk, 21)
    assert sim.next_id == 1764
    rec = ER.random_records(st, 70, 31)
    sim.emit(rec); chk.emit(rec)
    assert_track(sim, chk, "emit")
    assert np.array_equal(sim.particle_ids()[1764:], np.arange(1764, 1834, dtype=np.uint32))
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
    assert sim.next_id == 1764 + 70 + 35
    assert np.array_equal(sim.particle_ids()[-35:], np.arange(1834, 1869, dtype=np.uint32))
    # by id: every live particle's record at its id, the removed ids' entries untouched
    by_id = sim.download_particles_by_id()
    now, ids = sim.download_particles(), sim.particle_ids()
    small = ids < now.shape[0]
    assert by_id[ids[small]].tobytes() == now[small].tobytes()
    gone = np.setdiff1d(np.arange(now.shape[0]), ids)
    assert gone.size > 0 and not by_id[gone].view(np.uint8).any(), "entries no id names are left as they were"
    sim.set_particle_ids(np.arange(chk.n, dtype=np.uint32)[::-1].copy())
    assert sim.next_id == chk.next_id                    # upload_ids leaves next_id alone
    sim.track(1)                                         # a new enable starts over at the live count
    assert sim.next_id == chk.n
    sim.untrack()
    assert sim.next_id == 0
    sim.close(); chk.close()


# ---- 12. surface tension -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_surface_tension_across_an_emit_and_a_remove(fs, sort):
    sim, chk, tick, st = make(fs, 1764, sort=sort, surface_tension=True)
    sim.reserve(1950)
    steps(sim, chk, tick, 1, "before")
    assert np.array_equal(bits(sim.surface_tension_forces()), bits(chk.st))
    rec = ER.random_records(st, 150, 41)
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


# ---- 13. queries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_queries_wait_for_a_step_after_a_change(fs, sort):
    from tests.sample_ref import SampleChecker
    sim, chk, tick, st = make(fs, 1764, sort=sort, track=1)
    sim.reserve(1850)
    pts = np.zeros((4, 2), dtype=f32)

    def all_queries():
        return [lambda: sim.sample(pts), lambda: sim.sample(pts, attributes=True), lambda: sim.sample_grid(4, 4),
                lambda: sim.render_density(8, 8)]

    def change_emit():
        rec = ER.random_records(st, 13, 51)
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
    p = sim.download_particles()
    smp = SampleChecker(chk.settings(sim.particle_count), chk.offset)
    smp.load(p, sim.download_start_indices(), sim.uniform())
    own = p["predicted_position"].copy()
    assert sim.sample(own).tobytes() == smp.sample(own)[0].tobytes()
    smp.close(); sim.close(); chk.close()


# ---- 14. stream order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("n", [1764, 2025])
def test_nozzle_between_steps_without_a_sync(fs, n, sort):
    """1764 + 35 stays inside the padded size 2048 (the nozzle is a plain enqueue in either mode); 2025 + 35 crosses it (the
    bitonic mode drains the stream and moves its plan words)."""
    sim, chk, tick, st = make(fs, n, sort=sort)
    sim.reserve(n + 35)
    assert (n + 35 > 2048) == (n == 2025)
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


# ---- 15. renderer hand-off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_hand_off_registered(fs, sort):
    """fs_reserve is refused (the exported allocation cannot move); emission and removal are allowed, and after the next step the
    exported view — read at the address handed out before the change — holds the new state for the new count."""
    sim, chk, tick, st = make(fs, 1764, sort=sort, capacity=2000)
    steps(sim, chk, tick, 1, "before")
    handle = sim.export_handle()
    assert handle.bytes == 1764 * 32
    view = sim.particles_device_ptr()
    invalid(fs, lambda: sim.reserve(4000))
    invalid(fs, lambda: sim.reserve(100))
    assert sim.capacity == 2000
    lib = fs.load_library()

    def read_view(n):
        out = np.empty(n, dtype=fs.PARTICLE_DTYPE)
        sim.sync()
        assert lib.fs_import_read(C.c_void_p(view), 0, out.ctypes.data_as(C.c_void_p), n * 32) == fs._abi.FS_OK
        return out

    emit_to(sim, chk, st, 1900, 81)
    sim.tick(tick); chk.step(tick)
    assert read_view(1900).tobytes() == chk.rec.tobytes(), "the view after an emission and a step"
    assert sim.particles_device_ptr() == view
    assert_state(sim, chk, "emit, step")
    kill = np.random.default_rng(7).random(1900) < 0.2
    assert sim.remove(kill) == chk.remove(kill)
    assert_state(sim, chk, "removed: the view is re-materialised for a download")
    sim.tick(tick); chk.step(tick)
    assert read_view(chk.n).tobytes() == chk.rec.tobytes(), "the view after a removal and a step"
    sim.close(); chk.close()


# ---- 16. slab handles ----------------------------------------------------------------------------------------------------
def test_slab_handle_refuses_every_call(fs):
    st, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    lib = fs.load_library()
    bad = fs._abi.FS_ERR_INVALID
    rec = np.zeros(4, dtype=fs.PARTICLE_DTYPE)
    z = fs.Nozzle(fs.Vec2(0, 0), fs.Vec2(0.1, 0), fs.Vec2(0, 0.1), fs.Vec2(0, 0), 2, 2)
    a, b, removed = fs.Vec2(-1, -1), fs.Vec2(1, 1), C.c_uint32(9)
    flags = np.zeros(lib.fs_particle_count(slab._h), dtype=np.uint8)
    assert lib.fs_reserve(slab._h, 1 << 20) == bad
    assert lib.fs_emit_particles(slab._h, rec.ctypes.data_as(C.c_void_p), 4) == bad
    assert lib.fs_emit_particles(slab._h, None, 0) == bad
    assert lib.fs_emit_nozzle(slab._h, C.byref(z)) == bad
    assert lib.fs_remove_in_box(slab._h, C.byref(a), C.byref(b), C.byref(removed)) == bad and removed.value == 0
    assert lib.fs_remove_flagged(slab._h, flags.ctypes.data_as(C.c_void_p), flags.shape[0], C.byref(removed)) == bad
    slab.close()


# ---- 17. tolerance mode --------------------------------------------------------------------------------------------------
def test_tolerance_mode_keeps_its_contract_across_count_changes(fs):
    """1764 -> 2049 -> 2047, one step after each, each from the state the handle holds: cell keys, start_indices and predicted
    positions bit-exact, floats within the mode's contract as include/fluidsim.h states it (rtol 1e-5, atol 1e-4 h)."""
    sim, chk, tick, st = make(fs, 1764, mode=fs.FS_MATH_TOLERANCE)
    h = st.smoothing_radius
    sim.reserve(2049)

    def one_step(ctx):
        start = sim.download_particles()
        assert_records_equal(start, chk.rec, f"{ctx}: the change itself is a bit copy")
        sim.tick(tick)
        want = chk.step(tick)
        got = sim.download_particles()
        with np.errstate(all="ignore"):
            for fld in ("density", "velocity", "position"):
                d = np.abs(got[fld].astype(np.float64) - want[fld])
                print(f"[tolerance] {ctx}: {fld} abs {d.max():.3g}, beyond rtol {np.max(d - 1e-5 * np.abs(want[fld])):.3g} (atol {1e-4 * h:.3g})")
        assert np.array_equal(got["grid"], want["grid"]), f"{ctx}: cell keys must stay bit-exact in tolerance mode"
        assert np.array_equal(sim.download_start_indices(), chk.start), f"{ctx}: start_indices must stay bit-exact"
        assert np.array_equal(bits(got["predicted_position"]), bits(want["predicted_position"])), ctx
        for fld in ("density", "velocity", "position"):
            np.testing.assert_allclose(got[fld], want[fld], rtol=1e-5, atol=1e-4 * h, err_msg=f"{ctx}: {fld}")
        assert not np.array_equal(bits(got["velocity"]), bits(want["velocity"])), "really another mode"
        chk.set_particles(got)                           # the next step starts from the handle's state, as the contract says

    one_step("1764")
    emit_to(sim, chk, st, 2049, 61)
    one_step("2049")
    remove_slots(sim, chk, [17, 2040])
    one_step("2047")
    sim.close(); chk.close()


# ---- 18. the timing calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_timed_steps_and_the_profile_after_a_change(fs, sort):
    sim, chk, tick, st = make(fs, 1764, sort=sort)
    sim.reserve(1950)
    emit_to(sim, chk, st, 1900, 71)
    assert sim.timed_steps(tick, 2) > 0.0
    for _ in range(2):
        chk.step(tick)
    assert_state(sim, chk, "two timed steps")
    sim.profile(True)
    remove_slots(sim, chk, range(50))
    steps(sim, chk, tick, 2, "profiled")
    ms, count = sim.profile_read()
    assert count == 2 and all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    sim.close(); chk.close()


# ---- 19. the feature unused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("capacity", [0, 8192])
def test_a_handle_that_never_calls_them_stays_the_oracle(fs, orc, capacity, sort):
    """Against the plain oracle, six steps; once more with capacity = 2 x count given at create (other strides, another
    workgroup-to-block mapping, the same bits)."""
    from tests.track_ref import jitter_velocities
    st, off, tick = fs.dam_break_2d(4096)
    ref = orc.OracleSim(st, off)
    p = jitter_velocities(ref.particles(), 3)
    ref.set_particles(p)
    sim = fs.FluidSimulation(st, device=0, sort_mode=sort_mode(fs, sort), initial_offset=off, capacity=capacity)
    sim.upload_particles(p)
    assert sim.capacity == max(capacity, 4096) and sim.particle_count == 4096 and sim.next_id == 0
    for s in range(6):
        sim.tick(tick)
        ref.step(tick, stable_sort=sort == "counting")
        got, want = sim.download_particles(), ref.particles_view()
        assert_records_equal(got, want, f"step {s + 1}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices_view())
    sim.close(); ref.close()

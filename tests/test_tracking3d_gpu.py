"""GPU tests of the opt-in 3D particle tracking: the ids and channels k_track_carry moves behind k3_reorder
against the CPU checker (tests/track3d_ref.py: the unchanged 3D oracle plus the permutation its sort applies), bit for bit, and
the particle records against the oracle in the same runs — tracking changes no bit of the state.  No tolerance anywhere.

Scenes: tests/track3d_ref.py SCENES, velocities drawn uniformly and uploaded to both sides.  Every test asserts on the
CHECKER's ids that slots changed occupant, so none can pass on an identity permutation."""
import ctypes as C

import numpy as np
import pytest

from tests.bitcmp import POOL_TWELVE, assert_records_equal, assert_track_equal, bits, special_bits

pytestmark = pytest.mark.gpu


def assert_state_equal(sim, chk, ctx):
    assert_records_equal(sim.download_particles(), chk.particles_view(), ctx)


def assert_not_vacuous(chk, least=0.5):
    moved = (chk.ids != np.arange(chk.n)).mean()
    assert moved > least, f"only {moved:.2f} of the checker's slots changed occupant: the test shows nothing"


def make_pair(fs, side, seed=7, channels=0, track=True, mode=None):
    from tests.track3d_ref import SCENES, Track3Checker, jitter_velocities3, scene3
    box, spacing, vmax = SCENES[side]
    st, off, tick = scene3(fs, side, box, spacing)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_IEEE if mode is None else mode,
                               track=channels if track else None)
    chk = Track3Checker(st, off, channels=channels)
    p = jitter_velocities3(chk.particles(), seed, vmax)
    chk.set_particles(p)
    sim.upload_particles(p)
    return sim, chk, tick


# ---- 1. ids bit-exact against the checker, every step; the state stays the oracle's ------------------------------------
# 8: the moving 2^3 scene; 27: less than a wave; 4096: exactly one sort tile; 4913: two tiles, the ragged grid tail of the carry
@pytest.mark.parametrize("side,least", [(2, 0.0), (3, 0.0), (16, 0.5), (17, 0.5), (40, 0.5)])
def test_ids_follow_the_sort_bit_exact(fs, side, least):
    sim, chk, tick = make_pair(fs, side)
    n = side ** 3
    assert sim.track_channels == 0
    assert np.array_equal(sim.particle_ids(), np.arange(n, dtype=np.uint32))
    for s in range(3):
        sim.tick(tick)
        perm = chk.step(tick)
        assert not np.array_equal(perm, np.arange(n)), f"side {side} step {s}: the checker's permutation is the identity"
        assert_track_equal(sim, chk, f"side {side} step {s}")
        assert_state_equal(sim, chk, f"side {side} step {s}")
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(n, dtype=np.uint32))
    assert_not_vacuous(chk, least)
    sim.close(); chk.close()


def test_one_step_at_a_power_of_two_runs_the_global_sort_stages(fs):
    sim, chk, tick = make_pair(fs, 64, channels=1)
    n = 64 ** 3
    v = np.arange(n, dtype=np.float32)               # exact: every id is below 2^24
    sim.set_attribute(0, v)
    chk.attr[0] = v
    sim.tick(tick)
    chk.step(tick)
    assert_track_equal(sim, chk, "64^3 one step")
    assert_state_equal(sim, chk, "64^3 one step")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 2. every instantiation, channels as bit patterns ------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])
def test_every_channel_count_one_step(fs, channels):
    n = 17 ** 3
    sim, chk, tick = make_pair(fs, 17, seed=20 + channels, channels=channels)
    for c in range(channels):
        v = special_bits(n, 50 + c, POOL_TWELVE)
        if c == 1:                                   # arbitrary words: whatever float they encode
            v = np.random.default_rng(c).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        sim.set_attribute(c, v)
        chk.attr[c] = v
        assert np.array_equal(bits(sim.attribute(c)), bits(v)), f"channel {c}: upload / download is not a bit copy"
    sim.tick(tick)
    chk.step(tick)
    assert_track_equal(sim, chk, f"C={channels} one step")
    assert_state_equal(sim, chk, f"C={channels} one step")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 3. the sort's wide-key hand-over ----------------------------------------------------------------------------------
def test_shuffled_upload_onto_a_grid_of_more_than_2_pow_20_cells(fs, orc):
    """17^3 particles at spacing 1.35 in a 24^3 box, h 0.2: 1 815 848 cells.  After a random permutation of the records every
    4096-slot tile's key span exceeds 2^20 - 1, so every tile of the first sort kernel takes the wide-key hand-over, whose pairs
    the carry must read just the same."""
    from tests.track3d_ref import Track3Checker, predict_keys, wide_grid_scene
    st, off, tick, p = wide_grid_scene(fs, orc)
    n = p.shape[0]
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, track=1)
    chk = Track3Checker(st, off, channels=1)
    w, h, d = sim.grid_dims
    assert w * h * d == 1_815_848 > (1 << 20)
    sim.upload_particles(p)
    chk.set_particles(p)
    _, keys = predict_keys(st, sim.grid_dims, p, tick.delta)
    spans = [int(keys[a:a + 4096].max()) - int(keys[a:a + 4096].min()) for a in range(0, n, 4096)]
    assert min(spans) > (1 << 20) - 1, spans
    v = np.arange(n, dtype=np.float32)
    sim.set_attribute(0, v)
    chk.attr[0] = v
    sim.tick(tick)
    chk.step(tick)
    assert_track_equal(sim, chk, "shuffled upload, wide grid")
    assert_state_equal(sim, chk, "shuffled upload, wide grid")
    assert_not_vacuous(chk, 0.9)
    sim.close(); chk.close()


# ---- 4. off is off, and on changes nothing -----------------------------------------------------------------------------
def test_tracking_changes_no_bit_with_a_collider_and_surface_tension(fs):
    from tests.track3d_ref import SCENES, jitter_velocities3, scene3
    box, spacing, vmax = SCENES[17]
    st, off, tick = scene3(fs, 17, box, spacing)
    lib = fs.load_library()
    sims = []
    for tracked in (True, False):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        sim.upload_particles(jitter_velocities3(sim.download_particles(), 7, vmax))
        sim.set_collider_mask(fs.box_mask3d((box, box, box), (12, 12, 12), (-0.6, 0.2, -0.6), (0.6, 1.2, 0.6)))
        sim.set_surface_tension(0.5, 0.1)
        if tracked:
            sim.track(4)
            for c in range(4):
                sim.set_attribute(c, special_bits(17 ** 3, c, POOL_TWELVE))
        sims.append(sim)
    a, b = sims
    buf = np.zeros(17 ** 3, dtype=np.uint32)
    out = C.c_void_p()
    for s in range(3):
        a.tick(tick); b.tick(tick)
        assert a.download_particles().tobytes() == b.download_particles().tobytes(), f"step {s}: tracking changed the state"
        assert a.surface_tension_forces().tobytes() == b.surface_tension_forces().tobytes()
    assert (a.particle_ids() != np.arange(17 ** 3)).mean() > 0.5
    # the handle that never enabled tracking
    inv = fs._abi.FS_ERR_INVALID
    assert lib.fs3_track_channels(b._h) == -1 and b.track_channels == -1
    assert lib.fs3_track_download_ids(b._h, buf.ctypes.data_as(C.c_void_p), buf.shape[0]) == inv
    assert lib.fs3_track_download_attr(b._h, 0, buf.ctypes.data_as(C.c_void_p), buf.shape[0]) == inv
    assert lib.fs3_track_ids_device(b._h, C.byref(out)) == inv
    assert lib.fs3_track_attr_device(b._h, 0, C.byref(out)) == inv
    assert lib.fs3_download_particles_by_id(b._h, buf.ctypes.data_as(C.c_void_p), 0) == inv
    a.close(); b.close()


# ---- 5. call semantics -------------------------------------------------------------------------------------------------
def test_enable_mid_run_reset_and_disable(fs):
    n = 17 ** 3
    sim, chk, tick = make_pair(fs, 17, track=False)
    assert sim.track_channels == -1
    for _ in range(3):
        sim.tick(tick)
        chk.step(tick)
    sim.track()                                   # enqueued behind the three steps, no sync in between
    chk.reset(0)
    assert sim.track_channels == 0
    assert np.array_equal(sim.particle_ids(), np.arange(n, dtype=np.uint32))
    for s in range(3):
        sim.tick(tick)
        chk.step(tick)
        assert_track_equal(sim, chk, f"step {s} after the enable")
        assert_state_equal(sim, chk, f"step {s} after the enable")
    assert_not_vacuous(chk)
    sim.track(2)                                  # again, with another channel count: ids and channels start over
    chk.reset(2)
    assert sim.track_channels == 2
    assert np.array_equal(sim.particle_ids(), np.arange(n, dtype=np.uint32))
    assert not bits(sim.attribute(0)).any() and not bits(sim.attribute(1)).any()
    sim.set_attribute(1, np.arange(n, dtype=np.float32))
    chk.attr[1] = np.arange(n, dtype=np.float32)
    for s in range(2):
        sim.tick(tick)
        chk.step(tick)
    assert_track_equal(sim, chk, "after the second enable")
    assert_not_vacuous(chk)
    sim.untrack()
    assert sim.track_channels == -1
    sim.tick(tick)
    chk.step(tick)
    assert_state_equal(sim, chk, "after untrack")
    for call in (sim.particle_ids, lambda: sim.attribute(0), sim.download_particles_by_id, sim.particle_ids_device_ptr):
        with pytest.raises(fs.FluidSimError):
            call()
    sim.close(); chk.close()


def test_upload_particles_keeps_ids_and_channels(fs):
    n = 17 ** 3
    sim, chk, tick = make_pair(fs, 17, channels=1)
    v = np.arange(n, dtype=np.float32)
    sim.set_attribute(0, v)
    chk.attr[0] = v
    for _ in range(2):
        sim.tick(tick)
        chk.step(tick)
    ids = sim.particle_ids()
    p = sim.download_particles()
    p["velocity"] += np.random.default_rng(5).uniform(-1.0, 1.0, size=p["velocity"].shape).astype(np.float32)
    sim.upload_particles(p)
    chk.set_particles(p)
    assert np.array_equal(sim.particle_ids(), ids)
    assert np.array_equal(sim.attribute(0), ids.astype(np.float32))
    for s in range(2):
        sim.tick(tick)
        chk.step(tick)
        assert_track_equal(sim, chk, f"step {s} after the upload")
        assert_state_equal(sim, chk, f"step {s} after the upload")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


def test_timed_steps_run_ahead(fs):
    n = 17 ** 3
    sim, chk, tick = make_pair(fs, 17, channels=2)
    v = np.arange(n, dtype=np.float32)
    sim.set_attribute(1, v)
    chk.attr[1] = v
    sim.timed_steps(tick, 12)
    for _ in range(12):
        chk.step(tick)
    assert_track_equal(sim, chk, "12 timed steps")
    assert_state_equal(sim, chk, "12 timed steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


def test_profiled_steps_carry_too(fs):
    sim, chk, tick = make_pair(fs, 17, channels=1)
    sim.set_attribute(0, special_bits(17 ** 3, 99, POOL_TWELVE))
    chk.attr[0] = special_bits(17 ** 3, 99, POOL_TWELVE)
    sim.profile(True)
    for _ in range(3):
        sim.tick(tick)
        chk.step(tick)
    ms, steps = sim.profile_read()
    assert steps == 3
    assert_track_equal(sim, chk, "profiled steps")
    assert_state_equal(sim, chk, "profiled steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


def test_download_by_id(fs):
    n = 17 ** 3
    sim, chk, tick = make_pair(fs, 17)
    for _ in range(3):
        sim.tick(tick)
        chk.step(tick)
    assert_not_vacuous(chk)
    ids, rec = sim.particle_ids(), sim.download_particles()
    by_id = sim.download_particles_by_id()
    assert by_id[ids].tobytes() == rec.tobytes()
    # one id out of range: that record is skipped and its entry of dst keeps the caller's bytes
    k = 1234
    slot = int(np.nonzero(ids == k)[0][0])
    bad = ids.copy()
    bad[slot] = n + 7
    sim.set_particle_ids(bad)
    assert np.array_equal(sim.particle_ids(), bad)
    dst = np.frombuffer(bytes([0xA5]) * (n * 48), dtype=fs.PARTICLE3_DTYPE).copy()
    lib = fs.load_library()
    assert lib.fs3_download_particles_by_id(sim._h, dst.ctypes.data_as(C.c_void_p), n) == fs._abi.FS_OK
    assert dst[k].tobytes() == bytes([0xA5]) * 48
    keep = np.arange(n) != k
    assert dst[keep].tobytes() == by_id[keep].tobytes()
    # a shorter dst: only ids below its length land, nothing past it is written; a longer one: the tail stays
    m = 100
    dst = np.frombuffer(bytes([0xA5]) * ((m + 1) * 48), dtype=fs.PARTICLE3_DTYPE).copy()
    assert lib.fs3_download_particles_by_id(sim._h, dst.ctypes.data_as(C.c_void_p), m) == fs._abi.FS_OK
    assert dst[:m].tobytes() == by_id[:m].tobytes() and dst[m].tobytes() == bytes([0xA5]) * 48
    dst = np.frombuffer(bytes([0xA5]) * ((n + 9) * 48), dtype=fs.PARTICLE3_DTYPE).copy()
    assert lib.fs3_download_particles_by_id(sim._h, dst.ctypes.data_as(C.c_void_p), n + 9) == fs._abi.FS_OK
    assert dst[n + 7].tobytes() == rec[slot].tobytes() and dst[n + 8].tobytes() == bytes([0xA5]) * 48
    sim.close(); chk.close()


def test_one_tolerance_step_moves_the_ids_the_same_way(fs):
    """The keys come from the uploaded positions and velocities alone and stay bit-exact in FS_MATH_TOLERANCE."""
    sim, chk, tick = make_pair(fs, 17, channels=2, mode=fs.FS_MATH_TOLERANCE)
    v = special_bits(17 ** 3, 99, POOL_TWELVE)
    sim.set_attribute(0, v)
    chk.attr[0] = v
    sim.tick(tick)
    chk.step(tick)
    assert np.array_equal(sim.download_particles()["grid"], chk.particles_view()["grid"]), "cell keys differ"
    assert_track_equal(sim, chk, "tolerance")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


def test_errors(fs):
    n = 16 ** 3
    sim, chk, tick = make_pair(fs, 16, track=False)
    lib = fs.load_library()
    inv, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    h = sim._h
    assert lib.fs3_track_enable(h, 5) == inv and sim.track_channels == -1
    assert lib.fs3_track_enable(h, -1) == inv and sim.track_channels == -1
    buf = np.zeros(12 * (n + 1), dtype=np.uint32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    assert lib.fs3_track_download_ids(h, ptr, n) == inv
    assert lib.fs3_track_upload_ids(h, ptr, n) == inv
    sim.track(2)
    assert lib.fs3_track_download_ids(h, ptr, n) == ok
    for bad_n in (n - 1, n + 1, 0):
        assert lib.fs3_track_download_ids(h, ptr, bad_n) == inv
        assert lib.fs3_track_upload_ids(h, ptr, bad_n) == inv
        assert lib.fs3_track_download_attr(h, 0, ptr, bad_n) == inv
        assert lib.fs3_track_upload_attr(h, 0, ptr, bad_n) == inv
    for bad_c in (2, 3, 4, -1):
        assert lib.fs3_track_download_attr(h, bad_c, ptr, n) == inv
        assert lib.fs3_track_upload_attr(h, bad_c, ptr, n) == inv
        assert lib.fs3_track_attr_device(h, bad_c, C.byref(out)) == inv
    assert lib.fs3_track_download_ids(h, None, n) == inv
    assert lib.fs3_track_upload_ids(h, None, n) == inv
    assert lib.fs3_track_download_attr(h, 0, None, n) == inv
    assert lib.fs3_track_upload_attr(h, 0, None, n) == inv
    assert lib.fs3_track_ids_device(h, None) == inv
    assert lib.fs3_track_attr_device(h, 0, None) == inv
    assert lib.fs3_download_particles_by_id(h, None, n) == inv
    assert lib.fs3_download_particles_by_id(h, None, 0) == ok
    assert lib.fs3_track_ids_device(h, C.byref(out)) == ok and out.value
    assert sim.particle_ids_device_ptr() == out.value
    assert sim.attribute_device_ptr(1) - sim.attribute_device_ptr(0) == 4 * n
    sim.tick(tick)                                # the failed calls left the handle usable
    chk.reset(2)
    chk.step(tick)
    assert_track_equal(sim, chk, "after the refused calls")
    sim.close(); chk.close()

"""GPU tests of the opt-in particle tracking: k_track_carry's ids and channels against the CPU checker
(tests/track_ref.py: the unchanged oracle stepped pass by pass, plus the permutation its sort applies), bit for bit; and the
particle records against the oracle in the same runs — tracking changes no bit of the state.

Scene unless said otherwise: dam_break_2d(N) with velocities drawn uniformly from [-3, 3] uploaded to both sides.  Every test
asserts on the CHECKER's ids that more than half of the slots changed occupant, so none can pass on an identity permutation."""
import ctypes as C

import numpy as np
import pytest

from tests.bitcmp import POOL_TWELVE, assert_records_equal, assert_track_equal, bits, special_bits

pytestmark = pytest.mark.gpu


def assert_state_equal(sim, chk, ctx):
    assert_records_equal(sim.download_particles(), chk.particles_view(), ctx)
    assert np.array_equal(sim.download_start_indices(), chk.start_indices_view()), f"{ctx}: start_indices"


def assert_not_vacuous(chk):
    assert (chk.ids != np.arange(chk.n)).mean() > 0.5, "the checker's permutation is (nearly) the identity: the test shows nothing"


def make_pair(fs, n, seed=7, quirks=True, sort_mode=None, channels=0, track=True, **kw):
    from tests.track_ref import TrackChecker, jitter_velocities
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=quirks,
                             sort_mode=fs.FS_SORT_BITONIC if sort_mode is None else sort_mode,
                             track=channels if track else None, **kw)
    chk = TrackChecker(st, off, ref_quirks=quirks, channels=channels)
    p = jitter_velocities(chk.particles(), seed)
    chk.set_particles(p)
    sim.upload_particles(p)
    return sim, chk, tick


# ---- 1. ids bit-exact against the checker, every step; the state stays the oracle's ------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("n,counting", [(4096, False), (5000, False), (100_000, False), (5000, True), (100_000, True)])
def test_ids_follow_the_sort_bit_exact(fs, n, counting, quirks):
    sim, chk, tick = make_pair(fs, n, quirks=quirks, sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC)
    assert sim.track_channels == 0
    assert np.array_equal(sim.particle_ids(), np.arange(n, dtype=np.uint32))
    for s in range(8):
        sim.tick(tick)
        chk.step(tick, stable_sort=counting)
        assert_track_equal(sim, chk, f"n={n} counting={counting} quirks={quirks} step {s}")
        assert_state_equal(sim, chk, f"n={n} counting={counting} quirks={quirks} step {s}")
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(n, dtype=np.uint32))
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 2. channels ride along ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_channels_ride_along(fs, counting):
    n = 100_000
    sim, chk, tick = make_pair(fs, n, channels=4, sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC)
    x0 = np.ascontiguousarray(chk.particles()["position"][:, 0])
    vals = [np.arange(n, dtype=np.float32), x0, special_bits(n, 99, POOL_TWELVE)]
    for c, v in enumerate(vals):
        sim.set_attribute(c, v)
        chk.attr[c] = v
        assert np.array_equal(bits(sim.attribute(c)), bits(v)), f"channel {c}: upload / download is not a bit copy"
    assert not bits(sim.attribute(3)).any()                       # +0.0f from the enable
    for s in range(8):
        sim.tick(tick)
        chk.step(tick, stable_sort=counting)
    assert_track_equal(sim, chk, "C=4 after 8 steps")
    ids = sim.particle_ids()
    assert np.array_equal(sim.attribute(0), ids.astype(np.float32))      # exact below 2^24
    assert np.array_equal(bits(sim.attribute(1)), bits(x0[ids]))
    assert np.array_equal(bits(sim.attribute(2)), bits(vals[2][ids]))
    assert not bits(sim.attribute(3)).any()
    assert_state_equal(sim, chk, "C=4 after 8 steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


@pytest.mark.parametrize("channels", [1, 0])
def test_fewer_channels_ride_along(fs, channels):
    n = 100_000
    sim, chk, tick = make_pair(fs, n, channels=channels)
    if channels:
        v = special_bits(n, 99, POOL_TWELVE)
        sim.set_attribute(0, v)
        chk.attr[0] = v
    for s in range(8):
        sim.tick(tick)
        chk.step(tick)
    assert_track_equal(sim, chk, f"C={channels} after 8 steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 3. every instantiation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])
def test_every_channel_count_one_step(fs, channels, counting):
    n = 5000
    sim, chk, tick = make_pair(fs, n, seed=20 + channels, channels=channels,
                               sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC)
    rng = np.random.default_rng(channels)
    for c in range(channels):
        v = rng.standard_normal(n).astype(np.float32) if c else np.arange(n, dtype=np.float32)
        sim.set_attribute(c, v)
        chk.attr[c] = v
    sim.tick(tick)
    chk.step(tick, stable_sort=counting)
    assert_track_equal(sim, chk, f"C={channels} one step")
    assert_state_equal(sim, chk, f"C={channels} one step")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 4. by-id download -------------------------------------------------------------------------------------------------
def test_download_by_id(fs):
    n = 5000
    sim, chk, tick = make_pair(fs, n)
    for _ in range(4):
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
    dst = np.frombuffer(bytes([0xA5]) * (n * 32), dtype=fs.PARTICLE_DTYPE).copy()
    lib = fs.load_library()
    assert lib.fs_download_particles_by_id(sim._h, dst.ctypes.data_as(C.c_void_p), n) == fs._abi.FS_OK
    assert dst[k].tobytes() == bytes([0xA5]) * 32
    keep = np.arange(n) != k
    assert dst[keep].tobytes() == by_id[keep].tobytes()
    # a shorter dst: only ids below its length land, nothing past it is written
    m = 100
    dst = np.frombuffer(bytes([0xA5]) * ((m + 1) * 32), dtype=fs.PARTICLE_DTYPE).copy()
    assert lib.fs_download_particles_by_id(sim._h, dst.ctypes.data_as(C.c_void_p), m) == fs._abi.FS_OK
    assert dst[:m].tobytes() == by_id[:m].tobytes() and dst[m].tobytes() == bytes([0xA5]) * 32
    sim.close(); chk.close()


# ---- 5. upload keeps identity ------------------------------------------------------------------------------------------
def test_upload_particles_keeps_ids_and_channels(fs):
    n = 5000
    sim, chk, tick = make_pair(fs, n, channels=1)
    v = np.arange(n, dtype=np.float32)
    sim.set_attribute(0, v)
    chk.attr[0] = v
    for _ in range(3):
        sim.tick(tick)
        chk.step(tick)
    ids = sim.particle_ids()
    p = sim.download_particles()
    p["velocity"] += np.random.default_rng(5).uniform(-1.0, 1.0, size=p["velocity"].shape).astype(np.float32)
    sim.upload_particles(p)
    chk.set_particles(p)
    assert np.array_equal(sim.particle_ids(), ids)
    assert np.array_equal(sim.attribute(0), ids.astype(np.float32))
    for s in range(3):
        sim.tick(tick)
        chk.step(tick)
        assert_track_equal(sim, chk, f"step {s} after the upload")
        assert_state_equal(sim, chk, f"step {s} after the upload")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 6. enable mid-run, re-enable, disable -----------------------------------------------------------------------------
def test_enable_mid_run_reset_and_disable(fs):
    n = 5000
    sim, chk, tick = make_pair(fs, n, track=False)
    assert sim.track_channels == -1
    for _ in range(5):
        sim.tick(tick)
        chk.step(tick)
    sim.track()                                   # enqueued behind the five steps, no sync in between
    chk.reset(0)
    assert sim.track_channels == 0
    assert np.array_equal(sim.particle_ids(), np.arange(n, dtype=np.uint32))
    for s in range(5):
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
    for s in range(3):
        sim.tick(tick)
        chk.step(tick)
    assert_track_equal(sim, chk, "after the second enable")
    assert_not_vacuous(chk)
    sim.untrack()
    assert sim.track_channels == -1
    for s in range(3):
        sim.tick(tick)
        chk.step(tick)
    assert_state_equal(sim, chk, "after untrack")
    with pytest.raises(fs.FluidSimError):
        sim.particle_ids()
    with pytest.raises(fs.FluidSimError):
        sim.attribute(0)
    with pytest.raises(fs.FluidSimError):
        sim.download_particles_by_id()
    sim.close(); chk.close()


# ---- 7. in-flight ordering ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_timed_steps_run_ahead(fs, counting):
    n = 100_000
    sim, chk, tick = make_pair(fs, n, channels=2, sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC)
    v = np.arange(n, dtype=np.float32)
    sim.set_attribute(1, v)
    chk.attr[1] = v
    sim.timed_steps(tick, 20)
    for _ in range(20):
        chk.step(tick, stable_sort=counting)
    assert_track_equal(sim, chk, "20 timed steps")
    assert_state_equal(sim, chk, "20 timed steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


def test_profiled_steps_carry_too(fs):
    n = 5000
    sim, chk, tick = make_pair(fs, n, channels=1)
    sim.profile(True)
    for _ in range(4):
        sim.tick(tick)
        chk.step(tick)
    ms, steps = sim.profile_read()
    assert steps == 4
    assert_track_equal(sim, chk, "profiled steps")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 8. other step variants, one step each from an uploaded jittered state ---------------------------------------------
@pytest.mark.parametrize("variant", ["surface_tension", "tolerance", "wgsl_ulp"])
def test_one_step_of_the_other_step_variants(fs, variant):
    """The first step's keys come from the uploaded positions and velocities alone, so the plain checker's permutation applies."""
    n = 16384
    kw = {"surface_tension": dict(surface_tension=True), "tolerance": dict(math_mode=fs.FS_MATH_TOLERANCE),
          "wgsl_ulp": dict(math_mode=fs.FS_MATH_WGSL_ULP)}[variant]
    sim, chk, tick = make_pair(fs, n, channels=2, **kw)
    if variant == "surface_tension":
        tick.surface_tension_coefficient = 35.0
    v = special_bits(n, 99, POOL_TWELVE)
    sim.set_attribute(0, v)
    chk.attr[0] = v
    sim.tick(tick)
    chk.step(tick)
    assert np.array_equal(sim.download_particles()["grid"], chk.particles_view()["grid"]), f"{variant}: cell keys differ"
    assert_track_equal(sim, chk, variant)
    assert (chk.ids != np.arange(n)).mean() > 0.8
    sim.close(); chk.close()


# ---- 9. off is off -----------------------------------------------------------------------------------------------------
def test_off_is_off(fs, orc):
    n = 5000
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    ref = orc.OracleSim(st, off)
    assert getattr(sim, "track_channels", -1) == -1
    for name in ("particle_ids", "download_particles_by_id"):
        if hasattr(sim, name):
            with pytest.raises(fs.FluidSimError):
                getattr(sim, name)()
    for s in range(8):
        sim.tick(tick)
        ref.step(tick)
    assert_state_equal(sim, ref, "tracking never enabled")
    assert getattr(sim, "track_channels", -1) == -1
    sim.close(); ref.close()


# ---- 10. large ---------------------------------------------------------------------------------------------------------
def test_16m_ids_and_a_channel(fs, orc):
    import bench
    n = 1 << 24
    orc.set_threads(min(bench.usable_cores(), orc.max_threads()))
    try:
        sim, chk, tick = make_pair(fs, n, channels=1)
        v = np.arange(n, dtype=np.float32)       # exact: every id is below 2^24
        sim.set_attribute(0, v)
        chk.attr[0] = v
        for step in (1, 2):
            sim.tick(tick)
            chk.step(tick)
            assert_track_equal(sim, chk, f"16M step {step}")
            assert_state_equal(sim, chk, f"16M step {step}")
        assert_not_vacuous(chk)
        sim.close(); chk.close()
    finally:
        orc.set_threads(1)


def test_4m_shuffled_upload_takes_the_wide_tile_path(fs, orc):
    """After an upload of a permuted state every tile of the first sort kernel goes through the 64-bit wide-key kernel, whose
    pairs the carry pass must read just the same."""
    import bench
    from tests.track_ref import TrackChecker
    n = 1 << 22
    st, off, tick = fs.dam_break_2d(n)
    orc.set_threads(min(bench.usable_cores(), orc.max_threads()))
    try:
        sim = fs.FluidSimulation(st, device=0, initial_offset=off, track=1)
        chk = TrackChecker(st, off, channels=1)
        p = chk.particles()[np.random.default_rng(5).permutation(n)]
        sim.upload_particles(p)
        chk.set_particles(p)
        v = np.arange(n, dtype=np.float32)
        sim.set_attribute(0, v)
        chk.attr[0] = v
        sim.tick(tick)
        chk.step(tick)
        assert sim.sort_plan()["wide_tiles"] >= n // 4096 // 2, sim.sort_plan()
        assert_track_equal(sim, chk, "4M shuffled upload")
        assert_state_equal(sim, chk, "4M shuffled upload")
        assert_not_vacuous(chk)
        sim.close(); chk.close()
    finally:
        orc.set_threads(1)


# ---- 11. errors --------------------------------------------------------------------------------------------------------
def test_errors(fs):
    n = 4096
    st, off, tick = fs.dam_break_2d(n)
    lib = fs.load_library()
    inv, unsup, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_ERR_UNSUPPORTED, fs._abi.FS_OK
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    assert lib.fs_track_enable(sim._h, 5) == inv and sim.track_channels == -1
    assert lib.fs_track_enable(sim._h, -1) == inv and sim.track_channels == -1
    with pytest.raises(fs.FluidSimError):
        fs.FluidSimulation(st, device=0, initial_offset=off, track=5)
    buf = np.zeros(n + 1, dtype=np.uint32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    # off: every read call is invalid
    assert lib.fs_track_download_ids(sim._h, ptr, n) == inv
    assert lib.fs_track_ids_device(sim._h, C.byref(out)) == inv
    assert lib.fs_track_attr_device(sim._h, 0, C.byref(out)) == inv
    assert lib.fs_download_particles_by_id(sim._h, ptr, 0) == inv
    sim.track(2)
    assert lib.fs_track_download_ids(sim._h, ptr, n) == ok
    for bad_n in (n - 1, n + 1, 0):
        assert lib.fs_track_download_ids(sim._h, ptr, bad_n) == inv
        assert lib.fs_track_upload_ids(sim._h, ptr, bad_n) == inv
        assert lib.fs_track_download_attr(sim._h, 0, ptr, bad_n) == inv
        assert lib.fs_track_upload_attr(sim._h, 0, ptr, bad_n) == inv
    for bad_c in (2, 3, 4, -1):
        assert lib.fs_track_download_attr(sim._h, bad_c, ptr, n) == inv
        assert lib.fs_track_upload_attr(sim._h, bad_c, ptr, n) == inv
        assert lib.fs_track_attr_device(sim._h, bad_c, C.byref(out)) == inv
    assert lib.fs_track_download_ids(sim._h, None, n) == inv
    assert lib.fs_track_upload_ids(sim._h, None, n) == inv
    assert lib.fs_track_download_attr(sim._h, 0, None, n) == inv
    assert lib.fs_track_upload_attr(sim._h, 0, None, n) == inv
    assert lib.fs_track_ids_device(sim._h, None) == inv
    assert lib.fs_track_attr_device(sim._h, 0, None) == inv
    assert lib.fs_download_particles_by_id(sim._h, None, n) == inv
    assert lib.fs_track_ids_device(sim._h, C.byref(out)) == ok and out.value
    assert sim.particle_ids_device_ptr() == out.value
    assert sim.attribute_device_ptr(1) - sim.attribute_device_ptr(0) >= 4 * n
    sim.tick(tick)                                # the failed calls left the handle usable
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(n, dtype=np.uint32))
    sim.close()
    st2, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st2, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    assert lib.fs_track_enable(slab._h, 0) == unsup
    assert lib.fs_track_channels(slab._h) == -1
    assert lib.fs_track_download_ids(slab._h, ptr, n) == inv
    slab.close()

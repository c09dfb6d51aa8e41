"""CPU-side checks of the opt-in 3D particle tracking and of the channels in the 3D sampler: the checker of
tests/track3d_ref.py is sound (the permutation it derives is the one the 3D oracle's sort applies), the numpy restatement of
tests/sample_attr3d_ref.py is tied to the pinned 3D sampler by the two identities of the header, every host binding names every
new call, and the calls refuse a NULL handle without touching a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

TRACK3_CALLS = ("fs3_track_enable", "fs3_track_disable", "fs3_track_channels", "fs3_track_download_ids", "fs3_track_upload_ids",
                "fs3_track_download_attr", "fs3_track_upload_attr", "fs3_track_ids_device", "fs3_track_attr_device",
                "fs3_download_particles_by_id", "fs3_sample_attr_points", "fs3_sample_attr_points_device", "fs3_sample_attr_grid")


# side -> the least fraction of slots that must change occupant in every step (the scenes of tests/track3d_ref.py); the two
# tiny lattices span a few cells only, so all that is asked of them is that no step's permutation is the identity
@pytest.mark.parametrize("side,moved_min", [(2, 0.0), (3, 0.0), (16, 0.5), (17, 0.5)])
def test_checker_permutation_reproduces_the_oracles_sort(fs, orc, side, moved_min):
    """verify=True asserts inside step() that the oracle's sorted keys and predicted positions are the derived ones under the
    derived permutation, and that the predicted positions are distinct; the checker's state stays the plain oracle's; and no
    step's permutation is the identity."""
    from tests.track3d_ref import SCENES, jitter_velocities3, make_checker3, scene3
    chk, tick = make_checker3(fs, side, seed=side, verify=True)
    box, spacing, vmax = SCENES[side]
    st, off, _ = scene3(fs, side, box, spacing)
    ref = orc.OracleSim3D(st, off)
    ref.set_particles(jitter_velocities3(ref.particles(), side, vmax))
    n = side ** 3
    composed = np.arange(n, dtype=np.uint32)
    for _ in range(3):
        perm = chk.step(tick)
        ref.step(tick)
        assert chk.particles_view().tobytes() == ref.particles_view().tobytes()
        assert not np.array_equal(perm, np.arange(n)), "identity permutation: the scene shows nothing"
        assert (perm != np.arange(n)).mean() >= moved_min
        composed = composed[perm]
        assert np.array_equal(chk.ids, composed)
        assert np.array_equal(np.sort(chk.ids), np.arange(n, dtype=np.uint32))
    chk.close(); ref.close()


def test_reset_restarts_the_ids_and_channels_follow(fs, orc):
    from tests.track3d_ref import make_checker3
    chk, tick = make_checker3(fs, 16, seed=3, channels=2)
    chk.attr[1] = np.arange(4096, dtype=np.float32)
    for _ in range(2):
        chk.step(tick)
    assert np.array_equal(chk.attr[1], chk.ids.astype(np.float32)) and not chk.attr[0].any()
    chk.reset(channels=3)
    assert np.array_equal(chk.ids, np.arange(4096, dtype=np.uint32)) and chk.attr.shape == (3, 4096)
    perm = chk.step(tick)
    assert np.array_equal(chk.ids, perm)
    chk.close()


def test_shuffled_wide_grid_scene_spans_more_than_2_pow_20_keys_per_tile(fs, orc):
    """The scene of the GPU test of the sort's wide-key hand-over: 17^3 particles at spacing 1.35 in a 24^3 box give
    1 815 848 cells, and after a random permutation of the records every 4096-slot tile spans more than 2^20 - 1 keys."""
    from tests.track3d_ref import predict_keys, wide_grid_scene
    st, off, tick, p = wide_grid_scene(fs, orc)
    ref = orc.OracleSim3D(st, off)
    assert ref.grid_dims == (122, 122, 122)
    _, keys = predict_keys(st, ref.grid_dims, p, tick.delta)
    spans = [int(keys[a:a + 4096].max()) - int(keys[a:a + 4096].min()) for a in range(0, keys.shape[0], 4096)]
    assert len(spans) == 2 and min(spans) > (1 << 20) - 1, spans
    ref.close()


# ---- the numpy restatement of the channel sampler -------------------------------------------------------------------------
def sampler_state(fs, orc, side=17, steps=3, seed=7):
    """(settings, offset, tick, records after `steps` oracle steps of the tracking scene)."""
    from tests.track3d_ref import SCENES, jitter_velocities3, scene3
    box, spacing, vmax = SCENES[side]
    st, off, tick = scene3(fs, side, box, spacing)
    ref = orc.OracleSim3D(st, off)
    ref.set_particles(jitter_velocities3(ref.particles(), seed, vmax))
    for _ in range(steps):
        ref.step(tick)
    p, dims = ref.particles(), ref.grid_dims
    from tests.sample_attr3d_ref import poly6
    assert np.float32(ref.constants()[0]).tobytes() == poly6(st.smoothing_radius).tobytes()      # the oracle's poly6: host libm
    ref.close()
    return st, off, tick, p, dims


def query_sets(st, p):
    from tests.sample3d_ref import boundary_points, uniform_points
    return {"own": p["predicted_position"].copy(), "uniform": uniform_points(st, 2000, seed=2),
            "boundary": boundary_points(st, p, 100, seed=3)}


def test_restatement_meets_the_pinned_sampler_in_both_identities(fs, orc):
    """Channel 0 = 1.0f and channels 1-3 = the stored velocity components: weight == a_0 == fs3_sample.weight and
    a_1..a_3 == fs3_sample.velocity, bit for bit, against the checker the existing 3D sampler is pinned to."""
    from tests.sample3d_ref import Sample3Checker
    from tests.sample_attr3d_ref import sample_attr
    st, off, tick, p, dims = sampler_state(fs, orc)
    chk = Sample3Checker(st, off).load(p, tick.mass)
    attr = np.stack([np.ones(p.shape[0], dtype=np.float32)] + [np.ascontiguousarray(p["velocity"][:, a]) for a in range(3)])
    for name, pts in query_sets(st, p).items():
        want = chk.sample(pts)
        w, a = sample_attr(st, dims, tick.mass, p, attr, pts)
        assert w.dtype == np.float32 and a.dtype == np.float32
        assert w.tobytes() == want["weight"].tobytes(), name
        assert a[0].tobytes() == want["weight"].tobytes(), name
        assert np.ascontiguousarray(a[1:].T).tobytes() == want["velocity"].tobytes(), name
        if name == "uniform":
            assert (want["neighbours"] > 0).sum() > 50 and (want["neighbours"] == 0).sum() > 50
    chk.close()


def test_restatement_against_a_float64_sum(fs, orc):
    """Random channel values against the same sums in double, at the project's per-step contract of rtol 1e-5 (the sums are
    of a few dozen terms; weights are non-negative, channel sums are compared on the scale of their absolute sum)."""
    from tests.sample_attr3d_ref import sample_attr
    st, off, tick, p, dims = sampler_state(fs, orc)
    attr = np.random.default_rng(4).uniform(-2.0, 2.0, size=(4, p.shape[0])).astype(np.float32)
    for name, pts in query_sets(st, p).items():
        w32, a32 = sample_attr(st, dims, tick.mass, p, attr, pts)
        w64, a64 = sample_attr(st, dims, tick.mass, p, attr, pts, dtype=np.float64)
        _, scale = sample_attr(st, dims, tick.mass, p, np.abs(attr), pts, dtype=np.float64)
        assert np.allclose(w32, w64, rtol=1e-5, atol=0.0), name
        assert (np.abs(a32 - a64) <= 1e-5 * scale).all(), name


# ---- layers and NULL handles ----------------------------------------------------------------------------------------------
def test_every_layer_names_every_3d_tracking_call(fs):
    from tests.layers import assert_every_layer_names
    assert_every_layer_names(fs, TRACK3_CALLS, fs.FluidSimulation3D, (
        "track", "untrack", "track_channels", "particle_ids", "set_particle_ids", "attribute", "set_attribute",
        "download_particles_by_id", "particle_ids_device_ptr", "attribute_device_ptr", "sample_attr_device"))


def test_null_handle_is_invalid_without_a_device(fs):
    lib = fs.load_library()
    inv = fs._abi.FS_ERR_INVALID
    buf = (C.c_uint32 * 48)()
    out = C.c_void_p()
    view = fs._abi.View3(fs.Vec3(0, 0, 0), fs.Vec3(1, 1, 1), 2, 2, 2)
    assert lib.fs3_track_enable(None, 0) == inv
    assert lib.fs3_track_disable(None) == inv
    assert lib.fs3_track_channels(None) == -1
    assert lib.fs3_track_download_ids(None, buf, 4) == inv
    assert lib.fs3_track_upload_ids(None, buf, 4) == inv
    assert lib.fs3_track_download_attr(None, 0, buf, 4) == inv
    assert lib.fs3_track_upload_attr(None, 0, buf, 4) == inv
    assert lib.fs3_track_ids_device(None, C.byref(out)) == inv
    assert lib.fs3_track_attr_device(None, 0, C.byref(out)) == inv
    assert lib.fs3_download_particles_by_id(None, buf, 1) == inv
    assert lib.fs3_sample_attr_points(None, buf, 4, buf, buf) == inv
    assert lib.fs3_sample_attr_points_device(None, buf, 4, buf, buf) == inv
    assert lib.fs3_sample_attr_grid(None, C.byref(view), buf, buf) == inv
    assert b"null" in lib.fs_last_error()

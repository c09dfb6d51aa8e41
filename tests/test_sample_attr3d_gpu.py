"""The tracking channels in the 3D sampler on the GPU: fs3_sample_attr_points / _points_device / _grid against
the numpy restatement of tests/sample_attr3d_ref.py fed the state downloaded from the SAME handle, byte for byte, and against the
device's own fs3_sample_points through the two identities of the header.  No tolerance anywhere.

State: the 17^3 = 4913 tracking scene (two sort tiles, ragged against workgroup and wave) after three steps; the reference sums
are computed once for four channels of random values and shared: channel sums do not depend on the other channels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SIDE, N = 17, 17 ** 3
f = np.float32


def make_sim(fs, mode=None, steps=3, track=None):
    from tests.track3d_ref import SCENES, jitter_velocities3, scene3
    box, spacing, vmax = SCENES[SIDE]
    st, off, tick = scene3(fs, SIDE, box, spacing)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_IEEE if mode is None else mode, track=track)
    sim.upload_particles(jitter_velocities3(sim.download_particles(), 7, vmax))
    for _ in range(steps):
        sim.tick(tick)
    return sim, st, tick


def downloaded(sim):
    p = sim.download_particles()
    for fld in ("position", "predicted_position", "velocity", "density"):
        assert np.isfinite(p[fld]).all(), f"non-finite {fld}"
    return p


def query_sets(st, p):
    from tests.sample3d_ref import boundary_points, uniform_points
    return {"own": p["predicted_position"].copy(),                 # the particles' own predicted positions, slot order
            "uniform": uniform_points(st, 2000, seed=2),           # over 1.2 x the box: some outside, some wrapped cell columns
            "boundary": boundary_points(st, p, 100, seed=3)}


def raw_points(fs, sim, pts, channels, weights=True):
    """fs3_sample_attr_points itself: (weight or None, sums), outputs pre-filled with a pattern."""
    n = pts.shape[0]
    w = np.full(n, 7.5, dtype=np.float32)
    a = np.full((channels, n), 7.5, dtype=np.float32)
    st = fs.load_library().fs3_sample_attr_points(sim._h, pts.ctypes.data_as(C.c_void_p), n,
                                                  w.ctypes.data_as(C.c_void_p) if weights else None, a.ctypes.data_as(C.c_void_p))
    assert st == fs._abi.FS_OK, fs.load_library().fs_last_error()
    return (w if weights else None), a


@pytest.fixture(scope="module")
def state(fs):
    """One handle after three steps, its records, the query sets, four channels of random values and the reference sums."""
    from tests.sample_attr3d_ref import sample_attr
    sim, st, tick = make_sim(fs)
    p = downloaded(sim)
    attr = np.random.default_rng(4).uniform(-2.0, 2.0, size=(4, N)).astype(np.float32)
    sets = query_sets(st, p)
    want = {name: sample_attr(st, sim.grid_dims, tick.mass, p, attr, pts) for name, pts in sets.items()}
    yield {"sim": sim, "st": st, "tick": tick, "p": p, "attr": attr, "sets": sets, "want": want}
    sim.close()


def track_and_upload(sim, attr):
    sim.track(attr.shape[0])
    for c in range(attr.shape[0]):
        sim.set_attribute(c, attr[c])


# ---- 1. every C against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_points_match_the_restatement(fs, state, channels):
    sim = state["sim"]
    track_and_upload(sim, state["attr"][:channels])
    for name, pts in state["sets"].items():
        want_w, want_a = state["want"][name]
        w, a = raw_points(fs, sim, pts, channels)
        assert w.tobytes() == want_w.tobytes(), f"C={channels} {name}: weights"
        assert a.tobytes() == np.ascontiguousarray(want_a[:channels]).tobytes(), f"C={channels} {name}: channel sums"
        _, a2 = raw_points(fs, sim, pts, channels, weights=False)      # weight_out == NULL
        assert a2.tobytes() == a.tobytes()
        if name == "uniform":
            assert (want_w != 0).sum() > 50 and (want_w == 0).sum() > 50
    # ragged query counts against the wave and the workgroup
    own = state["sets"]["own"]
    want_w, want_a = state["want"]["own"]
    for m in (1, 63, 65, 257):
        w, a = raw_points(fs, sim, np.ascontiguousarray(own[100:100 + m]), channels)
        assert w.tobytes() == want_w[100:100 + m].tobytes() and a.tobytes() == np.ascontiguousarray(want_a[:channels, 100:100 + m]).tobytes()


def test_the_two_identities_against_the_devices_own_sampler(fs, state):
    """Channel 0 = 1.0f, channels 1-3 = the stored velocity: weight_out == a_0 == fs3_sample.weight, a_1..a_3 == its velocity."""
    sim, p = state["sim"], state["p"]
    track_and_upload(sim, np.stack([np.ones(N, dtype=np.float32)] + [np.ascontiguousarray(p["velocity"][:, k]) for k in range(3)]))
    for name, pts in state["sets"].items():
        rec = sim.sample(pts)
        w, a = raw_points(fs, sim, pts, 4)
        assert w.tobytes() == rec["weight"].tobytes(), name
        assert a[0].tobytes() == rec["weight"].tobytes(), name
        assert np.ascontiguousarray(a[1:].T).tobytes() == rec["velocity"].tobytes(), name
        rec2, a2 = sim.sample(pts, attributes=True)
        assert rec2.tobytes() == rec.tobytes() and a2.tobytes() == a.tobytes(), name
    rec, an = sim.sample(state["sets"]["own"], attributes=True, normalise=True)
    assert (an[0] == f(1.0)).all()                     # the wrapper's Shepard division of two equal floats


# ---- 2. grid forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 4])
def test_grid_forms_match_the_point_form(fs, state, channels):
    from tests.sample3d_ref import grid_points
    sim, st = state["sim"], state["st"]
    track_and_upload(sim, state["attr"][:channels])
    sx = st.size.x
    views = [(9, 7, 5, (-sx / 2, -sx / 2, -sx / 2), (sx / 2, sx / 2, sx / 2)),       # ragged against the 8 x 8 x 4 workgroup tile
             (17, 13, 1, (-1.2, -1.2, 0.05), (1.2, 1.2, 0.05)),                       # a slice: world_min.z == world_max.z
             (70, 1, 1, (-1.5, 0.03, 0.05), (1.5, 0.03, 0.05))]                       # a line
    lib = fs.load_library()
    for w, h, d, wmin, wmax in views:
        pts = grid_points(w, h, d, wmin, wmax)
        want_w, want_a = raw_points(fs, sim, pts, channels)
        assert (want_w != 0).any(), (w, h, d)
        rec, a = sim.sample_grid(w, h, d, wmin, wmax, attributes=True)
        assert a.shape == (channels, d, h, w) and rec.shape == (d, h, w)
        assert a.tobytes() == want_a.tobytes(), f"grid {w}x{h}x{d} C={channels}: channel sums against the point form"
        assert rec.ravel().tobytes() == sim.sample(pts).tobytes()
        view = sim._view3(w, h, d, wmin, wmax)
        gw = np.full(w * h * d, 7.5, dtype=np.float32)
        ga = np.full((channels, w * h * d), 7.5, dtype=np.float32)
        assert lib.fs3_sample_attr_grid(sim._h, C.byref(view), gw.ctypes.data_as(C.c_void_p), ga.ctypes.data_as(C.c_void_p)) == fs._abi.FS_OK
        assert gw.tobytes() == want_w.tobytes() and ga.tobytes() == want_a.tobytes(), f"grid {w}x{h}x{d} C={channels}: with weights"


# ---- 3. device pointers, stream-ordered with steps behind the call ----------------------------------------------------
@pytest.mark.parametrize("channels", [2])
def test_device_form_with_more_steps_enqueued_behind_it(fs, channels):
    sim, st, tick = make_sim(fs, track=channels)
    attr = np.random.default_rng(8).uniform(-2.0, 2.0, size=(channels, N)).astype(np.float32)
    for c in range(channels):
        sim.set_attribute(c, attr[c])
    sim.tick(tick)                                  # the channels have moved at least once
    pts = query_sets(st, downloaded(sim))["uniform"]
    m = pts.shape[0]
    want_w, want_a = raw_points(fs, sim, pts, channels)
    d_pts = fs.ResizableBuffer("points", np.float32, 3 * m)
    d_w = fs.ResizableBuffer("weights", np.float32, m + 1)
    d_a = fs.ResizableBuffer("sums", np.float32, channels * m + 1)
    d_pts.write(0, pts.ravel())
    d_w.write(0, np.full(m + 1, 7.5, dtype=np.float32))            # blocking copies: the buffers are ready before the enqueue
    d_a.write(0, np.full(channels * m + 1, 7.5, dtype=np.float32))
    sim.sample_attr_device(d_pts.device_ptr, m, d_w.device_ptr, d_a.device_ptr)
    for _ in range(2):
        sim.tick(tick)                              # behind the query: they ping-pong the channel arrays it reads
    sim.sync()
    got_w, got_a = d_w.read(), d_a.read()
    assert got_w[:m].tobytes() == want_w.tobytes() and got_w[m] == f(7.5)
    assert got_a[:channels * m].tobytes() == want_a.tobytes() and got_a[channels * m] == f(7.5)
    w2, _ = raw_points(fs, sim, pts, channels)
    assert w2.tobytes() != want_w.tobytes(), "the two sampled states must differ"
    # weight_out_dev == NULL
    d_a.write(0, np.full(channels * m + 1, 7.5, dtype=np.float32))
    _, want_a2 = raw_points(fs, sim, pts, channels)
    sim.sample_attr_device(d_pts.device_ptr, m, None, d_a.device_ptr)
    sim.sync()
    assert d_a.read()[:channels * m].tobytes() == want_a2.tobytes()
    for b in (d_pts, d_w, d_a):
        b.close()
    sim.close()


# ---- 4. the other math mode -------------------------------------------------------------------------------------------
def test_tolerance_handle_is_a_pure_function_of_the_stored_state(fs):
    from tests.sample_attr3d_ref import sample_attr
    sim, st, tick = make_sim(fs, mode=fs.FS_MATH_TOLERANCE, track=2)
    attr = np.random.default_rng(9).uniform(-2.0, 2.0, size=(2, N)).astype(np.float32)
    for c in range(2):
        sim.set_attribute(c, attr[c])
    p = downloaded(sim)
    for name, pts in query_sets(st, p).items():
        want_w, want_a = sample_attr(st, sim.grid_dims, tick.mass, p, attr, pts)
        w, a = raw_points(fs, sim, pts, 2)
        assert w.tobytes() == want_w.tobytes() and a.tobytes() == want_a.tobytes(), name
    sim.close()


def test_channels_sampled_are_the_carried_ones(fs):
    """Channels uploaded BEFORE the steps: the sampler reads the arrays the carry left, i.e. attribute(c) of the handle."""
    from tests.sample_attr3d_ref import sample_attr
    sim, st, tick = make_sim(fs, steps=0, track=3)
    attr = np.random.default_rng(10).uniform(-2.0, 2.0, size=(3, N)).astype(np.float32)
    for c in range(3):
        sim.set_attribute(c, attr[c])
    for _ in range(3):
        sim.tick(tick)
    ids = sim.particle_ids()
    assert (ids != np.arange(N)).mean() > 0.5
    carried = np.stack([sim.attribute(c) for c in range(3)])
    assert carried.tobytes() == np.ascontiguousarray(attr[:, ids]).tobytes()
    p = downloaded(sim)
    pts = query_sets(st, p)["uniform"]
    want_w, want_a = sample_attr(st, sim.grid_dims, tick.mass, p, carried, pts)
    w, a = raw_points(fs, sim, pts, 3)
    assert w.tobytes() == want_w.tobytes() and a.tobytes() == want_a.tobytes()
    sim.close()


# ---- 5. error paths, in the order of the header -----------------------------------------------------------------------
def test_error_paths(fs):
    lib = fs.load_library()
    inv, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    sim, st, tick = make_sim(fs, steps=0)            # created and uploaded to: no step yet, tracking off
    h = sim._h
    pts = np.zeros((8, 3), dtype=np.float32)
    wbuf = np.full(8, 7.5, dtype=np.float32)
    abuf = np.full((4, 8), 7.5, dtype=np.float32)
    P, W, A = pts.ctypes.data_as(C.c_void_p), wbuf.ctypes.data_as(C.c_void_p), abuf.ctypes.data_as(C.c_void_p)
    view = lambda w, hh, d: fs._abi.View3(fs.Vec3(-1, -1, -1), fs.Vec3(1, 1, 1), w, hh, d)      # noqa: E731
    err = lambda: lib.fs_last_error().decode()                                                   # noqa: E731

    def refused(status, text):
        assert status == inv and text in err(), (status, err())

    def handle_and_view():
        # 1. NULL handle
        refused(lib.fs3_sample_attr_points(None, P, 8, W, A), "null")
        refused(lib.fs3_sample_attr_points_device(None, P, 8, W, A), "null")
        refused(lib.fs3_sample_attr_grid(None, C.byref(view(2, 2, 2)), W, A), "null")
        # 2. grid form: NULL view, a zero extent, more than 2^28 voxels — before tracking is looked at
        refused(lib.fs3_sample_attr_grid(h, None, W, A), "null")
        for w, hh, d in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (1 << 14, 1 << 14, 2), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
            refused(lib.fs3_sample_attr_grid(h, C.byref(view(w, hh, d)), None, None), "grid size")

    def no_channels():
        # 3. tracking off or C == 0 — before n == 0 is looked at
        refused(lib.fs3_sample_attr_points(h, P, 8, W, A), "tracking")
        refused(lib.fs3_sample_attr_points(h, None, 0, None, None), "tracking")
        refused(lib.fs3_sample_attr_points_device(h, P, 8, W, A), "tracking")
        refused(lib.fs3_sample_attr_points_device(h, None, 0, None, None), "tracking")
        refused(lib.fs3_sample_attr_grid(h, C.byref(view(2, 1, 1)), W, A), "tracking")

    def arguments():
        # 4. n == 0: FS_OK, nothing touched
        assert lib.fs3_sample_attr_points(h, None, 0, None, None) == ok
        assert lib.fs3_sample_attr_points_device(h, None, 0, None, None) == ok
        # 5. NULL points / attr_out (weight_out may be NULL)
        refused(lib.fs3_sample_attr_points(h, None, 8, W, A), "null")
        refused(lib.fs3_sample_attr_points(h, P, 8, W, None), "null")
        refused(lib.fs3_sample_attr_points_device(h, None, 8, W, A), "null")
        refused(lib.fs3_sample_attr_points_device(h, P, 8, W, None), "null")
        refused(lib.fs3_sample_attr_grid(h, C.byref(view(2, 2, 1)), W, None), "null")
        # 6. n > 2^28
        refused(lib.fs3_sample_attr_points(h, P, (1 << 28) + 1, W, A), "2^28")
        refused(lib.fs3_sample_attr_points_device(h, P, (1 << 28) + 1, W, A), "2^28")

    def stale():
        # 7. the stale-state rule of 3D sampling
        refused(lib.fs3_sample_attr_points(h, P, 8, W, A), "needs a step")
        refused(lib.fs3_sample_attr_points_device(h, P, 8, W, A), "needs a step")
        refused(lib.fs3_sample_attr_grid(h, C.byref(view(2, 2, 2)), W, A), "needs a step")

    def valid():
        assert lib.fs3_sample_attr_points(h, P, 8, W, A) == ok
        assert lib.fs3_sample_attr_points(h, P, 8, None, A) == ok
        assert lib.fs3_sample_attr_grid(h, C.byref(view(2, 2, 2)), W, A) == ok

    handle_and_view()
    no_channels()                                    # off
    sim.track(0)
    no_channels()                                    # on with C == 0
    with pytest.raises(fs.FluidSimError):
        sim.sample(pts, attributes=True)
    sim.track(4)
    handle_and_view()
    arguments()
    stale()                                          # before the first step
    assert wbuf.tobytes() == np.full(8, 7.5, dtype=np.float32).tobytes() and (abuf == f(7.5)).all(), "a refused call wrote"
    sim.tick(tick)
    valid()
    handle_and_view()
    arguments()
    sim.upload_particles(sim.download_particles()[:10])     # a partial upload counts
    stale()
    sim.tick(tick)
    valid()
    sim.untrack()
    no_channels()                                    # off again, with a valid state
    sim.close()

"""2D moving bodies on the GPU (include/fluidsim.h "2D moving bodies").  The checker is the unchanged 2D oracle
plus the numpy operators of tests/bodies2d_ref.py (new state = B_7(...B_0(step(state)))); where no oracle is involved, a handle
with bodies is compared with B of a handle without.  Byte equality everywhere: no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies2d_ref as B
from tests.handle_helpers import _add, _same, _size
from tests.track_ref import jitter_velocities

pytestmark = pytest.mark.gpu
f32 = np.float32
SIDE = 64
SORTS = ["bitonic", "counting"]
MODES = ["ieee", "ulp", "tolerance"]


def _sort(fs, sort):
    return fs.FS_SORT_COUNTING if sort == "counting" else fs.FS_SORT_BITONIC


def _mode(fs, mode):
    return {"ieee": fs.FS_MATH_IEEE, "ulp": fs.FS_MATH_WGSL_ULP, "tolerance": fs.FS_MATH_TOLERANCE}[mode]


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texture", [False, True], ids=["plain", "texture"])
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("side", [64, 66])
def test_scene_matches_oracle_plus_operators(fs, orc, side, sort, texture):
    """FS_MATH_IEEE, dam_break_2d at 64^2 / 66^2 (whole and ragged 256-thread workgroups), both sort modes, 40 steps, a new pose
    before every step and no sync between steps: byte-equal to the oracle with the operators applied after every step, at steps 1,
    8 and 40.  With a non-zero force texture uploaded as well, the reference step's own push-out runs before the bodies."""
    run = B.oracle_run(fs, orc, side, sort, texture)
    sc = run["scene"]
    print(f"[bodies2d] side {side} {sort} texture {texture}: reference hits {run['hits'].sum(0).tolist()}, "
          f"re-clamped {run['reclamped'].sum(0).tolist()}")
    assert (run["hits"][0] > 0).all() and run["reclamped"][:8].sum() > 0
    if texture:
        plain = B.oracle_run(fs, orc, side, sort, False)
        assert plain["snap"][1].tobytes() != run["snap"][1].tobytes(), "the texture must act in step 1"
    sim = fs.FluidSimulation(sc.st, device=0, initial_offset=sc.off, sort_mode=_sort(fs, sort))
    if texture:
        sim.upload_force_field(run["texture"])
    for k, (mask, extent, field) in enumerate(zip(sc.masks, sc.extents, sc.fields)):
        slot, got = sim.add_body_mask(mask, extent, want_field=True)
        assert slot == k and got.tobytes() == field.tobytes(), f"body {k}: the producer's field"
    bodies = sc.bodies()
    for s in range(1, 41):
        for k, b in enumerate(sc.set_motions(bodies, s)):
            sim.set_body_motion(k, *b.motion())
        sim.tick(sc.tick)
        if s in run["snap"]:
            _same(sim.download_particles(), run["snap"][s], f"side {side} {sort} texture {texture} step {s}")
    sim.close()


@pytest.mark.parametrize("sort", SORTS)
def test_off_is_off(fs, orc, sort):
    """a handle whose bodies were all destroyed — with a step that read them still in flight — leaves the bytes of a handle that
    never had one: the oracle's, start_indices included"""
    st, off, tick = fs.dam_break_2d(SIDE ** 2)
    outs = []
    for variant in ("never", "destroyed"):
        sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=_sort(fs, sort))
        if variant == "destroyed":
            slots = _add(sim, _small_bodies(fs, 3))
            for k in slots:
                sim.set_body_motion(k, (50.0, 50.0))         # far outside the domain: the pass runs and touches nothing
        sim.tick(tick)
        if variant == "destroyed":
            for k in slots:
                sim.remove_body(k)
            assert sim.body_count == 0
        for _ in range(7):
            sim.tick(tick)
        outs.append((sim.download_particles(), sim.download_start_indices()))
        sim.close()
    assert outs[1][0].tobytes() == outs[0][0].tobytes(), "create + destroy changed the state"
    assert outs[1][1].tobytes() == outs[0][1].tobytes()
    ref = orc.OracleSim(st, initial_offset=off)
    for _ in range(8):
        ref.step(tick, stable_sort=sort == "counting")
    _same(outs[0][0], ref.particles(), "a handle without bodies, 8 steps")
    assert np.array_equal(outs[0][1], ref.start_indices())
    ref.close()


# ---- 2. the operator alone --------------------------------------------------------------------------------------------
_BASE = {}


def _make(fs, mode, sort, capacity=0):
    st, off, tick = fs.dam_break_2d(SIDE ** 2)
    return fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=mode, sort_mode=_sort(fs, sort), capacity=capacity)


def _base(fs, mode, sort="bitonic", prep=None, steps=1):
    """dam_break_2d(64^2) with jittered velocities: (settings, offset, tick, uploaded state, the state after `prep` and `steps`
    steps WITHOUT a body, ids, what prep returned, start_indices), per math mode, sort mode and prep; computed once"""
    key = (mode, sort, prep, steps)
    if key not in _BASE:
        st, off, tick = fs.dam_break_2d(SIDE ** 2)
        sim = _make(fs, mode, sort)
        p = jitter_velocities(sim.download_particles(), 11)
        sim.upload_particles(p)
        extra = prep(sim) if prep else None
        for _ in range(steps):
            sim.tick(tick)
        after = sim.download_particles()
        ids = sim.particle_ids() if sim.track_channels >= 0 else None
        starts = sim.download_start_indices()
        sim.close()
        after.setflags(write=False)
        _BASE[key] = (st, off, tick, p, after, ids, extra, starts)
    return _BASE[key]


def _one_step_with(fs, mode, bodies, sort="bitonic", prep=None, keep=False, before=None):
    st, off, tick, p = _base(fs, mode, sort, prep)[:4]
    sim = _make(fs, mode, sort)
    sim.upload_particles(p)
    if prep:
        prep(sim)
    _add(sim, bodies)
    if before:
        before(sim)
    sim.tick(tick)
    got = sim.download_particles()
    if keep:
        return got, sim
    sim.close()
    return got


def _moving_body(fs, field, extent=(1.6, 1.3), centre=(-5.9, 3.5), seed=1.0):
    """a body inside the initial block, at its corner between the -x wall and the floor, turned, translating and spinning"""
    c, rot = fs.rigid_motion2d(centre, (0.0, 0.0), 0.7 * seed, 1.0)
    return B.Body(field, extent, c, rot, (0.8, -0.5 * seed), 2.0 * seed)


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("mode", MODES)
def test_operator_alone_in_every_math_and_sort_mode(fs, mode, sort):
    """two handles of one mode, the same uploaded state, one with a body: its step is B of the other's step, byte for byte — also
    in FS_MATH_WGSL_ULP and FS_MATH_TOLERANCE, where the comparison with the oracle is only approximate"""
    m = _mode(fs, mode)
    st, _, tick, _, after, _, _, starts = _base(fs, m, sort)
    body = _moving_body(fs, B.random_field((13, 9), 3, fill=0.6, mag=0.6))
    want, hits, re = B.apply_body(after, body, _size(st), tick.damping_factor)
    print(f"[bodies2d] operator alone, {mode} {sort}: hit {hits}, re-clamped {re} of {after.shape[0]}")
    assert hits > 0 and re > 0
    got, sim = _one_step_with(fs, m, [body], sort, keep=True)
    _same(got, want, f"operator alone, {mode} {sort}")
    assert np.array_equal(sim.download_start_indices(), starts), "start_indices is not touched"
    sim.close()


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (1024, 1), (1, 257)])
def test_lookup_edges(fs, shape):
    """field shapes (W, H) with one pixel, with extents that divide nothing, with the largest extent and with a long thin axis"""
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    if shape == (1, 1):
        field = np.array([0.02, -0.03], dtype=f32).reshape(1, 1, 2)
    else:
        field = B.random_field(shape, sum(shape), fill=0.5)
    body = _moving_body(fs, field)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), want, f"lookup {shape}")


def test_vector_whose_squares_underflow_is_free_space(fs):
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    body = _moving_body(fs, np.full((1, 1, 2), 1e-30, dtype=f32))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits == 0 and want.tobytes() == after.tobytes()
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), after, "underflowing vector")
    field = np.zeros((1, 2, 2), dtype=f32)
    field[0, 0] = (1e-30, 1e-25)
    field[0, 1] = (0.0, -0.05)
    body = _moving_body(fs, field)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert 0 < hits < after.shape[0]
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), want, "underflowing vector beside a real one")


def test_two_overlapping_bodies_in_both_slot_orders(fs):
    """the operators do not commute: (P, Q) and (Q, P) give different bytes, each those of its own checker"""
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    p = _moving_body(fs, B.random_field((6, 5), 21, fill=0.7, mag=0.3))
    q = _moving_body(fs, B.random_field((3, 7), 22, fill=0.7, mag=0.3), extent=(1.3, 1.7), centre=(-5.6, 3.2), seed=-1.0)
    want_pq, hits_pq, _ = B.apply_bodies(after, [p, q], _size(st), tick.damping_factor)
    want_qp, hits_qp, _ = B.apply_bodies(after, [q, p], _size(st), tick.damping_factor)
    assert min(hits_pq) > 0 and min(hits_qp) > 0 and want_pq.tobytes() != want_qp.tobytes()
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [p, q]), want_pq, "bodies (P, Q)")
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [q, p]), want_qp, "bodies (Q, P)")


# ---- 3. slots ---------------------------------------------------------------------------------------------------------
def _small_bodies(fs, count):
    """`count` one-pixel bodies spread over the initial block, each with its own push, pose and velocity"""
    out = []
    for k in range(count):
        field = np.array([0.03 * (k % 3 - 1), 0.02 + 0.01 * k], dtype=f32).reshape(1, 1, 2)
        out.append(_moving_body(fs, field, extent=(0.7, 0.5), centre=(-5.5 + 0.6 * k, 3.0 - 0.5 * k), seed=0.5 + 0.25 * k))
    return out


def test_eight_bodies_and_the_ninth_is_refused(fs):
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    bodies = _small_bodies(fs, 8)
    want, hits, _ = B.apply_bodies(after, bodies, _size(st), tick.damping_factor)
    assert min(hits) > 0, hits
    got, sim = _one_step_with(fs, fs.FS_MATH_IEEE, bodies, keep=True)
    assert sim.body_count == fs._abi.FS_MAX_BODIES == 8
    _same(got, want, "eight bodies")
    with pytest.raises(fs.FluidSimError) as e:
        sim.add_body(bodies[0].field, bodies[0].extent)
    assert e.value.status == fs._abi.FS_ERR_INVALID and "slot" in str(e.value)
    with pytest.raises(fs.FluidSimError):
        sim.add_body_mask(np.zeros((1, 1), dtype=np.uint8), (1.0, 1.0))
    assert sim.body_count == 8
    sim.close()


def test_destroyed_slot_is_reused_and_the_others_stay(fs):
    st, off, tick, p, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    a, b, c, d = _small_bodies(fs, 4)
    sim = _make(fs, fs.FS_MATH_IEEE, "bitonic")
    sim.upload_particles(p)
    assert _add(sim, [a, b, c]) == [0, 1, 2]
    sim.remove_body(1)
    assert sim.body_count == 2
    with pytest.raises(fs.FluidSimError):
        sim.body_dims(1)
    assert sim.body_field(2).tobytes() == c.field.tobytes(), "body 2 stays body 2"
    assert _add(sim, [d]) == [1], "the lowest free slot"
    assert sim.body_count == 3
    sim.tick(tick)
    want, hits, _ = B.apply_bodies(after, [a, d, c], _size(st), tick.damping_factor)
    assert min(hits) > 0
    _same(sim.download_particles(), want, "slots 0, 1 (new), 2")
    sim.close()


# ---- 4. with the other features ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_live_aos_view(fs, sort):
    """after fs_export_handle the force pass writes the 32-byte records itself: a hit must reach them as well as the SoA state.
    The exported records, read through fs_import_read, and download_particles() are B of the step without a body; the second
    step, which reads the SoA arrays, equals that of a handle that never exported."""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after = _base(fs, m, sort)[:5]
    body = _moving_body(fs, B.random_field((6, 5), 41, fill=0.7, mag=0.6))
    want, hits, re = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0 and re > 0
    seen = {}

    def export(sim):
        handle = sim.export_handle()
        seen["view"] = sim.particles_device_ptr()
        assert handle.bytes == after.shape[0] * 32

    got, sim = _one_step_with(fs, m, [body], sort, keep=True, before=export)
    out = np.empty(after.shape[0], dtype=fs.PARTICLE_DTYPE)
    sim.sync()
    assert sim._lib.fs_import_read(C.c_void_p(seen["view"]), 0, out.ctypes.data_as(C.c_void_p), out.shape[0] * 32) == fs._abi.FS_OK
    _same(out, want, f"exported records, {sort}")
    _same(got, want, f"download_particles() of the exporting handle, {sort}")
    assert sim.particles_device_ptr() == seen["view"]
    sim.tick(tick)
    second = sim.download_particles()
    sim.close()
    _, plain = _one_step_with(fs, m, [body], sort, keep=True)
    plain.tick(tick)
    _same(second, plain.download_particles(), f"second step after an export, {sort}")
    plain.close()


def _prep_st_track(sim):
    sim.set_surface_tension(True)
    sim.track(1)
    sim.set_attribute(0, np.arange(sim.particle_count, dtype=f32))


def test_with_surface_tension_and_tracking(fs):
    """the pass changes no order: ids and channels are those of the handle without bodies, and the records by id are the records"""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after, ids = _base(fs, m, prep=_prep_st_track)[:6]
    plain = _base(fs, m)[4]
    assert after.tobytes() != plain.tobytes(), "surface tension must act in this scene"
    body = _moving_body(fs, B.random_field((6, 5), 31, fill=0.7, mag=0.3))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    got, sim = _one_step_with(fs, m, [body], prep=_prep_st_track, keep=True)
    _same(got, want, "surface tension + tracking + body")
    got_ids = sim.particle_ids()
    assert np.array_equal(got_ids, ids) and not np.array_equal(ids, np.arange(ids.shape[0])), "ids follow the sort, bodies or not"
    assert np.array_equal(sim.attribute(0), ids.astype(f32))
    _same(sim.download_particles_by_id()[got_ids], got, "records by id")
    sim.close()


def _emitted(dtype):
    rec = np.zeros(1, dtype=dtype)
    rec["position"] = (-5.9, 3.5)                        # the centre of _moving_body's box
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = (0.5, -0.5)
    return rec


def _prep_emit(sim):
    sim.reserve(4200)
    sim.emit(_emitted(sim._record))
    assert sim.particle_count == 4097 and sim.capacity == 4200
    return 0


def _prep_emit_remove(sim):
    _prep_emit(sim)
    return sim.remove_box((-2.0, -1.0), (-1.5, 0.5))


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("prep", [_prep_emit, _prep_emit_remove], ids=["emit", "emit+remove"])
def test_after_emission_and_removal(fs, prep, sort):
    """a live count of 4097 (one lane in the last workgroup) below a capacity of 4200, and a count a removal left"""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after, _, removed = _base(fs, m, sort, prep)[:7]
    n = 4097 - removed
    assert after.shape[0] == n and (removed > 0) == (prep is _prep_emit_remove)
    body = _moving_body(fs, np.full((2, 2, 2), 0.04, dtype=f32))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    got = _one_step_with(fs, m, [body], sort, prep=prep)
    _same(got, want, f"count {n}, {sort}")


@pytest.mark.parametrize("sort", SORTS)
def test_with_profiling_on(fs, sort):
    """the profiled step records its markers behind the bodies' pass instead of handing it the completion event: same bytes, and
    the pass's time lies inside FS_PASS_FORCE"""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after = _base(fs, m, sort)[:5]
    body = _moving_body(fs, B.random_field((6, 5), 51, fill=0.7, mag=0.3))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    got, sim = _one_step_with(fs, m, [body], sort, keep=True, before=lambda s: s.profile(True))
    _same(got, want, f"profiled step, {sort}")
    ms, steps = sim.profile_read()
    assert steps == 1 and ms["force"] > 0.0
    sim.close()


@pytest.mark.parametrize("sort", SORTS)
def test_through_timed_steps(fs, sort):
    """fs_timed_steps enqueues through the same path: three steps in one call equal three fs_step calls, both with the body at one
    pose, and differ from three steps without it"""
    m = fs.FS_MATH_IEEE
    tick = _base(fs, m, sort)[2]
    none = _base(fs, m, sort, steps=3)[4]
    body = _moving_body(fs, B.random_field((6, 5), 61, fill=0.7, mag=0.3))
    got, sim = _one_step_with(fs, m, [body], sort, keep=True)
    for _ in range(2):
        sim.tick(tick)
    want = sim.download_particles()
    sim.close()
    assert want.tobytes() != none.tobytes()
    st, off, tick, p = _base(fs, m, sort)[:4]
    sim = _make(fs, m, sort)
    sim.upload_particles(p)
    _add(sim, [body])
    assert sim.timed_steps(tick, 3) > 0.0
    _same(sim.download_particles(), want, f"timed_steps, {sort}")
    sim.close()


# ---- 5. the producer, the getters -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5), (65, 3), (5, 257), (1024, 2)])
def test_producer_matches_the_numpy_passes_on_the_bodys_box(fs, shape):
    sim = _make(fs, fs.FS_MATH_IEEE, "bitonic")
    w, h = shape
    extent = (0.7, 1.3)
    rng = np.random.default_rng(w * 31 + h * 7)
    for k, fill in enumerate((0.5, 0.97)):
        mask = np.where(rng.random((h, w)) < fill, rng.integers(129, 256, (h, w)), rng.integers(0, 129, (h, w))).astype(np.uint8)
        mask[0, 0] = 0
        want = B.producer_field(mask, extent)
        slot, got = sim.add_body_mask(mask, extent, want_field=True)
        assert slot == k and got.shape == want.shape and got.tobytes() == want.tobytes(), f"{shape} mask {k}: returned field"
        assert sim.body_field(slot).tobytes() == want.tobytes(), f"{shape} mask {k}: body_field()"
        assert sim.body_dims(slot) == ((w, h), tuple(float(f32(e)) for e in extent))
    sim.close()


def test_round_trips_and_nothing_goes_stale(fs):
    st, off, tick = fs.dam_break_2d(SIDE ** 2)
    sim = _make(fs, fs.FS_MATH_IEEE, "bitonic")
    assert sim.body_count == 0
    sim.tick(tick)
    pts = np.array([[-5.7, 3.2], [0.0, 0.0]], dtype=f32)
    before = sim.sample(pts)
    image = sim.render_density(16, 8)
    field = B.random_field((6, 5), 2)
    k = sim.add_body(field, (0.5, 0.25))
    assert k == 0 and sim.body_count == 1
    assert sim.sample(pts).tobytes() == before.tobytes(), "creating a body must not make sampling stale"
    c, r, u, w = sim.body_motion(k)
    assert c.tolist() == [0, 0] and r.reshape(4).tolist() == list(B.IDENTITY) and u.tolist() == [0, 0] and float(w) == 0.0
    rot = np.arange(4, dtype=f32) * f32(0.1) - f32(0.3)       # any finite floats: only finiteness is checked
    sim.set_body_motion(k, (0.1, -0.2), rot, (1.0, 2.0), -4.0)
    c, r, u, w = sim.body_motion(k)
    assert c.tobytes() == np.array([0.1, -0.2], dtype=f32).tobytes() and r.tobytes() == rot.tobytes()
    assert u.tolist() == [1.0, 2.0] and float(w) == -4.0
    assert sim.body_dims(k) == ((6, 5), (0.5, 0.25))
    back = sim.body_field(k)
    assert back.shape == (5, 6, 2) and back.tobytes() == field.tobytes()
    assert sim.sample(pts).tobytes() == before.tobytes(), "moving a body must not make sampling stale"
    assert sim.render_density(16, 8).tobytes() == image.tobytes()
    # a step with a body that hits: sampling and rendering are not refused afterwards
    sim.set_body_motion(k, (-5.9, 3.5))
    sim.tick(tick)
    assert sim.sample(pts).shape == (2,) and sim.sample_grid(4, 4).shape == (4, 4) and sim.render_density(16, 8).shape == (8, 16, 4)
    sim.remove_body(k)
    assert sim.sample(pts).shape == (2,), "destroying a body must not make sampling stale"
    sim.close()


# ---- 6. argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_the_headers_order_and_a_refused_call_changes_nothing(fs):
    st, off, tick, p, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    sim = _make(fs, fs.FS_MATH_IEEE, "bitonic")
    sim.upload_particles(p)
    lib, h, INV, OK = sim._lib, sim._h, fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    V = fs.Vec2
    err = lambda: lib.fs_last_error().decode()      # noqa: E731
    ok = np.zeros((2, 2, 2), dtype=f32)
    ok[0, 0] = (0.1, 0.0)
    bad = ok.copy()
    bad[1, 1, 1] = np.nan
    okp, badp = ok.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p)
    solid = np.full(4, 255, dtype=np.uint8)
    sp = solid.ctypes.data_as(C.c_void_p)
    slot, w = C.c_uint32(77), C.c_uint32()
    e1, ebad = V(1.0, 1.0), V(1.0, 0.0)
    mo = fs.BodyMotion()
    # 1. the handle, before anything else is looked at
    assert lib.fs_body_create(None, None, 0, 0, ebad, None) == INV and "null" in err()
    assert lib.fs_body_create_from_mask(None, None, 0, 0, ebad, None, None) == INV and "null" in err()
    assert lib.fs_body_set_motion(None, 0, None) == INV and lib.fs_body_get_motion(None, 0, None) == INV
    assert lib.fs_body_dims(None, 0, None, None, None) == INV and lib.fs_body_download(None, 0, None, 0) == INV
    assert lib.fs_body_destroy(None, 0) == INV and lib.fs_body_count(None) == 0
    # 3. the pointers, before the extents
    assert lib.fs_body_create(h, None, 0, 1025, ebad, C.byref(slot)) == INV and "null" in err()
    assert lib.fs_body_create(h, badp, 0, 1025, ebad, None) == INV and "null" in err()
    assert lib.fs_body_create_from_mask(h, None, 2, 0, ebad, None, C.byref(slot)) == INV and "null" in err()
    assert lib.fs_body_create_from_mask(h, sp, 2, 0, ebad, None, None) == INV and "null" in err()
    assert lib.fs_body_set_motion(h, 9, None) == INV and "null" in err()
    assert lib.fs_body_get_motion(h, 9, None) == INV and "null" in err()
    assert lib.fs_body_dims(h, 9, C.byref(w), C.byref(w), None) == INV and "null" in err()
    assert lib.fs_body_download(h, 9, None, 4) == INV and "null" in err()
    # 4. w and h, before the box (a bad box and a NaN in the array ride along)
    for dims in [(0, 2), (2, 0), (1025, 1), (1, 1025)]:
        assert lib.fs_body_create(h, badp, *dims, ebad, C.byref(slot)) == INV and "of 0 or above 1024" in err(), dims
        assert lib.fs_body_create_from_mask(h, sp, *dims, ebad, None, C.byref(slot)) == INV and "of 0 or above 1024" in err(), dims
    # 5. the box, before the values
    for box in [V(0.0, 1.0), V(1.0, -1.0), V(1.0, np.inf), V(np.nan, 1.0)]:
        assert lib.fs_body_create(h, badp, 2, 2, box, C.byref(slot)) == INV and "box" in err()
        assert lib.fs_body_create_from_mask(h, sp, 2, 2, box, None, C.byref(slot)) == INV and "box" in err()
    # 6. the values
    assert lib.fs_body_create(h, badp, 2, 2, e1, C.byref(slot)) == INV and "non-finite" in err()
    assert lib.fs_body_create_from_mask(h, sp, 2, 2, e1, None, C.byref(slot)) == INV and "free pixel" in err()
    assert slot.value == 77 and sim.body_count == 0, "a refused call sets nothing"
    # 8. a slot that holds no body
    for k in (0, 7, 8, 0xFFFFFFFF):
        assert lib.fs_body_set_motion(h, k, C.byref(mo)) == INV and "holds no body" in err()
        assert lib.fs_body_get_motion(h, k, C.byref(mo)) == INV and lib.fs_body_destroy(h, k) == INV
        assert lib.fs_body_download(h, k, okp, 4) == INV and "holds no body" in err()
    # a body, then 9. non-finite motion: refused whole, the motion set before stays
    body = B.Body(np.full((2, 2, 2), 0.04, dtype=f32), (1.6, 1.3)).set_motion(*_moving_body(fs, ok).motion())
    assert _add(sim, [body]) == [0]
    assert lib.fs_body_download(h, 0, okp, 3) == INV and "w * h" in err()
    for name, idx in (("centre", 1), ("rot", 3), ("velocity", 0), ("angular_velocity", None)):
        for value in (np.nan, np.inf, -np.inf):
            assert lib.fs_body_get_motion(h, 0, C.byref(mo)) == OK
            if name == "rot":
                mo.rot[idx] = value
            elif idx is None:
                mo.angular_velocity = value
            else:
                setattr(getattr(mo, name), "xy"[idx], value)
            assert lib.fs_body_set_motion(h, 0, C.byref(mo)) == INV and "non-finite" in err(), (name, value)
    # 7. no free slot comes after the values: with eight bodies a NaN field is still "non-finite"
    for k in range(1, 8):
        assert lib.fs_body_create(h, okp, 2, 2, V(1e-3, 1e-3), C.byref(slot)) == OK and slot.value == k
        sim.set_body_motion(k, (50.0, 50.0))             # far outside the domain
    assert lib.fs_body_create(h, badp, 2, 2, e1, C.byref(slot)) == INV and "non-finite" in err()
    assert lib.fs_body_create(h, okp, 2, 2, e1, C.byref(slot)) == INV and "slot" in err() and slot.value == 7
    # after all the refusals the step is that of the one real body with the motion it was given
    for got, want in zip(sim.body_motion(0), body.motion()):
        assert np.asarray(got).tobytes() == np.asarray(want, dtype=f32).tobytes()
    sim.tick(tick)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    _same(sim.download_particles(), want, "after the refused calls")
    sim.close()


def test_slab_handle_is_refused_as_unsupported(fs):
    """2. a slab handle, right after the NULL check and before the pointers"""
    st, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    lib, h, UNS = fs.load_library(), slab._h, fs._abi.FS_ERR_UNSUPPORTED
    slot, w = C.c_uint32(77), C.c_uint32()
    mo = fs.BodyMotion()
    field = np.zeros((1, 1, 2), dtype=f32)
    assert lib.fs_body_create(h, None, 0, 0, fs.Vec2(0, 0), None) == UNS and "slab" in lib.fs_last_error().decode()
    assert lib.fs_body_create(h, field.ctypes.data_as(C.c_void_p), 1, 1, fs.Vec2(1, 1), C.byref(slot)) == UNS
    assert lib.fs_body_create_from_mask(h, None, 0, 0, fs.Vec2(0, 0), None, None) == UNS
    assert lib.fs_body_set_motion(h, 0, None) == UNS and lib.fs_body_set_motion(h, 0, C.byref(mo)) == UNS
    assert lib.fs_body_get_motion(h, 0, None) == UNS and lib.fs_body_dims(h, 0, C.byref(w), C.byref(w), None) == UNS
    assert lib.fs_body_download(h, 0, None, 0) == UNS and lib.fs_body_destroy(h, 0) == UNS
    assert lib.fs_body_count(h) == 0 and slot.value == 77
    slab.close()

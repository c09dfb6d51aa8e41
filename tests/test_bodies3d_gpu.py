"""3D moving bodies on the GPU (include/fluidsim.h "3D moving bodies").  The checker is the unchanged 3D oracle
plus the numpy operators of tests/bodies3d_ref.py (new state = B_7(...B_0(C(step(state))))); where no oracle is involved, a handle
with bodies is compared with B of a handle without.  Byte equality everywhere: no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies3d_ref as B
from tests import collide3d_ref as CR
from tests.handle_helpers import _add, _same, _size
from tests.track_ref import jitter_velocities

pytestmark = pytest.mark.gpu
f32 = np.float32
SIDE = 16


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("static", [None, "a"])
@pytest.mark.parametrize("side", [16, 18])
def test_scene_matches_oracle_plus_operators(fs, orc, side, static):
    """FS_MATH_IEEE, dam_break_3d at 16^3 / 18^3 (whole and ragged 256-thread workgroups), 40 steps, a new pose before every step
    and no sync between steps: byte-equal to the oracle with the operators applied after every step, at steps 1, 8 and 40.  With
    §18's static scene (a) also set, C runs before the bodies."""
    run = B.oracle_run(fs, orc, side, static)
    sc = run["scene"]
    print(f"[bodies3d] side {side} static {static}: reference hits {run['hits'].sum(0).tolist()}, re-clamped {run['reclamped'].sum(0).tolist()}")
    assert (run["hits"][0] > 0).all() and run["reclamped"][:8].sum() > 0
    sim = fs.FluidSimulation3D(sc.st, device=0, initial_offset=sc.off)
    if static:
        sim.set_collider(run["static"])
    for k, (mask, extent, field) in enumerate(zip(sc.masks, sc.extents, sc.fields)):
        slot, got = sim.add_body_mask(mask, extent, want_field=True)
        assert slot == k and got.tobytes() == field.tobytes(), f"body {k}: the producer's field"
    bodies = sc.bodies()
    for s in range(1, 41):
        for k, b in enumerate(sc.set_motions(bodies, s)):
            sim.set_body_motion(k, *b.motion())
        sim.tick(sc.tick)
        if s in run["snap"]:
            _same(sim.download_particles(), run["snap"][s], f"side {side} static {static} step {s}")
    sim.close()


# ---- 2. the operator alone --------------------------------------------------------------------------------------------
_BASE = {}


def _base(fs, mode, prep=None):
    """dam_break_3d(16^3) with jittered velocities: (settings, offset, tick, uploaded state, the state after `prep` and one step
    WITHOUT a body), per math mode and prep; computed once"""
    key = (mode, prep)
    if key not in _BASE:
        st, off, tick = fs.dam_break_3d(SIDE ** 3)
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
        p = jitter_velocities(sim.download_particles(), 11)
        sim.upload_particles(p)
        extra = prep(sim) if prep else None
        sim.tick(tick)
        after = sim.download_particles()
        ids = sim.particle_ids() if sim.track_channels >= 0 else None
        sim.close()
        after.setflags(write=False)
        _BASE[key] = (st, off, tick, p, after, ids, extra)
    return _BASE[key]


def _one_step_with(fs, mode, bodies, prep=None, keep=False):
    st, off, tick, p = _base(fs, mode, prep)[:4]
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
    sim.upload_particles(p)
    if prep:
        prep(sim)
    _add(sim, bodies)
    sim.tick(tick)
    got = sim.download_particles()
    if keep:
        return got, sim
    sim.close()
    return got


def _moving_body(fs, field, extent=(1.0, 0.9, 1.2), centre=(-0.8, 0.3, 0.1), seed=1.0):
    """a body inside the initial block, turned about a skew axis, translating and spinning"""
    c, rot = fs.rigid_motion(centre, (0.0, 0.0, 0.0), (1.0, 2.0 * seed, 3.0), 0.7 * seed, 1.0)
    return B.Body(field, extent, c, rot, (0.8, -0.5 * seed, 0.3), (0.5, -1.0, 2.0 * seed))


@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_operator_alone_both_math_modes(fs, mode):
    """two handles of one mode, the same uploaded state, one with a body: its step is B of the other's step, byte for byte — also
    in FS_MATH_TOLERANCE, where the comparison with the oracle is only approximate"""
    m = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    st, _, tick, _, after = _base(fs, m)[:5]
    body = _moving_body(fs, CR.random_field((13, 9, 7), 3, fill=0.6, mag=0.4))
    want, hits, re = B.apply_body(after, body, _size(st), tick.damping_factor)
    print(f"[bodies3d] operator alone, {mode}: hit {hits}, re-clamped {re} of {after.shape[0]}")
    assert hits > 0 and re > 0
    _same(_one_step_with(fs, m, [body]), want, f"operator alone, {mode}")


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 2), (1024, 1, 1), (3, 1, 257)])
def test_lookup_edges(fs, shape):
    """field shapes (W, H, D) with one voxel, with extents that divide nothing, with the largest extent and with a long thin axis"""
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    if shape == (1, 1, 1):
        field = np.array([0.02, -0.03, 0.01], dtype=f32).reshape(1, 1, 1, 3)
    else:
        field = CR.random_field(shape, sum(shape), fill=0.5)
    body = _moving_body(fs, field)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), want, f"lookup {shape}")


def test_vector_whose_squares_underflow_is_free_space(fs):
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    body = _moving_body(fs, np.full((1, 1, 1, 3), 1e-30, dtype=f32))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits == 0 and want.tobytes() == after.tobytes()
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), after, "underflowing vector")
    field = np.zeros((1, 1, 2, 3), dtype=f32)
    field[0, 0, 0] = (1e-30, 0, 1e-25)
    field[0, 0, 1] = (0.0, -0.05, 0.0)
    body = _moving_body(fs, field)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert 0 < hits < after.shape[0]
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [body]), want, "underflowing vector beside a real one")


def test_two_overlapping_bodies_in_both_slot_orders(fs):
    """the operators do not commute: (P, Q) and (Q, P) give different bytes, each those of its own checker"""
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    p = _moving_body(fs, CR.random_field((6, 5, 4), 21, fill=0.7, mag=0.3))
    q = _moving_body(fs, CR.random_field((3, 7, 5), 22, fill=0.7, mag=0.3), extent=(0.9, 1.1, 0.8), centre=(-0.6, 0.2, -0.1), seed=-1.0)
    want_pq, hits_pq, _ = B.apply_bodies(after, [p, q], _size(st), tick.damping_factor)
    want_qp, hits_qp, _ = B.apply_bodies(after, [q, p], _size(st), tick.damping_factor)
    assert min(hits_pq) > 0 and min(hits_qp) > 0 and want_pq.tobytes() != want_qp.tobytes()
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [p, q]), want_pq, "bodies (P, Q)")
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, [q, p]), want_qp, "bodies (Q, P)")


# ---- 3. slots ---------------------------------------------------------------------------------------------------------
def _small_bodies(fs, count):
    """`count` one-voxel bodies spread over the initial block, each with its own push, pose and velocity"""
    out = []
    for k in range(count):
        field = np.array([0.03 * (k % 3 - 1), 0.02 + 0.01 * k, -0.02 * (k % 2)], dtype=f32).reshape(1, 1, 1, 3)
        out.append(_moving_body(fs, field, extent=(0.5, 0.4, 0.6), centre=(-1.3 + 0.15 * k, 0.6 - 0.1 * k, -0.4 + 0.1 * k), seed=0.5 + 0.25 * k))
    return out


def test_eight_bodies_and_the_ninth_is_refused(fs):
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    bodies = _small_bodies(fs, 8)
    want, hits, _ = B.apply_bodies(after, bodies, _size(st), tick.damping_factor)
    assert min(hits) > 0, hits
    got, sim = _one_step_with(fs, fs.FS_MATH_IEEE, bodies, keep=True)
    assert sim.body_count == fs._abi.FS3_MAX_BODIES == 8
    _same(got, want, "eight bodies")
    with pytest.raises(fs.FluidSimError) as e:
        sim.add_body(bodies[0].field, bodies[0].extent)
    assert e.value.status == fs._abi.FS_ERR_INVALID and "slot" in str(e.value)
    with pytest.raises(fs.FluidSimError):
        sim.add_body_mask(np.zeros((1, 1, 1), dtype=np.uint8), (1.0, 1.0, 1.0))
    assert sim.body_count == 8
    sim.close()


def test_destroyed_slot_is_reused_and_the_others_stay(fs):
    st, off, tick, p, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    a, b, c, d = _small_bodies(fs, 4)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
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


def test_off_is_off(fs, orc):
    """a handle whose bodies were all destroyed — with a step that read them still in flight — leaves the bytes of a handle that
    never had one: the oracle's"""
    st, off, tick = fs.dam_break_3d(SIDE ** 3)
    outs = []
    for variant in ("never", "destroyed"):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        if variant == "destroyed":
            slots = _add(sim, _small_bodies(fs, 3))
            for k in slots:
                sim.set_body_motion(k, (50.0, 50.0, 50.0))       # far outside the domain: the pass runs and touches nothing
        sim.tick(tick)
        if variant == "destroyed":
            for k in slots:
                sim.remove_body(k)
            assert sim.body_count == 0
        for _ in range(7):
            sim.tick(tick)
        outs.append(sim.download_particles())
        sim.close()
    assert outs[1].tobytes() == outs[0].tobytes(), "create + destroy changed the state"
    ref = orc.OracleSim3D(st, initial_offset=off)
    for _ in range(8):
        ref.step(tick)
    _same(outs[0], ref.particles(), "a handle without bodies, 8 steps")
    ref.close()


# ---- 4. with the other features ---------------------------------------------------------------------------------------
def _prep_st_track(sim):
    sim.set_surface_tension(0.02, 0.5)
    sim.track(1)
    sim.set_attribute(0, np.arange(sim.particle_count, dtype=f32))


def test_with_surface_tension_and_tracking(fs):
    """the pass changes no order: ids and channels are those of the handle without bodies, and the records by id are the records"""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after, ids, _ = _base(fs, m, _prep_st_track)
    plain = _base(fs, m)[4]
    assert after.tobytes() != plain.tobytes(), "surface tension must act in this scene"
    body = _moving_body(fs, CR.random_field((6, 5, 4), 31, fill=0.7, mag=0.3))
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
    rec["position"] = (-0.8, 0.3, 0.1)                   # the centre of _moving_body's box
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = (0.5, 0.0, -0.5)
    return rec


def _prep_emit(sim):
    sim.reserve(4200)
    sim.emit(_emitted(sim._record))
    assert sim.particle_count == 4097
    return 0


def _prep_emit_remove(sim):
    _prep_emit(sim)
    return sim.remove_box((-1.2, -0.2, -0.9), (-1.0, 0.4, 0.9))


@pytest.mark.parametrize("prep", [_prep_emit, _prep_emit_remove], ids=["emit", "emit+remove"])
def test_after_emission_and_removal(fs, prep):
    """a live count of 4097 (one lane in the last workgroup) below a capacity of 4200, and a count a removal left"""
    m = fs.FS_MATH_IEEE
    st, _, tick, _, after, _, removed = _base(fs, m, prep)
    n = 4097 - removed
    assert after.shape[0] == n and (removed > 0) == (prep is _prep_emit_remove)
    body = _moving_body(fs, np.full((2, 2, 2, 3), 0.04, dtype=f32))
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    got = _one_step_with(fs, m, [body], prep=prep)
    _same(got, want, f"count {n}")


# ---- 5. the producer, the getters -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5), (65, 3, 2), (5, 4, 257)])
def test_producer_matches_the_numpy_passes_on_the_bodys_box(fs, shape):
    st, off, _ = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    w, h, d = shape
    extent = (0.7, 1.3, 0.9)
    rng = np.random.default_rng(w * 31 + h * 7 + d)
    for k, fill in enumerate((0.5, 0.97)):
        mask = np.where(rng.random((d, h, w)) < fill, rng.integers(129, 256, (d, h, w)), rng.integers(0, 129, (d, h, w))).astype(np.uint8)
        mask[0, 0, 0] = 0
        want = CR.producer_field(mask, extent)
        slot, got = sim.add_body_mask(mask, extent, want_field=True)
        assert slot == k and got.shape == want.shape and got.tobytes() == want.tobytes(), f"{shape} mask {k}: returned field"
        assert sim.body_field(slot).tobytes() == want.tobytes(), f"{shape} mask {k}: body_field()"
        assert sim.body_dims(slot) == ((w, h, d), tuple(float(f32(e)) for e in extent))
    sim.close()


def test_round_trips_and_nothing_goes_stale(fs):
    st, off, tick = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    assert sim.body_count == 0
    sim.tick(tick)
    pts = np.array([[-0.7, 0.2, 0.0], [0.0, 0.0, 0.0]], dtype=f32)
    before = sim.sample(pts)
    field = CR.random_field((6, 5, 4), 2)
    k = sim.add_body(field, (0.5, 0.25, 2.0))
    assert k == 0 and sim.body_count == 1
    assert sim.sample(pts).tobytes() == before.tobytes(), "creating a body must not make sampling stale"
    c, r, u, w = sim.body_motion(k)
    assert c.tolist() == [0, 0, 0] and r.reshape(9).tolist() == list(B.IDENTITY) and u.tolist() == [0, 0, 0] and w.tolist() == [0, 0, 0]
    rot = np.arange(9, dtype=f32) * f32(0.1) - f32(0.3)       # any finite floats: only finiteness is checked
    sim.set_body_motion(k, (0.1, -0.2, 0.3), rot, (1.0, 2.0, 3.0), (-4.0, 5.0, -6.0))
    c, r, u, w = sim.body_motion(k)
    assert c.tobytes() == np.array([0.1, -0.2, 0.3], dtype=f32).tobytes() and r.tobytes() == rot.tobytes()
    assert u.tolist() == [1.0, 2.0, 3.0] and w.tolist() == [-4.0, 5.0, -6.0]
    assert sim.body_dims(k) == ((6, 5, 4), (0.5, 0.25, 2.0))
    back = sim.body_field(k)
    assert back.shape == (4, 5, 6, 3) and back.tobytes() == field.tobytes()
    assert sim.sample(pts).tobytes() == before.tobytes(), "moving a body must not make sampling stale"
    sim.remove_body(k)
    assert sim.sample(pts).tobytes() == before.tobytes(), "destroying a body must not make sampling stale"
    sim.close()


# ---- 6. argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_the_headers_order_and_a_refused_call_changes_nothing(fs):
    st, off, tick, p, after = _base(fs, fs.FS_MATH_IEEE)[:5]
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    lib, h, INV, OK = sim._lib, sim._h, fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    V = fs.Vec3
    err = lambda: lib.fs_last_error().decode()      # noqa: E731
    ok = np.zeros((2, 2, 2, 3), dtype=f32)
    ok[0, 0, 0] = (0.1, 0.0, 0.0)
    bad = ok.copy()
    bad[1, 1, 1, 2] = np.nan
    okp, badp = ok.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p)
    solid = np.full(8, 255, dtype=np.uint8)
    sp = solid.ctypes.data_as(C.c_void_p)
    slot, w = C.c_uint32(77), C.c_uint32()
    e1, ebad = V(1.0, 1.0, 1.0), V(1.0, 0.0, 1.0)
    mo = fs.BodyMotion3()
    # 1. the handle, before anything else is looked at
    assert lib.fs3_body_create(None, None, 0, 0, 0, ebad, None) == INV and "null" in err()
    assert lib.fs3_body_create_from_mask(None, None, 0, 0, 0, ebad, None, None) == INV and "null" in err()
    assert lib.fs3_body_set_motion(None, 0, None) == INV and lib.fs3_body_get_motion(None, 0, None) == INV
    assert lib.fs3_body_dims(None, 0, None, None, None, None) == INV and lib.fs3_body_download(None, 0, None, 0) == INV
    assert lib.fs3_body_destroy(None, 0) == INV and lib.fs3_body_count(None) == 0
    # 2. the pointers, before the extents
    assert lib.fs3_body_create(h, None, 0, 1025, 2, ebad, C.byref(slot)) == INV and "null" in err()
    assert lib.fs3_body_create(h, badp, 0, 1025, 2, ebad, None) == INV and "null" in err()
    assert lib.fs3_body_create_from_mask(h, None, 2, 2, 0, ebad, None, C.byref(slot)) == INV and "null" in err()
    assert lib.fs3_body_create_from_mask(h, sp, 2, 2, 0, ebad, None, None) == INV and "null" in err()
    assert lib.fs3_body_set_motion(h, 9, None) == INV and "null" in err()
    assert lib.fs3_body_get_motion(h, 9, None) == INV and "null" in err()
    assert lib.fs3_body_dims(h, 9, C.byref(w), C.byref(w), C.byref(w), None) == INV and "null" in err()
    assert lib.fs3_body_download(h, 9, None, 8) == INV and "null" in err()
    # 3. the extents, before the box (a bad box and a NaN in the array ride along)
    for dims in [(0, 2, 2), (2, 0, 2), (2, 2, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025)]:
        assert lib.fs3_body_create(h, badp, *dims, ebad, C.byref(slot)) == INV and "an extent of 0" in err(), dims
        assert lib.fs3_body_create_from_mask(h, sp, *dims, ebad, None, C.byref(slot)) == INV and "an extent of 0" in err(), dims
    # 4. the box, before the values
    for box in [V(0.0, 1.0, 1.0), V(1.0, -1.0, 1.0), V(1.0, 1.0, np.inf), V(np.nan, 1.0, 1.0)]:
        assert lib.fs3_body_create(h, badp, 2, 2, 2, box, C.byref(slot)) == INV and "box" in err()
        assert lib.fs3_body_create_from_mask(h, sp, 2, 2, 2, box, None, C.byref(slot)) == INV and "box" in err()
    # 5. the values
    assert lib.fs3_body_create(h, badp, 2, 2, 2, e1, C.byref(slot)) == INV and "non-finite" in err()
    assert lib.fs3_body_create_from_mask(h, sp, 2, 2, 2, e1, None, C.byref(slot)) == INV and "free voxel" in err()
    assert slot.value == 77 and sim.body_count == 0, "a refused call sets nothing"
    # 7. a slot that holds no body
    for k in (0, 7, 8, 0xFFFFFFFF):
        assert lib.fs3_body_set_motion(h, k, C.byref(mo)) == INV and "holds no body" in err()
        assert lib.fs3_body_get_motion(h, k, C.byref(mo)) == INV and lib.fs3_body_destroy(h, k) == INV
        assert lib.fs3_body_download(h, k, okp, 8) == INV and "holds no body" in err()
    # a body, then 8. non-finite motion: refused whole, the motion set before stays
    body = B.Body(np.full((2, 2, 2, 3), 0.04, dtype=f32), (1.0, 0.9, 1.2)).set_motion(*_moving_body(fs, ok).motion())
    assert _add(sim, [body]) == [0]
    assert lib.fs3_body_download(h, 0, okp, 7) == INV and "w * h * d" in err()
    for name, idx in (("centre", 1), ("rot", 8), ("velocity", 0), ("angular_velocity", 2)):
        for value in (np.nan, np.inf, -np.inf):
            assert lib.fs3_body_get_motion(h, 0, C.byref(mo)) == OK
            if name == "rot":
                mo.rot[idx] = value
            else:
                setattr(getattr(mo, name), "xyz"[idx], value)
            assert lib.fs3_body_set_motion(h, 0, C.byref(mo)) == INV and "non-finite" in err(), (name, value)
    # 6. no free slot comes after the values: with eight bodies a NaN field is still "non-finite"
    for k in range(1, 8):
        assert lib.fs3_body_create(h, okp, 2, 2, 2, V(1e-3, 1e-3, 1e-3), C.byref(slot)) == OK and slot.value == k
        sim.set_body_motion(k, (50.0, 50.0, 50.0))       # far outside the domain
    assert lib.fs3_body_create(h, badp, 2, 2, 2, e1, C.byref(slot)) == INV and "non-finite" in err()
    assert lib.fs3_body_create(h, okp, 2, 2, 2, e1, C.byref(slot)) == INV and "slot" in err() and slot.value == 7
    # after all the refusals the step is that of the one real body with the motion it was given
    for got, want in zip(sim.body_motion(0), body.motion()):
        assert got.tobytes() == np.asarray(want, dtype=f32).tobytes()
    sim.tick(tick)
    want, hits, _ = B.apply_body(after, body, _size(st), tick.damping_factor)
    assert hits > 0
    _same(sim.download_particles(), want, "after the refused calls")
    sim.close()

"""3D colliders on the GPU (include/fluidsim.h "3D colliders").  The checker is the unchanged 3D oracle plus the
numpy operator C of tests/collide3d_ref.py (new state = C(step(state))); the producer is compared with the numpy passes.  Byte
equality everywhere: no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from tests import collide3d_ref as R
from tests.handle_helpers import _same, _size
from tests.track_ref import jitter_velocities

pytestmark = pytest.mark.gpu
f32 = np.float32
SIDE = 16


_random_field = R.random_field


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["a", "b"])
@pytest.mark.parametrize("side", [16, 18])
def test_collider_step_matches_oracle_plus_operator(fs, orc, side, scene):
    """FS_MATH_IEEE, dam_break_3d at 16^3 / 18^3 (whole and ragged 256-thread workgroups), 40 steps: byte-equal to the oracle with C
    applied after every step, at steps 1, 8 and 40.  (a) a box on the floor in the dam's path, (b) a layer pushing through the wall."""
    run = R.oracle_run(fs, orc, side, scene)
    print(f"[collide3d] side {side} scene {scene}: reference pushed {run['pushed']}, re-clamped {run['reclamped']}")
    if scene == "a":
        assert run["pushed"] > 0, "the dam must reach the box"
    else:
        assert run["reclamped"] > 0, "the layer must push particles through the wall"
    st, off, tick = fs.dam_break_3d(side ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.set_collider(run["field"])
    for s in range(1, 41):
        sim.tick(tick)
        if s in run["snap"]:
            _same(sim.download_particles(), run["snap"][s], f"side {side} scene {scene} step {s}")
    sim.close()


# ---- 2. / 3. the operator alone ----------------------------------------------------------------------------------------
_BASE = {}


def _base(fs, mode):
    """dam_break_3d(16^3) with jittered velocities: (settings, offset, tick, uploaded state, the state after one step WITHOUT a
    collider), per math mode; computed once"""
    if mode not in _BASE:
        st, off, tick = fs.dam_break_3d(SIDE ** 3)
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
        p = jitter_velocities(sim.download_particles(), 11)
        sim.upload_particles(p)
        sim.tick(tick)
        after = sim.download_particles()
        sim.close()
        after.setflags(write=False)
        _BASE[mode] = (st, off, tick, p, after)
    return _BASE[mode]


def _one_step_with(fs, mode, field):
    st, off, tick, p, _ = _base(fs, mode)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
    sim.upload_particles(p)
    sim.set_collider(field)
    sim.tick(tick)
    got = sim.download_particles()
    sim.close()
    return got


@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_operator_alone_both_math_modes(fs, mode):
    """two handles of one mode, the same uploaded state, one with a collider: its step is C of the other's step, byte for byte —
    also in FS_MATH_TOLERANCE, where the comparison with the oracle is only approximate and a voxel edge could flip"""
    m = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    st, _, tick, _, after = _base(fs, m)
    field = _random_field((13, 9, 7), 3, fill=0.6, mag=0.4)
    want, pushed, reclamped = R.apply_collider(after, field, _size(st), tick.damping_factor)
    print(f"[collide3d] operator alone, {mode}: pushed {pushed}, re-clamped {reclamped} of {after.shape[0]}")
    assert pushed > 0 and reclamped > 0
    _same(_one_step_with(fs, m, field), want, f"operator alone, {mode}")


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 2), (1024, 1, 1), (3, 1, 257)])
def test_lookup_edges(fs, shape):
    """field shapes (W, H, D) with one voxel, with extents that divide nothing, with the largest extent and with a long thin axis"""
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)
    if shape == (1, 1, 1):
        field = np.array([0.02, -0.03, 0.01], dtype=f32).reshape(1, 1, 1, 3)
    else:
        field = _random_field(shape, sum(shape), fill=0.5)
    want, pushed, _ = R.apply_collider(after, field, _size(st), tick.damping_factor)
    assert pushed > 0
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, field), want, f"lookup {shape}")


def test_vector_whose_squares_underflow_is_free_space(fs):
    st, _, tick, _, after = _base(fs, fs.FS_MATH_IEEE)
    field = np.full((1, 1, 1, 3), 1e-30, dtype=f32)
    want, pushed, _ = R.apply_collider(after, field, _size(st), tick.damping_factor)
    assert pushed == 0 and want.tobytes() == after.tobytes()
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, field), after, "underflowing vector")
    # next to a real vector in one field
    field = np.zeros((1, 1, 2, 3), dtype=f32)
    field[0, 0, 0] = (1e-30, 0, 1e-25)
    field[0, 0, 1] = (0.0, -0.05, 0.0)
    want, pushed, _ = R.apply_collider(after, field, _size(st), tick.damping_factor)
    assert 0 < pushed < after.shape[0]
    _same(_one_step_with(fs, fs.FS_MATH_IEEE, field), want, "underflowing vector beside a real one")


# ---- 4. off is off ----------------------------------------------------------------------------------------------------
def test_off_is_off(fs):
    """an all-zero field, and an upload followed by clear, leave 8 steps byte-identical to a handle that never had a collider"""
    st, off, tick, p, _ = _base(fs, fs.FS_MATH_IEEE)
    outs = []
    for variant in ("never", "zero", "cleared"):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        sim.upload_particles(p)
        if variant == "zero":
            sim.set_collider(np.zeros((4, 5, 6, 3), dtype=f32))
        elif variant == "cleared":
            sim.set_collider(_random_field((6, 5, 4), 1))
            sim.clear_collider()
            assert sim.collider() is None and sim.collider_dims == (0, 0, 0)
        for _ in range(8):
            sim.tick(tick)
        outs.append(sim.download_particles())
        sim.close()
    assert outs[1].tobytes() == outs[0].tobytes(), "an all-zero field changed the state"
    assert outs[2].tobytes() == outs[0].tobytes(), "upload + clear changed the state"


# ---- 5. the producer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5), (65, 3, 2), (7, 130, 3), (5, 4, 257)])
def test_producer_matches_the_numpy_passes(fs, shape):
    """(W, H, D): lines shorter than a wave, ragged, and longer than one workgroup; random masks and a box"""
    st, off, _ = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    w, h, d = shape
    rng = np.random.default_rng(w * 31 + h * 7 + d)
    masks = [np.where(rng.random((d, h, w)) < fill, rng.integers(129, 256, (d, h, w)), rng.integers(0, 129, (d, h, w))).astype(np.uint8)
             for fill in (0.5, 0.97)]
    box = np.zeros((d, h, w), dtype=np.uint8)
    box[d // 4:d - d // 4, h // 4:h - h // 4, w // 4:w - w // 4] = 255
    box[0, 0, 0] = 0
    masks.append(box)
    for k, mask in enumerate(masks):
        mask[0, 0, 0] = 0
        want = R.producer_field(mask, _size(st))
        got = sim.set_collider_mask(mask, want_field=True)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{shape} mask {k}: returned field"
        assert sim.collider().tobytes() == want.tobytes(), f"{shape} mask {k}: collider()"
        assert sim.collider_dims == (w, h, d)
    sim.close()


def test_producer_all_free_and_all_solid(fs):
    st, off, _ = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    got = sim.set_collider_mask(np.full((3, 4, 70), 128, dtype=np.uint8), want_field=True)
    assert got.shape == (3, 4, 70, 3) and not got.view(np.uint32).any(), "an all-free mask gives +0 everywhere"
    keep = _random_field((5, 3, 2), 9)
    sim.set_collider(keep)
    with pytest.raises(fs.FluidSimError) as e:
        sim.set_collider_mask(np.full((2, 2, 2), 129, dtype=np.uint8))
    assert e.value.status == fs._abi.FS_ERR_INVALID
    assert sim.collider_dims == (5, 3, 2) and sim.collider().tobytes() == keep.tobytes(), "the earlier collider stays"
    sim.close()


# ---- 6. ordering and state --------------------------------------------------------------------------------------------
def test_upload_between_unsynced_steps(fs, orc):
    """three steps, a collider, three steps, no sync in between: the first three are the plain oracle's, the last three have C"""
    st, off, tick = fs.dam_break_3d(SIDE ** 3)
    size = _size(st)
    field = R.scene_layer_through_wall(size)
    ref = orc.OracleSim3D(st, initial_offset=off)
    ref.step(tick)
    assert R.apply_collider(ref.particles(), field, size, tick.damping_factor)[1] > 0, "C would act on step 1: an early field shows"
    ref.step(tick); ref.step(tick)
    for _ in range(3):
        ref.step(tick)
        ref.set_particles(R.apply_collider(ref.particles(), field, size, tick.damping_factor)[0])
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    for _ in range(3):
        sim.tick(tick)
    sim.set_collider(field)
    for _ in range(3):
        sim.tick(tick)
    _same(sim.download_particles(), ref.particles(), "collider uploaded between un-synced steps")
    # a second, smaller and a larger upload replace the first; the steps in flight keep the field they were enqueued with
    sim.tick(tick)
    sim.set_collider(np.zeros((1, 1, 1, 3), dtype=f32))
    ref.step(tick)
    ref.set_particles(R.apply_collider(ref.particles(), field, size, tick.damping_factor)[0])
    sim.tick(tick)
    ref.step(tick)
    big = R.scene_box_on_floor(size)
    sim.set_collider(big)
    sim.tick(tick)
    ref.step(tick)
    ref.set_particles(R.apply_collider(ref.particles(), big, size, tick.damping_factor)[0])
    _same(sim.download_particles(), ref.particles(), "replaced colliders")
    sim.close(); ref.close()


def test_state_calls_and_round_trip(fs):
    st, off, tick = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    assert sim.collider() is None and sim.collider_dims == (0, 0, 0)
    sim.tick(tick)
    pts = np.array([[-0.7, 0.2, 0.0], [0.0, 0.0, 0.0]], dtype=f32)
    before = sim.sample(pts)
    field = _random_field((6, 5, 4), 2)
    sim.set_collider(field)
    assert sim.sample(pts).tobytes() == before.tobytes(), "setting a collider must not make sampling stale"
    sim.clear_collider()
    assert sim.sample(pts).tobytes() == before.tobytes(), "clearing a collider must not make sampling stale"
    sim.set_collider(field)
    assert sim.collider_dims == (6, 5, 4)
    back = sim.collider()
    assert back.shape == (4, 5, 6, 3) and back.tobytes() == field.tobytes()
    lib, h = sim._lib, sim._h
    buf = np.zeros((4 * 5 * 6, 3), dtype=f32)
    assert lib.fs3_collider_download(h, buf.ctypes.data_as(C.c_void_p), 4 * 5 * 6 - 1) == fs._abi.FS_ERR_INVALID
    sim.clear_collider()
    assert lib.fs3_collider_download(h, buf.ctypes.data_as(C.c_void_p), 4 * 5 * 6) == fs._abi.FS_ERR_INVALID
    sim.close()


# ---- 7. argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_the_headers_order(fs):
    st, off, _ = fs.dam_break_3d(SIDE ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    lib, h, INV = sim._lib, sim._h, fs._abi.FS_ERR_INVALID
    err = lambda: lib.fs_last_error().decode()
    ok = np.zeros((2, 2, 2, 3), dtype=f32)
    ok[0, 0, 0] = (0.1, 0.0, 0.0)
    bad = ok.copy()
    bad[1, 1, 1, 2] = np.nan
    okp, badp = ok.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p)
    mask = np.zeros(8, dtype=np.uint8)
    mp = mask.ctypes.data_as(C.c_void_p)
    w = C.c_uint32()
    # 1. the handle, before anything else is looked at
    assert lib.fs3_collider_upload(None, None, 0, 0, 0) == INV and "null" in err()
    assert lib.fs3_collider_from_mask(None, None, 0, 0, 0, None) == INV
    assert lib.fs3_collider_clear(None) == INV and lib.fs3_collider_download(None, okp, 8) == INV
    assert lib.fs3_collider_dims(None, C.byref(w), C.byref(w), C.byref(w)) == INV
    # 2. the array, before the extents
    assert lib.fs3_collider_upload(h, None, 0, 1025, 2) == INV and "null" in err()
    assert lib.fs3_collider_from_mask(h, None, 2, 2, 0, None) == INV and "null" in err()
    assert lib.fs3_collider_download(h, None, 8) == INV and "null" in err()
    assert lib.fs3_collider_dims(h, None, C.byref(w), C.byref(w)) == INV and "null" in err()
    # 3. the extents, before the values (a NaN is in the array)
    for dims in [(0, 2, 2), (2, 0, 2), (2, 2, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025)]:
        assert lib.fs3_collider_upload(h, badp, *dims) == INV and "extent" in err(), dims
        assert lib.fs3_collider_from_mask(h, mp, *dims, None) == INV and "extent" in err(), dims
    # 4. the values
    assert lib.fs3_collider_upload(h, badp, 2, 2, 2) == INV and "non-finite" in err()
    bad[1, 1, 1, 2] = -np.inf
    assert lib.fs3_collider_upload(h, badp, 2, 2, 2) == INV and "non-finite" in err()
    assert sim.collider_dims == (0, 0, 0), "a refused call sets nothing"
    assert lib.fs3_collider_upload(h, okp, 2, 2, 2) == fs._abi.FS_OK
    assert lib.fs3_collider_upload(h, okp, 1, 1, 1) == fs._abi.FS_OK and sim.collider_dims == (1, 1, 1)
    line = np.zeros(1024, dtype=np.uint8)
    assert lib.fs3_collider_from_mask(h, line.ctypes.data_as(C.c_void_p), 1, 1024, 1, None) == fs._abi.FS_OK      # the largest extent
    sim.close()

"""3D moving bodies without a GPU (include/fluidsim.h "3D moving bodies"): the numpy statement of the operator B
does what the header says on numbers a reader can follow, reduces to the static operator C for a body at rest over the whole
domain, commutes with a 90-degree turn of body and mask, and the shared scene meets the conditions the GPU comparison relies on.
The built library exports and binds the new calls."""
import numpy as np
import pytest

from tests import bodies3d_ref as B
from tests import collide3d_ref as CR

f32 = np.float32
REC = [("position", "<f4", (3,)), ("predicted_position", "<f4", (3,)), ("velocity", "<f4", (3,)), ("density", "<f4"),
       ("grid", "<u4"), ("pad", "<u4")]
ROT_Z90 = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)      # world = R * local: local x -> world y


def _records(pos, vel):
    rec = np.zeros(len(pos), dtype=REC)
    rec["position"] = pos
    rec["velocity"] = vel
    return rec


@pytest.mark.parametrize("side", [16, 18])
def test_scene_meets_its_conditions(fs, orc, side):
    """every body hits at step 1, something is clamped again after a push by step 8, every position stays finite"""
    run = B.oracle_run(fs, orc, side)
    hits, re = run["hits"], run["reclamped"]
    print(f"[bodies3d] side {side}: step 1 hits {hits[0].tolist()} re-clamped {re[0].tolist()}; 40 steps hits "
          f"{hits.sum(0).tolist()} re-clamped {re.sum(0).tolist()}")
    assert (hits[0] > 0).all(), "paddle, stirrer and floor slab must all hit in step 1"
    assert re[:8].sum() > 0, "a push must leave the box by step 8"
    for s, rec in run["snap"].items():
        assert np.isfinite(rec["position"]).all(), f"step {s}"
    assert B.oracle_run(fs, orc, side)["snap"][40] is run["snap"][40], "the reference is computed once"


def test_operator_by_hand():
    """a 2 x 1 x 1 field over a 2 x 2 x 2 box at (1, 0, 0) that moves with u = (3, 0, 0): numbers a reader can follow"""
    field = np.zeros((1, 1, 2, 3), dtype=f32)
    field[0, 0, 0] = (-0.5, 0.0, 0.0)                    # the body's left half pushes left
    field[0, 0, 1] = (4.0, 0.0, 0.0)                     # its right half pushes through the +x wall
    body = B.Body(field, (2.0, 2.0, 2.0), centre=(1.0, 0.0, 0.0), velocity=(3.0, 0.0, 0.0))
    rec = _records([(0.5, 0.25, 0.0), (1.5, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.5, 1.5, 0.0)],
                   [(1.0, 2.0, 0.0), (1.0, 2.0, 0.0), (1.0, 2.0, 0.0), (1.0, 2.0, 0.0)])
    out, hits, reclamped = B.apply_body(rec, body, (8.0, 8.0, 8.0), 0.25)
    assert (hits, reclamped) == (2, 1)
    # particle 0: q = (-0.5, 0.25, 0) -> voxel 0; n = (-1, 0, 0); p = (0, 0.25, 0); us = (3, 0, 0); r = (-2, 2, 0); rn = 2;
    # k = 0.75 * 2 = 1.5; v = us + (r - k n) = (3 + (-2 + 1.5), 2, 0)
    assert out["position"][0].tolist() == [0.0, 0.25, 0.0] and out["velocity"][0].tolist() == [2.5, 2.0, 0.0]
    # particle 1: voxel 1; n = (1, 0, 0); p.x = 5.5 -> clamped to 4; rn = -2; k = -1.5; v.x = 3 + (-2 + 1.5) = 2.5, then * -0.25
    assert out["position"][1].tolist() == [4.0, 0.0, 0.0] and out["velocity"][1].tolist() == [-0.625, 2.0, 0.0]
    # particles 2 and 3 are outside the box in x and in y
    assert out[2:].tobytes() == rec[2:].tobytes()


def test_spinning_body_hands_over_its_surface_velocity():
    """w = (0, 0, 2) about the centre: the surface velocity at the pushed position s is w x s"""
    field = np.full((1, 1, 1, 3), 0.0, dtype=f32)
    field[0, 0, 0] = (0.0, 0.5, 0.0)
    body = B.Body(field, (2.0, 2.0, 2.0), angular_velocity=(0.0, 0.0, 2.0))
    rec = _records([(0.5, 0.0, 0.0)], [(0.0, 0.0, 0.0)])
    out, hits, _ = B.apply_body(rec, body, (8.0, 8.0, 8.0), 1.0)       # damping 1: k = 0, v = us + r = v ... exactly the old v
    assert hits == 1 and out["position"][0].tolist() == [0.5, 0.5, 0.0] and out["velocity"][0].tolist() == [0.0, 0.0, 0.0]
    out, _, _ = B.apply_body(rec, body, (8.0, 8.0, 8.0), 0.0)          # damping 0: the normal part becomes the surface's
    # s = (0.5, 0.5, 0); us = w x s = (-1, 1, 0); r = (1, -1, 0); n = (0, 1, 0); rn = -1; k = -1; v = us + (r - k n) = (0, 1, 0)
    assert out["velocity"][0].tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("seed", [1, 2])
def test_body_at_rest_over_the_domain_is_the_static_collider(seed):
    """identity pose at the origin, the domain as the box, a §18 field: equal as numbers to apply_collider on finite clamped positions"""
    size = (3.2, 2.0, 1.8)
    rng = np.random.default_rng(seed)
    field = CR.random_field((7, 5, 3), seed, fill=0.6, mag=0.4)
    b = np.array(size, dtype=f32) * f32(0.5)
    pos = rng.uniform(-1.0, 1.0, size=(4000, 3)).astype(f32) * b
    pos[:30] = np.sign(pos[:30]) * b                                   # corners and faces of the domain
    rec = _records(pos, rng.uniform(-3, 3, size=(4000, 3)).astype(f32))
    want, pushed, reclamped = CR.apply_collider(rec, field, size, 0.3)
    got, hits, re = B.apply_body(rec, B.Body(field, size), size, 0.3)
    assert pushed > 0 and reclamped > 0 and (hits, re) == (pushed, reclamped)
    assert np.array_equal(got["position"], want["position"]) and np.array_equal(got["velocity"], want["velocity"])


def test_quarter_turn_of_body_and_mask_gives_the_turned_answer():
    """R = 90 degrees about z (entries 0 and +-1) with the mask's x and y axes swapped accordingly: the answer is the unturned one
    with (x, y) -> (-y, x), exactly"""
    rng = np.random.default_rng(5)
    mask = np.where(rng.random((3, 4, 6)) < 0.6, 255, 0).astype(np.uint8)
    mask[0, 0, 0] = 0
    extent = (1.2, 0.8, 0.9)
    field = CR.producer_field(mask, extent)
    size = (4.0, 4.0, 4.0)
    pos = rng.uniform(-0.7, 0.7, size=(3000, 3)).astype(f32)
    vel = rng.uniform(-2, 2, size=(3000, 3)).astype(f32)
    plain, hits, _ = B.apply_body(_records(pos, vel), B.Body(field, extent, velocity=(0.5, -0.25, 0.0)), size, 0.3)
    turn = lambda a: np.stack([-a[:, 1], a[:, 0], a[:, 2]], axis=1)    # noqa: E731
    body = B.Body(field, extent, rot=ROT_Z90, velocity=(0.25, 0.5, 0.0))
    turned, hits_t, _ = B.apply_body(_records(turn(pos), turn(vel)), body, size, 0.3)
    assert hits > 100 and hits_t == hits
    assert np.array_equal(turned["position"], turn(plain["position"])) and np.array_equal(turned["velocity"], turn(plain["velocity"]))


def test_face_is_inside_and_nan_is_untouched():
    field = np.full((1, 1, 1, 3), 0.0, dtype=f32)
    field[0, 0, 0] = (0.0, 0.0, 0.125)
    body = B.Body(field, (1.0, 0.5, 0.25), centre=(0.0, 0.0, 0.0))
    eps = np.nextafter(f32(0.5), f32(1.0))
    rec = _records([(0.5, 0.25, 0.125), (-0.5, -0.25, -0.125), (eps, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.nan)],
                   [(0.0, 0.0, 0.0)] * 6)
    out, hits, _ = B.apply_body(rec, body, (8.0, 8.0, 8.0), 0.5)
    assert hits == 2
    assert out["position"][0].tolist() == [0.5, 0.25, 0.25] and out["position"][1].tolist() == [-0.5, -0.25, 0.0]
    assert out[2:].tobytes() == rec[2:].tobytes(), "just outside a face, and NaN in any coordinate: unchanged in every bit"


def test_translating_wall_hits_a_resting_particle():
    """a wall moving with u along its normal n hits a particle at rest: it leaves with u_n * (1 - damping) along n; with a velocity
    of its own, that velocity's normal part comes back damped on top"""
    field = np.full((1, 1, 1, 3), 0.0, dtype=f32)
    field[0, 0, 0] = (0.25, 0.0, 0.0)
    body = B.Body(field, (1.0, 1.0, 1.0), velocity=(2.0, 0.0, 0.0))
    d = f32(0.25)
    out, _, _ = B.apply_body(_records([(0.0, 0.0, 0.0)], [(0.0, 0.0, 0.0)]), body, (8.0, 8.0, 8.0), d)
    assert out["velocity"][0].tolist() == [float(f32(2.0) * (f32(1.0) - d)), 0.0, 0.0]
    # v = (-1, 3, 0): r = (-3, 3, 0), rn = -3, k = 0.75 * -3, v.x = 2 + (-3 + 2.25) = 1.25 = u_n (1 - d) + d * v_n; tangential kept
    out, _, _ = B.apply_body(_records([(0.0, 0.0, 0.0)], [(-1.0, 3.0, 0.0)]), body, (8.0, 8.0, 8.0), d)
    assert out["velocity"][0].tolist() == [1.25, 3.0, 0.0]


def test_rigid_motion_helper(fs):
    c, r = fs.rigid_motion((1.0, 2.0, 3.0), (0.5, 0.0, -1.0), (0, 0, 2.0), np.pi / 2, 1.0)
    assert c.dtype == np.float32 and r.dtype == np.float32 and r.shape == (9,)
    assert c.tolist() == [1.5, 2.0, 2.0]
    assert np.allclose(r.reshape(3, 3), np.array(ROT_Z90).reshape(3, 3), atol=1e-7)
    c, r = fs.rigid_motion((0, 0, 0), (0, 0, 0), (1, 0, 0), 0.0, 5.0)
    assert r.tolist() == list(B.IDENTITY)


def test_library_exports_and_binds_the_body_calls(fs):
    lib = fs.load_library()
    names = ["fs3_body_create", "fs3_body_create_from_mask", "fs3_body_set_motion", "fs3_body_get_motion", "fs3_body_dims",
             "fs3_body_download", "fs3_body_destroy", "fs3_body_count"]
    for n in names:
        assert hasattr(lib, n), f"libfluidsim_hip.so does not export {n}"
        assert n in fs._abi.PROTOTYPES
    for m in ("add_body", "add_body_mask", "set_body_motion", "body_motion", "body_dims", "body_field", "remove_body"):
        assert callable(getattr(fs.FluidSimulation3D, m))
    import ctypes as C
    assert C.sizeof(fs.BodyMotion3) == 72
    # the NULL-handle check comes first and needs no device
    INV = fs._abi.FS_ERR_INVALID
    assert lib.fs3_body_destroy(None, 0) == INV and lib.fs3_body_set_motion(None, 0, None) == INV
    assert lib.fs3_body_create(None, None, 0, 0, 0, fs.Vec3(0, 0, 0), None) == INV
    assert lib.fs3_body_count(None) == 0
    assert lib.fs_abi_version() == 2

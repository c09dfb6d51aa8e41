"""2D moving bodies without a GPU (include/fluidsim.h "2D moving bodies"): the numpy statement of the operator B
does what the header says on numbers a reader can follow, takes world-unit vectors, commutes with a quarter turn of body and
mask, and the shared scene meets the conditions the GPU comparison relies on.  The built library exports and binds the new calls."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies2d_ref as B
from tests.layers import assert_every_layer_names

f32 = np.float32
ROT_90 = (0.0, -1.0, 1.0, 0.0)      # world = R * local: local x -> world y
NAMES = ["fs_body_create", "fs_body_create_from_mask", "fs_body_set_motion", "fs_body_get_motion", "fs_body_dims",
         "fs_body_download", "fs_body_destroy", "fs_body_count"]
METHODS = ["add_body", "add_body_mask", "set_body_motion", "body_motion", "body_dims", "body_field", "remove_body", "body_count"]


def _records(fs, pos, vel):
    rec = np.zeros(len(pos), dtype=fs.PARTICLE_DTYPE)
    rec["position"] = pos
    rec["velocity"] = vel
    return rec


@pytest.mark.parametrize("side", [64, 66])
def test_scene_meets_its_conditions(fs, orc, side):
    """every body hits at step 1, something is clamped again after a push by step 8, every position stays finite"""
    run = B.oracle_run(fs, orc, side)
    hits, re = run["hits"], run["reclamped"]
    print(f"[bodies2d] side {side}: step 1 hits {hits[0].tolist()} re-clamped {re[0].tolist()}; 40 steps hits "
          f"{hits.sum(0).tolist()} re-clamped {re.sum(0).tolist()}")
    assert (hits[0] > 0).all(), "paddle, stirrer and slab must all hit in step 1"
    assert re[:8].sum() > 0, "a push must leave the box by step 8"
    assert re[:, 0].sum() > 0, "the paddle must reach the -x wall and push particles through it within the 40 steps"
    for s, rec in run["snap"].items():
        assert np.isfinite(rec["position"]).all(), f"step {s}"
    assert B.oracle_run(fs, orc, side)["snap"][40] is run["snap"][40], "the reference is computed once"


def test_operator_by_hand(fs):
    """a 2 x 1 field over a 2 x 2 box at (1, 0) that moves with u = (3, 0): numbers a reader can follow"""
    field = np.zeros((1, 2, 2), dtype=f32)
    field[0, 0] = (-0.5, 0.0)                      # the body's left half pushes left
    field[0, 1] = (4.0, 0.0)                       # its right half pushes through the +x wall
    body = B.Body(field, (2.0, 2.0), centre=(1.0, 0.0), velocity=(3.0, 0.0))
    rec = _records(fs, [(0.5, 0.25), (1.5, 0.0), (-0.5, 0.0), (0.5, 1.5)], [(1.0, 2.0)] * 4)
    out, hits, reclamped = B.apply_body(rec, body, (8.0, 8.0), 0.25)
    assert (hits, reclamped) == (2, 1)
    # particle 0: q = (-0.5, 0.25) -> pixel 0; n = (-1, 0); p = (0, 0.25); us = (3, 0); r = (-2, 2); rn = 2;
    # k = 0.75 * 2 = 1.5; v = us + (r - k n) = (3 + (-2 + 1.5), 2)
    assert out["position"][0].tolist() == [0.0, 0.25] and out["velocity"][0].tolist() == [2.5, 2.0]
    # particle 1: pixel 1; n = (1, 0); p.x = 5.5 -> clamped to 4; rn = -2; k = -1.5; v.x = 3 + (-2 + 1.5) = 2.5, then * -0.25
    assert out["position"][1].tolist() == [4.0, 0.0] and out["velocity"][1].tolist() == [-0.625, 2.0]
    # particles 2 and 3 are outside the box in x and in y
    assert out[2:].tobytes() == rec[2:].tobytes()


def test_spinning_body_hands_over_its_surface_velocity(fs):
    """w = 2 about the centre: the surface velocity at the pushed position s is w x s = (-w s.y, w s.x)"""
    field = np.zeros((1, 1, 2), dtype=f32)
    field[0, 0] = (0.0, 0.5)
    body = B.Body(field, (2.0, 2.0), angular_velocity=2.0)
    rec = _records(fs, [(0.5, 0.0)], [(0.0, 0.0)])
    out, hits, _ = B.apply_body(rec, body, (8.0, 8.0), 1.0)       # damping 1: k = 0, v = us + r: exactly the old v
    assert hits == 1 and out["position"][0].tolist() == [0.5, 0.5] and out["velocity"][0].tolist() == [0.0, 0.0]
    out, _, _ = B.apply_body(rec, body, (8.0, 8.0), 0.0)          # damping 0: the normal part becomes the surface's
    # s = (0.5, 0.5); us = (-1, 1); r = (1, -1); n = (0, 1); rn = -1; k = -1; v = us + (r - k n) = (0, 1)
    assert out["velocity"][0].tolist() == [0.0, 1.0]


def test_body_at_rest_over_the_domain_takes_world_unit_vectors(fs):
    """identity pose at the origin, the domain as the box: a particle moves by the vector itself, in world units — not by the
    vector times bounds * 2 / texture_size, the pixel scale of the force texture — and loses (1 - damping) of its normal velocity"""
    size = (12.8, 8.0)
    field = np.zeros((4, 8, 2), dtype=f32)
    field[1, 2] = (0.25, 0.0)                      # pixel (2, 1): x in [-3.2, -1.6), y in [-2, 0)
    body = B.Body(field, size)
    rec = _records(fs, [(-2.0, -1.0), (-2.0, 1.0), (-1.5, -1.0)], [(4.0, 1.0)] * 3)
    out, hits, _ = B.apply_body(rec, body, size, 0.5)
    assert hits == 1
    assert out["position"][0].tolist() == [-1.75, -1.0] and out["velocity"][0].tolist() == [2.0, 1.0]
    assert out[1:].tobytes() == rec[1:].tobytes(), "the pixel below, and the pixel to the right"
    # the same as a random field with many hits: every hit particle moved by exactly its pixel's vector
    rng = np.random.default_rng(3)
    field = B.random_field((7, 5), 3, fill=0.6, mag=0.4)
    b = np.array(size, dtype=f32) * f32(0.5)
    pos = (rng.uniform(-0.9, 0.9, size=(4000, 2)).astype(f32) * b).astype(f32)
    rec = _records(fs, pos, rng.uniform(-3, 3, size=(4000, 2)).astype(f32))
    out, hits, re = B.apply_body(rec, B.Body(field, size), size, 0.3)
    ix = np.minimum(((pos[:, 0] + b[0]) / f32(size[0]) * f32(7)).astype(np.int64), 6)
    iy = np.minimum(((pos[:, 1] + b[1]) / f32(size[1]) * f32(5)).astype(np.int64), 4)
    moved = out["position"] != rec["position"]
    assert hits > 1000 and re == 0 and moved.any(axis=1).sum() == hits
    assert np.array_equal(out["position"], pos + field[iy, ix])


def test_quarter_turn_of_body_and_mask_gives_the_turned_answer(fs):
    """R = a quarter turn (entries 0 and +-1): the answer is the unturned one with (x, y) -> (-y, x), exactly"""
    rng = np.random.default_rng(5)
    mask = np.where(rng.random((4, 6)) < 0.6, 255, 0).astype(np.uint8)
    mask[0, 0] = 0
    extent = (1.2, 0.8)
    field = B.producer_field(mask, extent)
    size = (4.0, 4.0)
    pos = rng.uniform(-0.7, 0.7, size=(3000, 2)).astype(f32)
    vel = rng.uniform(-2, 2, size=(3000, 2)).astype(f32)
    plain, hits, _ = B.apply_body(_records(fs, pos, vel), B.Body(field, extent, velocity=(0.5, -0.25), angular_velocity=1.5), size, 0.3)
    turn = lambda a: np.stack([-a[:, 1], a[:, 0]], axis=1)    # noqa: E731
    body = B.Body(field, extent, rot=ROT_90, velocity=(0.25, 0.5), angular_velocity=1.5)
    turned, hits_t, _ = B.apply_body(_records(fs, turn(pos), turn(vel)), body, size, 0.3)
    assert hits > 100 and hits_t == hits
    assert np.array_equal(turned["position"], turn(plain["position"])) and np.array_equal(turned["velocity"], turn(plain["velocity"]))


def test_edge_is_inside_and_nan_is_untouched(fs):
    field = np.zeros((1, 1, 2), dtype=f32)
    field[0, 0] = (0.0, 0.125)
    body = B.Body(field, (1.0, 0.5))
    eps = np.nextafter(f32(0.5), f32(1.0))
    rec = _records(fs, [(0.5, 0.25), (-0.5, -0.25), (eps, 0.0), (np.nan, 0.0), (0.0, np.nan)], [(0.0, 0.0)] * 5)
    out, hits, _ = B.apply_body(rec, body, (8.0, 8.0), 0.5)
    assert hits == 2
    assert out["position"][0].tolist() == [0.5, 0.375] and out["position"][1].tolist() == [-0.5, -0.125]
    assert out[2:].tobytes() == rec[2:].tobytes(), "just outside an edge, and NaN in either coordinate: unchanged in every bit"


def test_moving_wall_hits_a_resting_particle(fs):
    """a wall moving with u along its normal n hits a particle at rest: it leaves with u_n * (1 - damping) along n; with a velocity
    of its own, that velocity's normal part comes back damped on top"""
    field = np.zeros((1, 1, 2), dtype=f32)
    field[0, 0] = (0.25, 0.0)
    body = B.Body(field, (1.0, 1.0), velocity=(2.0, 0.0))
    d = f32(0.25)
    out, _, _ = B.apply_body(_records(fs, [(0.0, 0.0)], [(0.0, 0.0)]), body, (8.0, 8.0), d)
    assert out["velocity"][0].tolist() == [float(f32(2.0) * (f32(1.0) - d)), 0.0]
    # v = (-1, 3): r = (-3, 3), rn = -3, k = 0.75 * -3, v.x = 2 + (-3 + 2.25) = 1.25 = u_n (1 - d) + d * v_n; tangential kept
    out, _, _ = B.apply_body(_records(fs, [(0.0, 0.0)], [(-1.0, 3.0)]), body, (8.0, 8.0), d)
    assert out["velocity"][0].tolist() == [1.25, 3.0]


def test_rigid_motion2d_helper(fs):
    c, r = fs.rigid_motion2d((1.0, 2.0), (0.5, -1.0), np.pi / 2, 1.0)
    assert c.dtype == np.float32 and r.dtype == np.float32 and r.shape == (4,)
    assert c.tolist() == [1.5, 1.0]
    assert np.allclose(r, np.array(ROT_90), atol=1e-7)
    c, r = fs.rigid_motion2d((0, 0), (0, 0), 0.0, 5.0)
    assert r.tolist() == list(B.IDENTITY)
    c, r = fs.rigid_motion2d((0, 0), (2.0, 0), 0.25, 2.0)
    want = np.array([np.cos(0.5), -np.sin(0.5), np.sin(0.5), np.cos(0.5)]).astype(np.float32)
    assert r.tobytes() == want.tobytes() and c.tolist() == [4.0, 0.0], "float64, cast to float32 once"


def test_library_exports_and_binds_the_body_calls(fs):
    assert_every_layer_names(fs, NAMES, fs.FluidSimulation, METHODS)
    lib = fs.load_library()
    assert C.sizeof(fs.BodyMotion) == 36 and fs._abi.FS_MAX_BODIES == 8
    assert callable(fs.rigid_motion2d)
    # the NULL-handle check comes first and needs no device
    INV = fs._abi.FS_ERR_INVALID
    assert lib.fs_body_destroy(None, 0) == INV and lib.fs_body_set_motion(None, 0, None) == INV
    assert lib.fs_body_create(None, None, 0, 0, fs.Vec2(0, 0), None) == INV
    assert lib.fs_body_create_from_mask(None, None, 0, 0, fs.Vec2(0, 0), None, None) == INV
    assert lib.fs_body_count(None) == 0

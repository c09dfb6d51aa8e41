"""3D colliders without a GPU (include/fluidsim.h "3D colliders"): the numpy statement of the producer reaches the
true nearest free voxel, free voxels stay exactly +0, ties go where the header says, the operator's reference meets the conditions
the GPU comparison relies on, and the built library exports and binds the new calls."""
import numpy as np
import pytest

from tests import collide3d_ref as R
from tests import features3d as F

f32 = np.float32
SIZE = (3.2, 2.0, 1.8)


@pytest.mark.parametrize("shape,seed,fill", [((12, 12, 12), 1, 0.5), ((12, 12, 12), 2, 0.9), ((5, 12, 7), 3, 0.7), ((1, 1, 9), 4, 0.6),
                                             ((3, 1, 4), 5, 0.97), ((12, 9, 1), 6, 0.8)])
def test_producer_reaches_the_true_nearest_free_voxel(shape, seed, fill):
    rng = np.random.default_rng(seed)
    mask = np.where(rng.random(shape) < fill, 255, 0).astype(np.uint8)
    mask.reshape(-1)[rng.integers(mask.size)] = 0                   # at least one free voxel
    c, d2 = R.producer_passes(mask)
    assert np.array_equal(d2, R.brute_nearest_d2(mask))
    # the voxel it names is free and at that distance
    assert not (mask[c[..., 2], c[..., 1], c[..., 0]] > 128).any()
    own = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")[::-1], axis=-1)
    assert np.array_equal(((c - own) ** 2).sum(-1), d2)


def test_threshold_and_free_voxels_are_exactly_plus_zero():
    rng = np.random.default_rng(7)
    mask = rng.integers(0, 256, size=(6, 5, 9)).astype(np.uint8)
    mask[0, 0, :3] = (127, 128, 129)                                 # > 128 is solid: 128 is free
    field = R.producer_field(mask, SIZE)
    free = ~(mask > 128)
    assert free[0, 0, 1] and not free[0, 0, 2]
    assert not field[free].view(np.uint32).any(), "a free voxel's vector must be +0 in every bit"
    assert (np.abs(field[~free]).sum(-1) > 0).all(), "a solid voxel is pushed somewhere"


def test_tie_rules_on_a_symmetric_mask():
    # one solid voxel in the middle of 3 x 3 x 3: six free neighbours at distance 1.  X offers i' = 0 (ties to the smaller i'), Y
    # prefers j' = 0 (the row's own free voxel, distance 1, the smaller j'), Z prefers k' = 0: the answer is (1, 1, 0)
    mask = np.zeros((3, 3, 3), dtype=np.uint8)
    mask[1, 1, 1] = 255
    c, d2 = R.producer_passes(mask)
    assert tuple(c[1, 1, 1]) == (1, 1, 0) and d2[1, 1, 1] == 1
    field = R.producer_field(mask, (3.0, 6.0, 1.5))
    assert field[1, 1, 1].tolist() == [0.0, 0.0, -0.5]
    # a solid row between two free ends: the middle goes to the smaller index
    row = np.array([[[0, 255, 255, 255, 0]]], dtype=np.uint8)
    c, _ = R.producer_passes(row)
    assert c[0, 0, :, 0].tolist() == [0, 0, 0, 4, 4]
    # a mask without a free voxel has no answer
    c, _ = R.producer_passes(np.full((2, 2, 2), 200, dtype=np.uint8))
    assert (c == R.NONE).all()


def test_operator_reference_by_hand():
    """one particle, numbers a reader can follow: lookup, push, reflection of the normal velocity, second clamp"""
    rec = np.zeros(3, dtype=[("position", "<f4", (3,)), ("predicted_position", "<f4", (3,)), ("velocity", "<f4", (3,)),
                             ("density", "<f4"), ("grid", "<u4"), ("pad", "<u4")])
    rec["position"] = [(-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (np.nan, 1.0, -1.0)]
    rec["velocity"] = [(2.0, 1.0, 0.0), (2.0, 1.0, 0.0), (1.0, 1.0, 1.0)]
    field = np.zeros((1, 1, 2, 3), dtype=f32)
    field[0, 0, 0] = (0.5, 0.0, 0.0)                                 # the left half pushes right
    field[0, 0, 1] = (1.5, 0.0, 0.0)                                 # the right half pushes through the +x wall
    out, pushed, reclamped = R.apply_collider(rec, field, (4.0, 4.0, 4.0), 0.25)
    assert (pushed, reclamped) == (3, 1)                             # the NaN coordinate looks up voxel 0 and is pushed, not clamped
    assert out["position"][0].tolist() == [-0.5, 0.0, 0.0] and out["velocity"][0].tolist() == [0.5, 1.0, 0.0]
    assert out["position"][1].tolist() == [2.0, 0.0, 0.0] and out["velocity"][1].tolist() == [-0.125, 1.0, 0.0]
    tiny = np.full((1, 1, 1, 3), 1e-30, dtype=f32)                   # squares underflow: free space
    out, pushed, _ = R.apply_collider(rec, tiny, (4.0, 4.0, 4.0), 0.25)
    assert pushed == 0 and out.tobytes() == rec.tobytes()


@pytest.mark.parametrize("side", [16, 18])
def test_oracle_scenes_meet_their_conditions(fs, orc, side):
    """what the GPU comparison asserts about its scenes holds on the CPU alone: the dam reaches the box of scene (a), and the layer
    of scene (b) pushes particles through the wall"""
    a = R.oracle_run(fs, orc, side, "a")
    b = R.oracle_run(fs, orc, side, "b")
    print(f"[collide3d] side {side}: scene a pushed {a['pushed']} re-clamped {a['reclamped']}; scene b pushed {b['pushed']} "
          f"re-clamped {b['reclamped']}")
    assert a["pushed"] > 0
    assert b["reclamped"] > 0
    plain = R.oracle_run(fs, orc, side, "a")["snap"][40]
    assert plain is a["snap"][40], "the reference is computed once"


def test_library_exports_and_binds_the_collider_calls(fs):
    lib = fs.load_library()
    names = ["fs3_collider_upload", "fs3_collider_from_mask", "fs3_collider_clear", "fs3_collider_dims", "fs3_collider_download"]
    for n in names:
        assert hasattr(lib, n), f"libfluidsim_hip.so does not export {n}"
        assert n in fs._abi.PROTOTYPES
    for m in ("set_collider", "set_collider_mask", "clear_collider", "collider"):
        assert callable(getattr(fs.FluidSimulation3D, m))
    # the NULL-handle check comes first and needs no device
    assert lib.fs3_collider_clear(None) == fs._abi.FS_ERR_INVALID
    assert lib.fs3_collider_upload(None, None, 0, 0, 0) == fs._abi.FS_ERR_INVALID
    assert lib.fs_abi_version() == 2


# ---- the hard-input cases of test_3d_features_hard_inputs_gpu.py, on the checker alone -------------------------------------
COLLIDER_IDS = [c for c in F.CASE_IDS if c.endswith("+collide") or c.split("/")[0] in ("random", "edge")]


@pytest.mark.parametrize("cid", COLLIDER_IDS)
def test_hard_input_cases_push_and_reclamp(fs, orc, cid):
    """what the GPU file relies on, asked of the checker alone: every case with a collider pushes particles, the block driven into
    a + wall is clamped again after its push, thin and one-cell boxes run with a one-voxel field as well, and the tolerance-mode
    case leaves out at most 1 % of its particles"""
    case = F.case_by_id(fs, orc, cid)
    case.run()
    print(F.describe(case))
    fig = case.figures
    assert case.field is not None and case.field.any() and np.isfinite(case.field).all()
    assert fig["pushed"] > 0
    if cid.startswith("edge/wall/") and cid.endswith("+"):
        assert fig["reclamped"] > 0
    if cid.endswith("one_voxel"):
        assert case.field.shape == (1, 1, 1, 3)
    elif not cid.startswith("tol/"):
        assert case.field.shape[:3] == F.FIELD_SHAPE[::-1]
    if cid.startswith("tol/"):
        assert fig["left_out"] <= 0.01 * fig["n"]


def test_thin_boxes_have_both_fields():
    thin = [c for c in F.EDGE_CASES if c.startswith("thin/")]
    assert len(thin) == 10 and sum(c.endswith("one_voxel") for c in thin) == 5


def test_positions_on_plus_b_reach_the_last_voxel_only_through_the_clamp(fs, orc):
    """in step 1 some particle stands exactly on +b of every axis before C: its quotient is exactly 1, the unclamped index is the
    extent itself, and the voxel the clamp selects pushes"""
    case = F.guard_case(fs, orc, "positions_on_plus_b", "st+collide")
    chk = case.checker()
    _, pre, pushed, _, _ = case.checker_step(chk)
    chk.close()
    D, H, W = case.field.shape[:3]
    assert case.field[-1].any(-1).all() and case.field[:, -1].any(-1).all() and case.field[:, :, -1].any(-1).all()
    hit = 0
    for a, wa in enumerate((W, H, D)):
        size = f32(case.size[a])
        b = size * f32(0.5)
        on = pre["position"][:, a] == b
        assert on.any(), f"no particle on +b of axis {a}"
        x = ((pre["position"][on, a] + b) / size) * f32(wa)
        assert (R.u32_sat(x) == wa).all(), "the quotient of a particle on +b must be exactly the extent"
        lo = pre["position"][:, a] == -b
        assert lo.any() and (R.u32_sat(((pre["position"][lo, a] + b) / size) * f32(wa)) == 0).all()
        hit += int(on.sum())
    assert pushed >= hit > 0

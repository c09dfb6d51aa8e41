"""CPU companions of tests/test_emit3d_gpu.py (a 3D particle count that changes at run time): the checker of
tests/emit3d_ref.py alone.  The hard places of an emission do what they say, the numpy restatement of the nozzle agrees with a
float64 evaluation, and removing records from a sorted state leaves it sorted.  No GPU."""
import numpy as np
import pytest

from tests import emit3d_ref as ER

f32 = np.float32


def emitted_case(fs, name):
    """-> (checker one step after the emission, the emitted records, the state they met, tick, settings)"""
    chk, tick, st, off = ER.hard_scene(fs, name)
    chk.step(tick)
    before = chk.rec.copy()
    rec = ER.hard_records(name, before, st)
    chk.emit(rec)
    chk.step(tick)
    return chk, rec, before, tick, st


def half_box(st):
    return f32([st.size.x, st.size.y, st.size.z]) * f32(0.5)


def test_coincident_emission_is_a_pair_at_distance_zero(fs):
    chk, rec, before, tick, st = emitted_case(fs, "coincident")
    k = before.shape[0] // 2
    assert rec["position"].tobytes() == before["position"][k].tobytes() and rec["velocity"].tobytes() == before["velocity"][k].tobytes()
    pred = chk.rec["predicted_position"]
    _, inverse, counts = np.unique(pred, axis=0, return_inverse=True, return_counts=True)
    assert (counts == 2).sum() == 1 and counts.max() == 2, "exactly one pair shares its predicted position: dst == 0"
    # the pair took the PRNG direction: the two particles, identical before the step, now move apart
    twin = np.flatnonzero(inverse.ravel() == np.argmax(counts))
    assert twin.shape[0] == 2
    assert chk.rec["velocity"][twin[0]].tobytes() != chk.rec["velocity"][twin[1]].tobytes()
    assert chk.ticks == 2
    chk.close()


def test_the_tick_alignment_decides_the_coincident_pair(fs):
    """The same state stepped on an oracle whose tick counter was not advanced differs: the alignment is not vacuous."""
    from oracle import oracle as O
    chk, tick, st, off = ER.jittered_scene(fs, 12 ** 3)
    chk.step(tick)
    chk.emit(ER.hard_records("coincident", chk.rec, st))
    start = chk.rec.copy()
    aligned = chk.step(tick)
    fresh = O.OracleSim3D(chk.settings(start.shape[0]), off)
    fresh.set_particles(start)
    fresh.step(tick)
    assert fresh.particles()["velocity"].tobytes() != aligned["velocity"].tobytes()
    fresh.close(); chk.close()


def test_emission_outside_the_box_takes_the_clamp(fs):
    chk, rec, before, tick, st = emitted_case(fs, "outside")
    half = half_box(st)
    assert all(abs(rec["position"][a, a]) > half[a] for a in range(3))
    pred = chk.rec["predicted_position"]
    for a, sign in enumerate((1.0, -1.0, 1.0)):
        on_wall = (pred[:, a] == f32(sign) * half[a])
        assert on_wall.sum() >= 1, f"axis {a}: no predicted position on the wall"
    assert (np.abs(chk.rec["position"]) <= half[None, :]).all()
    chk.close()


def test_emission_on_plus_b_is_on_the_wall(fs):
    chk, rec, before, tick, st = emitted_case(fs, "on_plus_b")
    half = half_box(st)
    assert rec["position"][0].tobytes() == half.tobytes()
    gw, gh, gd = chk.grid_dims
    c = np.floor((half + half) / f32(st.smoothing_radius)).astype(np.uint32) + 1
    assert (c < np.array([gw, gh, gd])).all(), "the cell of +b lies inside the grid"
    chk.close()


def test_emission_with_a_nan_velocity_meets_the_nan_reset(fs):
    chk, rec, before, tick, st = emitted_case(fs, "nan_velocity")
    assert np.isnan(rec["velocity"]).sum() == 1
    assert np.isnan(chk.rec["predicted_position"]).any(), "the NaN reached the predicted position of the step"
    assert np.isfinite(chk.rec["velocity"]).all(), "and the step's NaN reset cleared the velocity"
    chk.close()


def test_emission_into_the_extreme_cells_is_alone_there(fs):
    chk, rec, before, tick, st = emitted_case(fs, "extreme_cells")
    # in the first step after the emission (the block's own particles spread into both corners' cells within a few steps)
    grid = chk.rec["grid"]
    assert (np.diff(grid.astype(np.int64)) >= 0).all()
    assert grid[-1] > grid[-2] and grid[0] < grid[1], "alone in the highest and in the lowest occupied cell"
    assert grid[-1] > before["grid"].max() and grid[0] < before["grid"].min()
    half = half_box(st)
    assert np.allclose(chk.rec["position"][-1], half - f32(0.01), atol=2e-3) and np.allclose(chk.rec["position"][0], -half + f32(0.01), atol=2e-3)
    chk.close()


@pytest.mark.parametrize("nu,nv", [(1, 1), (3, 5), (17, 16), (64, 64)])
def test_nozzle_restatement_agrees_with_float64(nu, nv):
    args = dict(origin=(0.13, -0.21, 0.07), u=(0.045, 0.004, -0.002), v=(-0.003, 0.002, 0.026))
    rec = ER.nozzle_records(velocity=(0.5, 2.0, -0.25), nu=nu, nv=nv, **args)
    want = ER.nozzle_positions_f64(nu=nu, nv=nv, **args)
    got = rec["position"].astype(np.float64)
    # 2 ulp of the largest magnitude the sum passes through (the two products, the partial sum and the result)
    sa = np.abs((np.arange(nu * nv) % nu + 0.5) - 0.5 * nu)[:, None]
    sb = np.abs((np.arange(nu * nv) // nu + 0.5) - 0.5 * nv)[:, None]
    scale = np.abs(f32(args["origin"]).astype(np.float64))[None, :] + sa * np.abs(f32(args["u"]).astype(np.float64))[None, :] \
        + sb * np.abs(f32(args["v"]).astype(np.float64))[None, :]
    ulp = np.spacing(scale.astype(f32)).astype(np.float64)
    assert (np.abs(got - want) <= 2.0 * ulp).all(), float((np.abs(got - want) / ulp).max())
    assert rec["predicted_position"].tobytes() == rec["position"].tobytes()
    assert (rec["velocity"] == f32([0.5, 2.0, -0.25])).all() and not rec["density"].any() and not rec["grid"].any()
    assert not np.signbit(rec["density"]).any()


def test_removal_leaves_a_sorted_state_sorted(fs):
    chk, tick, st, off = ER.jittered_scene(fs, 12 ** 3)
    chk.step(tick)
    kill = np.random.default_rng(2).random(chk.n) < 0.4
    ids = np.arange(chk.n)[~kill]
    before = chk.rec.copy()
    assert chk.remove(kill) == int(kill.sum())
    assert (np.diff(chk.rec["grid"].astype(np.int64)) >= 0).all()
    assert chk.rec.tobytes() == before[ids].tobytes(), "survivors keep their relative order"
    chk.close()


def test_box_edges_are_inclusive_and_nan_is_kept():
    rec = np.zeros(4, dtype=ER.DTYPE)
    rec["position"] = f32([[0, 0, 0], [1, 1, 1], [0.5, np.nan, 0.5], [1, 1, np.nextafter(f32(1), f32(2))]])
    assert ER.kill_box(rec, (0, 0, 0), (1, 1, 1)).tolist() == [True, True, False, False]

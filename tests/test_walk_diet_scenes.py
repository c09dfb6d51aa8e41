"""CPU-side proof that the scenes of tests/walk_diet_scenes.py are what they are named: numpy on the ORACLE's first step (its
sorted keys and predicted positions).  tests/test_walk_diet_gpu.py runs the same scenes on the engine.  No GPU."""
import numpy as np
import pytest

from tests import walk_diet_scenes as W

f32 = np.float32


def first_step(name):
    states, grid = W.oracle_states(name)
    rec = states[0][0]
    return rec["grid"], rec["predicted_position"], grid


def in_radius_counts(pred, h):
    """per particle, the candidates the scan admits: !(r2 > sqr_radius), the particle itself left out"""
    lim = f32(h) * f32(h)
    return (~(W.pair_r2(pred) > lim)).sum(axis=1)


@pytest.mark.parametrize("kind", ["pow2", "default"])
def test_rim_lattice_has_pairs_on_the_rim(orc, kind):
    st, ticks, p = W.rim(kind)
    keys, pred, grid = first_step(f"rim_{kind}")
    assert p.shape[0] <= 4096 and ticks[0].gravity.x == 0.0 and ticks[0].gravity.y == 0.0
    words = lambda a: np.sort(np.ascontiguousarray(a, dtype=f32).view(np.uint64).ravel())
    assert np.array_equal(words(pred), words(p["position"]))                    # at rest: the step sees the lattice
    h = f32(st.smoothing_radius)
    lim = h * h                                             # sqr_radius as the host forms it
    r2 = W.pair_r2(pred)
    on_rim = int((r2 == lim).sum())
    above = int((r2 == np.nextafter(lim, f32(np.inf))).sum())
    assert on_rim >= 256, on_rim
    if kind == "pow2":
        # every spacing exact: each axis neighbour ON the rim, nothing else admitted
        assert on_rim == 4 * W.RIM_SIDE * (W.RIM_SIDE - 1) == int((~(r2 > lim)).sum())
    else:
        assert above >= 256, above                          # ... and pairs the scan must refuse by one ulp
    # diagonals fall outside: what is admitted is an axis neighbour, within a few ulp of the rim
    admitted = r2[~(r2 > lim)]
    assert admitted.size <= 4 * W.RIM_SIDE * (W.RIM_SIDE - 1) and np.all(admitted > f32(0.999) * lim)


def test_exit_rows_hold_every_scan_trip_count(orc):
    keys, pred, grid = first_step("exit_rows")
    L = W.row_lengths(keys, grid)
    assert L.max() <= 32                                    # the mask sweep, not the chunked one
    for r in (0, 2):
        assert set(W.EXIT_LENGTHS) <= set(L[:, r].tolist()), r
    assert set(x for x in W.EXIT_LENGTHS if x) <= set(L[:, 1].tolist())        # the own row holds the lane itself
    assert sorted(set(-(-x // 4) for x in W.EXIT_LENGTHS)) == [0, 1, 2, 8]     # trips of four: none, one, two, all eight


def test_exit_waves_one_busy_lane_and_an_idle_wave(orc):
    st, ticks, p = W.exit_waves()
    keys, pred, grid = first_step("exit_waves")
    cnt = in_radius_counts(pred, st.smoothing_radius)
    wave0, wave1 = cnt[:64], cnt[64:128]
    assert int(wave0.max()) >= 20 and int((wave0 > 0).sum()) == 1
    assert int(wave1.max()) == 0
    assert W.row_lengths(keys, grid).max() <= 32


@pytest.mark.parametrize("n", W.DAM_N)
def test_small_dam_breaks_have_the_counts_they_are_named_after(orc, n):
    keys, pred, grid = first_step(f"dam_{n}")
    assert keys.shape[0] == n and W.row_lengths(keys, grid).max() <= 32


def test_density_trips_hold_every_row_length(orc):
    keys, pred, grid = first_step("density_trips")
    L = W.row_lengths(keys, grid)
    for r in (0, 2):
        assert set(W.TRIP_LENGTHS) <= set(L[:, r].tolist()), r
    assert set(range(1, 10)) <= set(L[:, 1].tolist())       # 0 cannot be: the lane is in its own row
    assert {x % 4 for x in W.TRIP_LENGTHS} == {0, 1, 2, 3} and {x // 4 for x in W.TRIP_LENGTHS} == {0, 1, 2}


def test_guard_scenes_sit_beside_the_fast_path(orc):
    keys, pred, grid = first_step("guard_tiny_dst")
    r2 = W.pair_r2(pred)
    dst = np.sqrt(r2.min(), dtype=f32)
    assert f32(2.0 ** -20) < dst < f32(2.0 ** -19) and r2.min() >= f32(2.0 ** -40)      # inside the proven range, at its low end
    keys, pred, grid = first_step("guard_coincident")
    assert int((W.pair_r2(pred) == 0.0).sum()) >= 2         # r2 == 0: the PRNG direction

"""CPU-side proof for the scenes of tests/slab_scenes.py, with the ORACLE (ref_quirks off, stable sort) and numpy alone:

  * every scene reaches the paths it is named after — per rank, on the rank's local live set in the rank's cell order (column-major
    ids for ranks with neighbours, row-major with FS_SLAB_ROWMAJOR and in the strips step), with prologue_scenes.block_rows;
  * over the STEPS steps the GPU tests run, no particle travels more than 1.5 columns in x per step, and the scene's boundary_cols
    is multi.boundary_columns for the largest speed the oracle reaches;
  * the tolerance of the GPU comparison is earned: the oracle's own spread under a permuted input (another order inside every cell)
    and under the x <-> y mirrored problem (the cells walked column-major) stays within a quarter of match_and_compare's defaults
    at the compared steps 1 and 2, cell keys identical, matching a bijection.

Each test prints what it measured (pytest -s).  tests/test_slab_hard_inputs_gpu.py runs the same scenes on slab handles.  No GPU."""
import numpy as np
import pytest

from tests import prologue_scenes as PS
from tests import slab_scenes as S

f32 = np.float32
CASES = [(name, world) for name in S.FIXED + ("cluster_with_coincident",) for world in (2, 3)] + [("obstacle_on_seam", 2)]
DEFAULTS = dict(rtol=1e-4, atol_vel=1e-3)            # tests/slab_oracle.py match_and_compare; position: 1e-4 * h


def get_scene(name, world):
    """-> (settings, tick, particles, bounds, boundary_cols, field)"""
    if name == "random":
        st, tick, p, bounds, field, z = S.random_settings(world)
        return st, tick, p, bounds, z, field
    return S.scene(name, world) + (S.scene_field(name),)


def finite(p):
    return np.isfinite(p["predicted_position"]).all(axis=1)


def spread(got, want, h):
    """Largest differences between two runs of one scene, particles matched by nearest predicted position:
    (density rel, velocity error in units of atol + rtol |v|, velocity abs, position abs, matching is a bijection, keys equal)."""
    from scipy.spatial import cKDTree
    a, b = got[finite(got)], want[finite(want)]
    assert a.shape == b.shape
    d, idx = cKDTree(b["predicted_position"].astype(np.float64)).query(a["predicted_position"].astype(np.float64))
    w = b[idx]
    ok = np.isfinite(w["density"])
    dens = np.abs(a["density"][ok].astype(np.float64) - w["density"][ok]) / np.abs(w["density"][ok])
    dv = np.abs(a["velocity"].astype(np.float64) - w["velocity"])
    vel = dv / (DEFAULTS["atol_vel"] + DEFAULTS["rtol"] * np.abs(w["velocity"].astype(np.float64)))
    pos = np.abs(a["position"].astype(np.float64) - w["position"])
    return dict(density_rel=float(dens.max()), velocity_units=float(vel.max()), velocity_abs=float(dv.max()),
                position_abs=float(max(pos.max(), d.max())), bijection=np.unique(idx).shape[0] == a.shape[0],
                keys_equal=bool(np.array_equal(a["grid"], w["grid"])))


def mirrored(st, tick, p, field):
    """The x <-> y mirrored problem: positions, velocities, size, gravity, mouse and the force field swapped."""
    import gpu_fluid_simulation_amd as g
    stm = g.SimulationSettings(st.particle_count, st.particle_spacing, st.smoothing_radius, (st.size.y, st.size.x),
                               (st.texture_size.y, st.texture_size.x))
    tm = type(tick).from_buffer_copy(tick)
    tm.gravity = g.Vec2(tick.gravity.y, tick.gravity.x)
    tm.mouse_pos = g.Vec2(tick.mouse_pos.y, tick.mouse_pos.x)
    q = p.copy()
    for k in ("position", "predicted_position", "velocity"):
        q[k] = p[k][:, ::-1]
    fm = None if field is None else np.ascontiguousarray(field.transpose(1, 0, 2)[:, :, ::-1])
    return stm, tm, q, fm


def mirror_back(st, out):
    gw = int(np.ceil(f32(st.size.x) / f32(st.smoothing_radius))) + 2
    gh = int(np.ceil(f32(st.size.y) / f32(st.smoothing_radius))) + 2
    q = out.copy()
    for k in ("position", "predicted_position", "velocity"):
        q[k] = out[k][:, ::-1]
    key = out["grid"].astype(np.int64)            # mirrored grid: gh columns; key = x_cell * gh + y_cell
    q["grid"] = ((key % gh) * gw + key // gh).astype(np.uint32)
    return q


def close_pairs(p):
    """Index pairs (i, j) with 0 < r2 < 2^-40 in f32, as the force sweep forms r2 from the predicted positions."""
    from scipy.spatial import cKDTree
    ok = np.nonzero(finite(p))[0]
    pr = p["predicted_position"][ok]
    pairs = cKDTree(pr.astype(np.float64)).query_pairs(2e-6, output_type="ndarray")
    d = pr[pairs[:, 0]] - pr[pairs[:, 1]]
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32)
    keep = (r2 > 0) & (r2 < f32(S.CLOSE_R2))
    return ok[pairs[keep]]


@pytest.fixture(scope="module")
def oracle_runs(orc):
    cache = {}

    def run(name, world):
        if (name, world) not in cache:
            st, tick, p, bounds, z, field = get_scene(name, world)
            cache[(name, world)] = S.step_oracle(st, tick, p, S.STEPS, field)
        return cache[(name, world)]
    return run


@pytest.mark.parametrize("name,world", CASES + [("random", k) for k in range(S.RANDOM_CASES)])
def test_travel_fits_the_zone(fs, orc, oracle_runs, name, world):
    from gpu_fluid_simulation_amd import multi
    st, tick, p, bounds, z, field = get_scene(name, world)
    states = oracle_runs(name, world)
    h, dt = st.smoothing_radius, tick.delta
    push = 0.0 if field is None else float(np.abs(field[..., 0]).max()) * 2.0 * st.size.x / st.texture_size.x
    vmax, travel = 0.0, 0.0
    for q in [p] + states:
        v = q["velocity"][np.isfinite(q["velocity"]).all(axis=1)].astype(np.float64)
        vmax = max(vmax, min(multi.SPEED_CLAMP, float(np.sqrt((v * v).sum(axis=1)).max())))
        travel = max(travel, (float(np.minimum(np.abs(v[:, 0]), multi.SPEED_CLAMP).max()) * dt + push) / h)
    accel = float(np.hypot(tick.gravity.x, tick.gravity.y))
    want = multi.boundary_columns(vmax, accel, dt, h, 1)
    print(f"{name}/{world}: largest speed {vmax:.4g}, largest x travel {travel:.3f} columns per step, boundary_cols {z} (formula {want}),"
          f" bounds {bounds}")
    assert travel <= 1.5
    assert z == want
    last = states[-1]
    ok = np.isfinite(last["velocity"]).all() and np.isfinite(last["position"]).all()
    assert ok, "the oracle's state after STEPS steps is not finite"


@pytest.mark.parametrize("name,world", CASES + [("random", k) for k in range(S.RANDOM_CASES)])
def test_order_spread_is_within_a_quarter_of_the_tolerance(fs, orc, oracle_runs, name, world):
    st, tick, p, bounds, z, field = get_scene(name, world)
    h = st.smoothing_radius
    base = oracle_runs(name, world)
    rng = np.random.default_rng(99)
    perm = S.step_oracle(st, tick, p[rng.permutation(p.shape[0])], max(S.COMPARED), field)
    stm, tm, q, fm = mirrored(st, tick, p, field)
    mirr = [mirror_back(st, o) for o in S.step_oracle(stm, tm, q, max(S.COMPARED), fm)]
    tol = dict(DEFAULTS, atol_pos=1e-4 * h, **S.tolerances(name))
    for step in S.COMPARED:
        for label, other in (("permuted", perm), ("mirrored", mirr)):
            if name == "cluster_with_coincident":
                continue          # a coincident pair's direction is drawn from the slot index: only equal slot orders compare
            m = spread(other[step - 1], base[step - 1], h)
            print(f"{name}/{world} step {step} {label}: density rel {m['density_rel']:.3g}, velocity abs {m['velocity_abs']:.3g}"
                  f" ({m['velocity_units']:.3g} of the tolerance), position abs {m['position_abs']:.3g}")
            assert m["bijection"] and m["keys_equal"]
            if name in S.TOLERANCES:          # its own tolerance: four times the measured spread
                assert m["density_rel"] <= tol["rtol"] / 4 and m["velocity_abs"] <= (tol["atol_vel"] + 0.0) / 4
                assert m["position_abs"] <= tol["atol_pos"] / 4
            else:
                assert m["density_rel"] <= DEFAULTS["rtol"] / 4
                assert m["velocity_units"] <= 0.25
                assert m["position_abs"] <= 1e-4 * h / 4


def rank_paths(st, tick, p, bounds, z, rank, column_major):
    """Per rank and layout: the local order, block_rows' model on it, and per sorted slot whether its column is edge zone / interior."""
    idx, keys, grid, col = S.local_order(st, tick, p, bounds, rank, column_major)
    cs, lane_len, lo, hi = PS.block_rows(keys, grid)
    adv_lo, adv_hi = S.zones(bounds, rank, z)
    owned = (col >= bounds[rank]) & (col < bounds[rank + 1])
    interior = owned & (col >= adv_lo) & (col < adv_hi)
    return idx, lane_len, hi - lo, owned & ~interior, interior


@pytest.mark.parametrize("name", ["cluster_on_seam", "cluster_with_coincident"])
@pytest.mark.parametrize("world", [2, 3])
def test_clusters_reach_the_chunked_and_the_unstaged_sweep_in_edge_zone_and_interior(fs, orc, name, world):
    st, tick, p, bounds, z, field = get_scene(name, world)
    seam = bounds.index(101)
    found_interior = 0
    for column_major in (True, False):
        for rank in range(world):
            idx, lane_len, span, edge, interior = rank_paths(st, tick, p, bounds, z, rank, column_major)
            nb = span.shape[0]
            blk = np.arange(idx.shape[0]) // S.BLOCK
            long_lane = lane_len.max(axis=1) > 32
            big_block = (span.max(axis=1) > S.NBF_TILE)[blk]
            counts = dict(edge_long=int((long_lane & edge).sum()), interior_long=int((long_lane & interior).sum()),
                          edge_unstaged=int(np.unique(blk[big_block & edge]).size), interior_unstaged=int(np.unique(blk[big_block & interior]).size))
            print(f"{name}/{world} rank {rank} {'column' if column_major else 'row'}-major: {nb} blocks, lanes with a row > 32:"
                  f" edge {counts['edge_long']} interior {counts['interior_long']}; blocks past NBF_TILE: edge {counts['edge_unstaged']}"
                  f" interior {counts['interior_unstaged']}")
            if rank in (seam - 1, seam):        # the ranks on either side of the seam at x = 0
                assert counts["edge_long"] > 0 and counts["edge_unstaged"] > 0
            if counts["interior_long"] > 0 and counts["interior_unstaged"] > 0:
                found_interior += 1
    assert found_interior >= 2                  # the second cluster: a rank's interior, in both layouts
    if name == "cluster_with_coincident":
        assert int((S.distinct_positions(p) == 2).sum()) == 64
    else:
        assert S.distinct_positions(p).shape[0] == p.shape[0]


@pytest.mark.parametrize("world", [2, 3])
def test_close_pairs_sit_on_both_sides_of_every_interior_edge(fs, orc, world):
    st, tick, p, bounds, z, field = get_scene("late_list_on_both_sides", world)
    pairs = close_pairs(p)
    assert pairs.shape[0] == 3 * len(S.pair_columns(world, z))
    assert S.distinct_positions(p).shape[0] == p.shape[0]          # close, never coincident
    for column_major in (True, False):
        for rank in range(world):
            idx, lane_len, span, edge, interior = rank_paths(st, tick, p, bounds, z, rank, column_major)
            slot = np.full(p.shape[0], -1, dtype=np.int64)
            slot[idx] = np.arange(idx.shape[0])
            mine = pairs[(slot[pairs] >= 0).all(axis=1)]
            sa, sb = slot[mine[:, 0]], slot[mine[:, 1]]
            in_edge = edge[sa] & edge[sb]
            in_int = interior[sa] & interior[sb]
            blocks_edge = set((sa[in_edge] // S.BLOCK).tolist()) | set((sb[in_edge] // S.BLOCK).tolist())
            blocks_int = set((sa[in_int] // S.BLOCK).tolist()) | set((sb[in_int] // S.BLOCK).tolist())
            mixed = sorted(blocks_edge & blocks_int)
            print(f"late_list/{world} rank {rank} {'column' if column_major else 'row'}-major: close pairs in the edge zone"
                  f" {int(in_edge.sum())}, in the interior {int(in_int.sum())}, blocks with both {mixed}")
            assert in_edge.sum() >= 1 and in_int.sum() >= 1
            assert mixed, "no 256-slot block holds a close pair on either side of adv_lo / adv_hi"


@pytest.mark.parametrize("world", [2, 3])
def test_mouse_and_field_cover_the_seam(fs, orc, oracle_runs, world):
    st, tick, p, bounds, z, field = get_scene("mouse_and_field_on_seam", world)
    col = S.predicted_columns(st, tick, p)
    seam = bounds.index(101)
    d = np.hypot(p["position"][:, 0] - tick.mouse_pos.x, p["position"][:, 1] - tick.mouse_pos.y)
    uv = (p["position"] / f32([st.size.x, st.size.y]) + f32(0.5)) * f32([st.texture_size.x, st.texture_size.y])
    tx, ty = uv[:, 0].astype(np.int64), uv[:, 1].astype(np.int64)
    pushed = (field[np.clip(ty, 0, 1023), np.clip(tx, 0, 1023)] != 0).any(axis=1)
    for rank in (seam - 1, seam):
        mine = (col >= bounds[rank]) & (col < bounds[rank + 1])
        print(f"mouse_and_field/{world} rank {rank}: {int((mine & (d <= tick.mouse_force_radius)).sum())} particles under the mouse,"
              f" {int((mine & pushed).sum())} in the field's band")
        assert (mine & (d <= tick.mouse_force_radius)).sum() > 100 and (mine & pushed).sum() > 100
    assert tick.mouse_state == 1


def test_obstacle_field_pushes_particles_on_both_sides_of_the_seam(fs, orc):
    st, tick, p, bounds, z, field = get_scene("obstacle_on_seam", 2)
    nz = np.nonzero((field != 0).any(axis=2))
    rows, cols = S.OBSTACLE_BAR
    assert nz[0].min() >= rows.start and nz[0].max() < rows.stop and nz[1].min() == cols.start and nz[1].max() == cols.stop - 1
    uv = (p["position"] / f32([st.size.x, st.size.y]) + f32(0.5)) * f32([st.texture_size.x, st.texture_size.y])
    pushed = (field[uv[:, 1].astype(np.int64), uv[:, 0].astype(np.int64)] != 0).any(axis=1)
    left, right = int((pushed & (p["position"][:, 0] < 0)).sum()), int((pushed & (p["position"][:, 0] >= 0)).sum())
    print(f"obstacle_on_seam: {left} particles inside the bar left of the seam, {right} right of it, longest push"
          f" {float(np.abs(field).max()):.3g} texels")
    assert left >= 5 and right >= 5


@pytest.mark.parametrize("world", [2, 3])
def test_bad_values_sit_where_they_are_named(fs, orc, oracle_runs, world):
    st, tick, p, bounds, z, field = get_scene("walls_and_bad_values", world)
    bs = f32([st.size.x, st.size.y]) / 2
    pos = p["position"]
    assert (pos[:, 0] > bs[0]).any() and (pos[:, 0] < -bs[0]).any() and (pos[:, 1] > bs[1]).any() and (pos[:, 1] < -bs[1]).any()
    bad = np.nonzero(~np.isfinite(p["velocity"]).all(axis=1))[0]
    assert bad.shape[0] == 2
    col = S.predicted_columns(st, tick, p)
    assert np.all(col[bad] == 1) and bounds[0] == 0 and bounds[-1] == S.GRID[0]      # a NaN prediction is keyed to column 1: rank 0's
    from gpu_fluid_simulation_amd import multi
    here = multi.global_columns(pos[bad, 0], st.size.x, st.smoothing_radius)
    adv_lo, adv_hi = S.zones(bounds, 0, z)
    assert sorted((here >= adv_lo) & (here < adv_hi)) == [False, True] and np.all(here < bounds[1])
    fast = np.nonzero(np.abs(p["velocity"][:, 1]) > 500)[0]
    assert fast.shape[0] == 1 and p["velocity"][fast[0], 0] == 0 and here.max() < 101 <= multi.global_columns(pos[fast, 0], st.size.x, st.smoothing_radius)[0]
    # what the reference makes of them: the NaN velocity is reset to zero and the particle stays where it was, density NaN at step 1
    first = oracle_runs("walls_and_bad_values", world)[0]
    for i in bad:
        k = np.nonzero((first["position"].view(np.uint32) == pos[i].view(np.uint32)).all(axis=1))[0]
        assert k.shape[0] == 1 and np.all(first["velocity"][k[0]] == 0) and first["grid"][k[0]] % S.GRID[0] == 1
    assert np.abs(first["velocity"]).max() <= 500.0 * (1 + 1e-6)


def test_random_settings_are_wide_enough_for_three_ranks(fs, orc):
    assert len(S.RANDOM_SEEDS) == S.RANDOM_CASES
    for case in range(S.RANDOM_CASES):
        st, tick, p, bounds, z, field = get_scene("random", case)
        gw = S.grid_width(st)
        print(f"random {case} (seed {S.RANDOM_SEEDS[case]}): n {p.shape[0]}, h {st.smoothing_radius:.3g}, grid width {gw}, bounds {bounds},"
              f" boundary_cols {z}, field {field is not None}, mouse {tick.mouse_state}")
        assert gw >= 24 and len(bounds) == 4 and bounds[0] == 0 and bounds[-1] == gw
        assert all(b - a >= 4 for a, b in zip(bounds, bounds[1:]))

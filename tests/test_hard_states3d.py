"""CPU companion of tests/test_3d_queries_hard_inputs_gpu.py: the registry of tests/hard_states3d.py tests what it says, on the
oracle and the checkers alone.  Which cases do not stay finite and which share keys; that the special query set reaches every
place it names; that the sampling checker agrees with the numpy restatements of the header on that set; that the renders and meshes
of the GPU test hold what it requires of them; that the offset-scan view puts vertices where the scan needs them.  No GPU."""
import numpy as np
import pytest

from tests import hard_states3d as H

f = np.float32
RESTATED = ["thin/0", "faces/exact", "radius/0.05", "radius/0.33"]      # 0.33: where numpy's float32 power is not libm's powf


def test_the_restatements_poly6_is_the_oracles_at_every_radius(fs, orc):
    """C6 names the host libm's powf.  tests/sample_attr3d_ref.poly6 once took numpy's float32 power, one ulp off at h = 0.33: every
    weight of the restatement was off with it, at a radius no test sampled channels at."""
    import paths3d
    from tests.sample_attr3d_ref import poly6
    for h in paths3d.RADII:
        case = H.case_by_id(fs, orc, f"radius/{h}")
        case.run()
        assert poly6(case.st.smoothing_radius).view(np.uint32) == f(case.constants[0]).view(np.uint32), h


def test_the_registry_holds_what_the_plain_tests_run(fs, orc):
    import paths3d
    assert len(set(H.CASE_IDS)) == len(H.CASE_IDS)
    for group in (H.NOT_FINITE_CASE_IDS, H.TIE_CASE_IDS, H.ONE_KEY_CASE_IDS, H.SURFACE_CASE_IDS, H.TOLERANCE_CASE_IDS):
        assert set(group) <= set(H.CASE_IDS)
    assert sum(c.startswith("guard/") for c in H.CASE_IDS) == len(paths3d.GUARD_CASES) + 3 == 15
    assert [c for c in H.CASE_IDS if c.startswith("radius/")] == [f"radius/{h}" for h in paths3d.RADII]
    shapes = set()
    for k in range(H.RANDOM_CASES):
        case = H.case_by_id(fs, orc, f"random/{k}")
        assert all(o != 0.0 for o in case.off), "a random box keeps its drawn, non-zero offset"
        shapes.add(k % 4)
    assert shapes == {0, 1, 2, 3}
    assert {c for c in H.SURFACE_CASE_IDS if c.startswith("random/")} == {"random/1", "random/2"}
    one, thin3 = H.case_by_id(fs, orc, "thin/0"), H.case_by_id(fs, orc, "thin/1")
    assert one.grid_dims == (3, 3, 3) and min(thin3.grid_dims) == 3
    assert H.case_by_id(fs, orc, "guard/density_across_2p20").tick.mass == 1500.0
    tiny = H.case_by_id(fs, orc, "guard/mass_tiny")
    assert (tiny.run()[0]["density"] == f(0.1)).all(), "after step 1 every density sits on the 0.1 floor"
    coin = H.case_by_id(fs, orc, f"scene/{H.SCENE_COINCIDENT}").start["position"]
    assert np.unique(coin, axis=0).shape[0] < coin.shape[0], "the coincident scene is uploaded with coincident particles"


def test_which_cases_do_not_stay_finite(fs, orc):
    got = [cid for cid in H.CASE_IDS if not H.case_by_id(fs, orc, cid).stays_finite]
    assert got == ["guard/inf_velocity", "guard/huge_pressure", "guard/unsafe_next_to_safe", "guard/nan_next_to_everyone"]
    assert got == H.NOT_FINITE_CASE_IDS


def test_tie_cases_are_what_they_say(fs, orc):
    """TIE_CASE_IDS: two records share a key after a step — every case, each holds more particles than occupied cells.
    ONE_KEY_CASE_IDS: ALL records share one key after EVERY step, so the sort's network (a swap needs key(lo) > key(hi)) moves
    nothing and the tracking statement is the identity there; everywhere else some step's permutation is not the identity."""
    from tests.track3d_ref import Track3Checker
    tie = [cid for cid in H.CASE_IDS if any(H.case_by_id(fs, orc, cid).shares_a_key())]
    one = [cid for cid in H.CASE_IDS if all(H.case_by_id(fs, orc, cid).one_key())]
    assert tie == H.TIE_CASE_IDS and one == H.ONE_KEY_CASE_IDS
    assert {"thin/0", f"scene/{H.SCENE_COINCIDENT}", "guard/nan_next_to_everyone"} <= set(tie)
    for cid in H.TIE_CASE_IDS:
        case = H.case_by_id(fs, orc, cid)
        chk = Track3Checker(case.st, case.off)
        chk.set_particles(case.start)
        with np.errstate(all="ignore"):
            moved = [not np.array_equal(chk.step(case.tick), np.arange(case.n)) for _ in range(case.steps)]
        for fld in ("grid", "predicted_position"):                       # the checker's oracle is the registry's
            assert chk.particles()[fld].tobytes() == case.run()[-1][fld].tobytes(), cid
        chk.close()
        assert any(moved) == (cid not in H.ONE_KEY_CASE_IDS), f"{cid}: moved {moved}"


@pytest.mark.parametrize("cid", H.CASE_IDS)
def test_the_special_set_reaches_what_it_names(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    b = f([case.st.size.x, case.st.size.y, case.st.size.z]) * f(0.5)
    inf = f(np.inf)
    for s in sorted({0, case.steps - 1}):
        p = case.run()[s]
        pts = H.special_queries3(case.st, p)
        assert pts.dtype == np.float32 and np.isfinite(pts).all(), "no non-finite coordinate"
        c = H.query_cells3(case.st, pts)
        for a in range(3):
            g = case.grid_dims[a]
            assert (c[:, a] == 0).any(), f"axis {a}: no query wraps to cell 0"
            assert (c[:, a] == g).any() and (c[:, a] == g + 1).any(), f"axis {a}: no query in cell grid and grid + 1"
            assert (c[:, a] == g - 1).any() and (c[:, a] == 1).any() and (c[:, a] == 2).any()
            for v in (-b[a], b[a]):
                inside = (np.abs(pts) <= b).all(axis=1)
                assert ((pts[:, a] == v) & inside).any(), f"axis {a}: no query on the face at {v}"
                for d in (-inf, inf):
                    assert (pts[:, a] == np.nextafter(v, d)).any()
            assert (pts[:, a] < -b[a] - f(4) * f(case.h)).any() and (pts[:, a] <= f(-1e10)).any(), "far below -b"
            assert (pts[:, a] >= f(4294967296.0) * f(case.h)).any()
        assert (c == 0).all(axis=1).any(), "no query wraps on all three axes at once"
        on_walls = (np.abs(pts) == b).sum(axis=1)
        assert np.unique(pts[on_walls == 3], axis=0).shape[0] >= 8, "the 8 corners"
        assert np.unique(pts[(on_walls == 2) & (pts == 0).any(axis=1)], axis=0).shape[0] >= 12, "the 12 edge mid-points"
        for key in (p["grid"][0], p["grid"][-1]):                        # the first and the last occupied cell
            for q in p["predicted_position"][p["grid"] == key]:
                assert not np.isfinite(q).all() or (pts == q).all(axis=1).any()
        for q in p[p["grid"] >= case.ncell]["predicted_position"]:      # records with keys past the table, where a state has them
            assert not np.isfinite(q).all() or (pts == q).all(axis=1).any()
        ids = H.query_cell_ids3(case.st, case.grid_dims, pts)
        from tests.sample3d_ref import Sample3Checker
        chk = Sample3Checker(case.st, case.off).load(p, case.tick.mass)
        with np.errstate(all="ignore"):
            out = chk.sample(pts)
        chk.close()
        assert np.array_equal(out["cell"], ids), "the checker's cell is the header's wrapping expression"
        assert (out["neighbours"] > 0).any() and (out["neighbours"] == 0).any(), "the special set hits the fluid and misses it"


def _restated(case, p, pts):
    """the records of tests/test_sampling3d.restatement at `pts`.  The restatement scans every record for every one of a query's 27
    cells; it is handed the records of those cells alone, in slot order — the slots with p[k].grid == id, ascending, all the same."""
    from tests.sample3d_ref import SAMPLE3_DTYPE
    from tests.test_sampling3d import restatement
    gw, gh, gd = case.grid_dims
    size = (f(case.st.size.x), f(case.st.size.y), f(case.st.size.z))
    h = f(case.st.smoothing_radius)
    c6 = f(case.constants[0])
    cells = H.query_cells3(case.st, pts).astype(np.int64)
    want = np.zeros(pts.shape[0], dtype=SAMPLE3_DTYPE)
    with np.errstate(all="ignore"):
        for k in range(pts.shape[0]):
            ids = {(((cells[k, 2] + oz) & 0xFFFFFFFF) * gh + ((cells[k, 1] + oy) & 0xFFFFFFFF)) * gw + ((cells[k, 0] + ox) & 0xFFFFFFFF)
                   for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)}
            sub = p[np.isin(p["grid"].astype(np.int64), sorted(i & 0xFFFFFFFF for i in ids))]
            d, w, v, g, nb, cell = restatement(sub, case.grid_dims, size, h, f(case.tick.mass), c6, pts[k])
            want[k] = (d, w, v, g, nb, cell)
    return want


@pytest.mark.parametrize("cid", RESTATED)
def test_checker_equals_the_numpy_restatements_on_the_special_set(fs, orc, cid):
    """the weight against tests/sample_attr3d_ref.sample_attr, every field against the restatement of tests/test_sampling3d.py"""
    from tests.sample3d_ref import Sample3Checker
    from tests.sample_attr3d_ref import sample_attr
    case = H.case_by_id(fs, orc, cid)
    assert case.stays_finite
    p = case.run()[-1]
    pts = H.special_queries3(case.st, p)
    chk = Sample3Checker(case.st, case.off).load(p, case.tick.mass)
    got = chk.sample(pts)
    chk.close()
    with np.errstate(all="ignore"):
        weight, _ = sample_attr(case.st, case.grid_dims, case.tick.mass, p, np.zeros((0, case.n), dtype=np.float32), pts)
    assert (got["weight"] > 0).sum() > 50 and (got["weight"] == 0).sum() > 50
    assert got["weight"].tobytes() == weight.tobytes(), "sample_attr's weight"
    want = _restated(case, p, pts)
    bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])
    assert bad.size == 0, f"{bad.size} of {got.size} records differ; first {bad[0]}: {pts[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("cid", H.NOT_FINITE_CASE_IDS)
def test_not_finite_cases_return_nan_and_finite_records(fs, orc, cid):
    """what the GPU test asserts on the checker fed the engine's download, here on the oracle's records: over the query sets of a
    non-finite state some returned record holds a NaN and some holds none"""
    from tests.sample3d_ref import Sample3Checker
    case = H.case_by_id(fs, orc, cid)
    seen_nan = seen_finite = 0
    for s in sorted({0, case.steps - 1}):
        p = case.run()[s]
        chk = Sample3Checker(case.st, case.off).load(p, case.tick.mass)
        for name, pts in H.query_sets3(case.st, p, finite_only=True).items():
            assert np.isfinite(pts).all()
            with np.errstate(all="ignore"):
                nan = H.nan_records(chk.sample(pts))
            seen_nan += int(nan.sum()); seen_finite += int((~nan).sum())
        chk.close()
    assert seen_nan > 0 and seen_finite > 0, (seen_nan, seen_finite)


@pytest.mark.parametrize("cid", H.SURFACE_CASE_IDS)
def test_renders_and_meshes_hold_what_the_gpu_test_requires(fs, orc, cid):
    """every case: a valid threshold; every radius case: hit kinds 0, 1 and 2 over its cameras, a non-empty mesh on (33, 33, 33)"""
    from tests.mesh3d_ref import Mesh3Checker
    from tests.render3d_ref import Render3Checker, iso_of
    case = H.case_by_id(fs, orc, cid)
    assert case.stays_finite
    p = case.run()[-1]
    iso = iso_of(p)
    assert np.isfinite(iso) and iso > 0.0
    if not cid.startswith("radius/"):
        return
    chk = Render3Checker(case.st, case.off).load(p, case.tick.mass)
    kinds = set()
    for ctx, cam, sp in H.surface_renders(case.st, p):
        if sp.refine == 0:                                               # the refinement moves t, not the kind
            kinds.update(np.unique(chk.render(cam, sp)["hit"]).tolist())
    chk.close()
    assert kinds == {0, 1, 2}, kinds
    chk = Mesh3Checker(case.st, case.off).load(p, case.tick.mass)
    most = 0
    for ctx, dims, wmin, wmax, iso in H.surface_meshes(case.st, p):
        if dims == H.LARGEST:
            most = max(most, chk.extract(dims, wmin, wmax, iso)[2][0])
    chk.close()
    assert most > 0


def test_a_candidate_exactly_on_the_radius_decides_a_ray_of_the_probe_case(fs, orc):
    """the probe of hard_states3d.radius_probe exists on the oracle's state, and the checker's two rays are what the GPU test
    needs: both start inside, the one at q returns a NaN velocity, the one a few ulps beyond a finite record"""
    from tests.render3d_ref import Render3Checker, iso_of
    case = H.case_by_id(fs, orc, H.PROBE_CASE_ID)
    p = case.run()[H.PROBE_STEP - 1]
    chk = Render3Checker(case.st, case.off).load(p, case.tick.mass)
    iso = iso_of(p)
    probe = H.radius_probe(case.st, p, chk.sample, iso)
    assert probe is not None
    q, beyond, j = probe
    d = p["predicted_position"][j] - q
    assert d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == f(case.st.smoothing_radius) * f(case.st.smoothing_radius)
    assert not np.isfinite(p["velocity"][j]).all()
    with np.errstate(all="ignore"):
        at_q, at_beyond = [chk.render(cam, sp)[0, 0] for cam, sp in H.probe_renders(case.st, q, beyond, iso)]
    chk.close()
    for rec in (at_q, at_beyond):
        assert rec["hit"] == 2 and rec["t"] == 0.0 and rec["steps"] == 0, rec
    assert np.isnan(at_q["velocity"]).any() and np.isfinite(at_q["density"]) and np.isfinite(at_q["normal"]).all()
    assert np.isfinite(at_beyond["velocity"]).all() and np.isfinite(at_beyond["density"])


def test_the_scan_view_puts_vertices_behind_node_256k_and_in_both_workgroup_parities(fs, orc):
    from tests.mesh3d_ref import Mesh3Checker
    from tests.render3d_ref import iso_of
    st, off, tick, start = H.scan_scene(fs)
    ref = orc.OracleSim3D(st, off)
    ref.set_particles(start)
    for _ in range(H.SCAN_STEPS):
        ref.step(tick)
    p = ref.particles()
    ref.close()
    chk = Mesh3Checker(st, off).load(p, tick.mass)
    wmin, wmax = H.scan_view(st, p)
    for dims, nwg, chunk in H.SCAN_LATTICES:
        verts, tris, counts, cells, _ = chk.extract(dims, wmin, wmax, iso_of(p), detail=True)
        fig = H.scan_figures(dims, cells)
        print(f"[scan] lattice {dims}: view {wmin} .. {wmax}, {counts[0]} vertices, {counts[1]} triangles, {fig}")
        assert (fig["nwg"], fig["chunk"]) == (nwg, chunk)
        assert fig["far"] > 0 and fig["even"] > 0 and fig["odd"] > 0, fig
        # the last owning thread's range is partial, and the threads behind it are clamped to an empty one
        assert nwg % chunk != 0 and (nwg + chunk - 1) // chunk < H.SCAN_THREADS
    chk.close()
    # the node index of a cell: cell (i, j, k) of a 3 x 4 x 5 lattice
    assert H.vertex_nodes((3, 4, 5), [(2 * 3 + 1) * 2 + 1]).tolist() == [(2 * 4 + 1) * 3 + 1]

"""Everything that reads the 3D state after a step — fs3_sample_points, fs3_sample_attr_points, fs3_render_surface,
fs3_extract_surface and the tracking carry — at the inputs at which tests/test_3d_paths_gpu.py holds the plain step: the registry
of tests/hard_states3d.py (operand guards, six smoothing radii, random boxes with offsets, faces, edges and corners, walls,
one-cell and thin grids, over-full cells).  The CPU companion tests/test_hard_states3d.py asserts without a GPU that the cases and
the query sets reach what they are named after.

Every test steps its case on the engine and downloads.  For a case that stays finite the download equals the oracle's records of
that step byte for byte; for the others word for word, a NaN of the oracle met by any NaN (the rule of
tests/test_3d_features_hard_inputs_gpu.py).  The checker of a query is then loaded with THAT download, as in the plain query tests,
and compared in bytes: no query and no state is masked.  Where a state is not finite the header's statement still holds (`if not
(r2 > h2)` admits a NaN distance; only non-finite QUERY coordinates are unspecified), and the records are compared word for word
under the same NaN rule.  FS_MATH_TOLERANCE: the queries are a function of the downloaded state in either mode, so bytes again."""
import numpy as np
import pytest

from tests import hard_states3d as H
from tests.bitcmp import POOL_TWELVE, assert_identical, assert_records_equal, assert_track_equal, special_bits
from tests.test_3d_features_hard_inputs_gpu import _same_words

pytestmark = pytest.mark.gpu
f32 = np.float32
EPSILON_F = np.float32(1.19209290e-07)
FINITE_CASE_IDS = [c for c in H.CASE_IDS if c not in H.NOT_FINITE_CASE_IDS]


def engine(fs, case, **kw):
    sim = fs.FluidSimulation3D(case.st, device=0, initial_offset=case.off, **kw)
    sim.upload_particles(case.start)
    return sim


def download(sim, case, step, ieee=True):
    """the handle's records after `step` steps; in FS_MATH_IEEE they are the oracle's: bytes where the case stays finite"""
    got, want = sim.download_particles(), case.run()[step - 1]
    ctx = f"{case.name} step {step}"
    if not ieee:                                         # no oracle to equal: the cell keys of one step from the upload, finite floats
        if step == 1:
            assert np.array_equal(got["grid"], want["grid"]), f"{ctx}: cell keys stay bit-exact in tolerance mode"
        for fld in H.FLOAT_FIELDS:
            assert np.isfinite(got[fld]).all(), f"{ctx}: non-finite {fld}"
        return got
    assert_records_equal(got, want, f"{ctx}: not the oracle's", nan_any=not case.stays_finite)
    return got


def same_sample_words(got, want, what):
    """fs3_sample records word for word, a NaN of the checker met by any NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert_records_equal(got, want, what, nan_any=True)


def stepped(sim, case, ieee=True):
    """(step, download) after step 1 and after case.steps"""
    done = 0
    for upto in sorted({1, case.steps}):
        while done < upto:
            sim.tick(case.tick)
            done += 1
        yield upto, download(sim, case, upto, ieee)


def check_sampler(sim, case, p, ctx, ieee):
    """the query sets of a finite state against the checker, and the identities of test_sampling3d_gpu.check_query_sets"""
    from tests.sample3d_ref import Sample3Checker
    chk = Sample3Checker(case.st, case.off).load(p, case.tick.mass)
    assert chk.grid_dims == sim.grid_dims == case.grid_dims
    sets = H.query_sets3(case.st, p)
    out = {name: sim.sample(pts) for name, pts in sets.items()}
    for name, pts in sets.items():
        assert_identical(out[name], chk.sample(pts), f"{ctx}: {name}")
    chk.close()
    own = out["own"]
    assert np.array_equal(own["cell"], p["grid"]), f"{ctx}: cell == grid at a particle's own position"
    assert (own["neighbours"] >= 1).all(), ctx
    if ieee:
        got = np.maximum(np.maximum(own["density"], EPSILON_F), f32(0.1))
        assert np.array_equal(got.view(np.uint32), p["density"].view(np.uint32)), f"{ctx}: density identity"
    assert np.array_equal(out["special"]["cell"], H.query_cell_ids3(case.st, case.grid_dims, sets["special"])), f"{ctx}: the wrapping cell id"
    hit, miss = int((out["uniform"]["neighbours"] > 0).sum()), int((out["uniform"]["neighbours"] == 0).sum())
    print(f"[queries3d] {ctx}: uniform set hits {hit}, misses {miss}; special set of {sets['special'].shape[0]} hits "
          f"{int((out['special']['neighbours'] > 0).sum())}")
    assert hit > 0, f"{ctx}: the uniform set never hits the fluid"
    if case.name in H.ONE_KEY_CASE_IDS:
        # a box smaller than h: no point of 1.2 x the box is farther than h from every particle; the special set misses instead
        assert (out["special"]["neighbours"] == 0).any(), ctx
    else:
        assert miss > 0, f"{ctx}: the uniform set never misses the fluid"


# ---- a. the sampler on every case that stays finite ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FINITE_CASE_IDS)
def test_sampler_on_finite_cases(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    assert case.stays_finite
    sim = engine(fs, case)
    for step, p in stepped(sim, case):
        check_sampler(sim, case, p, f"{cid} step {step}", ieee=True)
    sim.close()


# ---- b. the sampler on the cases that do not stay finite ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.NOT_FINITE_CASE_IDS)
def test_sampler_on_cases_that_do_not_stay_finite(fs, orc, cid):
    """own positions restricted to the finite ones, special and uniform; over the case some record of the checker holds a NaN and
    some holds none"""
    from tests.sample3d_ref import Sample3Checker
    case = H.case_by_id(fs, orc, cid)
    assert not case.stays_finite
    sim = engine(fs, case)
    nan = finite = 0
    for step, p in stepped(sim, case):
        chk = Sample3Checker(case.st, case.off).load(p, case.tick.mass)
        for name, pts in H.query_sets3(case.st, p, finite_only=True).items():
            assert np.isfinite(pts).all()
            with np.errstate(all="ignore"):
                want = chk.sample(pts)
            same_sample_words(sim.sample(pts), want, f"{cid} step {step}: {name}")
            nan += int(H.nan_records(want).sum()); finite += int((~H.nan_records(want)).sum())
        chk.close()
    print(f"[queries3d] {cid}: {nan} records of the checker hold a NaN, {finite} hold none")
    assert nan > 0 and finite > 0
    sim.close()


# ---- c. both math modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.TOLERANCE_CASE_IDS)
def test_sampler_in_tolerance_mode(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    sim = engine(fs, case, math_mode=fs.FS_MATH_TOLERANCE)
    for step, p in stepped(sim, case, ieee=False):
        check_sampler(sim, case, p, f"{cid} tolerance step {step}", ieee=False)
    sim.close()


# ---- d. tracking and channels on the tie cases ----------------------------------------------------------------------------------
def channel_values(n, channels):
    """channels 0 and 1: the bit patterns of bitcmp.special_bits's twelve-value pool (NaN payloads, infinities, -0.0, denormals);
    channels 2 and 3: the finite values of hard_states2d.sample_channel_values, whose sums are compared in bytes"""
    from tests.hard_states2d import sample_channel_values
    rows = [special_bits(n, 50, POOL_TWELVE), special_bits(n, 51, POOL_TWELVE)] + list(sample_channel_values(n, 2))
    return np.ascontiguousarray(np.stack(rows[:channels]))


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("cid", H.TIE_CASE_IDS)
def test_tracking_and_channels_on_tie_cases(fs, orc, cid, channels):
    from tests.sample_attr3d_ref import sample_attr
    from tests.test_sample_attr3d_gpu import raw_points
    from tests.track3d_ref import Track3Checker
    case = H.case_by_id(fs, orc, cid)
    sim = engine(fs, case, track=channels)
    chk = Track3Checker(case.st, case.off, channels=channels)
    chk.set_particles(case.start)
    values = channel_values(case.n, channels)
    for c in range(channels):
        sim.set_attribute(c, values[c])
        chk.attr[c] = values[c]
    moved = []
    for s in range(case.steps):
        sim.tick(case.tick)
        with np.errstate(all="ignore"):
            perm = chk.step(case.tick)
        moved.append(not np.array_equal(perm, np.arange(case.n)))
        assert_track_equal(sim, chk, f"{cid} C={channels} step {s + 1}")
        p = download(sim, case, s + 1)
    assert np.array_equal(np.sort(chk.ids), np.arange(case.n))
    # all records in one cell: the network swaps nothing and the statement is the identity; everywhere else slots change occupant
    assert any(moved) == (cid not in H.ONE_KEY_CASE_IDS), f"{cid}: the checker's permutations: {moved}"
    exact = case.stays_finite
    sets = H.query_sets3(case.st, p, finite_only=True)
    for name in ("own", "special"):
        pts = sets[name]
        with np.errstate(all="ignore"):
            want_w, want_a = sample_attr(case.st, sim.grid_dims, case.tick.mass, p, chk.attr, pts)
        w, a = raw_points(fs, sim, pts, channels)
        ctx = f"{cid} C={channels} {name}"
        if exact:
            assert w.tobytes() == want_w.tobytes(), f"{ctx}: weights"
            assert a[2:].tobytes() == np.ascontiguousarray(want_a[2:]).tobytes(), f"{ctx}: sums of the finite channels"
        else:
            _same_words(w, want_w, f"{ctx}: weights")
            _same_words(a[2:].T, want_a[2:].T, f"{ctx}: sums of the finite channels")
        _same_words(np.ascontiguousarray(a[:2].T), np.ascontiguousarray(want_a[:2].T), f"{ctx}: sums of the bit-pattern channels")
        _, a2 = raw_points(fs, sim, pts, channels, weights=False)
        assert a2.tobytes() == a.tobytes(), f"{ctx}: weight_out == NULL"
    sim.close(); chk.close()


# ---- e. the renderer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.SURFACE_CASE_IDS)
def test_renderer(fs, orc, cid):
    from tests.render3d_ref import Render3Checker
    from tests.test_render3d_gpu import product_render
    case = H.case_by_id(fs, orc, cid)
    sim = engine(fs, case)
    for _ in range(case.steps):
        sim.tick(case.tick)
    p = download(sim, case, case.steps)
    chk = Render3Checker(case.st, case.off).load(p, case.tick.mass)
    render = product_render(fs, sim)
    kinds = set()
    for ctx, cam, sp in H.surface_renders(case.st, p):
        want = chk.render(cam, sp)
        assert_identical(render(cam, sp), want, f"{cid}: {ctx}")
        kinds.update(np.unique(want["hit"]).tolist())
    print(f"[queries3d] {cid}: hit kinds {sorted(kinds)}")
    if cid.startswith("radius/"):
        assert kinds == {0, 1, 2}, cid
    chk.close(); sim.close()


def test_renderer_admits_a_candidate_exactly_on_the_radius(fs, orc):
    """`if not (r2 > h2)` of the full-sample walk.  In a finite state a candidate with r2 == h2 adds +-0 to sums that start at +0:
    no bit shows whether it was admitted.  guard/huge_pressure after one step holds records with a NaN velocity and a finite
    position; a ray that starts at exactly h from one of them (hard_states3d.radius_probe) returns a NaN velocity by the statement,
    and the ray a few ulps beyond a finite one.  Word for word, a NaN of the checker met by any NaN."""
    from tests.render3d_ref import Render3Checker, iso_of
    from tests.test_render3d_gpu import product_render
    case = H.case_by_id(fs, orc, H.PROBE_CASE_ID)
    sim = engine(fs, case)
    for _ in range(H.PROBE_STEP):
        sim.tick(case.tick)
    p = download(sim, case, H.PROBE_STEP)
    chk = Render3Checker(case.st, case.off).load(p, case.tick.mass)
    iso = iso_of(p)
    probe = H.radius_probe(case.st, p, chk.sample, iso)
    assert probe is not None, "no record with a non-finite velocity has a point at exactly h"
    q, beyond, j = probe
    render = product_render(fs, sim)
    wants = []
    for name, (cam, sp) in zip(("on the radius", "beyond it"), H.probe_renders(case.st, q, beyond, iso)):
        with np.errstate(all="ignore"):
            want = chk.render(cam, sp)
        got = render(cam, sp)
        for fld in ("t", "density", "normal", "velocity"):
            _same_words(got[fld].reshape(1, -1), want[fld].reshape(1, -1), f"ray {name}: {fld}")
        assert got["hit"][0, 0] == want["hit"][0, 0] == 2 and got["steps"][0, 0] == want["steps"][0, 0], name
        wants.append(want[0, 0])
    assert np.isnan(wants[0]["velocity"]).any() and np.isfinite(wants[1]["velocity"]).all(), "record j alone decides"
    chk.close(); sim.close()


# ---- f. the extractor -----------------------------------------------------------------------------------------------------------
def check_mesh(sim, chk, dims, wmin, wmax, iso, ctx):
    want_v, want_t, want_c = chk.extract(dims, wmin, wmax, iso)
    got_v, got_t = sim.extract_surface(*dims, iso, wmin, wmax)
    assert (got_v.shape[0], got_t.shape[0]) == want_c, f"{ctx}: counts {(got_v.shape[0], got_t.shape[0])} != {want_c}"
    assert_identical(got_v, want_v, ctx + " vertices")
    assert_identical(got_t, want_t, ctx + " triangles")
    return want_c


@pytest.mark.parametrize("cid", H.SURFACE_CASE_IDS)
def test_extractor(fs, orc, cid):
    from tests.mesh3d_ref import Mesh3Checker
    case = H.case_by_id(fs, orc, cid)
    sim = engine(fs, case)
    for _ in range(case.steps):
        sim.tick(case.tick)
    p = download(sim, case, case.steps)
    chk = Mesh3Checker(case.st, case.off).load(p, case.tick.mass)
    most = 0
    for ctx, dims, wmin, wmax, iso in H.surface_meshes(case.st, p):
        V, T = check_mesh(sim, chk, dims, wmin, wmax, iso, f"{cid}: {ctx}")
        if dims == H.LARGEST:
            most = max(most, V)
    print(f"[queries3d] {cid}: up to {most} vertices on {H.LARGEST}")
    if cid.startswith("radius/"):
        assert most > 0, cid
    chk.close(); sim.close()


# ---- g. the offset scan with real work --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nwg,chunk", H.SCAN_LATTICES)
def test_offset_scan_with_more_than_one_sum_per_thread(fs, dims, nwg, chunk):
    """k3_mesh_scan gives each of its 1024 threads `chunk` workgroup sums.  Every other lattice with a surface in the suite has at
    most 1024 sums (chunk 1).  (65, 65, 65): 1073 sums, chunk 2; (129, 129, 65): 4226 sums, chunk 5, the last owning thread's
    range partial and the threads behind it clamped to an empty one.  The view ends inside the fluid (hard_states3d.scan_view), so
    the checker's mesh holds vertices at nodes from 256 * 1024 on and in even and odd workgroups alike."""
    from tests.mesh3d_ref import Mesh3Checker
    from tests.render3d_ref import iso_of
    st, off, tick, start = H.scan_scene(fs)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(start)
    for _ in range(H.SCAN_STEPS):
        sim.tick(tick)
    p = sim.download_particles()
    for fld in H.FLOAT_FIELDS:
        assert np.isfinite(p[fld]).all(), f"non-finite {fld}"
    chk = Mesh3Checker(st, off).load(p, tick.mass)
    wmin, wmax = H.scan_view(st, p)
    iso = iso_of(p)
    _, _, counts, cells, _ = chk.extract(dims, wmin, wmax, iso, detail=True)
    fig = H.scan_figures(dims, cells)
    print(f"[queries3d] scan {dims}: view {wmin} .. {wmax}, {counts[0]} vertices, {counts[1]} triangles, {fig}")
    assert (fig["nwg"], fig["chunk"]) == (nwg, chunk)
    assert fig["far"] > 0 and fig["even"] > 0 and fig["odd"] > 0, fig
    assert check_mesh(sim, chk, dims, wmin, wmax, iso, f"scan {dims}") == counts
    chk.close(); sim.close()

"""Field sampling (k_sample) at the inputs at which the plain 2D step is held, and at queries whose cell
coordinates saturate, wrap or leave the grid.  The states are the cases of tests/hard_states2d.py, stepped on the engine in their
sort mode and quirks setting; the checker is tests/sample_ref.SampleChecker loaded from the handle's download, as in
tests/test_sampling_gpu.py, and every comparison is of bytes.  tests/test_sampling.py shows without a GPU that the checker is
the header's statement at the wrapped and saturated cells (a plain numpy restatement agrees with it on every byte), and that
the special query set reaches what it names.

No query and no state is masked.  The sampler is specified on finite states, so the registry's cases whose oracle records do
not stay finite are not sampled; they are
    guard/inf_velocity   an infinite and a NaN velocity: non-finite records after every step
    nan_clamp            a NaN velocity: non-finite records after step 1 (the step zeroes it afterwards)
and stay with tests/test_tracking_hard_inputs_gpu.py and the plain parity tests (tests/test_tracking.py asserts that these two
are the only ones)."""
import numpy as np
import pytest

from tests import hard_states2d as H
from tests import prologue_scenes as S
from tests.test_sampling_gpu import EPSILON_F, assert_samples_equal, load_checker, query_sets

pytestmark = pytest.mark.gpu
NOT_FINITE = ("guard/inf_velocity", "nan_clamp")
SAMPLED_IDS = [cid for cid in H.CASE_IDS if cid not in NOT_FINITE]


def engine(fs, case, track=None, **kw):
    sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, ref_quirks=case.quirks,
                             sort_mode=fs.FS_SORT_COUNTING if case.stable else fs.FS_SORT_BITONIC, track=track, **kw)
    sim.upload_particles(case.start)
    if case.start_indices is not None:
        sim.upload_start_indices(case.start_indices)
    if case.field is not None:
        sim.upload_force_field(case.field)
    return sim


def check_sets(fs, sim, case, ieee, ctx, uniform=True):
    """own (with the identities that tie the sampler to the step), shuffled, the special set and, with `uniform`, points drawn
    over 1.2 x the box, against the checker loaded from the handle's download"""
    chk, p, attr = load_checker(fs, sim, case.st, case.off, case.quirks)
    sets = query_sets(case.st, p, np.random.default_rng(5))
    sets["special"] = H.special_queries(case.st, p)
    del sets["boundaries"]                                            # part of the special set
    sets["uniform"] = H.uniform_queries(case.st)
    if not uniform:
        del sets["uniform"]
    for name, pts in sets.items():
        got = assert_samples_equal(sim, chk, pts, attr, f"{ctx} {name}")
        if name == "own":
            assert np.array_equal(got["cell"], p["grid"]), f"{ctx}: cell of a particle's own position"
            if ieee:
                d = np.maximum(np.maximum(got["density"], EPSILON_F), np.float32(0.1))
                assert np.array_equal(d.view(np.uint32), p["density"].view(np.uint32)), f"{ctx}: density identity"
        if name == "uniform":
            assert got["neighbours"].any() and not got["neighbours"].all(), f"{ctx}: the random set must hit the fluid and miss it"
        if name == "special":
            cell = H.query_cells(case.st, pts)
            gw = sim.grid_dims[0]
            assert np.array_equal(got["cell"], ((cell[:, 1] * gw + cell[:, 0]) & 0xFFFFFFFF).astype(np.uint32)), f"{ctx}: wrapping cell id"
    chk.close()
    return p, attr


# ---- 1. every case that stays finite, after one step and after the case's steps ------------------------------------------------
@pytest.mark.parametrize("cid", SAMPLED_IDS)
def test_sampler_at_the_hard_inputs(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    assert case.stays_finite, case.describe()
    sim = engine(fs, case)
    done = 0
    for steps in (1, case.steps):
        while done < steps:
            sim.tick(case.tick)
            done += 1
        p, _ = check_sets(fs, sim, case, True, f"{cid} steps={steps}")
        assert p.tobytes() == case.run()[steps - 1].rec.tobytes(), f"{cid}: the sampled state is not the oracle's after {steps} steps"
    sim.close()


# ---- 2. the three density sources -----------------------------------------------------------------------------------------------
SOURCES = {"rcp": dict(mass=1.0, mode="FS_MATH_IEEE"), "rho2x": dict(mass=1.25, mode="FS_MATH_IEEE"),
           "rho": dict(mass=1.0, mode="FS_MATH_TOLERANCE")}


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("cid", ["corners/quirks/bitonic", "corners/noquirks/counting", "one_cell/bitonic", "one_cell/counting"])
def test_density_sources(fs, orc, cid, source):
    """m / rho_k is |rho2[k].y| (the reciprocal the IEEE density pass keeps; mass 1 only), m / rho2[k].x (IEEE, another mass) or
    m / rho[k] (FS_MATH_TOLERANCE keeps its densities in an array of their own) — on row ranges at the ends of the cell table
    and on a row of 256 candidates.  The checker is loaded from the download in each; FS_MATH_TOLERANCE has no density
    identity."""
    from tests.features2d import copy_tick
    case = H.case_by_id(fs, orc, cid)
    src = SOURCES[source]
    tick = copy_tick(case.tick, mass=src["mass"])
    sim = engine(fs, case, math_mode=getattr(fs, src["mode"]))
    done = 0
    for steps in (1, case.steps):
        while done < steps:
            sim.tick(tick)
            done += 1
        assert float(np.float32(sim.uniform().particle_mass)) == src["mass"]
        check_sets(fs, sim, case, src["mode"] == "FS_MATH_IEEE", f"{cid} {source} steps={steps}")
    sim.close()


# ---- 3. channels on the tie cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("cid", H.TIE_CASE_IDS)
def test_channels_on_the_tie_cases(fs, orc, cid, channels):
    """A channel that followed the wrong arrangement of equal keys shows in the channel sums: the ids are those of the tracking
    checker (hard_states2d.Case.ids), the channels are the uploaded values at those ids, and the sums — over values with +-0.0,
    denormals and 1e30 — are the checker's bytes."""
    case = H.case_by_id(fs, orc, cid)
    assert case.tie_case and case.stays_finite
    sim = engine(fs, case, track=channels)
    vals = H.sample_channel_values(case.n, channels)
    for c in range(channels):
        sim.set_attribute(c, vals[c])
    ids = case.ids()
    for s in range(case.steps):
        sim.tick(case.tick)
        if s in (0, case.steps - 1):
            assert np.array_equal(sim.particle_ids(), ids[s]), f"{cid} C={channels} step {s}: ids"
            _, attr = check_sets(fs, sim, case, True, f"{cid} C={channels} step {s}", uniform=False)
            assert attr.view(np.uint32).tobytes() == vals[:, ids[s]].view(np.uint32).tobytes(), f"{cid} C={channels} step {s}: channels"
    sim.close()


# ---- 4. the grid form on ragged views -------------------------------------------------------------------------------------------
VIEW_SIZES = [(1, 1), (15, 17), (16, 16), (33, 1)]


@pytest.mark.parametrize("framing", ["inside", "straddling", "outside"])
def test_grid_views(fs, orc, framing):
    """Views of 1 x 1, 15 x 17, 16 x 16 and 33 x 1 pixels (k_sample takes a grid in 16 x 16 tiles) on the corners scene: inside
    the box, straddling its (+x, +y) corner — where the coincident cluster of the last cell sits — and wholly outside, from just
    past that corner on.  sample_grid is sample() on the pixel centres and the checker's grid."""
    from tests.sample_ref import grid_points
    case = H.case_by_id(fs, orc, "corners/quirks/bitonic")
    sx, sy = S.CORNER_BOX
    wmin, wmax = {"inside": ((-sx / 4, -sy / 4), (sx / 4, sy / 4)),
                  "straddling": ((sx / 2 - 1.0, sy / 2 - 1.0), (sx / 2 + 1.0, sy / 2 + 1.0)),
                  "outside": ((sx / 2 + 0.05, sy / 2 + 0.05), (sx / 2 + 1.5, sy / 2 + 1.5))}[framing]
    sim = engine(fs, case, track=2)
    vals = H.sample_channel_values(case.n, 2)
    for c in range(2):
        sim.set_attribute(c, vals[c])
    for _ in range(case.steps):
        sim.tick(case.tick)
    chk, _, attr = load_checker(fs, sim, case.st, case.off, case.quirks)
    hit = 0
    for (w, h) in VIEW_SIZES:
        g, ga = sim.sample_grid(w, h, wmin, wmax, attributes=True)
        q, qa = sim.sample(grid_points(w, h, wmin, wmax), attributes=True)
        assert g.shape == (h, w) and ga.shape == (2, h, w)
        assert g.tobytes() == q.tobytes() and ga.tobytes() == qa.tobytes(), f"{framing} {w}x{h}: grid != points"
        want, wa = chk.sample_grid(w, h, wmin, wmax, attr)
        assert g.tobytes() == want.tobytes() and ga.tobytes() == wa.tobytes(), f"{framing} {w}x{h}: grid != checker"
        hit += int(g["neighbours"].any())
    assert hit >= 2, f"{framing}: the views must see the fluid"
    chk.close(); sim.close()

"""The 3D surface-tension statement on the CPU (include/fluidsim.h "3D surface tension"): the checker's restated
step is the oracle's when the feature is off, the formulas are the gradient and the Laplacian of the 3D poly6 kernel, the
checker's f32 pass is the f64 sum within the bound of an f32 sum, and the constants the models share with the kernel are read
from the sources.  No GPU."""
import re

import numpy as np
import pytest

import paths3d
from tests import features3d as F
from tests import st3d_ref as R

f32 = np.float32
# the statement's constants as this file's float64 model uses them; test_constants_match_the_sources reads them from the sources
GRAD_C, LAP_R2, LAP_H2 = 6.0, 7.0, 3.0
SCENE_ST = F.SCENE_ST               # (sigma, tau) of the path scenes, shared with test_surface_tension3d_gpu.py


def _same_records(a, b, ctx):
    for name in ("position", "predicted_position", "velocity", "density", "grid"):
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.tobytes() == y.tobytes(), f"{ctx}: {name} differs"


# ---- 1. the restatement is the oracle's step ----------------------------------------------------------------------------
def test_checker_step_without_the_feature_is_the_oracle_dam_break(fs, orc):
    st, off, tick = fs.dam_break_3d(16 ** 3)
    ref, chk = orc.OracleSim3D(st, off), R.ST3Checker(st, off)
    for s in range(10):
        ref.step(tick); chk.step(tick, None)
        _same_records(chk.particles(), ref.particles(), f"dam_break_3d(16^3) step {s + 1}")
    ref.close(); chk.close()


@pytest.mark.parametrize("name", ["row65", "coincident_chunked", "extent401"])
def test_checker_step_without_the_feature_is_the_oracle_path_scenes(fs, orc, name):
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    ref, chk = orc.OracleSim3D(st), R.ST3Checker(st)
    ref.set_particles(p); chk.set_particles(p)
    for s in range(scene.steps):
        ref.step(tick); chk.step(tick, None)
        _same_records(chk.particles(), ref.particles(), f"{name} step {s + 1}")
    ref.close(); chk.close()


@pytest.mark.parametrize("name", sorted(paths3d.scenes()))
def test_path_scenes_keep_their_paths_with_surface_tension(fs, name):
    """the GPU test runs every path scene with SCENE_ST: on the checker alone, the scene still reaches the sweep it is named after
    at every compared step, stays finite, and surface tension acts (some particle takes the upper branch)"""
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    chk = R.ST3Checker(st)
    chk.set_particles(p)
    acted = False
    for s in range(scene.steps):
        chk.step(tick, SCENE_ST)
        state = chk.particles()
        paths3d.check_scene(scene, [state], chk.grid_dims)
        assert np.isfinite(state["position"]).all() and np.isfinite(state["velocity"]).all() and np.isfinite(chk.st).all()
        acted |= bool(np.any(chk.st != 0))
    assert acted
    chk.close()


# ---- 2. the formulas, in float64 ----------------------------------------------------------------------------------------
H64 = 0.2
C64 = 315.0 / (64.0 * np.pi * H64 ** 9)


def _W(x):
    """poly6 in 3D at the points x [..., 3]"""
    r2 = (x * x).sum(-1)
    return np.where(r2 <= H64 * H64, C64 * np.maximum(H64 * H64 - r2, 0.0) ** 3, 0.0)


def _grad_model(x):
    """grad W at x as the statement writes it: 6C d^2 (q_j - x) with q_j the origin"""
    r2 = (x * x).sum(-1)
    d = H64 * H64 - r2
    return ((GRAD_C * C64) * d * d)[..., None] * (0.0 - x)


def _lap_model(r2):
    d = H64 * H64 - r2
    return (GRAD_C * C64) * d * (LAP_R2 * r2 - LAP_H2 * H64 * H64)


def _radial_integral(g, m=200001):
    """int_0^h 4 pi r^2 g(r^2) dr by Simpson's rule (the integrands are polynomials of degree <= 8)"""
    r = np.linspace(0.0, H64, m)
    y = 4.0 * np.pi * r * r * g(r * r)
    w = np.ones(m); w[1:-1:2] = 4.0; w[2:-1:2] = 2.0
    return float((w * y).sum() * (r[1] - r[0]) / 3.0)


def test_kernel_integrates_to_one_and_its_laplacian_to_zero():
    one = _radial_integral(lambda r2: C64 * (H64 * H64 - r2) ** 3)
    np.testing.assert_allclose(one, 1.0, rtol=1e-6)
    # the two signed parts of the Laplacian cancel: compare their sum with their size
    pos = _radial_integral(lambda r2: np.maximum(_lap_model(r2), 0.0))
    neg = _radial_integral(lambda r2: np.minimum(_lap_model(r2), 0.0))
    assert pos > 0 and neg < 0
    assert abs(pos + neg) <= 1e-6 * pos


def _points(count, seed):
    """random points with 0.05 h <= r <= 0.9 h: the 4th-order stencils below stay inside the support"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((count, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * (rng.uniform(0.05, 0.9, size=(count, 1)) * H64)


def test_gradient_is_the_finite_difference_of_the_kernel():
    x = _points(400, 1)
    e = 1e-3 * H64
    fd = np.zeros_like(x)
    for a in range(3):
        u = np.zeros(3); u[a] = e
        fd[:, a] = (-_W(x + 2 * u) + 8 * _W(x + u) - 8 * _W(x - u) + _W(x - 2 * u)) / (12 * e)    # error O(e^4)
    g = _grad_model(x)
    err = np.linalg.norm(fd - g, axis=1)
    assert (err <= 1e-6 * np.linalg.norm(g, axis=1)).all(), float((err / np.linalg.norm(g, axis=1)).max())


def test_laplacian_is_the_finite_difference_of_the_kernel():
    """rtol 1e-6 of the value; the points keep |7 r^2 - 3 h^2| >= 0.2 h^2, away from the Laplacian's zero where no relative bound
    can hold for a difference quotient"""
    x = _points(2000, 2)
    r2 = (x * x).sum(-1)
    x = x[np.abs(LAP_R2 * r2 - LAP_H2 * H64 * H64) >= 0.2 * H64 * H64][:400]
    assert x.shape[0] == 400
    e = 2e-3 * H64
    fd = np.zeros(x.shape[0])
    for a in range(3):
        u = np.zeros(3); u[a] = e
        fd += (-_W(x + 2 * u) + 16 * _W(x + u) - 30 * _W(x) + 16 * _W(x - u) - _W(x - 2 * u)) / (12 * e * e)
    np.testing.assert_allclose(fd, _lap_model((x * x).sum(-1)), rtol=1e-6)


# ---- 3. the checker's f32 pass against a float64 sum over all pairs -------------------------------------------------------
def _pass_against_float64(chk, rec, mass, h):
    """the checker's n and L on the state its last step left against the float64 sum over all pairs, per particle under the bound
    of an f32 sum of K terms, (K + 8) 2^-24 sum|term|: (n, L, worst error as a share of the bound).  The f64 sum takes the f32
    inputs and the f32 constants (Cg, h2, 3 h2) as they are.  The state must be finite."""
    n = rec.shape[0]
    assert np.isfinite(rec["predicted_position"]).all() and np.isfinite(rec["density"]).all()
    poly6 = f32(chk.constants()[0])
    cg, h2 = f32(GRAD_C) * poly6, f32(h) * f32(h)
    h2x3 = f32(LAP_H2) * h2
    nv, Lv, _ = chk.surface_tension_pass(1.0, 0.0)
    q = rec["predicted_position"].astype(np.float64)
    w = float(f32(mass)) / rec["density"].astype(np.float64)
    u = 2.0 ** -24
    worst = 0.0
    for i in range(n):
        o = q - q[i]
        r2 = (o * o).sum(1)
        near = r2 <= float(h2)
        o, r2, wj = o[near], r2[near], w[near]
        d = float(h2) - r2
        tn = (wj * (float(cg) * d * d))[:, None] * o
        tl = wj * (float(cg) * d * (LAP_R2 * r2 - float(h2x3)))
        K = int(near.sum())
        assert K >= 1
        bound_n = (K + 8) * u * np.abs(tn).sum(0)
        bound_l = (K + 8) * u * np.abs(tl).sum()
        en, el = np.abs(nv[i].astype(np.float64) - tn.sum(0)), abs(float(Lv[i]) - tl.sum())
        assert (en <= bound_n).all() and el <= bound_l, (i, K, en, bound_n, el, bound_l)
        worst = max(worst, float((en / np.maximum(bound_n, 1e-300)).max()), el / max(bound_l, 1e-300))
    return nv, Lv, worst


def test_checker_pass_against_float64_sum_over_all_pairs(fs):
    """13^3 = 2197 random particles in a 1.6^3 box, h = 0.2 (about 18 in radius).  Per component of n and for L:
    |f32 - f64| <= (K + 8) 2^-24 sum|term|, K = the particle's in-radius count: K - 1 roundings of the running sum and at most
    eight of a term (o, the three products and two sums of r2, d, w, k or lk, the products) — the bound of an f32 sum of K terms,
    not a measured figure.  The f64 sum takes the f32 inputs and the f32 constants (Cg, h2, 3 h2) as they are."""
    n = 13 ** 3
    h, size = 0.2, 1.6
    st = fs.Settings3(n, 0.1, h, fs.Vec3(size, size, size))
    tick = fs.TickSettings3(float(f32(1) / f32(120)), fs.Vec3(0.0, 0.0, 0.0), 1.0, 0.0, 0.0, 0.1, 0.0)
    rng = np.random.default_rng(42)
    chk = R.ST3Checker(st)
    p = chk.particles()
    p["position"] = rng.uniform(-0.79, 0.79, size=(n, 3)).astype(f32)
    p["predicted_position"] = p["position"]
    p["velocity"] = 0
    chk.set_particles(p)
    chk.step(tick, None)                                   # sorts, leaves this state's densities (nothing moves: no force, no speed)
    rec = chk.particles()
    assert np.array_equal(np.sort(rec["predicted_position"], axis=0), np.sort(p["position"], axis=0))
    nv, Lv, worst = _pass_against_float64(chk, rec, tick.mass, h)
    print(f"[st3d] f32 pass against f64: worst error {worst:.3f} of the bound")
    # the threshold: both branches, and st is the statement's closed form of the checker's own n and L
    nl = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
    sigma, tau = f32(0.7), f32(np.median(nl))
    _, _, stv = chk.surface_tension_pass(sigma, tau)
    upper = (nl > tau) & (nl > 0)
    assert upper.sum() >= n // 4 and (~upper).sum() >= n // 4
    with np.errstate(all="ignore"):
        sc = (-sigma * Lv) / nl
    want = np.where(upper[:, None], sc[:, None] * nv, f32(0)).astype(f32)
    assert want.tobytes() == stv.tobytes()
    chk.close()


# ---- 4. the hard-input cases of test_3d_features_hard_inputs_gpu.py, on the checker alone ---------------------------------
NO_FORCE_IN_STEP_1 = ("guard/nan_next_to_everyone/st", "guard/nan_next_to_everyone/st+collide")
# SCENE_ST's threshold is fixed (0.5, shared with the IEEE scene tests): in this scene the over-full cells leave only two of the 174
# particles with a colour gradient at or below it.  Both branches are still taken; the 1 % rule cannot be met.
TOL_UNDER_ONE_PERCENT = ("tol/mixed_wave",)


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_hard_input_cases_exercise_the_pass(fs, orc, cid):
    """what the GPU file relies on, asked of the checker alone: no case is empty, the pass produces a force, both branches of the
    threshold are taken, and where at least 100 particles have a colour gradient the threshold leaves at least 1 % of the
    particles on each side (tau is chosen for that; the tolerance cases keep SCENE_ST's fixed tau and meet it too, except
    TOL_UNDER_ONE_PERCENT).  In the tolerance cases the threshold must also sit in a gap of the |n| values (1e-3 relative, a
    hundred times the mode's density contract), so that no particle changes its branch.  The exception of NO_FORCE_IN_STEP_1:
    every |n| of its first step is a NaN, which takes the not-above branch (all of step 1), and with tau = 0 every
    particle of steps 2 and 3 takes the other."""
    case = F.case_by_id(fs, orc, cid)
    run = case.run()
    print(F.describe(case))
    fig = case.figures
    assert len(run) == case.steps >= 1 and fig["n"] == case.start.shape[0] >= 8
    assert np.isfinite(case.sigma) and case.sigma > 0 and np.isfinite(case.tau)
    forces = [bool(np.any(st != 0)) for _, st in run]
    if cid in NO_FORCE_IN_STEP_1:       # every |n| is a NaN in step 1 (see features3d._nan_next_to_everyone): admitted, so no force
        assert not forces[0] and all(forces[1:]) and np.all(run[0][0]["density"] == f32(0.1))
        return
    assert forces[0], "the pass produced no force in step 1"
    assert fig["above"] > 0 and fig["below"] > 0, fig
    if fig["with_n"] >= 100 and cid not in TOL_UNDER_ONE_PERCENT:
        assert fig["above"] >= fig["n"] / 100 and fig["below"] >= fig["n"] / 100, fig
    if cid.startswith("tol/"):
        assert fig["tau_gap"] > 1e-3 and (fig["sensitivity"] <= 1.0 or fig["st_dv_max"] < 1.0), fig
        return
    # sigma puts the pass at the order of the step's own velocity change, wherever that is finite
    if fig["own_dv"] > 0:
        assert 0.1 <= fig["st_dv"] / fig["own_dv"] <= 10.0, fig


def test_nan_and_infinite_operands_reach_the_pass(fs, orc):
    """inf_velocity, huge_pressure and unsafe_next_to_safe carry NaN predicted positions into the pass, mass_tiny holds every
    density at the floor in step 1, density_across_2p20 has densities on both sides of 2^20"""
    for name in ("inf_velocity", "huge_pressure", "unsafe_next_to_safe"):
        run = F.guard_case(fs, orc, name, "st+collide").run()
        assert any(np.isnan(rec["predicted_position"]).any() for rec, _ in run), name
    rec = F.guard_case(fs, orc, "mass_tiny", "st").run()[0][0]
    case = F.guard_case(fs, orc, "mass_tiny", "st")
    assert np.all(rec["density"] == f32(0.1)) and 0 < f32(case.tick.mass) / f32(0.1) < 1e-2
    rec = F.guard_case(fs, orc, "density_across_2p20", "st").run()[0][0]
    assert rec["density"].min() < 2 ** 20 < rec["density"].max()


@pytest.mark.parametrize("name", ["density_across_2p20", "mass_tiny"])
def test_checker_pass_against_float64_at_extreme_mass_over_density(fs, orc, name):
    """the same float64 evaluation at m / rho = 1500 / (5e5 .. 2e6) and at m / 0.1 with m ~ 4e-5: a mistake in the weight that
    checker and kernel share (1 / rho for m / rho: a factor 1500, or 4e-5) cannot pass"""
    case = F.guard_case(fs, orc, name, "st")
    chk = case.checker()
    chk.step(case.tick, None)
    rec = chk.particles()
    _, _, worst = _pass_against_float64(chk, rec, case.tick.mass, case.h)
    print(f"[st3d] {name}: f32 pass against f64: worst error {worst:.3f} of the bound")
    chk.close()


# ---- 5. source pins -------------------------------------------------------------------------------------------------------
def _header_text():
    import os
    with open(os.path.join(os.path.dirname(paths3d.__file__), "..", "include", "fluidsim.h")) as fh:
        return fh.read()


def test_constants_match_the_sources():
    k3d = paths3d.source_text("kernels_density3d.hip")
    eng = paths3d.source_text("engine_3d.h")
    with open(R.SOURCES[0]) as fh:
        chk = fh.read()
    num = r"([0-9]+\.[0-9]+)f"
    # the Laplacian's 7 r^2 - 3 h^2: the kernel takes 3 h^2 from the host
    m = re.search(num + r" \* r2\) - T\.h2x3", k3d)
    assert m and float(m.group(1)) == LAP_R2
    m = re.search(r"const Tension3 T\{P\.h2, " + num + r" \* P\.poly6, " + num + r" \* P\.h2,", eng)
    assert m and float(m.group(1)) == GRAD_C and float(m.group(2)) == LAP_H2
    # the checker restates the same three
    m = re.search(r"const float cg = " + num + r" \* s\.poly6;", chk)
    assert m and float(m.group(1)) == GRAD_C
    m = re.search(r"const float h2x3 = " + num + r" \* h2;", chk)
    assert m and float(m.group(1)) == LAP_H2
    m = re.search(num + r" \* r2\) - h2x3", chk)
    assert m and float(m.group(1)) == LAP_R2
    # ... and the header states them
    hdr = _header_text()
    assert "Cg = 6.0f * poly6" in hdr and "((7.0f * r2) - h2x3)" in hdr and "h2x3 = 3.0f * h2" in hdr
    # the kernel shares k3_density's block size and tile, and asks the same plane classes
    body = k3d[k3d.index("void k3_surface_tension("):]
    body = body[:body.index("\n}\n")]
    assert "__launch_bounds__(B3F) void k3_surface_tension(" in k3d
    # ... by construction: block mapping, row look-up, tile bounds and plane classes are the plane driver's (fs_sweep3.h; pinned
    # there by test_3d_paths.py), and the plane walk is k3_density's with other terms
    assert "sweep3_lane(" in body and "sweep3_planes(" in body and "PlaneTerms3<TensionPass>" in body
    assert "PlaneTerms3<DensityPass<MODE>>" in k3d and "block_tile_bounds" not in k3d and "plane_class(R" not in k3d
    assert "atomic" not in body

"""CPU tests of the opt-in diffusion and buoyancy of the tracking channels of the 3D step: the restated step with
nothing set against st3_step and orc3_step, the formulas in float64, the checker (tests/diffuse3d_checker.cpp through
tests/diffuse3d_ref.py) against a float64 restatement, conservation, the maximum principle, that the scenes
tests/test_diffusion3d_gpu.py runs are not vacuous and reach every sweep path, and the layers of the bindings.  No GPU.

Rounding bounds, as in DESIGN.md §27: u = 2^-24.  A term w ((Cg d) d) (A_j - A_i) carries five roundings (the quotient w, three
products, the difference), a sum of K terms adds at most K - 1 more per term, and the tail adds three (g acc, the product with
u_i, u_i itself): (K + 8) u on sum |term| to first order, and one more u on |A'| for the final addition.  K counts the candidates
in the radius: a skipped candidate adds exactly +0.  The float64 restatement takes q, r2 and d as the f32 values the statement
forms, so the bound covers everything the two sides do differently."""
import ctypes as C

import numpy as np
import pytest

import paths3d
from tests import diffuse3d_cases as DC
from tests import diffuse3d_ref as DR
from tests import st3d_ref
from tests import track3d_ref as TR

f32 = np.float32
U = 2.0 ** -24
SLACK = 1.01                        # the second-order terms of the first-order bounds


# ---- nothing set: the oracle's step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dam16"] + sorted(paths3d.scenes()))
def test_nothing_set_is_the_oracles_step(fs, orc, name):
    """the restated step with no conductivity and no buoyancy channel: byte-equal to st3_step with enable = 0 and to orc3_step"""
    st, tick, p, steps = DC.scene_state(fs, name)
    chk = DR.Diffuse3Checker(st, channels=2)
    ref = st3d_ref.ST3Checker(st)
    o = orc.OracleSim3D(st)
    for s in (chk, ref, o):
        s.set_particles(p)
    chk.attr[0] = np.arange(chk.n, dtype=f32)
    for k in range(max(steps, 3)):
        chk.step(tick); ref.step(tick); o.step(tick)
        assert chk.particles_view().tobytes() == ref.particles_view().tobytes(), f"{name}: step {k + 1} differs from st3_step"
        assert chk.particles_view().tobytes() == o.particles_view().tobytes(), f"{name}: step {k + 1} differs from orc3_step"
        assert chk.fb is None and chk.st is None
    assert sorted(chk.attr[0].tolist()) == list(range(chk.n))           # the carry alone moved the channel
    for s in (chk, ref, o):
        s.close()


# ---- float64 checks of the formulas ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.05, 0.2, 1.0])
def test_weight_integrals(h):
    """int r^2 Cg (h^2 - r^2)^2 dV = 3 and int Cg (h^2 - r^2)^2 dV = 9 / h^2 with Cg = 6 * 315 / (64 pi h^9), by the midpoint rule
    in r (error O(1/M^2))"""
    M = 200_000
    r = (np.arange(M) + 0.5) * (h / M)
    k = 6.0 * 315.0 / (64.0 * np.pi * h ** 9) * (h * h - r * r) ** 2 * 4.0 * np.pi * r * r * (h / M)
    assert abs((k * r * r).sum() / 3.0 - 1.0) < 1e-6
    assert abs(k.sum() * h * h / 9.0 - 1.0) < 1e-6


def lattice_sum(A, spacing_per_h, seed=3):
    """2 sum_j (m / rho_j) Cg d^2 (A_j - A_i) in float64 at the interior particles of a jittered lattice (h = 1, jitter 0.1 of the
    spacing, SPH poly6 densities) for A given as a function of (x, y, z): the values at the particles with |q| < 1 on every axis
    (their neighbours' neighbourhoods are full: the lattice fills [-3, 3]^3)"""
    from scipy.spatial import cKDTree
    h, s = 1.0, 1.0 / spacing_per_h
    side = int(round(6.0 / s))
    g = (np.arange(side) + 0.5) * s - 3.0
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = q + np.random.default_rng(seed).uniform(-0.1 * s, 0.1 * s, q.shape)
    keep = (np.abs(q) < 2.05).all(1)                                   # rho is needed (and right) within reach of the interior only
    tree = cKDTree(q)
    rows = np.flatnonzero(keep)
    nb = tree.query_ball_point(q[rows], h)
    i = np.repeat(rows, [len(x) for x in nb])
    j = np.concatenate([np.asarray(x, dtype=np.int64) for x in nb])
    o = q[j] - q[i]
    d = h * h - (o * o).sum(1)
    n = q.shape[0]
    cg, poly6 = 6.0 * 315.0 / (64.0 * np.pi), 315.0 / (64.0 * np.pi)
    rho = np.bincount(i, poly6 * d ** 3, n)                            # m = 1
    a = A(q[:, 0], q[:, 1], q[:, 2])
    inner = (np.abs(q) < 1.0).all(1)
    m = inner[i]
    lap = 2.0 * np.bincount(i[m], (1.0 / rho[j[m]]) * cg * d[m] * d[m] * (a[j[m]] - a[i[m]]), n)
    return lap[inner]


def test_the_sum_approaches_the_laplacian():
    """A = x^2 - y^2 (harmonic: 0) and A = x^2 (2), worst interior particle, at spacings h / 2 and h / 4: halving the spacing at
    least halves the error.  No threshold is fixed in advance; the measured values are in DESIGN.md §28."""
    err = {}
    for k in (2, 4):
        harm = lattice_sum(lambda x, y, z: x * x - y * y, k)
        quad = lattice_sum(lambda x, y, z: x * x, k)
        err[k] = (float(np.abs(harm).max()), float(np.abs(quad - 2.0).max()))
        print(f"[laplacian3d] s = h/{k}: max |sum| for x^2 - y^2 {err[k][0]:.4g}, max |sum - 2| for x^2 {err[k][1]:.4g}")
    assert err[4][0] <= err[2][0] / 2 and err[4][1] <= err[2][1] / 2


def test_diffusion_limit(fs):
    st, _, tick = fs.dam_break_3d(4096)
    want = 30.0 * 0.2 * 0.2 / (18.0 * float(tick.delta))
    assert abs(fs.FluidSimulation3D.diffusion_limit(st, tick, 30.0) / want - 1.0) < 1e-6
    assert isinstance(fs.FluidSimulation3D.__dict__["diffusion_limit"], staticmethod)


# ---- the checker against a float64 restatement ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dam(fs):
    """the jittered 16^3 dam break after two plain steps, then one step with two diffusing channels (x, and a constant) at
    g R = 1/2 at the slot where R is largest: (checker, tick, A before the pass, kappa)"""
    st, tick, p, _ = DC.scene_state(fs, "dam16")
    chk = DR.Diffuse3Checker(st, channels=2)
    chk.set_particles(p)
    for _ in range(2):
        chk.step(tick)
    chk.attr[0] = chk.particles()["position"][:, 0]
    chk.attr[1] = 1.5
    probe = DC.pass_of_next_step(chk, tick)                              # R of the step to come, on a scratch copy
    kappa = DC.kappa_for(probe["R"], float(tick.delta), 0.5)
    chk.kappa[0] = chk.kappa[1] = kappa
    chk.step(tick)
    return chk, tick, probe["attr"], kappa


def _bounds(dam):
    chk, tick, before, kappa = dam
    g = float((f32(2.0) * f32(kappa)) * f32(tick.delta))
    want, tabs, K, R = DC.restatement(chk, chk.particles(), before[0], tick.mass, g)
    return g, want, tabs, K, R, SLACK * U * (np.abs(want) + (K + 8) * tabs)


def test_checker_against_the_float64_restatement(dam):
    chk, tick, before, kappa = dam
    g, want, tabs, K, R, bound = _bounds(dam)
    share = np.abs(chk.attr[0].astype(np.float64) - want) / bound
    print(f"[restatement3d] worst share of the rounding bound {share.max():.3f}; K up to {K.max()}; g R up to {(g * R).max():.3f}")
    assert (share <= 1.0).all()
    assert np.allclose(R, chk.R, rtol=1e-5)                             # the checker's R is the restatement's (f32 weights, f64 sum)
    assert (np.abs(chk.acc[0]) > 0).mean() > 0.5


def test_conservation(dam):
    """sum_i A_i is conserved in exact arithmetic (the weight is symmetric in i and j, the neighbour relation of the 3D oracle
    is symmetric, the masses are equal; the term carries w_j inside and u_i outside the sum, so in f32 only to rounding).
    Asserted: the float64 restatement conserves sum A to its own rounding; the f32 checker's drift stays inside the sum of the
    per-slot rounding bounds; a constant channel is a fixed point bit for bit (every difference is +0)."""
    chk, tick, before, kappa = dam
    g, want, tabs, K, R, bound = _bounds(dam)
    a0 = before[0].astype(np.float64)
    # the restatement weighs with u_i w_j = m / (rho_i rho_j): symmetric, so its sum moves by float64 rounding only
    assert abs(want.sum() - a0.sum()) <= 64 * 2.0 ** -53 * (np.abs(a0).sum() + tabs.sum())
    drift = abs(chk.attr[0].astype(np.float64).sum() - a0.sum())
    print(f"[conservation3d] f32 drift of sum A {drift:.3e}, bound {bound.sum():.3e} (sum |A| {np.abs(a0).sum():.3e})")
    assert drift <= bound.sum()
    assert np.array_equal(chk.attr[1].view(np.uint32), before[1].view(np.uint32))
    assert not chk.acc[1].view(np.uint32).any()


def test_max_principle(dam):
    """g R_i <= 1 at every slot makes A'_i a convex combination of A_i and its neighbours' values in exact arithmetic; in f32 it
    may leave [min A, max A] by the per-slot rounding bound at most."""
    chk, tick, before, kappa = dam
    g, want, tabs, K, R, bound = _bounds(dam)
    assert (g * chk.R <= 1.0).all()
    a = chk.attr[0].astype(np.float64)
    lo, hi = float(before[0].min()), float(before[0].max())
    assert (a >= lo - bound).all() and (a <= hi + bound).all()
    assert (want >= lo - 1e-12 * max(abs(lo), abs(hi))).all() and (want <= hi + 1e-12 * max(abs(lo), abs(hi))).all()


# ---- the GPU file's scenes are not vacuous and reach every path ---------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.NONVACUOUS)
def test_scenes_are_not_vacuous(fs, name):
    """kappa from the checker alone (g R = 1/2 where R is largest): the channel moves on more than half of the slots and both
    signs of s occur.  The path scenes are a feature among background particles that are alone within h by construction
    (tests/paths3d.py: one per cell at most, in every other cell): there the share is taken over the slots that have a
    neighbour, and the share over all slots is printed."""
    run = DC.planned_run(fs, name)
    print(f"[diffuse3d_cases] {name}: n {run.n}, kappa {run.kappa:.4g}, moving share {run.moved_all:.3f} of all slots, "
          f"{run.moved_paired:.3f} of the {run.paired} slots with a neighbour, s > 0 {run.s_pos}, s < 0 {run.s_neg}")
    assert run.n >= 64
    if name in paths3d.scenes():
        assert run.paired >= 60 and run.moved_paired > 0.5
    else:
        assert run.moved_all > 0.5
    assert run.s_pos > 0 and run.s_neg > 0


def test_every_path_is_reached(fs):
    """each of the four sweeps of fs_sweep3.h carries a wave-plane of some scene, per the CPU model fed the checker's keys"""
    seen = dict.fromkeys(paths3d.PATHS, 0)
    for name, scene in sorted(paths3d.scenes().items()):
        st, tick, p, steps = DC.scene_state(fs, name)
        chk = DR.Diffuse3Checker(st, channels=1)
        chk.set_particles(p)
        chk.kappa[0] = 0.01
        chk.step(tick)
        m = paths3d.PathModel(chk.particles_view()["grid"], chk.grid_dims)
        for path in paths3d.PATHS:
            seen[path] += m.count(path)
        chk.close()
    print(f"[paths3d] wave-planes per path over the scenes: {seen}")
    assert all(seen[p] > 0 for p in paths3d.PATHS), seen


@pytest.mark.parametrize("name", sorted(paths3d.scenes()))
def test_path_scenes_hold_their_paths_under_the_gpu_plan(fs, name):
    """the plan tests/test_diffusion3d_gpu.py runs a path scene with (DC.scene_plan) leaves every particle in its cell for the
    compared steps: the asserted row lengths and block extents hold after every step"""
    scene = paths3d.scenes()[name]
    st, tick, p, _ = DC.scene_state(fs, name)
    chk = DR.Diffuse3Checker(st, channels=4)
    chk.set_particles(p)
    chk.attr[:] = DC.fill_channels(p, 4)
    subset, buoy = DC.scene_plan(name)
    k = DC.kappa_for(DC.pass_of_next_step(chk, tick)["R"], tick.delta, 0.5)
    for c in subset:
        chk.kappa[c] = k
    chk.buoyancy = buoy
    for _ in range(DC.SCENE_STEPS):
        chk.step(tick)
        paths3d.check_scene(scene, [chk.particles()], chk.grid_dims)
    chk.close()


def test_kernel_constants_are_the_models():
    text = paths3d.source_text("kernels_diffuse3d.hip")
    for word in ("sweep3_lane", "sweep3_planes", "masks3_plane", "masks3_row128", "xcd_grid3", "TILE3_LDS + 64", "__fdiv_rn(P.mass, c.w)"):
        assert word in text, word
    assert int(paths3d.parse_define(paths3d.source_text("fs_sweep3.h"), "TILE3")) == paths3d.TILE3


# ---- layers, prototypes, refusals without a device --------------------------------------------------------------------------------
CALLS = ["fs3_set_diffusion", "fs3_get_diffusion", "fs3_set_buoyancy", "fs3_get_buoyancy", "fs3_download_buoyancy"]


def test_every_layer_names_every_call(fs):
    from tests.layers import assert_every_layer_names, header_text
    assert_every_layer_names(fs, CALLS, fs.FluidSimulation3D, (
        "set_diffusion", "diffusion", "set_buoyancy", "clear_buoyancy", "buoyancy", "buoyancy_forces", "diffusion_limit"))
    head = header_text()
    for name in CALLS:
        assert head.index(name) > head.index("fs3_download_particles_by_id"), f"{name}: the section follows the 3D tracking calls"
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "rho0 h^2 / 18" in open(os.path.join(root, "include", "fluidsim.h")).read()
    assert "\n## 28." in open(os.path.join(root, "DESIGN.md")).read()


def test_null_handle_is_invalid_without_a_device(fs):
    lib = fs.load_library()
    inv = fs._abi.FS_ERR_INVALID
    k, c, buf = C.c_float(), C.c_int(), (C.c_float * 12)()
    assert lib.fs3_set_diffusion(None, 0, 1.0) == inv
    assert b"null" in lib.fs_last_error()
    assert lib.fs3_get_diffusion(None, 0, C.byref(k)) == inv
    assert lib.fs3_set_buoyancy(None, 0, 1.0, 0.0) == inv
    assert lib.fs3_get_buoyancy(None, C.byref(c), C.byref(k), C.byref(k)) == inv
    assert lib.fs3_download_buoyancy(None, buf, 4) == inv
    assert b"null" in lib.fs_last_error()

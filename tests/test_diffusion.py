"""CPU tests of the opt-in diffusion and buoyancy of the tracking channels: the formulas in float64, the checker
(tests/diffuse_checker.cpp through tests/diffuse_ref.py) against a float64 restatement, conservation, the maximum principle, that
the cases tests/test_diffusion_gpu.py runs are not vacuous, and the layers of the bindings.  No GPU.

Rounding bounds, as in DESIGN.md §11: u = 2^-24.  A term w ((Cg d) d) (A_j - A_i) carries five roundings (the quotient w, three
products, the difference), a sum of K terms adds at most K - 1 more per term, and the tail adds three (g acc, the product with
u_i, u_i itself): (K + 8) u on sum |term| to first order, and one more u on |A'| for the final addition.  The float64
restatement takes q, r2 and d as the f32 values the statement forms (numpy's f32 element operations are the IEEE ones), so the
bound covers everything the two sides do differently."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import diffuse_cases as DC
from tests import features2d as F
from tests import hard_states2d as H
from tests import parity_states as PS

f32 = np.float32
U = 2.0 ** -24
SLACK = 1.01                        # the second-order terms of the first-order bounds


# ---- float64 checks of the formulas ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.05, 0.2, 1.0])
def test_weight_integrals(h):
    """int r^2 Cg (h^2 - r^2)^2 dA = 2 and int Cg (h^2 - r^2)^2 dA = 8 / h^2, by the midpoint rule in r (error O(1/M^2))"""
    M = 200_000
    r = (np.arange(M) + 0.5) * (h / M)
    k = 24.0 / (np.pi * h ** 8) * (h * h - r * r) ** 2 * 2.0 * np.pi * r * (h / M)
    assert abs((k * r * r).sum() - 2.0) < 1e-8
    assert abs(k.sum() * h * h / 8.0 - 1.0) < 1e-8


def lattice_sum(A, spacing_per_h, seed=3):
    """2 sum_j (m / rho_j) Cg d^2 (A_j - A_i) in float64 at the interior particles of a jittered lattice (h = 1, jitter 0.1 of the
    spacing, SPH poly6 densities) for A given as a function of (x, y): the values, and the particles' positions"""
    h, s = 1.0, 1.0 / spacing_per_h
    side = int(round(6.0 / s))
    g = (np.arange(side) + 0.5) * s - 3.0
    q = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    q = q + np.random.default_rng(seed).uniform(-0.1 * s, 0.1 * s, q.shape)
    i, j = F.pairs_within(q, h)
    o = q[j] - q[i]
    r2 = (o * o).sum(1)
    near = r2 <= h * h
    i, j, r2 = i[near], j[near], r2[near]
    d = h * h - r2
    n = q.shape[0]
    rho = np.bincount(i, 4.0 / (np.pi * h ** 8) * d ** 3, n)           # m = 1
    a = A(q[:, 0], q[:, 1])
    lap = 2.0 * np.bincount(i, (1.0 / rho[j]) * 24.0 / (np.pi * h ** 8) * d * d * (a[j] - a[i]), n)
    inner = (np.abs(q) < 1.5).all(1)                                   # a full neighbourhood of full neighbourhoods
    return lap[inner], q[inner]


def test_the_sum_approaches_the_laplacian():
    """A = x^2 - y^2 (harmonic: 0) and A = x^2 (2), worst interior particle.  "Approaches": halving the spacing from h / 4 to
    h / 8 at least halves the error (first order at the least; the quadrature of the smooth compact kernel alone is second
    order, (s / h)^2 = 1.6 % at h / 8, and the jitter adds a first-moment term that is not bounded more sharply here), and at
    h / 8 the error is below 10 % of the moment's 2."""
    err = {}
    for k in (4, 8):
        harm, _ = lattice_sum(lambda x, y: x * x - y * y, k)
        quad, _ = lattice_sum(lambda x, y: x * x, k)
        err[k] = (float(np.abs(harm).max()), float(np.abs(quad - 2.0).max()))
        print(f"[laplacian] s = h/{k}: max |sum| for x^2 - y^2 {err[k][0]:.4g}, max |sum - 2| for x^2 {err[k][1]:.4g}")
    assert err[8][0] <= err[4][0] / 2 and err[8][1] <= err[4][1] / 2
    assert err[8][0] < 0.2 and err[8][1] < 0.2


def test_gaussian_variance_grows_as_4Dt():
    """A Gaussian blob under the explicit update on a regular lattice at rho0 (float64): its variance <r^2> grows as 4 D t with
    D = kappa / rho0.  The relative error of the measured growth is reported, not bounded in advance; that sum A stays put to
    float64 rounding and that the variance grows are asserted."""
    h, s = 1.0, 0.25
    side = 64
    g = (np.arange(side) + 0.5) * s - side * s / 2
    q = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    i, j = F.pairs_within(q, h)
    o = q[j] - q[i]
    r2 = (o * o).sum(1)
    near = r2 <= h * h
    i, j, r2 = i[near], j[near], r2[near]
    d = h * h - r2
    n = q.shape[0]
    rho = np.bincount(i, 4.0 / (np.pi * h ** 8) * d ** 3, n)
    rho0 = float(np.median(rho))
    wk = (1.0 / rho[j]) * 24.0 / (np.pi * h ** 8) * d * d
    dt = 1.0 / 120.0
    kappa = 0.25 * rho0 * h * h / (16.0 * dt)                          # a quarter of the documented limit
    a = np.exp(-(q * q).sum(1) / (2.0 * 1.0 ** 2))
    rr = (q * q).sum(1)
    var0, tot0 = (a * rr).sum() / a.sum(), a.sum()
    steps = 40
    for _ in range(steps):
        a = a + (2.0 * kappa * dt) * np.bincount(i, wk * (a[j] - a[i]), n) / rho
    var1 = (a * rr).sum() / a.sum()
    want = 4.0 * (kappa / rho0) * steps * dt
    print(f"[gaussian] variance {var0:.6f} -> {var1:.6f}: growth {var1 - var0:.6f}, 4 D t = {want:.6f}, relative error {(var1 - var0) / want - 1:+.3%}")
    assert var1 > var0
    assert abs(a.sum() / tot0 - 1.0) < 1e-12


# ---- the checker against a float64 restatement ------------------------------------------------------------------------------------
def restatement(rec, attr, cg, h2, mass, g):
    """The pass in float64 over every ordered pair within h (O(N^2) in spirit: the pairs come from tests/features2d.pairs_within, a
    superset filtered by the statement's own f32 test) on the records after a checker step — their predicted positions and
    densities are what the pass read.  q, r2 and d are the statement's f32 values; everything behind them is float64.
    -> (A' [N], sum_j |term_ij| [N], K [N], R [N])"""
    q32 = rec["predicted_position"].astype(f32)
    n = q32.shape[0]
    i, j = F.pairs_within(q32.astype(np.float64), float(np.sqrt(np.float64(h2))) * (1 + 1e-6))
    ox, oy = q32[j, 0] - q32[i, 0], q32[j, 1] - q32[i, 1]
    r2 = ox * ox + oy * oy
    near = ~(r2 > f32(h2))
    i, j, r2 = i[near], j[near], r2[near]
    d = (f32(h2) - r2).astype(np.float64)
    rho = rec["density"].astype(np.float64)
    wk = (float(mass) / rho[j]) * (float(cg) * d * d)
    a = attr.astype(np.float64)
    t = wk * (a[j] - a[i])
    acc, tabs = np.bincount(i, t, n), np.bincount(i, np.abs(t), n)
    K = np.bincount(i, minlength=n)
    u = 1.0 / rho
    return a + float(g) * acc * u, float(g) * tabs * u, K, u * np.bincount(i, wk, n)


@pytest.fixture(scope="module")
def dam(fs, orc):
    """the jittered 4096 dam break with ref_quirks off (a symmetric neighbour relation) after two plain steps, then one step with
    two diffusing channels (x, and a constant) at g R = 1/2 at the slot where R is largest: (checker, tick, A before the pass)"""
    from tests.diffuse_ref import DiffuseChecker
    st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, 12)
    chk = DiffuseChecker(st, off, ref_quirks=False, channels=2)
    chk.set_particles(p)
    for _ in range(2):
        chk.step(tick)
    chk.attr[0] = chk.particles()["position"][:, 0]
    chk.attr[1] = 1.5
    probe = DC.pass_of_next_step(chk, tick)                              # R of the step to come, on a scratch copy
    kappa = DC.kappa_for(probe["R"], float(tick.delta), 0.5)
    chk.kappa[0] = chk.kappa[1] = kappa
    chk.step(tick)
    before = probe["attr"]
    return chk, tick, before, kappa


def test_checker_against_the_float64_restatement(fs, dam):
    chk, tick, before, kappa = dam
    u = fs.build_uniform(chk.settings, tick, 1)
    g = float((f32(2.0) * f32(kappa)) * f32(tick.delta))
    rec = chk.particles()
    want, tabs, K, R = restatement(rec, before[0], u.poly6_kernel_derivative, u.sqr_radius, u.particle_mass, g)
    got = chk.attr[0].astype(np.float64)
    bound = SLACK * U * (np.abs(want) + (K + 8) * tabs)
    share = np.abs(got - want) / bound
    print(f"[restatement] worst share of the rounding bound {share.max():.3f}; K up to {K.max()}; g R up to {(g * R).max():.3f}")
    assert (share <= 1.0).all()
    assert np.allclose(R, chk.R, rtol=1e-5)                             # the checker's R is the restatement's (f32 weights, f64 sum)
    assert (np.abs(chk.acc[0]) > 0).mean() > 0.5


def test_conservation(fs, dam):
    """Which identity holds.  Bit for bit, for every pair: r2, d and k = (Cg d) d are symmetric and A_j - A_i = -(A_i - A_j), so
    k (A_j - A_i) is antisymmetric — and that is all.  The statement's term carries w_j inside the rounded product and u_i outside
    the sum, so term(i, j) u_i and -term(j, i) u_j agree only to rounding even at m = 1, where w_j = u_j: what is conserved is
    sum_i A_i, in exact arithmetic, over a symmetric neighbour relation (ref_quirks = 0) of equal masses.  Asserted: the float64
    restatement conserves sum A to its own rounding; the f32 checker's drift stays inside the sum of the per-slot rounding
    bounds; a constant channel is a fixed point bit for bit (every difference is +0)."""
    chk, tick, before, kappa = dam
    u = fs.build_uniform(chk.settings, tick, 1)
    g = float((f32(2.0) * f32(kappa)) * f32(tick.delta))
    want, tabs, K, _ = restatement(chk.particles(), before[0], u.poly6_kernel_derivative, u.sqr_radius, u.particle_mass, g)
    a0 = before[0].astype(np.float64)
    scale = np.abs(a0).sum() + tabs.sum()
    assert abs(want.sum() - a0.sum()) <= 64 * 2.0 ** -53 * scale         # pairwise float64 sums of 4096 + ~10^5 terms
    drift = abs(chk.attr[0].astype(np.float64).sum() - a0.sum())
    bound = (SLACK * U * (np.abs(want) + (K + 8) * tabs)).sum()
    print(f"[conservation] f32 drift of sum A {drift:.3e}, bound {bound:.3e} (sum |A| {np.abs(a0).sum():.3e})")
    assert drift <= bound
    assert np.array_equal(chk.attr[1].view(np.uint32), before[1].view(np.uint32))
    assert not chk.acc[1].view(np.uint32).any()


def test_max_principle(fs, dam):
    """g R_i <= 1 at every slot makes A'_i a convex combination of A_i and its neighbours' values in exact arithmetic; in f32 it
    may leave [min A, max A] by the per-slot rounding bound at most."""
    chk, tick, before, kappa = dam
    u = fs.build_uniform(chk.settings, tick, 1)
    g = float((f32(2.0) * f32(kappa)) * f32(tick.delta))
    assert (g * chk.R <= 1.0).all()
    want, tabs, K, _ = restatement(chk.particles(), before[0], u.poly6_kernel_derivative, u.sqr_radius, u.particle_mass, g)
    bound = SLACK * U * (np.abs(want) + (K + 8) * tabs)
    a = chk.attr[0].astype(np.float64)
    lo, hi = float(before[0].min()), float(before[0].max())
    assert (a >= lo - bound).all() and (a <= hi + bound).all()
    assert (want >= lo - 1e-12 * max(abs(lo), abs(hi))).all() and (want <= hi + 1e-12 * max(abs(lo), abs(hi))).all()


def test_diffusion_limit(fs):
    st = fs.SimulationSettings(4096, 0.1, 0.2, (20.0, 10.0))
    tick = fs.default_tick_settings()
    want = 30.0 * 0.2 * 0.2 / (16.0 * float(tick.delta))
    assert abs(fs.FluidSimulation.diffusion_limit(st, tick, 30.0) / want - 1.0) < 1e-6


# ---- the GPU file's cases are not vacuous -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.CASE_IDS)
def test_registry_cases_are_not_vacuous(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    case.run()
    for sort in DC.SORTS:
        run = DC.registry_run(fs, case, sort)
        print(f"[diffuse_cases] {cid}/{sort}: kappa {run.kappa}, moving acc share {run.acc_share:.3f}, s > 0 {run.s_pos}, s < 0 {run.s_neg}, "
              f"longest row range {run.longest_row}")
        if case.n >= 64:
            assert run.acc_share > 0.5
        if case.n >= 2:
            assert run.s_pos > 0 and run.s_neg > 0
        if case.family == "dense_scene":
            assert run.longest_row > DC.NB_TILE


# ---- layers, prototypes, refusals without a device --------------------------------------------------------------------------------
CALLS = ["fs_set_diffusion", "fs_get_diffusion", "fs_set_buoyancy", "fs_get_buoyancy", "fs_download_buoyancy"]


def test_every_layer_names_every_call(fs):
    from tests.layers import assert_every_layer_names, header_text
    assert_every_layer_names(fs, CALLS, fs.FluidSimulation, (
        "set_diffusion", "diffusion", "set_buoyancy", "clear_buoyancy", "buoyancy", "buoyancy_forces", "diffusion_limit"))
    head = header_text()
    for name in CALLS:
        assert head.index(name) > head.index("fs_sort_plan_read"), f"{name}: the additions are appended to the ABI"
    assert isinstance(fs.FluidSimulation.__dict__["diffusion_limit"], staticmethod)
    from gpu_fluid_simulation_amd import _handle
    assert not hasattr(_handle._Tracking, "set_diffusion")              # the 3D handle shares the mixin and has no such call


def test_null_handle_is_invalid_without_a_device(fs):
    lib = fs.load_library()
    inv = fs._abi.FS_ERR_INVALID
    k, c, buf = C.c_float(), C.c_int(), (C.c_float * 8)()
    assert lib.fs_set_diffusion(None, 0, 1.0) == inv
    assert b"null" in lib.fs_last_error()
    assert lib.fs_get_diffusion(None, 0, C.byref(k)) == inv
    assert lib.fs_set_buoyancy(None, 0, 1.0, 0.0) == inv
    assert lib.fs_get_buoyancy(None, C.byref(c), C.byref(k), C.byref(k)) == inv
    assert lib.fs_download_buoyancy(None, buf, 4) == inv
    assert b"null" in lib.fs_last_error()


def test_header_and_design_state_the_pass(fs):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = open(os.path.join(root, "include", "fluidsim.h")).read()
    assert re.search(r"fs_track_enable[^\n]*\n[^\n]*fs_track_disable clear every conductivity", head)
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert re.search(r"^## 27\.", design, flags=re.M) and "rho0 h^2 / 16" in head

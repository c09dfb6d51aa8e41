"""CPU checks of the opt-in surface-tension model and of its checker (tests/st_checker.cpp).

The formulas: the 2D poly6 kernel the density pass uses, W = 4/(pi h^8)(h^2 - r^2)^3, its gradient Cg d^2 (q - x) and its
2D Laplacian Cl d (3 r^2 - h^2) with d = h^2 - r^2, Cg = 24/(pi h^8), Cl = 48/(pi h^8) — checked in float64 against
quadrature and finite differences.  Then the checker against an O(N^2) float64 sum, and its move pass against the oracle's."""
import numpy as np
import pytest

H = 0.2


def W(r2, h=H):
    d = np.maximum(h * h - r2, 0.0)
    return 4.0 / (np.pi * h ** 8) * d ** 3


def grad_W(x, y, h=H):          # grad_x W(|x - q|) at q = 0: Cg d^2 (q - x)
    r2 = x * x + y * y
    d = np.maximum(h * h - r2, 0.0)
    cg = 24.0 / (np.pi * h ** 8)
    return cg * d * d * (-x), cg * d * d * (-y)


def lap_W(r2, h=H):
    d = np.where(r2 <= h * h, h * h - r2, 0.0)
    cl = 48.0 / (np.pi * h ** 8)
    return cl * d * (3.0 * r2 - h * h)


def _radial_integral(f, h=H, n=64):
    """2 pi int_0^h f(r) r dr by Gauss-Legendre (exact for the polynomials here)."""
    t, w = np.polynomial.legendre.leggauss(n)
    r = 0.5 * h * (t + 1.0)
    return 2.0 * np.pi * np.sum(0.5 * h * w * f(r) * r)


@pytest.mark.parametrize("h", [0.2, 0.05, 1.7])
def test_poly6_normalised_over_the_disc(h):
    assert _radial_integral(lambda r: W(r * r, h), h) == pytest.approx(1.0, rel=1e-12)
    # a 3D normalisation (315 / (64 pi h^9) (h^2 - r^2)^3) does not integrate to 1 in 2D
    assert abs(_radial_integral(lambda r: 315.0 / (64.0 * np.pi * h ** 9) * (h * h - r * r) ** 3, h) - 1.0) > 0.05


@pytest.mark.parametrize("h", [0.2, 0.05, 1.7])
def test_laplacian_integrates_to_zero(h):
    scale = _radial_integral(lambda r: np.abs(lap_W(r * r, h)), h)
    assert abs(_radial_integral(lambda r: lap_W(r * r, h), h)) < 1e-12 * scale


@pytest.mark.parametrize("frac", [0.1, 0.3, 0.5, 0.577, 0.7, 0.9])
@pytest.mark.parametrize("angle", [0.0, 0.7, 2.0])
def test_gradient_and_laplacian_match_finite_differences(frac, angle):
    r = frac * H
    x, y = r * np.cos(angle), r * np.sin(angle)
    e = 1e-5 * H
    f = lambda a, b: W(a * a + b * b)
    gx = (f(x + e, y) - f(x - e, y)) / (2 * e)
    gy = (f(x, y + e) - f(x, y - e)) / (2 * e)
    ax, ay = grad_W(x, y)
    scale = 24.0 / (np.pi * H ** 8) * H ** 5
    assert abs(gx - ax) < 1e-6 * scale and abs(gy - ay) < 1e-6 * scale
    e = 1e-4 * H
    lap = (f(x + e, y) + f(x - e, y) + f(x, y + e) + f(x, y - e) - 4 * f(x, y)) / (e * e)
    assert abs(lap - lap_W(r * r)) < 1e-5 * 48.0 / (np.pi * H ** 8) * H ** 4
    # the 3D Laplacian of the same kernel (factor (h^2 - r^2)(7 r^2 - 3 h^2)) is another function
    lap3 = 24.0 / (np.pi * H ** 8) * (H * H - r * r) * (7 * r * r - 3 * H * H)
    assert abs(lap3 - lap_W(r * r)) > 1e-3 * abs(lap_W(r * r)) + 1.0


def test_uniform_constant_is_the_statements_cg(fs):
    """Cg is the uniform's poly6_kernel_derivative (src/simulation.rs:487), 24/(pi h^8) in f32; Cl = 2 Cg exactly."""
    for h in (0.2, 0.05, 0.37):
        st = fs.SimulationSettings(4096, 0.1, h, (10.0, 10.0))
        u = fs.build_uniform(st, fs.default_tick_settings(), 1)
        assert u.poly6_kernel_derivative == pytest.approx(24.0 / (np.pi * h ** 8), rel=2e-6)
        assert u.poly6_kernel_derivative == pytest.approx(6.0 * u.poly6_kernel_volume, rel=1e-6)


# ---------------------------------------------------------------------------------------------------- the checker
def _random_scene(fs, n, seed, h=H):
    size = (6.0, 5.0)
    st = fs.SimulationSettings(n, 0.1, h, size)
    tick = fs.default_tick_settings(gravity=(0.0, 9.81))
    rng = np.random.default_rng(seed)
    side = np.sqrt(n) * 0.09               # ~ the reference's spacing: neighbourhoods of a few dozen, across cell edges
    pos = rng.uniform(-side / 2, side / 2, size=(n, 2)) + rng.uniform(-1.0, 1.0, size=2)
    return st, tick, pos.astype(np.float32)


def _checker_after_density(fs, n, seed, quirks):
    from tests.st_ref import STChecker
    st, tick, pos = _random_scene(fs, n, seed)
    c = STChecker(st, ref_quirks=quirks)
    p = c.particles()
    p["position"] = pos
    p["predicted_position"] = pos
    p["velocity"] = 0.0
    c.set_particles(p)
    c.begin_tick(tick); c.predict(); c.spatial_lookup(); c.sort(); c.cell_starts(); c.density()
    return c, tick


def _brute_force(c, h2, m):
    p = c.particles()
    q = p["predicted_position"].astype(np.float64)
    rho = p["density"].astype(np.float64)
    cg = 24.0 / (np.pi * H ** 8)
    cl = 2.0 * cg
    n = q.shape[0]
    out = np.zeros((n, 3))
    scale = np.zeros((n, 2))
    for i in range(n):
        o = q - q[i]
        r2 = (o * o).sum(1)
        k = r2 <= h2
        d = h2 - r2[k]
        w = m / rho[k]
        tn = (w * cg * d * d)[:, None] * o[k]
        tl = w * cl * d * (3.0 * r2[k] - h2)
        out[i, :2] = tn.sum(0)
        out[i, 2] = tl.sum()
        scale[i, 0] = np.abs(tn).sum()
        scale[i, 1] = np.abs(tl).sum()
    return out, scale


@pytest.mark.parametrize("n,seed,quirks", [(1000, 1, True), (2500, 2, False), (4000, 3, True), (1500, 4, False)])
def test_checker_matches_brute_force_float64(fs, n, seed, quirks):
    """n and L within 1e-5 of the sum of the terms' magnitudes (f32 accumulation of a few dozen terms); st where |n| is
    well away from 0 (the direction is ill-conditioned there) within 1e-4 of sigma times L's magnitude sum."""
    c, tick = _checker_after_density(fs, n, seed, quirks)
    st, nl = c.surface_tension_pass()
    u = fs.build_uniform(c.settings, tick, 1)
    want, scale = _brute_force(c, float(np.float32(u.sqr_radius)), float(tick.mass))
    cross = np.abs(want[:, :2]).sum(1) > 0
    assert cross.mean() > 0.5, "the scene has too few neighbour pairs"
    assert np.all(np.abs(nl[:, 0] - want[:, 0]) <= 1e-5 * scale[:, 0] + 1e-30)
    assert np.all(np.abs(nl[:, 1] - want[:, 1]) <= 1e-5 * scale[:, 0] + 1e-30)
    assert np.all(np.abs(nl[:, 2] - want[:, 2]) <= 1e-5 * scale[:, 1] + 1e-30)
    nn = np.hypot(want[:, 0], want[:, 1])
    ok = (nn > 1e-2 * scale[:, 0]) & (nn > tick.surface_tension_treshold * 1.001)
    assert ok.sum() > 50
    sig = tick.surface_tension_coefficient
    want_st = (-sig * want[:, 2] / np.where(nn > 0, nn, 1.0))[:, None] * want[:, :2]
    err = np.abs(st[ok].astype(np.float64) - want_st[ok]).max(1)
    assert np.all(err <= 1e-4 * sig * scale[ok, 1])
    below = nn < tick.surface_tension_treshold * 0.999          # below the threshold: exactly zero
    assert np.all(st[below] == 0.0)


def test_checker_move_without_st_is_the_oracles(fs, orc):
    """ST off in the checker: its restated move pass is byte-identical to the oracle's over a 4096-particle dam break."""
    from tests.st_ref import STChecker
    st, off, tick = fs.dam_break_2d(4096)
    ref = orc.OracleSim(st, off)
    chk = STChecker(st, off)
    for s in range(20):
        ref.step(tick)
        chk.step(tick, surface_tension=False)
        assert ref.particles().tobytes() == chk.particles().tobytes(), f"step {s}"
        assert np.array_equal(ref.start_indices(), chk.start_indices())
    # and the ST pass with sigma = 0 adds nothing but zeros: the same values as the plain step (== : signed zeros may differ)
    tick.surface_tension_coefficient = 0.0
    chk.step(tick, surface_tension=True)
    ref.step(tick)
    a, b = chk.particles(), ref.particles()
    for f in ("position", "predicted_position", "velocity", "density"):
        assert np.array_equal(a[f], b[f])


def test_checker_move_with_st_uses_the_forces(fs):
    """Sanity of the restated move: with ST on (default knobs) the dam break's free surface moves differently."""
    from tests.st_ref import STChecker
    st, off, tick = fs.dam_break_2d(4096)
    a, b = STChecker(st, off), STChecker(st, off)
    a.step(tick, surface_tension=True)
    b.step(tick, surface_tension=False)
    moved = np.any(a.particles()["velocity"] != b.particles()["velocity"], axis=1)
    pushed = np.any(a.st != 0.0, axis=1)
    assert moved.sum() > 100 and not np.any(moved & ~pushed)

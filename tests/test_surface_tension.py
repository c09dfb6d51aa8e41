"""CPU checks of the opt-in surface-tension model and of its checker (tests/st_checker.cpp).

The formulas: the 2D poly6 kernel the density pass uses, W = 4/(pi h^8)(h^2 - r^2)^3, its gradient Cg d^2 (q - x) and its
2D Laplacian Cl d (3 r^2 - h^2) with d = h^2 - r^2, Cg = 24/(pi h^8), Cl = 48/(pi h^8) — checked in float64 against
quadrature and finite differences.  Then the checker against an O(N^2) float64 sum, and its move pass against the oracle's.
Last, the hard-input cases of tests/features2d.py on the checker alone: every case that tests/test_surface_tension_hard_inputs_gpu.py
runs on the engine tests what it says (both threshold branches, exact-zero and NaN |n|, tau on a particle's |n|, the floor)."""
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


# ------------------------------------------- the hard-input cases of tests/test_surface_tension_hard_inputs_gpu.py, on the checker alone
from tests import features2d as F                                  # noqa: E402
from tests import parity_states as PS                              # noqa: E402

f32 = np.float32
ALL_BELOW = ("guard/tau_nan",)                                     # nl > NaN is false: the point of the case
NO_FORCE_IN_STEP_1 = ("guard/nan_next_to_everyone",)               # every |n| of step 1 is a NaN: the point of the case
SET_BY_HAND = ("guard/isolated/tau0", "guard/isolated/tau-1", "guard/tau_exact", "guard/sigma-35", "guard/sigma_inf", "guard/tau_nan")
NAN_REACHES_THE_PASS = ("inf_velocity", "nan_clamp", "nan_next_to_everyone", "sigma_inf")
UNSAFE_FLAG = ("tiny_velocities", "huge_velocities", "inf_velocity", "huge_pressure")


def _same(a, b):
    """equal values, a NaN met by a NaN"""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_hard_input_cases_exercise_the_pass(fs, orc, cid):
    """What the GPU file relies on, asked of the checker alone.  The registry's step (the calls of stc_step one by one, to keep n
    and L) gives STChecker.step's bytes; every force is the statement's closed form of that step's n and L, zero on the
    not-above branch; over the case's steps both branches of `nl > tau && nl > 0` are taken (ALL_BELOW and step 1 of
    NO_FORCE_IN_STEP_1 assert that one is empty instead); where sigma and tau were chosen and at least 100 particles have a
    colour gradient, step 1 leaves at least 1 % of the particles on each side and the pass changes velocities by 0.1 to 10 times
    what the step itself does."""
    case = F.case_by_id(fs, orc, cid)
    run = case.run()
    print(F.describe(case))
    fig = case.figures
    n = case.start.shape[0]
    assert len(run) == case.steps >= 1 and fig["n"] == n >= 2 and np.isfinite(fig["own_dv"])
    chk = case.checker()
    sigma, tau = f32(case.sigma), f32(case.tau)
    for k, s in enumerate(run):
        with np.errstate(all="ignore"):
            chk.step(case.tick, stable_sort=case.stable)
            assert chk.particles().tobytes() == s.rec.tobytes() and chk.st.tobytes() == s.st.tobytes(), f"step {k}"
            assert np.array_equal(chk.start_indices(), s.start)
            up = s.above(tau)
            sc = (-sigma * s.nl3[:, 2]) / s.nl
            want = np.where(up[:, None], sc[:, None] * s.nl3[:, :2], f32(0)).astype(f32)
        assert _same(want, s.st), f"step {k}: st is not the closed form of n and L"
        assert fig["above"][k] == int(up.sum()) and fig["below"][k] == n - int(up.sum())
    chk.close()
    forces = [bool(np.any(s.st != 0)) for s in run]
    if cid in ALL_BELOW:
        assert sum(fig["above"]) == 0 and not any(forces)
        return
    if cid in NO_FORCE_IN_STEP_1:
        assert fig["nan_n"][0] == n and fig["above"][0] == 0 and not forces[0] and np.all(run[0].rec["density"] == f32(0.1))
        assert all(forces[1:]) and fig["above"][1:] == [n] * (case.steps - 1)
        return
    assert any(forces) and (forces[0] or n < 100), "the pass produced no force"
    assert sum(fig["above"]) > 0 and sum(fig["below"]) > 0, fig
    if cid not in SET_BY_HAND:
        if fig["with_n"] >= 100:
            assert fig["above"][0] >= n / 100 and fig["below"][0] >= n / 100, fig
        if fig["own_dv"] > 0:
            assert 0.1 <= fig["st_dv"] / fig["own_dv"] <= 10.0, fig


@pytest.mark.parametrize("name", ["isolated/tau0", "isolated/tau-1"])
def test_isolated_particles_have_no_gradient_and_no_force(fs, orc, name):
    """n == (0, 0) exactly for the four particles farther than h from everyone (the self term adds 0); with tau <= 0 only
    `nl > 0` keeps their force at zero — and L is not zero, so a kernel without the second comparison divides -sigma L by 0 —
    while every other particle gets a force"""
    case = F.guard_case(fs, orc, name)
    assert case.tau <= 0
    for s in case.run():
        alone = (s.nl3[:, 0] == 0) & (s.nl3[:, 1] == 0)
        assert alone.sum() == len(F.ISOLATED) and np.all(s.rec["predicted_position"][alone, 0] >= 2.5)
        assert np.all(s.nl3[alone, 2] < 0)
        assert not s.st[alone].any() and np.all(np.any(s.st[~alone] != 0, axis=1))


def test_tau_exact_sits_on_one_particles_gradient(fs, orc):
    case = F.guard_case(fs, orc, "tau_exact")
    s = case.run()[0]
    k, nxt = case.figures["exact"], case.figures["next"]
    tau = f32(case.tau)
    assert s.nl[k:k + 1].view(np.uint32)[0] == np.array([tau]).view(np.uint32)[0] and (s.nl == tau).sum() == 1
    assert not s.st[k].any()                                        # nl > tau is false at equality
    assert s.nl[nxt] > tau and not np.any((s.nl > tau) & (s.nl < s.nl[nxt])) and s.st[nxt].any()
    assert s.nl[nxt] <= tau * f32(1.01)                             # ... and `>=` would be the only difference nearby


def test_mass_tiny_holds_every_density_at_the_floor(fs, orc):
    case = F.guard_case(fs, orc, "mass_tiny")
    for s in case.run():
        assert np.all(s.rec["density"] == f32(0.1))
    assert 0 < f32(case.tick.mass) / f32(0.1) < 1e-2 and np.isfinite(case.sigma) and any(s.st.any() for s in case.run())


def test_guard_cases_still_carry_their_operands(fs, orc):
    """A NaN reaches the pass (|n| is a NaN for some particle of some step) in NAN_REACHES_THE_PASS, an infinite force in sigma_inf;
    UNSAFE_FLAG, the guard scenes of the plain step that do, still set the density pass's unsafe flag for some particle of step 1
    (tiny_offsets, zero_aligned, near_zero_coordinates and small_operands_on_the_fast_path leave every particle safe) — evaluated from
    the checker's predicted positions, velocities and densities with the rules of csrc/fs_device.h (kin_safe; rho <= 2^20;
    |k (rho - rho0)| <= 2^39)."""
    for name in NAN_REACHES_THE_PASS:
        assert sum(F.guard_case(fs, orc, name).run() and F.guard_case(fs, orc, name).figures["nan_n"]) > 0, name
    assert any(np.isinf(s.st).any() for s in F.guard_case(fs, orc, "sigma_inf").run())
    for name in UNSAFE_FLAG:
        case = F.guard_case(fs, orc, name)
        chk = case.checker()
        F.density_state(chk, case.tick, case.stable)
        p = chk.particles()
        chk.close()
        with np.errstate(all="ignore"):
            c = np.concatenate([p["predicted_position"], p["velocity"]], axis=1)
            lo_safe = (c == 0) | (np.abs(c) >= f32(2.0 ** -53))
            kin = lo_safe.all(axis=1) & (np.abs(p["velocity"]) <= f32(2.0 ** 59)).all(axis=1)
            press = f32(case.tick.pressure_constant) * (p["density"] - f32(case.tick.rest_density))
            safe = kin & (p["density"] <= f32(2.0 ** 20)) & (np.abs(press) <= f32(2.0 ** 39))
        assert (~safe).sum() > 0, name


def test_settings_guards(fs, orc):
    """tau = NaN: no force, and the records are the plain oracle's; sigma = -35: the force of +35 with the other sign"""
    case = F.guard_case(fs, orc, "tau_nan")
    ref = orc.OracleSim(case.st, case.off)
    ref.set_particles(case.start)
    for s in case.run():
        ref.step(case.tick)
        assert ref.particles().tobytes() == s.rec.tobytes() and np.array_equal(ref.start_indices(), s.start)
    ref.close()
    neg = F.guard_case(fs, orc, "sigma-35")
    pos = F.Case("sigma+35", neg.st, neg.off, neg.tick, neg.start, 1).set_st(sigma=35.0, tau=neg.tau)
    assert np.array_equal(neg.run()[0].st, -pos.run()[0].st) and neg.run()[0].st.any()


@pytest.mark.parametrize("name", F.TOL_CASES)
def test_tolerance_cases_keep_their_branches(fs, orc, name):
    """tau keeps 1e-3 (a hundred times the density contract of FS_MATH_TOLERANCE) from every |n|, and no particle's |n| can reach
    tau under that contract (features2d.choose_tolerance_threshold); both branches are taken"""
    case = F.tolerance_case(fs, orc, name)
    case.run()
    print(F.describe(case))
    fig = case.figures
    assert fig["tau_gap"] > F.TOL_GAP and fig["tau_margin"] > 1.0 and fig["above"][0] > 0 and fig["below"][0] > 0, fig


def test_host_and_switch_cases_take_both_branches(fs, orc):
    for case in (F.host_case(fs, orc), F.host_case(fs, orc, "counting", False)) + F.switch_cases(fs, orc):
        case.run()
        print(F.describe(case))
        assert min(case.figures["above"]) > 0 and min(case.figures["below"]) > 0


def test_tiny_offsets_reach_the_passes(fs, orc):
    """tiny_offsets_at_rest keeps its offsets through the predict step: the first step's predicted positions hold the origin and
    six distinct points between 2^-149 and 1e-7 from it.  (tiny_offsets of the plain suite does not: its seven particles coincide.)"""
    want = sorted(float(f32(d)) for d in (1e-45, 1e-40, 1e-30, 1e-19, 3e-13, 1e-7))
    for name, kept in (("tiny_offsets_at_rest", True), ("tiny_offsets", False)):
        case = F.guard_case(fs, orc, name)
        chk = case.checker()
        F.density_state(chk, case.tick, case.stable)
        q = chk.particles()["predicted_position"]
        chk.close()
        x = q[(np.abs(q) <= f32(1e-7)).all(axis=1)]
        assert (sorted(float(v) for v in x[:, 0] if v != 0) == want) == kept, name
        if kept:
            assert x.shape[0] == 7 and np.unique(x, axis=0).shape[0] == 7

"""GPU tests of the opt-in diffusion and buoyancy of the tracking channels of the 3D step: the engine against the
checker (tests/diffuse3d_checker.cpp through tests/diffuse3d_ref.py), bit for bit in FS_MATH_IEEE — ids, every channel, fb, every
float of the state and the keys, a NaN met by any NaN — over at least three steps.  What the scenes reach and that they are not
vacuous is asserted without a GPU in tests/test_diffusion3d.py."""
import numpy as np
import pytest

import paths3d
from oracle import oracle as O
from tests import bitcmp
from tests import collide3d_ref as CR
from tests import diffuse3d_cases as DC
from tests import diffuse3d_ref as DR

pytestmark = pytest.mark.gpu
f32 = np.float32
SUBSETS = DC.SUBSETS
ST_CFG = (0.4, 0.05)


def stable_kappa(chk, tick, target=0.5):
    """the conductivity at g R = target where R is largest in the step to come, from the checker alone"""
    return DC.kappa_for(DC.pass_of_next_step(chk, tick)["R"], tick.delta, target)


def step_both(sim, chk, tick, field=None):
    sim.tick(tick)
    chk.step(tick)
    if field is not None:
        size = (chk.settings.size.x, chk.settings.size.y, chk.settings.size.z)
        with np.errstate(all="ignore"):
            chk.set_particles(CR.apply_collider(chk.particles(), field, size, tick.damping_factor)[0])


def run(fs, name, subset, buoyancy, steps=3, surface_tension=None, field=None, compare_at=None, tick_over=None, env=None,
        monkeypatch=None, check=None):
    st, tick, p, _ = DC.scene_state(fs, name)
    if tick_over:
        tick = DR.tick_of(fs, tick, **tick_over)
    if env:
        monkeypatch.setenv(*env)
    sim, chk = DC.make_pair(fs, st, p, 4)
    if env:
        monkeypatch.delenv(env[0], raising=False)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    if field is not None:
        sim.set_collider(field)
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {c: k for c in subset}, buoyancy, surface_tension)
    for s in range(steps):
        step_both(sim, chk, tick, field)
        if check:
            check(chk)
        if compare_at is None or s + 1 in compare_at:
            DC.assert_same(sim, chk, f"{name} {subset} {buoyancy} step {s + 1}")
    if not subset and buoyancy is None:
        assert chk.fb is None
    sim.close(); chk.close()


# ---- every sweep path, with the masks handed over and with the pass's own scan -------------------------------------------------
@pytest.mark.parametrize("handoff", ["handoff", "own_scan"])
@pytest.mark.parametrize("name", sorted(paths3d.scenes()))
def test_path_scene_matches_checker(fs, monkeypatch, name, handoff):
    """every step of every path scene: the model (fed the checker's keys) says the named sweep carries a wave-plane, and ids,
    channels, fb, state and keys equal the checker's.  FS3_HANDOFF=0 is read per handle at create: no masks are handed over, the
    pass scans the staged plane itself.  The diffusing subset and the buoyancy channel (inside or outside it) go round by scene."""
    subset, buoy = DC.scene_plan(name)
    scene = paths3d.scenes()[name]
    run(fs, name, subset, buoy, steps=DC.SCENE_STEPS, env=("FS3_HANDOFF", "0") if handoff == "own_scan" else None, monkeypatch=monkeypatch,
        check=lambda chk: paths3d.check_scene(scene, [chk.particles()], chk.grid_dims))


def test_dam_break_steps_1_and_8(fs):
    run(fs, "dam16", (0, 2), (0, 0.5, 0.0), steps=8, compare_at=(1, 8))


@pytest.mark.parametrize("subset", SUBSETS)
def test_diffusing_subsets(fs, subset):
    """D = 1, D = 2 and both launch groupings (2, 2 + 1, 2 + 2); no buoyancy: the state is the plain step's"""
    run(fs, "pair12", subset, None)


# ---- counts that are no cube, capacity > n: two workgroups, a ragged last wave ---------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 257, 4097])
def test_counts_with_spare_capacity(fs, n):
    side = 2 if n < 8 else int(np.floor(n ** (1.0 / 3.0) + 1e-9))
    st, off, tick = fs.dam_break_3d(side ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.reserve(n + 100)
    sim.track(4)
    rec = sim.download_particles()
    if n < rec.shape[0]:
        flags = np.ones(rec.shape[0], dtype=np.uint8); flags[:n] = 0
        assert sim.remove(flags) == rec.shape[0] - n
    else:
        extra = rec[:n - rec.shape[0]].copy()
        extra["position"] += f32(0.03)
        extra["predicted_position"] = extra["position"]
        sim.emit(extra)
    assert sim.particle_count == n and sim.capacity > n
    sim.tick(tick)
    sim, chk = reseeded(fs, sim, st)
    DC.set_channels(sim, chk, DC.fill_channels(chk.particles(), 4, seed=n))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k, 1: k, 3: k}, (3, 0.5, 0.0))
    for s in range(3):
        step_both(sim, chk, tick)
        DC.assert_same(sim, chk, f"n {n} step {s + 1}")
    sim.close(); chk.close()


def reseeded(fs, sim, st):
    """a checker at the handle's count, seeded from its downloads: records, ids, channels and the tick count"""
    rec = sim.download_particles()
    n = rec.shape[0]
    chk = DR.Diffuse3Checker(fs.Settings3(int(n), st.particle_spacing, st.smoothing_radius, st.size), channels=sim.track_channels,
                             tick_count=sim.tick_count)
    chk.set_particles(rec)
    chk.ids = sim.particle_ids()
    chk.attr = np.stack([sim.attribute(c) for c in range(chk.channels)])
    return sim, chk


def test_after_emit_and_remove_box(fs):
    st, tick, p, _ = DC.scene_state(fs, "pair12")
    sim, chk = DC.make_pair(fs, st, p, 4, capacity=2000)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k, 2: k}, (0, 0.5, 0.0))
    step_both(sim, chk, tick)
    DC.assert_same(sim, chk, "before the count changes")
    extra = p[:100].copy()
    extra["position"] += f32(0.04)
    sim.emit(extra)
    bitcmp.expect_invalid(fs, sim.buoyancy_forces)                       # the count changed: fb no longer belongs to the state
    assert sim.remove_box((-0.2, -0.2, -0.2), (0.0, 0.0, 0.0)) > 0
    assert sim.buoyancy == (0, 0.5, 0.0) and sim.diffusion(2) == float(f32(k))      # the settings stay
    chk.close()
    sim, chk = reseeded(fs, sim, st)
    chk.kappa[0] = chk.kappa[2] = float(f32(k))
    chk.buoyancy = (0, 0.5, 0.0)
    for s in range(3):
        step_both(sim, chk, tick)
        DC.assert_same(sim, chk, f"after emit and remove, step {s + 1}")
    sim.close(); chk.close()


# ---- channels that do not diffuse -------------------------------------------------------------------------------------------------
def tracking_only_twin(fs, name, mode=None, steps=3):
    """two handles on one scene with the same channel contents, one with every conductivity set to 0 and buoyancy cleared, one
    that never heard of the feature: the same bytes everywhere"""
    st, tick, p, _ = DC.scene_state(fs, name)
    kw = {} if mode is None else dict(math_mode=mode)
    a, b = fs.FluidSimulation3D(st, device=0, **kw), fs.FluidSimulation3D(st, device=0, **kw)
    for sim in (a, b):
        sim.upload_particles(p)
        sim.track(4)
        for c in range(4):
            sim.set_attribute(c, bitcmp.special_bits(p.shape[0], 40 + c, bitcmp.POOL_TWELVE))
    for c in range(4):
        a.set_diffusion(c, 0.0)
    a.set_buoyancy(1, 2.0, 0.5)
    a.clear_buoyancy()
    for s in range(steps):
        a.tick(tick); b.tick(tick)
        assert a.download_particles().tobytes() == b.download_particles().tobytes(), f"step {s + 1}"
        assert np.array_equal(a.particle_ids(), b.particle_ids())
        for c in range(4):
            assert a.attribute(c).tobytes() == b.attribute(c).tobytes(), f"channel {c}, step {s + 1}"
    bitcmp.expect_invalid(fs, a.buoyancy_forces)
    a.close(); b.close()


def test_kappa_zero_is_tracking_only(fs):
    tracking_only_twin(fs, "pair12")


def test_tolerance_mode_with_nothing_set_is_tracking_only(fs):
    tracking_only_twin(fs, "pair12", mode=fs.FS_MATH_TOLERANCE)


def test_channel_contents(fs):
    """finite values to 1e30 (diffusing), NaN payloads, +-inf, -0.0 and denormals diffusing and at kappa = 0, one channel at four
    times the stable kappa"""
    st, tick, p, _ = DC.scene_state(fs, "pair12")
    sim, chk = DC.make_pair(fs, st, p, 4)
    n = p.shape[0]
    vals = DC.fill_channels(p, 4)
    vals[0] = vals[2]                                                    # to 1e30
    vals[1] = bitcmp.special_bits(n, 7, bitcmp.POOL_TWELVE)
    vals[2] = bitcmp.special_bits(n, 8, bitcmp.POOL_TWELVE)
    DC.set_channels(sim, chk, vals)
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k, 1: k, 3: 4.0 * stable_kappa(chk, tick, 1.0)})
    kept = chk.attr[2].copy()
    for s in range(3):
        step_both(sim, chk, tick)
        DC.assert_same(sim, chk, f"contents step {s + 1}")
        kept = kept[chk.last_perm]
        assert sim.attribute(2).tobytes() == kept.tobytes()              # kappa = 0: payloads, -0.0 and denormals bit for bit
    assert np.isnan(chk.attr[1]).any() and np.isfinite(chk.attr[0]).all()
    sim.close(); chk.close()


# ---- buoyancy -----------------------------------------------------------------------------------------------------------------------
def test_buoyancy_alone(fs):
    run(fs, "pair12", (), (1, 0.002, 0.0))


def test_buoyancy_with_diffusion_inside_and_outside_the_set(fs):
    run(fs, "pair12", (0, 1), (1, 0.002, 0.0))
    run(fs, "pair12", (0, 3), (1, 0.002, 0.0))


def test_buoyancy_with_surface_tension(fs):
    """fb = st + bv, and surface_tension_forces() is still st (assert_same compares both)"""
    run(fs, "pair12", (0,), (0, 0.5, 0.0), surface_tension=ST_CFG)
    run(fs, "pair12", (), (0, 0.5, 0.0), surface_tension=ST_CFG)


@pytest.mark.parametrize("with_st", [False, True])
def test_buoyancy_with_a_collider(fs, with_st):
    field = CR.random_field((12, 10, 8), 4, fill=0.3, mag=0.05)
    run(fs, "pair12", (0, 2), (0, 0.5, 0.0), surface_tension=ST_CFG if with_st else None, field=field)


def test_beta_zero(fs):
    run(fs, "pair12", (0,), (0, 0.0, 1.0))


@pytest.mark.parametrize("gravity", [(0.3, 0.0, -0.2), (0.0, 9.81, 0.0), (0.0, 0.0, 0.0)])
def test_gravity_with_zero_components(fs, gravity):
    run(fs, "pair12", (3,), (0, 0.5, 0.0), tick_over=dict(gravity=gravity))


def test_buoyancy_set_mid_run_and_cleared_again(fs):
    st, tick, p, _ = DC.scene_state(fs, "pair12")
    sim, chk = DC.make_pair(fs, st, p, 4)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {1: k})
    step_both(sim, chk, tick)
    DC.assert_same(sim, chk, "diffusion only")
    bitcmp.expect_invalid(fs, sim.buoyancy_forces)
    DC.configure(sim, chk, buoyancy=(1, 0.002, 0.0))
    bitcmp.expect_invalid(fs, sim.buoyancy_forces)                       # set, but no step since
    step_both(sim, chk, tick)
    DC.assert_same(sim, chk, "buoyancy on")
    DC.configure(sim, chk, buoyancy=None)
    assert sim.buoyancy is None
    bitcmp.expect_invalid(fs, sim.buoyancy_forces)
    for s in range(2):
        step_both(sim, chk, tick)
        DC.assert_same(sim, chk, f"cleared, step {s + 1}")
    sim.track(2)                                                          # a re-initialising enable clears every setting
    assert sim.diffusion(1) == 0.0 and sim.buoyancy is None
    sim.close(); chk.close()


@pytest.mark.parametrize("mass", [1.0, 1.25])
@pytest.mark.parametrize("h", [0.1, 0.2, 0.4])
def test_radius_and_mass(fs, h, mass):
    ref, st, tick, p = paths3d.pair3_state(fs, O, 12, h=h, mass=mass)
    ref.close()
    sim, chk = DC.make_pair(fs, st, p, 4)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k, 1: k, 2: k}, (2, 1e-30, 0.0))
    for s in range(3):
        step_both(sim, chk, tick)
        DC.assert_same(sim, chk, f"h {h} m {mass} step {s + 1}")
    sim.close(); chk.close()


# ---- the step's other entrances -------------------------------------------------------------------------------------------------
def test_tick_timed_and_profiled_steps_and_calls_between_unsynchronised_steps(fs):
    st, tick, p, _ = DC.scene_state(fs, "pair12")
    sim, chk = DC.make_pair(fs, st, p, 4)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k}, (0, 0.5, 0.0))
    sim.tick(tick); chk.step(tick)
    DC.configure(sim, chk, {0: 0.5 * k, 3: k}, (3, 0.25, 0.1))           # no sync: the step in flight keeps what it was enqueued with
    sim.tick(tick); chk.step(tick)
    DC.configure(sim, chk, {0: 0.0})
    sim.timed_steps(tick, 2); chk.step(tick); chk.step(tick)
    DC.assert_same(sim, chk, "after tick, tick, timed_steps(2)")
    sim.profile(True)
    sim.tick(tick); chk.step(tick)
    ms, steps = sim.profile_read()
    assert steps == 1
    sim.profile(False)
    DC.assert_same(sim, chk, "after a profiled step")
    sim.close(); chk.close()


def test_refusals_in_the_headers_order(fs):
    st, tick, p, _ = DC.scene_state(fs, "pair12")
    sim = fs.FluidSimulation3D(st, device=0)
    inv = lambda call: bitcmp.expect_invalid(fs, call)                   # noqa: E731
    # 2. tracking off comes before the channel and the values
    inv(lambda: sim.set_diffusion(-1, float("nan")))
    assert b"tracking is off" in fs.load_library().fs_last_error()
    inv(lambda: sim.diffusion(0)); inv(lambda: sim.set_buoyancy(0, 1.0, 0.0)); inv(lambda: sim.buoyancy)
    sim.track(2)
    # 3. the channel comes before the values
    inv(lambda: sim.set_diffusion(2, -1.0))
    assert b"no such channel" in fs.load_library().fs_last_error()
    inv(lambda: sim.set_diffusion(-1, 1.0)); inv(lambda: sim.diffusion(2))
    inv(lambda: sim.set_buoyancy(2, float("inf"), 0.0))
    assert b"no such channel" in fs.load_library().fs_last_error()
    inv(lambda: sim.set_buoyancy(-2, 1.0, 0.0))
    # 4. and 5. the values
    for bad in (-1.0, float("nan"), float("inf")):
        inv(lambda: sim.set_diffusion(0, bad))
    for bad in (float("nan"), float("inf"), -float("inf")):
        inv(lambda: sim.set_buoyancy(0, bad, 0.0)); inv(lambda: sim.set_buoyancy(0, 1.0, bad))
    assert sim.diffusion(0) == 0.0 and sim.buoyancy is None              # a refused call changes nothing
    # fs3_download_buoyancy: a channel is set, a step since, n
    inv(sim.buoyancy_forces)
    sim.set_buoyancy(1, 0.5, 0.25)
    assert sim.buoyancy == (1, 0.5, 0.25)
    inv(sim.buoyancy_forces)
    sim.tick(tick)
    assert sim.buoyancy_forces().shape == (sim.particle_count, 3)
    buf = np.zeros((5, 3), dtype=f32)
    inv(lambda: sim._call("download_buoyancy", buf.ctypes.data, 5))
    sim.untrack()
    inv(lambda: sim.diffusion(0))
    sim.track(1)
    assert sim.buoyancy is None
    sim.close()


# ---- tolerance mode ---------------------------------------------------------------------------------------------------------------
def test_tolerance_mode_scene_within_the_bound(fs):
    """One FS_MATH_TOLERANCE step of a path scene against the checker.  The pass is the IEEE one in both; its perturbed inputs are
    the densities, which the mode's contract holds to 1e-5 relative (the 3D density contract): w_j = m / rho_j and
    u_i = 1 / rho_i each move by 1e-5, and the two f32 sums round differently once their terms differ.  With the terms t_j
    evaluated in float64 on the checker's state and K the in-radius count:
        |A' - A'_chk| <= (2e-5 + 2 (K + 8) 2^-24) g u_i sum_j |t_j| + 2 * 2^-24 |A'|
    The keys come from the uploaded state alone, so the carry is the checker's bit for bit.  The worst share is printed."""
    name = "probes100"
    st, tick, p, _ = DC.scene_state(fs, name)
    sim, chk = DC.make_pair(fs, st, p, 4, math_mode=fs.FS_MATH_TOLERANCE)
    DC.set_channels(sim, chk, DC.fill_channels(p, 4))
    k = stable_kappa(chk, tick)
    DC.configure(sim, chk, {0: k, 1: k})
    step_both(sim, chk, tick)
    assert np.array_equal(sim.particle_ids(), chk.ids)
    rec = chk.particles()
    worst = 0.0
    for c in (0, 1):
        g = float((f32(2.0) * f32(k)) * f32(tick.delta))
        want, tabs, K, _ = DC.restatement(chk, rec, chk.attr_in[c], tick.mass, g)
        got = sim.attribute(c).astype(np.float64)
        ref = chk.attr[c].astype(np.float64)
        bound = (2e-5 + 2 * (K + 8) * 2.0 ** -24) * tabs + 2 * 2.0 ** -24 * np.abs(ref)
        moved = tabs > 0
        assert (np.abs(got - ref) <= bound).all(), f"channel {c}: worst excess {np.max(np.abs(got - ref) - bound):.3e}"
        worst = max(worst, float(np.max(np.abs(got - ref)[moved] / bound[moved])))
    for c in (2, 3):
        assert sim.attribute(c).tobytes() == chk.attr[c].tobytes()
    print(f"[tolerance3d] {name}: worst share of the bound {worst:.3f}")
    sim.close(); chk.close()

"""GPU tests of the opt-in surface tension: k_surface_tension + the ST instantiations of the force kernels
against the CPU checker (tests/st_checker.cpp: the oracle plus the statement), bit for bit in FS_MATH_IEEE — every field of
every particle, start_indices and the st buffer — and within the per-step contract in the other math modes.
The pass at the plain step's hard inputs (operand guards, radii, random configurations, grid edges, mouse and field, the force in
the other math modes, host paths, A/B switches): tests/test_surface_tension_hard_inputs_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests.bitcmp import assert_records_equal, bits
from tests.dense_scene import dense_scene

pytestmark = pytest.mark.gpu
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")


def assert_state_equal(sim, chk, ctx, st=True):
    assert_records_equal(sim.download_particles(), chk.particles_view(), ctx)
    assert np.array_equal(sim.download_start_indices(), chk.start_indices_view()), f"{ctx}: start_indices"
    if st:
        a, b = bits(sim.surface_tension_forces()), bits(chk.st)
        assert np.array_equal(a, b), f"{ctx}: st not bit-exact ({int((a != b).sum())} words differ)"


def make_pair(fs, st, off=(0.0, 0.0), quirks=True, sort_mode=None, seed=None, **kw):
    from tests.st_ref import STChecker
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=quirks,
                             sort_mode=fs.FS_SORT_BITONIC if sort_mode is None else sort_mode, surface_tension=True, **kw)
    chk = STChecker(st, off, ref_quirks=quirks)
    if seed is not None:
        rng = np.random.default_rng(seed)
        p = chk.particles()
        p["position"] += rng.uniform(-0.025, 0.025, size=p["position"].shape).astype(np.float32)
        p["predicted_position"] = p["position"]
        p["velocity"] = rng.uniform(-1.0, 1.0, size=p["velocity"].shape).astype(np.float32)
        chk.set_particles(p)
        sim.upload_particles(p)
    return sim, chk


def run_compare(sim, chk, tick, steps, ctx, stable=False, every=1):
    for s in range(steps):
        sim.tick(tick)
        chk.step(tick, stable_sort=stable)
        if s % every == every - 1 or s == steps - 1:
            assert_state_equal(sim, chk, f"{ctx} step {s}")
    assert np.any(chk.st != 0.0), f"{ctx}: no particle felt surface tension"


def test_two_particle_known_answer(fs):
    """Two particles at r < h, no gravity, pressure or viscosity: st and the velocity after one step equal the float64
    closed form of the statement (independent of the checker)."""
    h, r = 0.2, (0.1, 0.03)
    st = fs.SimulationSettings(2, 0.1, h, (4.0, 4.0))
    tick = fs.default_tick_settings(gravity=(0.0, 0.0))
    tick.pressure_constant = 0.0
    tick.viscosity_coefficient = 0.0
    tick.surface_tension_coefficient = 35.0
    sim = fs.FluidSimulation(st, device=0, surface_tension=True)
    p = sim.download_particles()
    p["position"] = np.float32([[0.31, -0.42], [0.31 + r[0], -0.42 + r[1]]])
    p["predicted_position"] = p["position"]
    p["velocity"] = 0.0
    sim.upload_particles(p)
    sim.tick(tick)
    got = sim.download_particles()
    f = sim.surface_tension_forces().astype(np.float64)
    x = got["predicted_position"].astype(np.float64)
    o = x[1] - x[0]
    r2 = float(o @ o)
    h2 = h * h
    c = 4.0 / (np.pi * h ** 8)
    rho = c * (h2 ** 3 + (h2 - r2) ** 3)
    cg, cl = 24.0 / (np.pi * h ** 8), 48.0 / (np.pi * h ** 8)
    d = h2 - r2
    for i, sgn in ((0, 1.0), (1, -1.0)):
        n = (1.0 / rho) * cg * d * d * (sgn * o)
        L = (1.0 / rho) * (cl * h2 * (-h2) + cl * d * (3.0 * r2 - h2))
        want = (-35.0 * L / np.linalg.norm(n)) * n
        np.testing.assert_allclose(f[i], want, rtol=1e-5)
        np.testing.assert_allclose(got["velocity"][i], want / rho * tick.delta, rtol=1e-5)
    np.testing.assert_allclose(got["density"], [rho, rho], rtol=1e-5)
    assert np.linalg.norm(f[0]) > 1.0                     # a real force, pulling the pair together
    assert f[0] @ o > 0 and f[1] @ o < 0
    sim.close()


def test_bitexact_dam_break_bitonic(fs):
    st, off, tick = fs.dam_break_2d(4096)
    sim, chk = make_pair(fs, st, off)
    run_compare(sim, chk, tick, 24, "bitonic 4096")


def test_bitexact_counting_sort(fs):
    st, off, tick = fs.dam_break_2d(4096)
    sim, chk = make_pair(fs, st, off, sort_mode=fs.FS_SORT_COUNTING, seed=3)
    run_compare(sim, chk, tick, 20, "counting 4096", stable=True)


@pytest.mark.parametrize("n", [5000, 4097, 1029])
def test_bitexact_ragged_mass_and_no_quirks(fs, n):
    """Ragged N, particle_mass != 1 (the w = m / rho_j division, not the MASS1 reciprocal) and ref_quirks off."""
    st, off, tick = fs.dam_break_2d(n)
    tick.mass = 1.25
    tick.rest_density = 120.0
    sim, chk = make_pair(fs, st, off, quirks=False, seed=n)
    run_compare(sim, chk, tick, 12, f"ragged {n}")


def test_long_run_exercises_stale_quirk(fs):
    st, off, tick = fs.dam_break_2d(4096)
    sim, chk = make_pair(fs, st, off)
    hits = 0
    for s in range(260):
        sim.tick(tick)
        chk.step(tick)
        if s % 10 == 9 or s > 250:
            assert_state_equal(sim, chk, f"long step {s}")
            si = chk.start_indices()
            hits += int(si[chk.particles()["grid"][0]] != 0)
    assert hits > 0, "the stale-min-cell quirk never fired; the test lost its point"


@pytest.mark.parametrize("n", [1 << 20, 1 << 24])
def test_bitexact_large(fs, n):
    """1 M and the 16 M dam break, two steps each: the LDS-tile path and the unfit-block fallback at scale."""
    import bench
    from tests import st_ref
    st, off, tick = fs.dam_break_2d(n)
    sim, chk = make_pair(fs, st, off)
    st_ref.set_threads(min(bench.usable_cores(), int(st_ref.lib().orc_max_threads())))
    try:
        for s in range(2):
            sim.tick(tick)
            chk.step(tick)
            assert_state_equal(sim, chk, f"{n} step {s}")
    finally:
        st_ref.set_threads(1)
    sim.close(); chk.close()


@pytest.mark.parametrize("path", ["general", "quad", "aos"])
def test_every_force_path_bitexact(fs, monkeypatch, path):
    """A dense cluster (rows longer than the tiles: k_force_general and the unstaged ST sweep), FS_FORCE_QUAD_ALWAYS
    (k_force_quad) and a registered export handle (the AOS instantiations: the force pass writes the records itself)."""
    from tests.st_ref import STChecker
    st, tick, p = dense_scene(fs)
    if path == "quad":
        monkeypatch.setenv("FS_FORCE_QUAD_ALWAYS", "1")
    sim = fs.FluidSimulation(st, device=0, surface_tension=True)
    monkeypatch.delenv("FS_FORCE_QUAD_ALWAYS", raising=False)
    chk = STChecker(st)
    sim.upload_particles(p); chk.set_particles(p)
    if path == "aos":
        sim.export_handle(fs._abi.FS_EXPORT_PARTICLES)
    for s in range(4):
        sim.tick(tick)
        chk.step(tick)
        assert_state_equal(sim, chk, f"{path} step {s}")
        if path == "aos":
            lib = fs.load_library()
            rec = np.empty(st.particle_count, dtype=fs.PARTICLE_DTYPE)
            assert lib.fs_import_read(sim.particles_device_ptr(), 0, rec.ctypes.data_as(C.c_void_p), rec.nbytes) == 0
            assert rec.tobytes() == sim.download_particles().tobytes()
    cells, cnt = np.unique(chk.particles()["grid"], return_counts=True)
    assert cnt.max() > 150
    sim.close(); chk.close()


@pytest.mark.parametrize("mode", ["tolerance", "ulp"])
def test_other_math_modes_within_contract(fs, mode):
    """One step from the same (disordered) state: keys, start_indices and predicted positions exact; density rtol 1e-5,
    velocity rtol 1e-5 / atol 2e-5, position atol 1e-4 h — the modes' per-step contract against the IEEE statement."""
    from tests.st_ref import STChecker
    from tests.parity_states import disordered_dam_break
    st, off, tick, p = disordered_dam_break(fs)
    chk = STChecker(st, off)
    chk.set_particles(p)
    for _ in range(3):
        chk.step(tick)
    mm = fs.FS_MATH_TOLERANCE if mode == "tolerance" else fs.FS_MATH_WGSL_ULP
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=mm, surface_tension=True)
    sim.upload_particles(chk.particles())
    sim.upload_start_indices(chk.start_indices())
    sim.tick(tick)
    chk.step(tick)
    got, want = sim.download_particles(), chk.particles()
    h = st.smoothing_radius
    assert np.array_equal(got["grid"], want["grid"])
    assert np.array_equal(sim.download_start_indices(), chk.start_indices())
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32))
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h)
    assert np.any(chk.st != 0.0)
    sim.close(); chk.close()


def test_off_by_default_and_disable_returns_to_the_plain_step(fs, orc):
    st, off, tick = fs.dam_break_2d(4096)
    plain = fs.FluidSimulation(st, device=0, initial_offset=off)
    assert not plain.surface_tension_enabled
    plain.close()
    sim, chk = make_pair(fs, st, off)
    assert sim.surface_tension_enabled
    run_compare(sim, chk, tick, 5, "enabled")
    sim.set_surface_tension(False)
    assert not sim.surface_tension_enabled
    ref = orc.OracleSim(st, off)
    ref.set_particles(sim.download_particles())
    ref.start_indices_view()[:] = sim.download_start_indices()
    for s in range(5):
        sim.tick(tick)
        ref.step(tick)
        got, want = sim.download_particles(), ref.particles()
        assert got.tobytes() == want.tobytes(), f"disabled step {s}"
        assert np.array_equal(sim.download_start_indices(), ref.start_indices())
    sim.close()


@pytest.mark.parametrize("knob", ["tau_inf", "sigma_zero"])
def test_neutral_settings_equal_the_plain_step(fs, knob):
    st, off, tick = fs.dam_break_2d(4096)
    if knob == "tau_inf":
        tick.surface_tension_treshold = float("inf")
    else:
        tick.surface_tension_coefficient = 0.0
    on = fs.FluidSimulation(st, device=0, initial_offset=off, surface_tension=True)
    off_ = fs.FluidSimulation(st, device=0, initial_offset=off)
    for s in range(8):
        on.tick(tick); off_.tick(tick)
        a, b = on.download_particles(), off_.download_particles()
        assert np.array_equal(a["grid"], b["grid"])
        for f in FLOAT_FIELDS:
            assert np.array_equal(a[f], b[f]), f"{knob} step {s}: {f}"
    assert np.all(on.surface_tension_forces() == 0.0)
    on.close(); off_.close()


def _block_spread(fs, surface_tension, steps=50):
    """A 30 x 30 lattice block (spacing 0.1, h 0.2) in zero gravity with rest_density 100 (its interior density is 101.46):
    RMS distance from the centroid and the mean distance of the four outermost particles (the corners)."""
    st = fs.SimulationSettings(900, 0.1, 0.2, (10.0, 10.0))
    tick = fs.default_tick_settings(gravity=(0.0, 0.0))
    tick.rest_density = 100.0
    tick.surface_tension_coefficient = 35.0
    sim = fs.FluidSimulation(st, device=0, surface_tension=surface_tension)
    for _ in range(steps):
        sim.tick(tick)
    p = sim.download_particles()["position"].astype(np.float64)
    sim.close()
    d = np.hypot(*(p - p.mean(0)).T)
    return np.sqrt((d ** 2).mean()), np.sort(d)[-4:].mean()


def test_physics_block_rounds_up(fs):
    """CPU checker, same scene: off rms 1.250 / corners 2.032, on rms 1.121 / corners 1.808 after 50 steps (the block
    starts at rms 1.22 / corners 2.05).  Asserted: both at least 5 % smaller with surface tension."""
    rms_off, cor_off = _block_spread(fs, False)
    rms_on, cor_on = _block_spread(fs, True)
    assert rms_on < 0.95 * rms_off, (rms_on, rms_off)
    assert cor_on < 0.95 * cor_off, (cor_on, cor_off)


def test_errors(fs):
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    with pytest.raises(fs.FluidSimError) as e:                   # never enabled
        sim.surface_tension_forces()
    assert e.value.status == fs._abi.FS_ERR_INVALID
    sim.tick(tick)
    sim.set_surface_tension(True)
    with pytest.raises(fs.FluidSimError) as e:                   # enabled, but no ST step yet
        sim.surface_tension_forces()
    assert e.value.status == fs._abi.FS_ERR_INVALID
    sim.tick(tick)
    assert sim.surface_tension_forces().shape == (4096, 2)
    lib = fs.load_library()
    buf = np.empty((4095, 2), dtype=np.float32)
    assert lib.fs_download_surface_tension(sim._h, buf.ctypes.data_as(C.c_void_p), 4095) == fs._abi.FS_ERR_INVALID
    sim.set_surface_tension(False); sim.set_surface_tension(True)  # re-enabled: the last forces are no longer "this enable's"
    with pytest.raises(fs.FluidSimError) as e:
        sim.surface_tension_forces()
    assert e.value.status == fs._abi.FS_ERR_INVALID
    sim.close()
    st2, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st2, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    assert lib.fs_set_surface_tension(slab._h, 1) == fs._abi.FS_ERR_UNSUPPORTED
    assert lib.fs_surface_tension_enabled(slab._h) == 0
    slab.close()

"""GPU tests of the opt-in diffusion and buoyancy of the tracking channels: k_diffuse / k_buoyancy against the CPU
checker (tests/diffuse_checker.cpp through tests/diffuse_ref.py).  FS_MATH_IEEE is compared bit for bit: ids, channels, fb, every
float of the state, keys and start_indices; a float that is a NaN on the checker must be a NaN on the engine (payload and sign
of a NaN are not compared: host and device default NaNs differ).  Every case runs at least 3 steps.  That the cases are not
vacuous is asserted without a GPU in tests/test_diffusion.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import diffuse_cases as DC
from tests import features2d as F
from tests import hard_states2d as H
from tests import parity_states as PS
from tests.bitcmp import assert_records_equal, assert_track_equal, bits, same_words

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24


def assert_step_equal(sim, ref, ctx, state=True):
    assert_track_equal(sim, ref, ctx, nan_any=True)
    if ref.fb is not None:
        ok = same_words(sim.buoyancy_forces(), ref.fb)
        assert ok.all(), f"{ctx}: fb differs in {int((~ok).sum())} words"
    if not state:
        return
    assert_records_equal(sim.download_particles(), ref.particles_view(), ctx, nan_any=True)
    assert np.array_equal(sim.download_start_indices(), ref.start_indices_view()), f"{ctx}: start_indices"


def engine(fs, st, off, quirks, sort, start, start_indices=None, field=None, channels=4, **kw):
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=quirks,
                             sort_mode=fs.FS_SORT_COUNTING if sort == "counting" else fs.FS_SORT_BITONIC, track=channels, **kw)
    sim.upload_particles(start)
    if start_indices is not None:
        sim.upload_start_indices(start_indices)
    if field is not None:
        sim.upload_force_field(field)
    return sim


def checker(st, off, quirks, start, channels=4, start_indices=None, field=None):
    from tests.diffuse_ref import DiffuseChecker
    chk = DiffuseChecker(st, off, ref_quirks=quirks, channels=channels)
    chk.set_particles(start)
    if start_indices is not None:
        chk.start_indices_view()[:] = start_indices
    if field is not None:
        chk.texture_view()[:] = field
    return chk


def configure(sim, chk, values, kappa, buoyancy=None):
    """the same channels and settings on both sides"""
    for c, v in enumerate(values):
        sim.set_attribute(c, v)
        chk.attr[c] = v
    for c, k in enumerate(kappa):
        sim.set_diffusion(c, k)
        assert sim.diffusion(c) == float(f32(k))
    chk.kappa = [float(f32(k)) for k in kappa] + [0.0] * (4 - len(kappa))
    if buoyancy is not None:
        sim.set_buoyancy(*buoyancy)
        assert sim.buoyancy == (buoyancy[0], float(f32(buoyancy[1])), float(f32(buoyancy[2])))
    chk.buoyancy = buoyancy


def run_both(sim, chk, tick, steps, stable, ctx, state=True):
    with np.errstate(all="ignore"):
        for s in range(steps):
            sim.tick(tick)
            chk.step(tick, stable)
            assert_step_equal(sim, DC.Ref(chk), f"{ctx} step {s}", state)


def stable_kappa(chk, tick, stable, target=0.5):
    return DC.kappa_for(DC.pass_of_next_step(chk, tick, stable)["R"], float(tick.delta), target)


# ---- 1. the registry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", DC.SORTS)
@pytest.mark.parametrize("cid", H.CASE_IDS)
def test_registry(fs, orc, cid, sort):
    case = H.case_by_id(fs, orc, cid)
    case.run()                                          # settles the upload order (hard_states2d.Case.run)
    run = DC.registry_run(fs, case, sort)
    sim = engine(fs, case.st, case.off, case.quirks, sort, case.start, case.start_indices, case.field)
    for c in range(DC.CHANNELS):
        sim.set_attribute(c, run.values[c])
        sim.set_diffusion(c, run.kappa[c])
    sim.set_buoyancy(0, DC.BETA, DC.REFERENCE)
    for s, ref in enumerate(run.steps):
        sim.tick(case.tick)
        assert_step_equal(sim, ref, f"{cid}/{sort} step {s}")
    sim.close()


# ---- 2. counts, strides, subsets ------------------------------------------------------------------------------------------------------
def dam(fs, orc, n, **over):
    return PS.jittered_dam_break(fs, orc, n, n, size=PS.RAGGED_BOX, **over)


@pytest.mark.parametrize("sort", DC.SORTS)
@pytest.mark.parametrize("n", [2, 3, 5, 257, 4097])
def test_counts_with_capacity_above_n(fs, orc, n, sort):
    """one block and a lane, a block and a lane more than sixteen; the channel stride is the capacity, not n"""
    st, off, tick, p = dam(fs, orc, n)
    sim = engine(fs, st, off, True, sort, p, capacity=n + 300)
    chk = checker(st, off, True, p)
    assert sim.attribute_device_ptr(1) - sim.attribute_device_ptr(0) >= 4 * (n + 300)
    k = stable_kappa(chk, tick, sort == "counting")
    configure(sim, chk, DC.channel_values(n), [k, 0.0, 4.0 * k, k], (2, 0.02, 0.1))
    run_both(sim, chk, tick, 3, sort == "counting", f"n={n} {sort}")
    sim.close(); chk.close()


SUBSETS = [(0,), (1, 3), (0, 1, 2), (0, 1, 2, 3)]


@pytest.mark.parametrize("subset", SUBSETS, ids=["".join(map(str, s)) for s in SUBSETS])
def test_diffusing_subsets(fs, orc, subset):
    """D = 1 .. 4 with the compact channel list; a channel outside the subset is a bit copy of what tracking alone gives"""
    n = 4097
    st, off, tick, p = dam(fs, orc, n)
    sim = engine(fs, st, off, True, "bitonic", p)
    plain = engine(fs, st, off, True, "bitonic", p)
    chk = checker(st, off, True, p)
    k = stable_kappa(chk, tick, False)
    vals = DC.channel_values(n)
    configure(sim, chk, vals, [k * (c + 1) if c in subset else 0.0 for c in range(4)])
    for c in range(4):
        plain.set_attribute(c, vals[c])
    with np.errstate(all="ignore"):
        for s in range(3):
            sim.tick(tick); plain.tick(tick); chk.step(tick)
            assert_step_equal(sim, DC.Ref(chk), f"subset {subset} step {s}")
            for c in set(range(4)) - set(subset):
                assert np.array_equal(bits(sim.attribute(c)), bits(plain.attribute(c))), f"channel {c} (kappa 0) is no bit copy"
    assert max((bits(chk.acc[c]) << 1 != 0).mean() for c in subset) > 0.5      # (channel 1 is constant: its sums are +0)
    sim.close(); plain.close(); chk.close()


CHILD = '''
import sys
import numpy as np
sys.path.insert(0, ".")
import gpu_fluid_simulation_amd as fs
from oracle import oracle as orc
from tests import test_diffusion_gpu as T
T.switch_scenes(fs, orc)
print("ok")
'''


def switch_scenes(fs, orc):
    """what a child with a switch in its environment runs: the 4097 dam break and dense_scene, four diffusing channels and a
    buoyancy channel, 3 steps against the checker"""
    from tests.dense_scene import dense_scene
    st, off, tick, p = dam(fs, orc, 4097)
    st2, tick2, p2 = dense_scene(fs)
    for name, (st, off, tick, p) in {"dam4097": (st, off, tick, p), "dense": (st2, (0.0, 0.0), tick2, p2)}.items():
        n = p.shape[0]
        sim = engine(fs, st, off, True, "bitonic", p)
        chk = checker(st, off, True, p)
        k = stable_kappa(chk, tick, False)
        configure(sim, chk, DC.channel_values(n), [k, 2.0 * k, 3.0 * k, k], (1, 0.02, 0.1))
        run_both(sim, chk, tick, 3, False, name)
        sim.close(); chk.close()


SWITCHES = [("FS_DIFFUSE_SPLIT", "0"), ("FS_NO_BLOCK_BOUNDS", "1"), ("FS_NO_MASS1", "1")]


@pytest.mark.parametrize("var,value", SWITCHES, ids=[f"{v}={x}" for v, x in SWITCHES])
def test_ab_switch(fs, orc, var, value):
    """The switches are read once per process, so each runs in a child with the variable in its environment only: D = 4 as one
    launch (FS_DIFFUSE_SPLIT=0; two launches of D = 2 are the default and what every other test runs, against the same checker:
    equal bytes), the pass's own reduction of the block ranges (FS_NO_BLOCK_BOUNDS) and the density pass's general form at mass 1."""
    switch_scenes(fs, orc)                             # the same scenes in this process, without the switch
    env = dict(os.environ)
    env[var] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ---- 3. scenes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [1.0, 1.25])
@pytest.mark.parametrize("h", [0.05, 0.2, 1.0])
def test_radii_and_masses(fs, orc, h, mass):
    """Cg = 24/(pi h^8) from 1.5 (h = 1) to 2e11 (h = 0.05); both forms of the weight (MASS1 and the division)"""
    case = F.radius_case(fs, orc, h)
    tick = F.copy_tick(case.tick, mass=mass)
    n = case.start.shape[0]
    sim = engine(fs, case.st, case.off, True, "bitonic", case.start)
    chk = checker(case.st, case.off, True, case.start)
    k = stable_kappa(chk, tick, False)
    configure(sim, chk, DC.channel_values(n), [k, 0.0, 4.0 * k, k], (0, 0.02, 0.0))
    run_both(sim, chk, tick, 3, False, f"h={h} m={mass}")
    assert (bits(chk.acc[0]) << 1 != 0).mean() > 0.5
    sim.close(); chk.close()


# ---- 4. buoyancy ------------------------------------------------------------------------------------------------------------------------
BUOYANCY = ["alone", "with_diffusion", "with_surface_tension", "beta0", "gravity_x0", "gravity_y0"]


@pytest.mark.parametrize("sort", DC.SORTS)
@pytest.mark.parametrize("variant", BUOYANCY)
def test_buoyancy(fs, orc, variant, sort):
    """k_buoyancy alone, the tail of k_diffuse, fb = st + b, beta = 0 and gravity with one zero component; the pass is enabled
    after two plain steps (the first step after enabling mid-run), and the surface tension's own forces keep their meaning"""
    n = 4097
    grav = {"gravity_x0": (0.0, 9.81), "gravity_y0": (-3.0, 0.0)}.get(variant, (1.5, 9.81))
    st, off, tick, p = dam(fs, orc, n)
    tick = F.copy_tick(tick, gravity=type(tick.gravity)(*grav))
    stn = variant == "with_surface_tension"
    sim = engine(fs, st, off, True, sort, p, surface_tension=stn)
    chk = checker(st, off, True, p)
    chk.surface_tension = stn
    stable = sort == "counting"
    vals = DC.channel_values(n)
    vals[0] = np.random.default_rng(5).uniform(-2.0, 3.0, n).astype(f32)
    configure(sim, chk, vals, [0.0] * 4)
    run_both(sim, chk, tick, 2, stable, f"{variant} plain")
    with pytest.raises(fs.FluidSimError):
        sim.buoyancy_forces()                           # no step with a buoyancy channel yet
    k = stable_kappa(chk, tick, stable)
    kappa = [k, 0.0, 0.0, k] if variant != "alone" else [0.0] * 4
    configure(sim, chk, [], kappa, (0, 0.0 if variant == "beta0" else 0.05, 0.5))
    run_both(sim, chk, tick, 3, stable, f"{variant}/{sort}")
    s = f32(0.05) * (f32(0.5) - chk.attr_in[0])
    assert (s > 0).any() and (s < 0).any()
    if stn:
        ok = same_words(sim.surface_tension_forces(), chk.st)
        assert ok.all(), "surface_tension_forces() no longer holds st alone"
        assert (bits(chk.st) << 1 != 0).any() and not np.array_equal(bits(chk.st), bits(chk.fb))
    sim.clear_buoyancy()
    assert sim.buoyancy is None
    chk.buoyancy = None
    run_both(sim, chk, tick, 1, stable, f"{variant}/{sort} after clear_buoyancy")
    sim.close(); chk.close()


# ---- 5. the state is untouched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "wgsl_ulp", "tolerance"])
@pytest.mark.parametrize("sort", DC.SORTS)
def test_state_untouched_without_buoyancy(fs, orc, sort, mode):
    n = 4097
    st, off, tick, p = dam(fs, orc, n)
    mm = {"ieee": fs.FS_MATH_IEEE, "wgsl_ulp": fs.FS_MATH_WGSL_ULP, "tolerance": fs.FS_MATH_TOLERANCE}[mode]
    a = engine(fs, st, off, True, sort, p, math_mode=mm)
    b = engine(fs, st, off, True, sort, p, math_mode=mm)
    vals = DC.channel_values(n)
    for c in range(4):
        a.set_attribute(c, vals[c]); b.set_attribute(c, vals[c])
        a.set_diffusion(c, 0.5 * (c + 1))
    for s in range(3):
        a.tick(tick); b.tick(tick)
        assert a.download_particles().tobytes() == b.download_particles().tobytes(), f"{sort}/{mode} step {s}: state"
        assert np.array_equal(a.download_start_indices(), b.download_start_indices())
        assert np.array_equal(a.particle_ids(), b.particle_ids())
    assert not np.array_equal(bits(a.attribute(0)), bits(b.attribute(0)))           # the pass did run
    a.close(); b.close()


# ---- 6. host paths ----------------------------------------------------------------------------------------------------------------------
def test_tick_timed_and_profiled_steps_give_the_same_bytes(fs, orc):
    n = 4097
    st, off, tick, p = dam(fs, orc, n)
    chk = checker(st, off, True, p)
    k = stable_kappa(chk, tick, False)
    chk.close()
    out = []
    for path in ("tick", "timed", "profiled"):
        sim = engine(fs, st, off, True, "bitonic", p)
        vals = DC.channel_values(n)
        for c in range(4):
            sim.set_attribute(c, vals[c])
            sim.set_diffusion(c, k)
        sim.set_buoyancy(0, 0.02, 0.0)
        if path == "timed":
            sim.timed_steps(tick, 3)
        else:
            if path == "profiled":
                sim.profile(True)
            for _ in range(3):
                sim.tick(tick)
            if path == "profiled":
                ms, steps = sim.profile_read()
                assert steps == 3
        out.append((sim.download_particles().tobytes(), [sim.attribute(c).tobytes() for c in range(4)], sim.buoyancy_forces().tobytes()))
        sim.close()
    assert out[0] == out[1] == out[2]


def reseeded(fs, sim, st, off, ticks, tick, stable):
    """a checker at the handle's current count holding its download: records, start indices, ids, channels — and its tick count
    (the oracle seeds its coincident-pair PRNG with it and has no setter: a fresh oracle is first advanced on its own lattice)"""
    n = sim.particle_count
    st2 = fs.SimulationSettings(n, st.particle_spacing, st.smoothing_radius, (st.size.x, st.size.y), (st.texture_size.x, st.texture_size.y))
    from tests.diffuse_ref import DiffuseChecker
    chk = DiffuseChecker(st2, off, ref_quirks=True, channels=sim.track_channels)
    with np.errstate(all="ignore"):
        for _ in range(ticks):
            chk.step(tick, stable)
    chk.reset()
    chk.set_particles(sim.download_particles())
    chk.start_indices_view()[:] = sim.download_start_indices()
    chk.ids = sim.particle_ids()
    for c in range(chk.channels):
        chk.attr[c] = sim.attribute(c)
    return chk


@pytest.mark.parametrize("sort", DC.SORTS)
def test_after_emit_and_remove_box(fs, orc, sort):
    n = 4097
    st, off, tick, p = dam(fs, orc, n)
    stable = sort == "counting"
    sim = engine(fs, st, off, True, sort, p, capacity=n + 512)
    chk = checker(st, off, True, p)
    k = stable_kappa(chk, tick, stable)
    kappa, buoy = [k, 0.0, 2.0 * k, k], (0, 0.02, 0.1)
    configure(sim, chk, DC.channel_values(n), kappa, buoy)
    run_both(sim, chk, tick, 2, stable, "before the emit")
    chk.close()
    ticks = 2
    extra = p[:300].copy()
    extra["position"] += f32(0.013); extra["predicted_position"] = extra["position"]
    sim.emit(extra)
    assert sim.particle_count == n + 300
    with pytest.raises(fs.FluidSimError):
        sim.buoyancy_forces()                           # the count changed: fb no longer belongs to the state
    sim.set_attribute(0, np.random.default_rng(8).uniform(-1, 1, n + 300).astype(f32))
    for what in ("emit", "remove_box"):
        if what == "remove_box":
            removed = sim.remove_box((-1.0, -10.0), (0.5, 10.0))
            assert 0 < removed < sim.particle_count + removed
        chk = reseeded(fs, sim, st, off, ticks, tick, stable)
        chk.kappa, chk.buoyancy = [float(f32(x)) for x in kappa], buoy
        assert sim.diffusion(0) == chk.kappa[0] and sim.buoyancy is not None       # a count change keeps the settings
        run_both(sim, chk, tick, 1, stable, f"after {what}")
        ticks += 1
        chk.close()
    sim.close()


def test_track_again_and_untrack_clear_the_settings(fs, orc):
    st, off, tick, p = dam(fs, orc, 257)
    sim = engine(fs, st, off, True, "bitonic", p)
    sim.set_diffusion(2, 0.25); sim.set_buoyancy(1, 0.5, 2.0)
    assert sim.diffusion(2) == 0.25 and sim.buoyancy == (1, 0.5, 2.0)
    sim.track(3)
    assert [sim.diffusion(c) for c in range(3)] == [0.0] * 3 and sim.buoyancy is None
    sim.set_diffusion(2, 0.25); sim.set_buoyancy(1, 0.5, 2.0)
    sim.untrack()
    with pytest.raises(fs.FluidSimError):
        sim.diffusion(2)
    sim.track(3)
    assert sim.diffusion(2) == 0.0 and sim.buoyancy is None
    for _ in range(3):
        sim.tick(tick)                                  # nothing set: the plain step
    with pytest.raises(fs.FluidSimError):
        sim.buoyancy_forces()
    sim.close()


def test_refusals(fs, orc):
    lib = fs.load_library()
    inv, uns = fs._abi.FS_ERR_INVALID, fs._abi.FS_ERR_UNSUPPORTED
    st, off, tick, p = dam(fs, orc, 257)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    k, c = C.c_float(), C.c_int()
    buf = np.zeros((257, 2), dtype=f32)
    h = sim._h
    # tracking off
    assert lib.fs_set_diffusion(h, 0, 1.0) == inv and lib.fs_get_diffusion(h, 0, C.byref(k)) == inv
    assert lib.fs_set_buoyancy(h, 0, 1.0, 0.0) == inv and lib.fs_set_buoyancy(h, -1, 0.0, 0.0) == inv
    assert lib.fs_get_buoyancy(h, C.byref(c), C.byref(k), C.byref(k)) == inv
    sim.track(2)
    for ch in (-1, 2, 5):
        assert lib.fs_set_diffusion(h, ch, 1.0) == inv and lib.fs_get_diffusion(h, ch, C.byref(k)) == inv
    for ch in (-2, 2, 5):
        assert lib.fs_set_buoyancy(h, ch, 1.0, 0.0) == inv
    for bad in (-1.0, -1e-45, np.inf, -np.inf, np.nan):
        assert lib.fs_set_diffusion(h, 0, float(bad)) == inv
    for bad in (np.inf, -np.inf, np.nan):
        assert lib.fs_set_buoyancy(h, 0, float(bad), 0.0) == inv and lib.fs_set_buoyancy(h, 0, 1.0, float(bad)) == inv
    assert lib.fs_get_diffusion(h, 0, None) == inv and lib.fs_get_buoyancy(h, None, C.byref(k), C.byref(k)) == inv
    assert sim.diffusion(0) == 0.0 and sim.buoyancy is None          # no refused call left a trace
    assert lib.fs_download_buoyancy(h, buf.ctypes.data_as(C.c_void_p), 257) == inv          # no buoyancy step yet
    sim.set_buoyancy(1, 0.5, 0.0)
    sim.tick(tick)
    assert lib.fs_download_buoyancy(h, buf.ctypes.data_as(C.c_void_p), 256) == inv          # n must equal the count
    assert lib.fs_download_buoyancy(h, None, 257) == inv
    assert lib.fs_download_buoyancy(h, buf.ctypes.data_as(C.c_void_p), 257) == 0
    sim.set_buoyancy(0, 0.5, 0.0)                                   # another channel: wait for a step of this setting
    assert lib.fs_download_buoyancy(h, buf.ctypes.data_as(C.c_void_p), 257) == inv
    assert lib.fs_set_diffusion(None, 0, 1.0) == inv and b"null" in lib.fs_last_error()
    sim.close()
    # a slab handle
    st2, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st2, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    for r in (lib.fs_set_diffusion(slab._h, 0, 1.0), lib.fs_get_diffusion(slab._h, 0, C.byref(k)), lib.fs_set_buoyancy(slab._h, 0, 1.0, 0.0),
              lib.fs_get_buoyancy(slab._h, C.byref(c), C.byref(k), C.byref(k)), lib.fs_download_buoyancy(slab._h, buf.ctypes.data_as(C.c_void_p), 257)):
        assert r == uns
    slab.close()


# ---- 7. the other math modes ------------------------------------------------------------------------------------------------------------
def checker_state(fs, orc, mass):
    """the disordered 16384 dam break after three checker steps: records and start_indices (features2d.tolerance_case's state)"""
    st, off, tick, p = PS.disordered_dam_break(fs)
    tick = F.copy_tick(tick, mass=mass)
    chk = checker(st, off, True, p, channels=2)
    with np.errstate(all="ignore"):
        for _ in range(3):
            chk.step(tick)
    return st, off, tick, chk


def test_wgsl_ulp_is_bit_equal_where_the_densities_are(fs, orc):
    st, off, tick, chk = checker_state(fs, orc, 1.0)
    n = chk.n
    sim = engine(fs, st, off, True, "bitonic", chk.particles(), chk.start_indices(), channels=2, math_mode=fs.FS_MATH_WGSL_ULP)
    k = stable_kappa(chk, tick, False)
    vals = [np.random.default_rng(3).uniform(-1, 1, n).astype(f32), DC.special_bits(n)]
    chk.ids = np.arange(n, dtype=np.uint32)
    configure(sim, chk, vals, [k, k])
    sim.tick(tick); chk.step(tick)
    rec, want = sim.download_particles(), chk.particles_view()
    assert np.array_equal(rec["grid"], want["grid"])
    bad = bits(rec["density"]) != bits(want["density"])
    i, j = F.pairs_within(want["predicted_position"].astype(np.float64), float(st.smoothing_radius))
    touched = np.bincount(i, bad[j], n) > 0               # a slot one of whose candidates has another density
    print(f"[wgsl_ulp] densities differ in {int(bad.sum())} slots, {int(touched.sum())} slots see one")
    for c in range(2):
        ok = same_words(sim.attribute(c), chk.attr[c]) | touched
        assert ok.all(), f"channel {c}: {int((~ok).sum())} slots differ although every density they read is the checker's"
    assert (~touched).mean() > 0.5
    sim.close(); chk.close()


@pytest.mark.parametrize("mass", [1.0, 1.25])
def test_tolerance_mode_within_the_derived_bound(fs, orc, mass):
    """One step from a checker state.  The pass is the IEEE one; its perturbed inputs are the densities, 1e-5 relative by the
    mode's contract, so w_j = m / rho_j and u_i = 1 / rho_i move by 1e-5 each, and the two f32 sums round differently once their
    terms differ: 2 (K + 8) 2^-24 on sum |term_j| (float64 terms on the checker's state).  The final addition rounds once on each
    side: 2 * 2^-24 |A'|.  The worst share of the bound is printed (recorded in DESIGN.md §27)."""
    from tests.test_diffusion import restatement
    st, off, tick, chk = checker_state(fs, orc, mass)
    n = chk.n
    sim = engine(fs, st, off, True, "bitonic", chk.particles(), chk.start_indices(), channels=2, math_mode=fs.FS_MATH_TOLERANCE)
    k = stable_kappa(chk, tick, False)
    vals = [np.random.default_rng(3).uniform(-1, 1, n).astype(f32), (chk.particles()["position"][:, 1]).astype(f32)]
    chk.ids = np.arange(n, dtype=np.uint32)
    configure(sim, chk, vals, [k, 0.5 * k])
    sim.tick(tick); chk.step(tick)
    assert np.array_equal(sim.download_particles()["grid"], chk.particles_view()["grid"])
    assert np.array_equal(sim.particle_ids(), chk.ids)
    u = fs.build_uniform(st, tick, 1)
    for c, kc in enumerate(chk.kappa[:2]):
        g = float((f32(2.0) * f32(kc)) * f32(tick.delta))
        want, tabs, K, _ = restatement(chk.particles(), chk.attr_in[c], u.poly6_kernel_derivative, u.sqr_radius, u.particle_mass, g)
        bound = (2e-5 + 2 * (K + 8) * U) * tabs + 2 * U * np.abs(want)
        err = np.abs(sim.attribute(c).astype(np.float64) - chk.attr[c].astype(np.float64))
        print(f"[tolerance] mass {mass} channel {c}: worst share of the bound {float((err / bound).max()):.4f}")
        assert (err <= bound).all()
    sim.close(); chk.close()

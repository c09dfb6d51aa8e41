"""3D step against the 3D oracle where the kernels choose between paths from the data: every sweep (64-bit masks, two-word
masks, staged and unstaged chunks; masks handed over or scanned by the force pass), the operand classification of the
shared-reciprocal quotients, random configurations, walls and grid edges.  Bit equality everywhere except the tolerance-mode
tests, which use the contract stated in include/fluidsim.h (rtol 1e-5, velocity atol 2e-5, position atol 1e-4 h).
Which path a scene runs is asserted from the CPU model in tests/paths3d.py, fed with the oracle's keys."""
import os

import numpy as np
import pytest

import paths3d
from test_3d import _assert_equal3

pytestmark = pytest.mark.gpu
f32 = np.float32


def _assert_tolerance(got, want, h, ctx):
    """the stated contract of FS_MATH_TOLERANCE, one step from an identical state; prints the measured figures first"""
    with np.errstate(all="ignore"):
        d = np.abs(got["density"].astype(np.float64) / want["density"] - 1).max()
        dv = np.abs(got["velocity"].astype(np.float64) - want["velocity"])
        v = (dv - 1e-5 * np.abs(want["velocity"].astype(np.float64))).max()
        x = np.abs(got["position"].astype(np.float64) - want["position"]).max()
    print(f"[tolerance] {ctx}: density rel {d:.3g}, velocity abs {dv.max():.3g} (over rtol part {v:.3g}, atol 2e-5), "
          f"position abs {x:.3g} (atol {1e-4 * h:.3g})")
    assert np.array_equal(got["grid"], want["grid"]), f"{ctx}: cell keys must stay bit-exact in tolerance mode"
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32)), ctx
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5, err_msg=ctx)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5, err_msg=ctx)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h, err_msg=ctx)


# ---- 2. path scenes ---------------------------------------------------------------------------------------------------
SCENES = sorted(paths3d.scenes())


@pytest.mark.parametrize("handoff", ["handoff", "own_scan"])
@pytest.mark.parametrize("name", SCENES)
def test_path_scene_matches_oracle(fs, orc, monkeypatch, name, handoff):
    """every step of the scene: the model says the named sweep carries a wave-plane, and the engine equals the oracle bit for
    bit.  FS3_HANDOFF=0 (read per handle at create): the force pass scans the candidates itself."""
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    if handoff == "own_scan":
        monkeypatch.setenv("FS3_HANDOFF", "0")
    sim = fs.FluidSimulation3D(st, device=0)
    monkeypatch.delenv("FS3_HANDOFF", raising=False)
    ref = orc.OracleSim3D(st)
    ref.set_particles(p); sim.upload_particles(p)
    for s in range(scene.steps):
        sim.tick(tick); ref.step(tick)
        want = ref.particles()
        paths3d.check_scene(scene, [want], ref.grid_dims)
        _assert_equal3(sim.download_particles(), want, f"scene {name}/{handoff} step {s}")
    sim.close(); ref.close()


@pytest.mark.parametrize("name", SCENES)
def test_path_scene_tolerance_mode(fs, orc, name):
    """the same scenes in FS_MATH_TOLERANCE, one step from the uploaded state, under the mode's stated contract"""
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    sim = fs.FluidSimulation3D(st, device=0, math_mode=fs.FS_MATH_TOLERANCE)
    ref = orc.OracleSim3D(st)
    ref.set_particles(p); sim.upload_particles(p)
    sim.tick(tick); ref.step(tick)
    want = ref.particles()
    paths3d.check_scene(scene, [want], ref.grid_dims)
    _assert_tolerance(sim.download_particles(), want, float(st.smoothing_radius), f"scene {name}")
    sim.close(); ref.close()


# ---- 3. operand guards ------------------------------------------------------------------------------------------------
def make_pair3(fs, orc, side, **kw):
    """the state of paths3d.pair3_state and an engine handle for it"""
    ref, st, tick, p = paths3d.pair3_state(fs, orc, side, **kw)
    sim = fs.FluidSimulation3D(st, device=0)
    return sim, ref, st, tick, p


def run3(sim, ref, tick, p, steps, ctx):
    p["predicted_position"] = p["position"]
    ref.set_particles(p); sim.upload_particles(p)
    with np.errstate(all="ignore"):
        for s in range(steps):
            sim.tick(tick); ref.step(tick)
            _assert_equal3(sim.download_particles(), ref.particles(), f"{ctx} step {s}")
    sim.close(); ref.close()


GUARD_CASES = paths3d.GUARD_CASES


@pytest.mark.parametrize("case", GUARD_CASES)
def test_3d_force_quotient_guards(fs, orc, case):
    """Operands on both sides of every guard of the shared-reciprocal quotients (lo_safe / 2^59 in k3_reorder, kernels_3d.hip;
    FS_RCP_HI / FS_PRESSURE_HI in k3_density, kernels_density3d.hip; FS_SQRT_LO / num_lo_ok3 / the 2^-20 branch in terms3*,
    kernels_force3d.hip): whatever the
    classification decides, the step equals the oracle bit for bit, 3 steps."""
    sim, ref, st, tick, p = make_pair3(fs, orc, 12, **paths3d.guard_overrides(case))
    p = paths3d.guard_state(orc, st, p, case)
    run3(sim, ref, tick, p, 3, f"guards3d/{case}")


@pytest.mark.parametrize("h", paths3d.RADII)
def test_3d_smoothing_radii_with_the_shared_path_on_and_off(fs, orc, h):
    """h * spiky = 15 / (pi h^4) <= 2^19 enables the shared-reciprocal path: on for h >= 0.1, off for h = 0.05 (7.6e5)"""
    hspiky = 15.0 / (3.14159265359 * h ** 4)
    assert (hspiky <= 2 ** 19) == (h >= 0.1)
    sim, ref, st, tick, p = make_pair3(fs, orc, 12, h=h, spacing=h / 2, seed=int(h * 100), rest_density=1.0)
    run3(sim, ref, tick, p, 3, f"h={h}")


def test_3d_true_division_path_without_shared_reciprocals(fs):
    """FS_NO_SHAREDIV=1: prove_rcp_sqrt (read at every create) reports both proofs as not done and the 3D handle keeps every `/`
    a true division.  A 3D handle has no status call; that the switch took is known from the 2D handle created in the same
    environment (fs_constdiv_status bits 4|8 clear).  A second 3D handle created after the variable is removed (shared path
    on) must give the same bits, and both equal the oracle.  Child process: the 2D engine latches the variable."""
    import subprocess, sys
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gpu_fluid_simulation_amd as fs
from oracle import oracle as orc
assert os.environ.get("FS_NO_SHAREDIV") == "1"
st2, off2, tick2 = fs.dam_break_2d(4096)
sim2 = fs.FluidSimulation(st2, device=0, initial_offset=off2)
assert fs.load_library().fs_constdiv_status(sim2._h) & 12 == 0, "shared path should be off"
st, off, tick = fs.dam_break_3d(14 ** 3)
tick.rest_density = 20.0
rng = np.random.default_rng(3)
ref = orc.OracleSim3D(st, off)
p = ref.particles()
p["position"] += rng.uniform(-0.03, 0.03, size=p["position"].shape).astype(np.float32)
p["predicted_position"] = p["position"]
p["velocity"] = rng.uniform(-1, 1, size=p["velocity"].shape).astype(np.float32)
ref.set_particles(p)
off_sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
del os.environ["FS_NO_SHAREDIV"]
on_sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
off_sim.upload_particles(p); on_sim.upload_particles(p)
for s in range(3):
    off_sim.tick(tick); on_sim.tick(tick); ref.step(tick)
    a, b, c = off_sim.download_particles(), on_sim.download_particles(), ref.particles()
    assert np.array_equal(a["grid"], c["grid"]) and np.array_equal(b["grid"], c["grid"])
    for f in ("position", "predicted_position", "velocity", "density"):
        assert np.array_equal(a[f].view(np.uint32), c[f].view(np.uint32)), ("true division", s, f)
        assert np.array_equal(b[f].view(np.uint32), c[f].view(np.uint32)), ("shared", s, f)
print("ok")
'''
    env = dict(os.environ, FS_NO_SHAREDIV="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ---- 4. random configurations -----------------------------------------------------------------------------------------
RANDOM_CASES = 12


@pytest.mark.parametrize("case", range(RANDOM_CASES))
def test_3d_random_configurations(fs, orc, case):
    st, off, tick, mutate, desc = paths3d.random_case(fs, case)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    ref = orc.OracleSim3D(st, off)
    assert sim.grid_dims == ref.grid_dims
    p = mutate(ref.particles())
    ref.set_particles(p); sim.upload_particles(p)
    with np.errstate(all="ignore"):
        for s in range(4):
            sim.tick(tick); ref.step(tick)
            _assert_equal3(sim.download_particles(), ref.particles(), f"random3d {desc} step {s}")
    sim.close(); ref.close()


def _oracle_ulp_sensitivity(fs, orc, st, off, tick, p, base):
    """largest change of the oracle's OWN velocities, in units of the contract (2e-5 + 1e-5 |v|), when the particle mass moves
    by one ulp either way: above 1 no implementation that is not bit-identical can be expected to meet the contract there"""
    worst = 0.0
    for towards in (10.0, -10.0):
        t2 = fs.TickSettings3.from_buffer_copy(tick)
        t2.mass = float(np.nextafter(f32(tick.mass), f32(towards)))
        o = orc.OracleSim3D(st, off)
        o.set_particles(p); o.step(t2)
        q = o.particles(); o.close()
        if not np.array_equal(q["grid"], base["grid"]):
            return np.inf
        d = np.abs(q["velocity"].astype(np.float64) - base["velocity"]) / (2e-5 + 1e-5 * np.abs(base["velocity"].astype(np.float64)))
        worst = max(worst, float(np.nanmax(d)))
    return worst


@pytest.mark.parametrize("case", range(RANDOM_CASES))
def test_3d_random_configurations_tolerance_mode(fs, orc, case):
    """One FS_MATH_TOLERANCE step from the oracle's state of the same cases: keys and predicted positions bit-exact, floats
    under the stated contract (figures printed per case).

    Measured on an MI355X with every case as drawn: 11 of 12 inside the contract (velocity error 5e-8 .. 1.5e-5, the cases with
    rest density 1000 / 20 / 1 among them: no loss from fma(k, rho, -k rho0) at these densities); case 10 (side 22, h 0.1,
    squeeze 0.25, k 500, mass 2, |v| ~ 100: 580 particles per cell, densities up to 6e5, 531 particles thrown onto the same
    wall points) missed it on 26 of 31 944 velocity components, worst 6.0e-4.  In that scene a step's velocity change is a
    cancelling sum of pair terms of ~1e2 m/s per particle and the ORACLE's own f32 evaluation is as far from the exact
    one: 3.5e-4 from a float64 evaluation of the same step (9 components over the contract), 2.1e-4 when the mass moves
    by one ulp.  The contract cannot hold for any re-association there, so the SCENE is restricted, by a rule that asks the
    oracle alone: a case whose oracle moves by more than the contract under a one-ulp change of the mass is drawn again
    without its squeeze factor and with the velocity scale 2 in place of 100 (no pile-up on the walls; everything else as
    drawn), and must then be stable.  The tolerance is the stated one."""
    st, off, tick, mutate, desc = paths3d.random_case(fs, case)
    with np.errstate(all="ignore"):
        ref = orc.OracleSim3D(st, off)
        p = mutate(ref.particles())
        ref.set_particles(p); ref.step(tick)
        sens = _oracle_ulp_sensitivity(fs, orc, st, off, tick, p, ref.particles())
        print(f"[tolerance] case {case}: the oracle moves by {sens:.3g} x the contract under a 1-ulp change of the mass")
        if sens > 1.0:
            ref.close()
            st, off, tick, mutate, desc = paths3d.random_case(fs, case, squeeze=1.0, vel=2.0)
            desc += " (restricted: no squeeze, velocity scale 2)"
            ref = orc.OracleSim3D(st, off)
            p = mutate(ref.particles())
            ref.set_particles(p); ref.step(tick)
            sens = _oracle_ulp_sensitivity(fs, orc, st, off, tick, p, ref.particles())
            assert sens <= 1.0, f"{desc}: the restricted scene is still ill-conditioned on the oracle ({sens:.3g} x the contract)"
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_TOLERANCE)
        sim.upload_particles(p)
        sim.tick(tick)
        _assert_tolerance(sim.download_particles(), ref.particles(), float(st.smoothing_radius), f"random3d {desc}")
    sim.close(); ref.close()


# ---- 5. walls, grid edges ---------------------------------------------------------------------------------------------
_box, _tick = paths3d.box_settings, paths3d.box_tick


@pytest.mark.parametrize("exact_multiple", [True, False])
def test_3d_particles_on_every_face_edge_and_corner(fs, orc, exact_multiple):
    """uploads exactly at +b and -b: 6 faces, 12 edges, 8 corners (26 sign patterns), far outside the box, and the rest of
    the particles near them; with sides that are exact multiples of h cell gw - 1 is reached only by these particles"""
    st, tick, p = paths3d.faces_state(fs, orc, exact_multiple)
    sim = fs.FluidSimulation3D(st, device=0)
    ref = orc.OracleSim3D(st)
    ref.set_particles(p); sim.upload_particles(p)
    gw, gh, gd = ref.grid_dims
    for s in range(4):
        sim.tick(tick); ref.step(tick)
        want = ref.particles()
        _assert_equal3(sim.download_particles(), want, f"walls exact={exact_multiple} step {s}")
        if s == 0:
            top = (gd - 1) * gh * gw + (gh - 1) * gw + gw - 1 if exact_multiple else None
            assert top is None or want["grid"].max() == top, "the +++ corner particle must sit in the last reachable cell"
            assert want["grid"].min() == (gh + 1) * gw + 1
    sim.close(); ref.close()


@pytest.mark.parametrize("axis,sign", paths3d.WALLS)
def test_3d_driven_into_each_wall(fs, orc, axis, sign):
    """gravity and initial velocity towards one wall: the block piles up on it (clamp, damped bounce, cell gw - 1 / 1)"""
    ref, st, tick, p = paths3d.wall_state(fs, orc, axis, sign)
    sim = fs.FluidSimulation3D(st, device=0)
    b = f32(st.size.x) * f32(0.5)
    ref.set_particles(p); sim.upload_particles(p)
    hit = False
    with np.errstate(all="ignore"):
        for s in range(6):
            sim.tick(tick); ref.step(tick)
            want = ref.particles()
            _assert_equal3(sim.download_particles(), want, f"wall axis {axis} sign {sign} step {s}")
            hit |= bool((want["position"][:, axis] == sign * b).any())
    assert hit, "no particle reached the wall: the scene lost its point"
    sim.close(); ref.close()


@pytest.mark.parametrize("size", paths3d.THIN_SIZES)
def test_3d_one_cell_and_thin_grids(fs, orc, size):
    """a 3 x 3 x 3 grid (the whole domain one cell) and grids three cells thick along one axis"""
    st, tick, p = paths3d.thin_state(fs, orc, size)
    sim = fs.FluidSimulation3D(st, device=0)
    ref = orc.OracleSim3D(st)
    want_dims = tuple(int(np.ceil(f32(s) / f32(0.2))) + 2 for s in size)
    assert sim.grid_dims == ref.grid_dims == want_dims
    run3(sim, ref, tick, p, 3, f"thin {size}")

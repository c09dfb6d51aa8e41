"""3D surface tension on the GPU (include/fluidsim.h "3D surface tension") against the checker of
tests/st3d_checker.cpp: the 3D oracle's step with the pass and the changed `acc` line.  Byte equality everywhere except the
tolerance-mode test, which applies the contract of FS_MATH_TOLERANCE as tests/test_3d.py states it."""
import ctypes as C

import numpy as np
import pytest

import paths3d
from tests import collide3d_ref as CR
from tests.handle_helpers import _same
from tests import st3d_ref as R
from tests.test_surface_tension3d import SCENE_ST
from tests.track_ref import jitter_velocities

pytestmark = pytest.mark.gpu
f32 = np.float32
SIGMA = 100.0          # dam_break_3d: |st| is then about a tenth of the pressure + viscosity sum, |st| dt / rho up to ~1.5 m/s
TOL_SIGMA = 10.0       # the tolerance-mode step: |st| dt / rho up to ~0.15 m/s, well below the scene's speeds (jitter: 3 m/s)


def _same_st(got, want, ctx):
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{ctx}: st differs in {int(bad.sum())} particles, first {int(np.argmax(bad))}: {got[np.argmax(bad)]} / {want[np.argmax(bad)]}"


def _norm(n):
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


# ---- 1. two particles ---------------------------------------------------------------------------------------------------
def test_two_particle_known_answer(fs):
    """8 particles: six more than 2 h from everything (|n| = 0: no force), a pair 0.6 h apart (equal and opposite forces), tau = 0,
    one step from rest.  Expected: the statement evaluated here in np.float32 scalars — with two terms per sum their order does
    not matter.  poly6 is the host's constant, read back from the checker."""
    h = f32(0.25)
    st = fs.Settings3(8, 0.1, float(h), fs.Vec3(4.0, 4.0, 4.0))
    tick = fs.TickSettings3(float(f32(1) / f32(120)), fs.Vec3(0.0, 9.81, 0.0), 1.5, 50.0, 0.0, 0.1, 25.0)
    sigma = f32(3.0)
    p = np.zeros(8, dtype=fs.PARTICLE3_DTYPE)
    lone = [(-1.5, -1.5, -1.5), (1.5, -1.5, -1.5), (-1.5, 1.5, -1.0), (1.5, 1.5, -1.5), (-1.5, -1.0, 1.5), (1.0, 1.5, 1.5)]
    a = np.array([0.11, -0.07, 0.23], dtype=f32)
    d = np.array([2.0, -1.0, 2.0], dtype=np.float64) / 3.0 * 0.6 * float(h)
    b = (a.astype(np.float64) + d).astype(f32)
    p["position"] = np.array(lone + [tuple(a), tuple(b)], dtype=f32)
    p["predicted_position"] = p["position"]
    chk = R.ST3Checker(st)
    chk.set_particles(p); chk.step(tick, (float(sigma), 0.0))
    poly6 = f32(chk.constants()[0])
    m, h2 = f32(tick.mass), h * h
    cg, h2x3 = f32(6.0) * poly6, f32(3.0) * h2

    def pair(x, q):
        o = q - x
        r2 = o[0] * o[0] + o[1] * o[1] + o[2] * o[2]
        assert r2 < h2 and abs(float(np.sqrt(r2)) / float(h) - 0.6) < 1e-3
        dd = h2 - r2
        rho = f32(0) + m * (poly6 * h2 * h2 * h2) * f32(1)
        rho = rho + m * (poly6 * dd * dd * dd) * f32(1)
        rho = max(max(rho, f32(1.19209290e-07)), f32(0.1))
        w = m / rho
        k = (cg * dd) * dd
        n = np.array([w * (k * o[0]), w * (k * o[1]), w * (k * o[2])], dtype=f32)
        L = w * ((cg * h2) * ((f32(7.0) * f32(0)) - h2x3)) + w * ((cg * dd) * ((f32(7.0) * r2) - h2x3))
        nl = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        s = (-sigma * L) / nl
        return np.array([s * n[0], s * n[1], s * n[2]], dtype=f32)

    fa, fb = pair(a, b), pair(b, a)
    assert np.array_equal(fa, -fb) and np.all(fa != 0)
    sim = fs.FluidSimulation3D(st, device=0)
    sim.upload_particles(p)
    sim.set_surface_tension(float(sigma), 0.0)
    assert sim.surface_tension_enabled and sim.surface_tension_params == (3.0, 0.0)
    sim.tick(tick)
    got, rec = sim.surface_tension_forces(), sim.download_particles()
    assert got.shape == (8, 3) and got.dtype == np.float32
    for slot in range(8):
        q = rec["predicted_position"][slot]
        want = fa if np.array_equal(q, a) else fb if np.array_equal(q, b) else np.zeros(3, f32)
        if want is not fa and want is not fb:
            assert any(np.array_equal(q, np.array(t, f32)) for t in lone)
        assert got[slot].tobytes() == want.tobytes(), (slot, got[slot], want)
    _same_st(got, chk.st, "two particles, against the checker")
    sim.close(); chk.close()


# ---- 2. dam break ---------------------------------------------------------------------------------------------------------
_DAM = {}


def _dam_reference(fs, side, steps=40, keep=(1, 8, 40)):
    """dam_break_3d(side^3) with jittered velocities on the checker alone: tau = the median |n| at step 8 of a run with tau = 0,
    then the run with (SIGMA, tau).  Computed once, never changed."""
    if side not in _DAM:
        st, off, tick = fs.dam_break_3d(side ** 3)
        chk = R.ST3Checker(st, off)
        start = jitter_velocities(chk.particles(), 11)
        chk.set_particles(start)
        for _ in range(8):
            chk.step(tick, (SIGMA, 0.0))
        tau = float(np.median(_norm(chk.surface_tension_pass(SIGMA, 0.0)[0])))
        chk.close()
        chk = R.ST3Checker(st, off)
        chk.set_particles(start)
        snap = {}
        for s in range(1, steps + 1):
            chk.step(tick, (SIGMA, tau))
            if s in keep:
                snap[s] = (chk.particles(), chk.st.copy(), _norm(chk.surface_tension_pass(SIGMA, tau)[0]))
        chk.close()
        _DAM[side] = dict(st=st, off=off, tick=tick, start=start, tau=tau, snap=snap)
    return _DAM[side]


@pytest.mark.parametrize("side", [16, 18])
def test_dam_break_matches_checker(fs, side):
    """whole and ragged 256-thread workgroups, 40 steps, FS_MATH_IEEE: every field of every particle and st at steps 1, 8 and 40"""
    ref = _dam_reference(fs, side)
    n, tau = side ** 3, ref["tau"]
    nl8 = ref["snap"][8][2]
    upper = int(((nl8 > f32(tau)) & (nl8 > 0)).sum())
    print(f"[st3d] side {side}: sigma {SIGMA}, tau {tau:.6g}; step 8: {upper} of {n} particles above the threshold")
    assert upper >= n // 100 and n - upper >= n // 100, "both branches of the threshold must be taken at step 8"
    sim = fs.FluidSimulation3D(ref["st"], device=0, initial_offset=ref["off"])
    sim.upload_particles(ref["start"])
    sim.set_surface_tension(SIGMA, tau)
    for s in range(1, 41):
        sim.tick(ref["tick"])
        if s in ref["snap"]:
            want, want_st, _ = ref["snap"][s]
            _same(sim.download_particles(), want, f"side {side} step {s}")
            _same_st(sim.surface_tension_forces(), want_st, f"side {side} step {s}")
    sim.close()


# ---- 3. every sweep path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handoff", ["handoff", "own_scan"])
@pytest.mark.parametrize("name", sorted(paths3d.scenes()))
def test_path_scene_matches_checker(fs, monkeypatch, name, handoff):
    """every step of every path scene with surface tension on: the model (fed the checker's keys) says the named sweep carries a
    wave-plane, and state and st equal the checker's.  FS3_HANDOFF=0 (read per handle at create): no masks are handed over, the
    pass scans the staged plane itself."""
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    if handoff == "own_scan":
        monkeypatch.setenv("FS3_HANDOFF", "0")
    sim = fs.FluidSimulation3D(st, device=0)
    monkeypatch.delenv("FS3_HANDOFF", raising=False)
    chk = R.ST3Checker(st)
    chk.set_particles(p); sim.upload_particles(p)
    sim.set_surface_tension(*SCENE_ST)
    for s in range(scene.steps):
        sim.tick(tick); chk.step(tick, SCENE_ST)
        want = chk.particles()
        paths3d.check_scene(scene, [want], chk.grid_dims)
        _same(sim.download_particles(), want, f"scene {name}/{handoff} step {s}")
        _same_st(sim.surface_tension_forces(), chk.st, f"scene {name}/{handoff} step {s}")
    sim.close(); chk.close()


# ---- 4. with a collider -------------------------------------------------------------------------------------------------------
def test_with_a_collider_matches_operator_of_checker_step(fs):
    """dam_break_3d(16^3), the box on the floor of test_collide3d_gpu.py: new state = C(checker step) at steps 1, 8 and 40 — the
    ST x COLLIDE instantiation of the force pass"""
    ref = _dam_reference(fs, 16)
    st, off, tick, tau = ref["st"], ref["off"], ref["tick"], ref["tau"]
    size = (st.size.x, st.size.y, st.size.z)
    field = CR.scene_box_on_floor(size)
    chk = R.ST3Checker(st, off)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.set_collider(field)
    sim.set_surface_tension(SIGMA, tau)
    pushed = 0
    for s in range(1, 41):
        chk.step(tick, (SIGMA, tau))
        rec, np_, _ = CR.apply_collider(chk.particles(), field, size, tick.damping_factor)
        chk.set_particles(rec)
        pushed += np_
        sim.tick(tick)
        if s in (1, 8, 40):
            _same(sim.download_particles(), rec, f"collider step {s}")
            _same_st(sim.surface_tension_forces(), chk.st, f"collider step {s}")
    assert pushed > 0, "the dam must reach the box"
    sim.close(); chk.close()


# ---- 5. tolerance mode ----------------------------------------------------------------------------------------------------------
def test_tolerance_mode_within_tolerance(fs):
    """dam_break_3d(16^3) with jittered velocities, 5 IEEE steps on the checker, then one FS_MATH_TOLERANCE step with surface
    tension on against the checker's step: exactly the assertions of test_3d_tolerance_mode_within_tolerance.  The tolerance-mode
    density differs by up to 1e-5 relative, and with it n: tau is put into a gap of the checker's own |n| values (asserted: no |n|
    within 1e-3 relative of it), so no particle changes its branch.  With SIGMA the checker's |st| dt / rho reaches 1.4 m/s at the
    least dense particles, where 1e-5 relative of it is most of the velocity contract's 2e-5; the step compared here therefore
    runs with TOL_SIGMA, for which it is asserted below 1 m/s (the scene's speeds: 3 m/s of jitter and more).  The contract is
    the stated one."""
    ref = _dam_reference(fs, 16)
    st, off, tick = ref["st"], ref["off"], ref["tick"]
    chk = R.ST3Checker(st, off)
    chk.set_particles(ref["start"])
    for _ in range(5):
        chk.step(tick, (SIGMA, ref["tau"]))
    state = chk.particles()
    probe = R.ST3Checker(st, off)
    probe.set_particles(state); probe.step(tick, (TOL_SIGMA, 0.0))
    nl = np.sort(_norm(probe.surface_tension_pass(TOL_SIGMA, 0.0)[0]).astype(np.float64))
    probe.close()
    mid = nl[len(nl) // 4: 3 * len(nl) // 4]
    k = int(np.argmax(mid[1:] / mid[:-1]))
    tau = float(f32(np.sqrt(mid[k] * mid[k + 1])))
    assert np.abs(nl / tau - 1).min() > 1e-3, "no gap in |n| to put the threshold into"
    chk.step(tick, (TOL_SIGMA, tau))
    want = chk.particles()
    dv = np.linalg.norm(chk.st, axis=1) * float(tick.delta) / want["density"]
    print(f"[st3d] tolerance: tau {tau:.6g}, {int((chk.st != 0).any(axis=1).sum())} of {len(nl)} with a force, |st| dt / rho up to {dv.max():.3g}")
    assert (chk.st != 0).any() and (chk.st == 0).all(axis=1).any() and dv.max() < 1.0
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_TOLERANCE)
    sim.upload_particles(state)
    sim.set_surface_tension(TOL_SIGMA, tau)
    sim.tick(tick)
    got = sim.download_particles()
    assert np.array_equal(got["grid"], want["grid"]), "cell keys must stay bit-exact in tolerance mode"
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32))
    h = float(st.smoothing_radius)
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h)
    sim.close(); chk.close()


# ---- 6. off is off ------------------------------------------------------------------------------------------------------------
def test_off_is_off(fs, orc):
    """10 steps: a handle that never enabled the feature and one that enabled and disabled it equal the plain oracle.  Enabled with
    sigma = 0 (st = +-0) or tau = +inf (st = +0), `acc + st` differs from `acc` only where acc is -0.0f and st is +0: positions
    and velocities equal the plain step's wherever the plain step's acc is not -0.0f.  That exclusion is empty — fp starts at
    +0, a sum of f32 terms that starts at +0 is never -0, and fp + x is -0 only if both are — and is asserted empty here on the
    checker's acc values."""
    ref = _dam_reference(fs, 16)
    st, off, tick, start = ref["st"], ref["off"], ref["tick"], ref["start"]
    plain = orc.OracleSim3D(st, off)
    plain.set_particles(start)
    chk = R.ST3Checker(st, off)
    chk.set_particles(start)
    sims = {}
    for variant in ("never", "disabled", "sigma0", "tau_inf"):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        sim.upload_particles(start)
        if variant == "disabled":
            sim.set_surface_tension(SIGMA, 1.0)
            sim.clear_surface_tension()
            assert not sim.surface_tension_enabled and sim.surface_tension_params is None
        elif variant == "sigma0":
            sim.set_surface_tension(0.0, 0.0)
        elif variant == "tau_inf":
            sim.set_surface_tension(SIGMA, float("inf"))
        sims[variant] = sim
    for s in range(10):
        plain.step(tick)
        acc = chk.step(tick, None, want_acc=True)
        assert not (acc.view(np.uint32) == 0x80000000).any(), "the plain step's acc holds a -0.0f: the exclusion is not empty"
        want = plain.particles()
        for variant, sim in sims.items():
            sim.tick(tick)
            _same(sim.download_particles(), want, f"{variant} step {s}")
    assert not sims["tau_inf"].surface_tension_forces().view(np.uint32).any(), "tau = +inf: st is +0 everywhere"
    assert not (sims["sigma0"].surface_tension_forces() != 0).any()
    for sim in sims.values():
        sim.close()
    plain.close(); chk.close()


# ---- 7. stream order ----------------------------------------------------------------------------------------------------------
def test_calls_between_unsynchronised_steps_take_effect_in_stream_order(fs):
    """plain, enabled, another sigma and tau, disabled, enabled again: two steps each with no sync in between"""
    ref = _dam_reference(fs, 16)
    st, off, tick, start, tau = ref["st"], ref["off"], ref["tick"], ref["start"], ref["tau"]
    plan = [None, (SIGMA, tau), (0.25 * SIGMA, 2.0 * tau), None, (2.0 * SIGMA, 0.5 * tau)]
    chk = R.ST3Checker(st, off)
    chk.set_particles(start)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(start)
    for cfg in plan:
        if cfg is None:
            sim.clear_surface_tension()
        else:
            sim.set_surface_tension(*cfg)
        for _ in range(2):
            sim.tick(tick); chk.step(tick, cfg)
    _same(sim.download_particles(), chk.particles(), "after the last phase")
    _same_st(sim.surface_tension_forces(), chk.st, "after the last phase")
    sim.close(); chk.close()


# ---- 8. arguments and state -----------------------------------------------------------------------------------------------------
def test_argument_checks_and_state_rules_in_the_headers_order(fs):
    st, off, tick = fs.dam_break_3d(8 ** 3)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    lib, h, INV, OK = sim._lib, sim._h, fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    err = lambda: lib.fs_last_error().decode()
    n = 8 ** 3
    nan = float("nan")
    buf = np.zeros((n, 3), dtype=f32)
    bp = buf.ctypes.data_as(C.c_void_p)
    c, t = C.c_float(), C.c_float()
    # the handle first, whatever else is wrong
    assert lib.fs3_set_surface_tension(None, 1, nan, nan) == INV and "null" in err()
    assert lib.fs3_surface_tension_enabled(None) == 0
    assert lib.fs3_surface_tension_params(None, C.byref(c), C.byref(t)) == INV and "null" in err()
    assert lib.fs3_download_surface_tension(None, bp, n) == INV and "null" in err()
    # NaN arguments in the header's order; nothing is enabled by a refused call
    assert lib.fs3_set_surface_tension(h, 1, nan, nan) == INV and "coefficient" in err()
    assert lib.fs3_set_surface_tension(h, 1, 1.0, nan) == INV and "threshold" in err()
    assert lib.fs3_surface_tension_enabled(h) == 0
    assert lib.fs3_set_surface_tension(h, 0, nan, nan) == OK, "enable == 0 ignores the two floats"
    # download: NULL dst, then the feature off (a wrong n as well), and params while off
    assert lib.fs3_download_surface_tension(h, None, n) == INV and "null" in err()
    assert lib.fs3_download_surface_tension(h, bp, n - 1) == INV and "not enabled" in err()
    assert lib.fs3_surface_tension_params(h, C.byref(c), C.byref(t)) == INV and "not enabled" in err()
    sim.tick(tick)
    assert lib.fs3_download_surface_tension(h, bp, n) == INV and "not enabled" in err()
    # enabled: no step yet (a wrong n as well), then n
    assert lib.fs3_set_surface_tension(h, 1, 2.0, float("-inf")) == OK and lib.fs3_surface_tension_enabled(h) == 1
    assert lib.fs3_surface_tension_params(h, C.byref(c), None) == INV and "null" in err()
    assert lib.fs3_surface_tension_params(h, C.byref(c), C.byref(t)) == OK and (c.value, t.value) == (2.0, float("-inf"))
    assert lib.fs3_download_surface_tension(h, bp, n + 1) == INV and "no step" in err()
    sim.tick(tick)
    assert lib.fs3_download_surface_tension(h, bp, n - 1) == INV and "particle count" in err()
    assert lib.fs3_download_surface_tension(h, bp, 0) == INV
    assert lib.fs3_download_surface_tension(h, bp, n) == OK and np.isfinite(buf).all() and buf.any()
    # changing the coefficients keeps the last step's forces; disabling and enabling again asks for a new step
    assert lib.fs3_set_surface_tension(h, 1, 3.0, 0.0) == OK
    assert lib.fs3_download_surface_tension(h, bp, n) == OK
    assert lib.fs3_set_surface_tension(h, 0, 0.0, 0.0) == OK and lib.fs3_set_surface_tension(h, 1, 3.0, 0.0) == OK
    assert lib.fs3_download_surface_tension(h, bp, n) == INV and "no step" in err()
    sim.close()

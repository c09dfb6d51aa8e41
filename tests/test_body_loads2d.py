"""2D body loads without a GPU (include/fluidsim.h "2D body loads"): the hit record that tests/body_loads2d_ref.py
takes from the operator of tests/bodies2d_ref.py agrees with that operator's records and counts, Q rounds as the header says, the fixed-point sums are the
momentum the particles lost, the shared scene meets the conditions the GPU comparison relies on, BodyDynamics2D integrates a
scripted sequence of loads as computed by hand, and every layer names the four calls."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bodies2d_ref as B
from tests import body_loads2d_ref as L
from tests.layers import ROOT, assert_every_layer_names

f32 = np.float32
NAMES = ["fs_body_loads_enable", "fs_body_loads_enabled", "fs_body_loads", "fs_body_loads_device"]
METHODS = ["enable_body_loads", "body_loads_enabled", "body_loads", "body_loads_device_ptr"]


def test_restated_operator_is_the_operator(fs, orc):
    """side 64, steps 1 .. 8, each of the three bodies on the state the one before left: the same bytes, the same number of hits
    and of re-clamped particles as bodies2d_ref.apply_body, whose counts are derived from the record's masks (one statement of the
    operator: bodies2d_ref.apply_body_record); and the run's snapshots are bodies2d_ref.oracle_run's"""
    run = L.scene_run(fs, orc, 64)
    sc = run["scene"]
    bodies = sc.bodies()
    for s in range(1, 9):
        rec = run["before"][s]
        for k, body in enumerate(sc.set_motions(bodies, s)):
            want, hits, clamps = B.apply_body(rec, body, sc.size, sc.tick.damping_factor)
            got, r = L.apply_body(rec, body, sc.size, sc.tick.damping_factor)
            assert got.tobytes() == want.tobytes(), f"step {s} body {k}"
            assert (int(r["hit"].sum()), int(r["clamped"].sum())) == (hits, clamps)
            assert r["v0"].shape == r["v1"].shape == r["s"].shape == (hits, 2)
            assert r["v0"].tobytes() == rec["velocity"][r["hit"]].tobytes(), "v0 is the velocity on entry"
            free = ~r["clamped"]
            assert got["velocity"][r["hit"]][free].tobytes() == r["v1"][free].tobytes(), "v1 is what an un-clamped hit leaves with"
            rec = got
        assert rec.tobytes() == run["snap"][s].tobytes()
    ref = B.oracle_run(fs, orc, 64)
    for s in (1, 8, 40):
        assert run["snap"][s].tobytes() == ref["snap"][s].tobytes(), f"snapshot {s}"
    assert [[w[3] for w in ws] for ws in run["words"]] == ref["hits"].tolist()


def test_q_on_hand_picked_values():
    u = 2.0 ** -20
    # ties go to the even neighbour, on both sides of zero
    for k in (0, 1, 2, 3, 1000, 1001, 2 ** 22 - 1):
        x = f32((k + 0.5) * u)
        assert float(x) == (k + 0.5) * u, "representable"
        even = k if k % 2 == 0 else k + 1
        assert L.Q([x]) == [even] and L.Q([-x]) == [-even] and L.is_tie([x, -x]).all()
    assert L.Q([f32(-0.0)]) == [0] and L.Q([f32(0.0)]) == [0]
    assert L.Q([f32(1.0)]) == [1 << 20] and L.Q([f32(-3.25)]) == [-(13 << 18)]
    assert L.Q([f32(0.4 * u)]) == [0] and L.Q([f32(0.6 * u)]) == [1] and not L.is_tie([f32(0.4 * u)]).any()
    # the largest value below 2^14 is kept: (2^14 - 2^-10) * 2^20 = 2^34 - 2^10, exactly
    top = np.nextafter(f32(16384.0), f32(0.0))
    assert L.in_range(top) and L.in_range(-top) and L.Q([top, -top]) == [(1 << 34) - (1 << 10), -((1 << 34) - (1 << 10))]
    # exactly 2^14, NaN and the infinities are dropped
    for bad in (16384.0, -16384.0, np.nan, np.inf, -np.inf, 1e6):
        assert not L.in_range(f32(bad)), bad
    # the words: a dropped hit counts in hits and in dropped and adds nothing, whichever of the three is out of range
    rec = {"v0": np.array([[1.0, 0.0], [1e6, 0.0], [np.nan, 0.0], [100.0, 0.0], [0.5, 0.25]], dtype=f32),
           "v1": np.zeros((5, 2), dtype=f32),
           "s": np.array([[0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [0.0, 1000.0], [2.0, 4.0]], dtype=f32)}
    # hit 0: j = (1, 0), tz = 0*0 - 1*1 = -1; hit 3: j = (100, 0) but tz = -1e5: dropped; hit 4: j = (0.5, 0.25), tz = 2*0.25 - 4*0.5 = -1.5
    w = L.words(rec)
    assert w[3:] == [5, 3]
    assert [L.signed(x) for x in w[:3]] == [(1 << 20) + (1 << 19), 1 << 18, -(1 << 20) - (3 << 19)]


@pytest.mark.parametrize("side", [64, 66])
def test_fixed_point_sums_are_the_momentum_the_particles_lost(fs, orc, side):
    """Over the hits that were not re-clamped, sum (v_after - v_before) in float64 equals -sum Q(j) * 2^-20 within
    hits * 2^-21 (each Q is within half a unit of j * 2^20) plus the f32 rounding of j = fl(v0 - v1) itself, at most
    2^-24 * |j| per hit (half an ulp, relative 2^-24)."""
    run = L.scene_run(fs, orc, side)
    for s, recs in run["recs"].items():
        for k, r in enumerate(recs):
            free = ~r["clamped"]
            if not free.any():
                continue
            sub = {name: r[name][free] for name in ("v0", "v1", "s")}
            jx, jy, _ = L.contributions(sub)
            assert L.in_range(jx).all() and L.in_range(jy).all()
            for a, j in enumerate((jx, jy)):
                lost = float((sub["v1"][:, a].astype(np.float64) - sub["v0"][:, a].astype(np.float64)).sum())
                fixed = -sum(L.Q(j)) * 2.0 ** -20
                bound = j.shape[0] * 2.0 ** -21 + float(np.abs(j.astype(np.float64)).sum()) * 2.0 ** -24
                assert abs(lost - fixed) <= bound, f"side {side} step {s} body {k} axis {a}: {lost} vs {fixed}, bound {bound}"


@pytest.mark.parametrize("side", [64, 66])
def test_scene_meets_the_conditions_the_gpu_tests_rely_on(fs, orc, side):
    run = L.scene_run(fs, orc, side)
    per_step = run["words"]
    assert len(per_step) == 40
    total = L.accumulated(per_step, 40)
    print(f"[body_loads2d] side {side}: step 1 {[[L.signed(x) for x in w] for w in per_step[0]]}; 40 steps "
          f"{[[L.signed(x) for x in w] for w in total]}")
    assert all(w[4] == 0 for ws in per_step for w in ws), "nothing is dropped in the scene"
    assert all(w[3] > 0 for w in per_step[0]), "paddle, stirrer and slab all hit in step 1"
    if side == 64:
        assert [w[3] for w in per_step[0]] == [576, 24, 16], "DESIGN.md §24"
    assert L.signed(per_step[0][0][0]) > 0, "the paddle moves towards -x into fluid at rest: the fluid pushes it towards +x"
    assert L.signed(total[1][2]) != 0 and L.signed(per_step[0][1][2]) != 0, "the stirrer takes a torque"
    assert L.accumulated(per_step, 8) != total and L.scene_run(fs, orc, side) is run


class _ScriptedSim:
    """what BodyDynamics2D.advance uses of a handle: scripted loads out, the motions it sets in"""

    def __init__(self, fs, script):
        self.fs, self.script, self.motions, self.resets = fs, list(script), [], []

    def body_loads(self, slot, reset=False):
        self.resets.append((slot, reset))
        (ix, iy), ang = self.script.pop(0)
        return self.fs.BodyLoads((int(ix * 2 ** 20), int(iy * 2 ** 20)), int(ang * 2 ** 20), 1, 0, 1)

    def set_body_motion(self, slot, centre, rot, velocity, angular_velocity):
        self.motions.append((slot, centre, rot, velocity, angular_velocity))


class _Tick:
    delta = 0.5


SCRIPT = [((2.0, -1.0), 2.0), ((0.0, 0.0), 0.0), ((-4.0, 2.0), -4.0)]


def test_body_dynamics_three_steps_by_hand(fs):
    """mass 2, inertia 4, gravity (0, 2), dt 0.5, particle mass 1; the impulses (2, -1), (0, 0), (-4, 2) and the angular impulses
    2, 0, -4.  Semi-implicit Euler: v += impulse / m + g dt, then c += v dt with the NEW v; every number is dyadic.
      1: v = (1, -0.5) + (0, 1) = (1, 0.5), c = (0.5, 0.25); w = 0.5, angle = 0.25
      2: v = (1, 1.5), c = (1, 1); w = 0.5, angle = 0.5
      3: v = (1, 1.5) + (-2, 1) + (0, 1) = (-1, 3.5), c = (0.5, 2.75); w = 0.5 - 1 = -0.5, angle = 0.25"""
    dyn = fs.BodyDynamics2D(2.0, 4.0, (0.0, 0.0), gravity=(0.0, 2.0))
    sim = _ScriptedSim(fs, SCRIPT)
    want = [((1.0, 0.5), (0.5, 0.25), 0.5, 0.25), ((1.0, 1.5), (1.0, 1.0), 0.5, 0.5), ((-1.0, 3.5), (0.5, 2.75), -0.5, 0.25)]
    for step, (v, c, w, angle) in enumerate(want):
        loads = dyn.advance(sim, 3, _Tick)
        assert loads.steps == 1 and sim.resets[-1] == (3, True), "reads AND resets the slot"
        assert dyn.velocity.tolist() == list(v) and dyn.centre.tolist() == list(c), step
        assert dyn.angular_velocity == w and dyn.angle == angle, step
        slot, mc, mrot, mv, mw = sim.motions[-1]
        assert slot == 3 and mc.dtype == np.float32 and mc.tolist() == list(c) and mv.tolist() == list(v) and float(mw) == w
        assert mrot.tobytes() == fs.rigid_motion2d((0, 0), (0, 0), angle, 1.0)[1].tobytes(), "rigid_motion2d's rotation"
    # the particle mass scales the impulse
    dyn = fs.BodyDynamics2D(2.0, 4.0, (0.0, 0.0), particle_mass=0.5)
    dyn.advance(_ScriptedSim(fs, SCRIPT), 0, _Tick)
    assert dyn.velocity.tolist() == [0.5, -0.25] and dyn.angular_velocity == 0.25


def test_body_dynamics_locks(fs):
    def run(**locks):
        dyn = fs.BodyDynamics2D(2.0, 4.0, (1.0, 2.0), velocity=(0.0, 0.0), gravity=(0.0, 2.0), **locks)
        sim = _ScriptedSim(fs, SCRIPT)
        for _ in range(3):
            dyn.advance(sim, 0, _Tick)
        return dyn

    free = run()
    assert free.centre.tolist() == [1.5, 4.75] and free.angle == 0.25
    hinge = run(lock_x=True, lock_y=True)                    # torque only
    assert hinge.centre.tolist() == [1.0, 2.0] and hinge.velocity.tolist() == [0.0, 0.0]
    assert hinge.angle == 0.25 and hinge.angular_velocity == -0.5
    slider = run(lock_y=True, lock_rotation=True)            # one axis
    assert slider.centre.tolist() == [1.5, 2.0] and slider.velocity.tolist() == [-1.0, 0.0]
    assert slider.angle == 0.0 and slider.angular_velocity == 0.0
    other = run(lock_x=True)
    assert other.centre.tolist() == [1.0, 4.75] and other.angle == 0.25
    with pytest.raises(ValueError):
        fs.BodyDynamics2D(0.0, 1.0, (0, 0))


def test_body_loads_record(fs):
    r = fs.BodyLoads((3 << 20, -(1 << 19)), -(5 << 20), 7, 1, 4)
    assert r.impulse(2.0).dtype == np.float64 and r.impulse(2.0).tolist() == [6.0, -1.0] and r.angular_impulse(0.5) == -2.5
    assert r.mean_force(2.0, 0.5).tolist() == [3.0, -0.5] and r.mean_torque(0.5, 0.25) == -2.5
    assert r.words() == [3 << 20, (1 << 64) - (1 << 19), (1 << 64) - (5 << 20), 7, 1]
    zero = fs.BodyLoads((0, 0), 0, 0, 0, 0)
    assert zero.mean_force(1.0, 0.1).tolist() == [0.0, 0.0] and zero.mean_torque(1.0, 0.1) == 0.0


def test_every_layer_names_the_four_calls(fs):
    assert_every_layer_names(fs, NAMES, fs.FluidSimulation, METHODS)
    lib = fs.load_library()
    assert C.sizeof(fs.BodyLoad) == 48 and fs._abi.FS_BODY_LOAD_SHIFT == 20
    header = open(os.path.join(ROOT, "include", "fluidsim.h")).read()
    assert "#define FS_BODY_LOAD_SHIFT 20" in header and "2D body loads" in header
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NAMES:
            assert name in text, f"{doc} does not name {name}"
    # the NULL-handle check comes first and needs no device
    INV = fs._abi.FS_ERR_INVALID
    assert lib.fs_body_loads_enable(None, 1) == INV and lib.fs_body_loads_enabled(None) == 0
    assert lib.fs_body_loads(None, 0, None, 0) == INV and lib.fs_body_loads_device(None, None) == INV

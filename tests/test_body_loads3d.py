"""3D body loads without a GPU (include/fluidsim.h "3D body loads"): the operator restated in
tests/body_loads3d_ref.py is the operator of tests/bodies3d_ref.py, the eight words follow the header's drop rule on a hand-made
record, the fixed-point sums are the momentum the particles lost, the shared scene meets the conditions the GPU comparison relies
on, BodyDynamics3D integrates scripted loads as computed by hand and as a float64 restatement does, the BodyLoads3D record, and
every layer names the four calls."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bodies3d_ref as B
from tests import body_loads3d_ref as L
from tests.layers import ROOT, assert_every_layer_names

f32 = np.float32
NAMES = ["fs3_body_loads_enable", "fs3_body_loads_enabled", "fs3_body_loads", "fs3_body_loads_device"]
METHODS = ["enable_body_loads", "body_loads_enabled", "body_loads", "body_loads_device_ptr"]
# step-1 hits (paddle, stirrer, slab) and the slab's step-1 re-clamps, from the unchanged CPU oracle and the numpy operator
STEP1 = {16: ([256, 288, 322], 283), 18: ([324, 324, 368], 303)}


@pytest.mark.parametrize("side", [16, 18])
def test_restated_operator_is_the_operator(fs, orc, side):
    """steps 1 .. 8, each of the three bodies on the state the one before left: the same bytes, the same number of hits and of
    re-clamped particles as bodies3d_ref.apply_body; v0 is the velocity on entry, v1 what an un-clamped hit leaves with; and the
    run's snapshots are bodies3d_ref.oracle_run's"""
    run = L.scene_run(fs, orc, side)
    sc = run["scene"]
    bodies = sc.bodies()
    for s in range(1, 9):
        rec = run["before"][s]
        for k, body in enumerate(sc.set_motions(bodies, s)):
            want, hits, clamps = B.apply_body(rec, body, sc.size, sc.tick.damping_factor)
            got, r = L.apply_body_record(rec, body, sc.size, sc.tick.damping_factor)
            assert got.tobytes() == want.tobytes(), f"step {s} body {k}"
            assert (int(r["hit"].sum()), int(r["clamped"].sum())) == (hits, clamps)
            assert r["v0"].shape == r["v1"].shape == r["s"].shape == (hits, 3)
            assert r["v0"].tobytes() == rec["velocity"][r["hit"]][:, :3].astype(f32).tobytes(), "v0 is the velocity on entry"
            free = ~r["clamped"]
            assert got["velocity"][r["hit"]][free][:, :3].tobytes() == r["v1"][free].tobytes(), "v1: what an un-clamped hit leaves with"
            rec = got
        assert rec.tobytes() == run["snap"][s].tobytes()
    ref = B.oracle_run(fs, orc, side)
    for s in (1, 8, 40):
        assert run["snap"][s].tobytes() == ref["snap"][s].tobytes(), f"snapshot {s}"
    assert [[w[6] for w in ws] for ws in run["words"]] == ref["hits"].tolist()


def test_words_on_a_hand_made_record():
    """kept and dropped hits; for each of the six values one hit where only that value is out of range; a NaN, an exact tie, -0"""
    u = 2.0 ** -20
    z3 = [0.0, 0.0, 0.0]
    v0, v1, s = [], [], []

    def hit(a, b, c):
        v0.append(a), v1.append(b), s.append(c)

    hit([1.0, 0.0, 0.0], z3, [0.0, 1.0, 0.0])              # 0 kept: j = (1,0,0); t = (0, 0, -1)
    hit([0.5, 0.25, -2.0], z3, [2.0, 4.0, 8.0])            # 1 kept: t = (4*-2 - 8*.25, 8*.5 - 2*-2, 2*.25 - 4*.5) = (-10, 8, -1.5)
    hit([1e6, 0.0, 0.0], z3, z3)                           # 2 dropped: only j.x
    hit([0.0, -1e6, 0.0], z3, z3)                          # 3 dropped: only j.y
    hit([0.0, 0.0, 16384.0], z3, z3)                       # 4 dropped: only j.z (exactly 2^14)
    hit([0.0, 0.0, 100.0], z3, [0.0, 1000.0, 0.0])         # 5 dropped: only t.x = 1000 * 100
    hit([100.0, 0.0, 0.0], z3, [0.0, 0.0, 1000.0])         # 6 dropped: only t.y = 1000 * 100
    hit([0.0, 100.0, 0.0], z3, [1000.0, 0.0, 0.0])         # 7 dropped: only t.z = 1000 * 100
    hit([np.nan, 0.0, 0.0], z3, z3)                        # 8 dropped: NaN
    hit([2.5 * u, -1.5 * u, 0.0], z3, z3)                  # 9 kept: exact ties -> 2, -2
    hit([-0.0, 0.0, 0.0], [0.0, 0.0, 0.0], z3)             # 10 kept: -0 - 0 = -0 -> 0
    rec = {k: np.array(a, dtype=f32) for k, a in (("v0", v0), ("v1", v1), ("s", s))}
    six = L.contributions(rec)
    for k, only in zip(range(2, 8), range(6)):
        bad = [not bool(L.in_range(a[k])) for a in six]
        assert bad == [c == only for c in range(6)], f"hit {k}: only value {only} is out of range"
    assert np.signbit(six[0][10]) and six[0][10] == 0.0
    w, ties = L.words(rec, want_ties=True)
    assert w[6:] == [11, 7] and ties >= 2
    one = 1 << 20
    assert [L.signed(x) for x in w[:6]] == [one + one // 2 + 2, one // 4 - 2, -2 * one, -10 * one, 8 * one, -one - 3 * one // 2]
    assert L.words({k: a[:0] for k, a in rec.items()}) == L.ZERO


@pytest.mark.parametrize("side", [16, 18])
def test_fixed_point_sums_are_the_momentum_the_particles_lost(fs, orc, side):
    """Over the hits that were not re-clamped, per body and axis, sum (v1 - v0) in float64 equals -sum Q(j.a) * 2^-20 within
    hits * 2^-21 (each Q is within half a unit of j * 2^20) plus the f32 rounding of j = fl(v0 - v1) itself, at most 2^-24 * |j|
    per hit: the bound derived in tests/test_body_loads2d.py."""
    run = L.scene_run(fs, orc, side)
    for s, recs in run["recs"].items():
        for k, r in enumerate(recs):
            free = ~r["clamped"]
            if not free.any():
                continue
            sub = {name: r[name][free] for name in ("v0", "v1", "s")}
            six = L.contributions(sub)
            for a, j in enumerate(six[:3]):
                assert L.in_range(j).all()
                lost = float((sub["v1"][:, a].astype(np.float64) - sub["v0"][:, a].astype(np.float64)).sum())
                fixed = -sum(L.Q(j)) * 2.0 ** -20
                bound = j.shape[0] * 2.0 ** -21 + float(np.abs(j.astype(np.float64)).sum()) * 2.0 ** -24
                assert abs(lost - fixed) <= bound, f"side {side} step {s} body {k} axis {a}: {lost} vs {fixed}, bound {bound}"


@pytest.mark.parametrize("side", [16, 18])
def test_scene_meets_the_conditions_the_gpu_tests_rely_on(fs, orc, side):
    run = L.scene_run(fs, orc, side)
    per_step = run["words"]
    assert len(per_step) == 40
    total = L.accumulated(per_step, 40)
    sg = [[L.signed(x) for x in w[:6]] for w in total]
    print(f"[body_loads3d] side {side}: step 1 {[[L.signed(x) for x in w] for w in per_step[0]]}; 40 steps {sg}")
    assert all(w[7] == 0 for ws in per_step for w in ws), "nothing is dropped in the scene"
    for s in (1, 8, 40):      # the steps bodies3d_ref.oracle_run keeps and the GPU tests compare at
        assert all(w[6] > 0 for w in per_step[s - 1]), f"paddle, stirrer and slab are all hit in kept step {s}"
    # (in between a body may hit nothing: at side 18 the paddle's step 4 is such a step, so the run also takes the loads
    # kernel's "no lane hit" branch for a whole body)
    assert min(w[6] for ws in per_step for w in ws) == (0 if side == 18 else 1)
    hits1, slab_clamps = STEP1[side]
    assert [w[6] for w in per_step[0]] == hits1
    assert int(run["recs"][1][2]["clamped"].sum()) == slab_clamps, "the slab's re-clamps: v1 is taken before the wall"
    paddle, stirrer, slab = sg
    assert paddle[0] > 0, "the paddle moves towards -x into fluid at rest: the fluid pushes it towards +x"
    assert paddle[1] == 0 and paddle[2] == 0 and paddle[3] == 0
    assert stirrer[5] != 0, "the stirrer takes a torque about z"
    assert slab[3] != 0, "the slab, turned about x, takes a torque about x"
    for c in range(6):
        assert any(b[c] != 0 for b in sg), f"word {c} is exercised by some body"
    ties = [sum(L.words(r, want_ties=True)[1] for r in recs) for recs in run["recs"].values()]
    assert min(ties) >= 24, f"dozens of contributions per step are exact ties: {ties}"
    assert L.accumulated(per_step, 8) != total and L.scene_run(fs, orc, side) is run


class _ScriptedSim:
    """what BodyDynamics3D.advance uses of a handle: scripted loads out, the motions it sets in"""

    def __init__(self, fs, script):
        self.fs, self.script, self.motions, self.resets = fs, list(script), [], []

    def body_loads(self, slot, reset=False):
        self.resets.append((slot, reset))
        imp, ang = self.script.pop(0)
        return self.fs.BodyLoads3D([int(x * 2 ** 20) for x in imp], [int(x * 2 ** 20) for x in ang], 1, 0, 1)

    def set_body_motion(self, slot, centre, rot, velocity, angular_velocity):
        self.motions.append((slot, centre, rot, velocity, angular_velocity))


class _Tick:
    delta = 0.5


# tests/test_body_loads2d.py's script, about z
SCRIPT = [((2.0, -1.0, 0.0), (0.0, 0.0, 2.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((-4.0, 2.0, 0.0), (0.0, 0.0, -4.0))]
RZ = lambda th: np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])      # noqa: E731
# float64 products of two or three rotations: a few units of 2^-53 per entry
ROT_TOL = 1e-14


def test_body_dynamics_three_steps_by_hand(fs):
    """mass 2, moments (3, 5, 4), gravity (0, 2, 0), dt 0.5, particle mass 1; impulses and angular impulses about z as in the 2D
    test.  Semi-implicit Euler: v += impulse / m + g dt, L += angular impulse, w = R diag(1/I) R^T L, c += v dt, R turned by
    |w| dt about w.  A rotation about the principal axis z keeps w = (0, 0, Lz / 4) exactly; every number but R is dyadic.
      1: v = (1, 0.5, 0), c = (0.5, 0.25, 0); Lz = 2, wz = 0.5, angle 0.25
      2: v = (1, 1.5, 0), c = (1, 1, 0); wz = 0.5, angle 0.5
      3: v = (-1, 3.5, 0), c = (0.5, 2.75, 0); Lz = -2, wz = -0.5, angle 0.25        — the 2D test's numbers"""
    dyn = fs.BodyDynamics3D(2.0, (3.0, 5.0, 4.0), (0.0, 0.0, 0.0), gravity=(0.0, 2.0, 0.0))
    sim = _ScriptedSim(fs, SCRIPT)
    want = [((1.0, 0.5), (0.5, 0.25), 0.5, 0.25), ((1.0, 1.5), (1.0, 1.0), 0.5, 0.5), ((-1.0, 3.5), (0.5, 2.75), -0.5, 0.25)]
    for step, (v, c, w, angle) in enumerate(want):
        loads = dyn.advance(sim, 3, _Tick)
        assert loads.steps == 1 and sim.resets[-1] == (3, True), "reads AND resets the slot"
        assert dyn.velocity.tolist() == list(v) + [0.0] and dyn.centre.tolist() == list(c) + [0.0], step
        assert dyn.angular_velocity.tolist() == [0.0, 0.0, w], step
        assert np.abs(dyn.rot - RZ(angle)).max() <= ROT_TOL, step
        slot, mc, mrot, mv, mw = sim.motions[-1]
        assert slot == 3 and all(a.dtype == np.float32 for a in (mc, mrot, mv, mw)) and mrot.shape == (9,)
        assert mc.tolist() == list(c) + [0.0] and mv.tolist() == list(v) + [0.0] and mw.tolist() == [0.0, 0.0, w]
        assert np.abs(mrot.astype(np.float64) - fs.rigid_motion((0, 0, 0), (0, 0, 0), (0, 0, 1), angle, 1.0)[1]).max() <= 2.0 ** -23
    dyn = fs.BodyDynamics3D(2.0, (3.0, 5.0, 4.0), (0.0, 0.0, 0.0), particle_mass=0.5)
    dyn.advance(_ScriptedSim(fs, SCRIPT), 0, _Tick)
    assert dyn.velocity.tolist() == [0.5, -0.25, 0.0] and dyn.angular_velocity.tolist() == [0.0, 0.0, 0.25]


def test_body_dynamics_unequal_moments_against_a_restatement(fs):
    """moments (1, 2, 4), a start rotation off the axes and torques off the principal axes: the same trajectory as a float64
    restatement written here (the rotation as cos I + sin [a]x + (1 - cos) a a^T)"""
    script = [((1.0, 2.0, -1.0), (1.0, -2.0, 0.5)), ((0.0, -0.5, 0.25), (0.25, 0.5, -1.0)), ((-1.0, 0.0, 3.0), (-2.0, 1.0, 1.0))]
    a0 = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)          # a float64 rotation (rigid_motion's is rounded to float32)
    x0 = np.array([[0.0, -a0[2], a0[1]], [a0[2], 0.0, -a0[0]], [-a0[1], a0[0], 0.0]])
    r0 = np.cos(0.7) * np.eye(3) + np.sin(0.7) * x0 + (1.0 - np.cos(0.7)) * np.outer(a0, a0)
    dyn = fs.BodyDynamics3D(3.0, (1.0, 2.0, 4.0), (0.5, -1.0, 2.0), rot=r0, velocity=(0.25, 0.0, -0.5), angular_momentum=(0.5, 0.0, 0.0),
                            gravity=(0.0, 9.81, 0.0), particle_mass=0.25)
    sim = _ScriptedSim(fs, script)
    m, inertia, pm, dt, g = 3.0, np.array([1.0, 2.0, 4.0]), 0.25, 0.5, np.array([0.0, 9.81, 0.0])
    c, r, v, ang = np.array([0.5, -1.0, 2.0]), r0.copy(), np.array([0.25, 0.0, -0.5]), np.array([0.5, 0.0, 0.0])
    for imp, tor in script:
        dyn.advance(sim, 1, _Tick)
        v = v + np.array(imp) * pm / m + g * dt
        ang = ang + np.array(tor) * pm
        w = r @ np.diag(1.0 / inertia) @ r.T @ ang
        c = c + v * dt
        th = np.linalg.norm(w) * dt
        a = w / np.linalg.norm(w)
        ax = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        r = (np.cos(th) * np.eye(3) + np.sin(th) * ax + (1.0 - np.cos(th)) * np.outer(a, a)) @ r
        assert np.abs(dyn.velocity - v).max() <= 1e-14 and np.abs(dyn.centre - c).max() <= 1e-14
        assert np.abs(dyn.angular_momentum - ang).max() <= 1e-14 and np.abs(dyn.rot - r).max() <= ROT_TOL
        assert np.abs(dyn.rot @ dyn.rot.T - np.eye(3)).max() <= ROT_TOL, "R stays a rotation"
        w_next = r @ np.diag(1.0 / inertia) @ r.T @ ang
        assert np.abs(sim.motions[-1][4].astype(np.float64) - w_next).max() <= 2.0 ** -22 * max(1.0, np.abs(w_next).max())
    assert np.abs(dyn.rot - r0).max() > 0.1, "it turned"


def test_body_dynamics_locks(fs):
    def run(**locks):
        dyn = fs.BodyDynamics3D(2.0, (3.0, 5.0, 4.0), (1.0, 2.0, 3.0), gravity=(0.0, 2.0, 0.0), **locks)
        sim = _ScriptedSim(fs, [((2.0, -1.0, 4.0), (0.0, 0.0, 2.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((-4.0, 2.0, -8.0), (0.0, 0.0, -4.0))])
        for _ in range(3):
            dyn.advance(sim, 0, _Tick)
        return dyn

    # z: v = 2, 2, -2; c.z = 3 + 1 + 1 - 1 = 4
    free = run()
    assert free.centre.tolist() == [1.5, 4.75, 4.0] and free.velocity.tolist() == [-1.0, 3.5, -2.0]
    assert np.abs(free.rot - RZ(0.25)).max() <= ROT_TOL and free.angular_momentum.tolist() == [0.0, 0.0, -2.0]
    hinge = run(lock_x=True, lock_y=True, lock_z=True)       # torque only
    assert hinge.centre.tolist() == [1.0, 2.0, 3.0] and hinge.velocity.tolist() == [0.0, 0.0, 0.0]
    assert np.abs(hinge.rot - RZ(0.25)).max() <= ROT_TOL and hinge.angular_velocity.tolist() == [0.0, 0.0, -0.5]
    for axis, name in enumerate(("lock_x", "lock_y", "lock_z")):
        one = run(**{name: True})
        want_c, want_v = [1.5, 4.75, 4.0], [-1.0, 3.5, -2.0]
        want_c[axis], want_v[axis] = [1.0, 2.0, 3.0][axis], 0.0
        assert one.centre.tolist() == want_c and one.velocity.tolist() == want_v, name
    still = run(lock_rotation=True)
    assert still.rot.tolist() == np.eye(3).tolist() and still.angular_momentum.tolist() == [0.0, 0.0, 0.0]
    assert still.centre.tolist() == [1.5, 4.75, 4.0]
    with pytest.raises(ValueError):
        fs.BodyDynamics3D(0.0, (1.0, 1.0, 1.0), (0, 0, 0))
    with pytest.raises(ValueError):
        fs.BodyDynamics3D(1.0, (1.0, 0.0, 1.0), (0, 0, 0))


def test_body_loads3d_record(fs):
    r = fs.BodyLoads3D((3 << 20, -(1 << 19), 1 << 21), (-(5 << 20), 0, 1 << 18), 7, 1, 4)
    assert r.impulse(2.0).dtype == np.float64 and r.impulse(2.0).tolist() == [6.0, -1.0, 4.0]
    assert r.angular_impulse(0.5).dtype == np.float64 and r.angular_impulse(0.5).tolist() == [-2.5, 0.0, 0.125]
    assert r.mean_force(2.0, 0.5).tolist() == [3.0, -0.5, 2.0] and r.mean_torque(0.5, 0.25).tolist() == [-2.5, 0.0, 0.125]
    m = 1 << 64
    assert r.words() == [3 << 20, m - (1 << 19), 1 << 21, m - (5 << 20), 0, 1 << 18, 7, 1]
    zero = fs.BodyLoads3D((0, 0, 0), (0, 0, 0), 0, 0, 0)
    assert zero.mean_force(1.0, 0.1).tolist() == [0.0, 0.0, 0.0] and zero.mean_torque(1.0, 0.1).tolist() == [0.0, 0.0, 0.0]
    assert zero.words() == [0] * 8
    with pytest.raises(ValueError):
        fs.BodyLoads3D((0, 0), (0, 0, 0), 0, 0, 0)


def test_every_layer_names_the_four_calls(fs):
    assert_every_layer_names(fs, NAMES, fs.FluidSimulation3D, METHODS)
    lib = fs.load_library()
    assert C.sizeof(fs.Body3Load) == 72 and fs._abi.FS_BODY_LOAD_SHIFT == 20
    header = open(os.path.join(ROOT, "include", "fluidsim.h")).read()
    assert "3D body loads" in header and "typedef struct fs3_body_load" in header
    assert header.index("3D moving bodies (build extension") < header.index("3D body loads (build extension")
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NAMES:
            assert name in text, f"{doc} does not name {name}"
    assert hasattr(fs, "BodyLoads3D") and hasattr(fs, "BodyDynamics3D")
    # the NULL-handle check comes first and needs no device
    INV = fs._abi.FS_ERR_INVALID
    assert lib.fs3_body_loads_enable(None, 1) == INV and lib.fs3_body_loads_enabled(None) == 0
    assert lib.fs3_body_loads(None, 0, None, 0) == INV and lib.fs3_body_loads_device(None, None) == INV

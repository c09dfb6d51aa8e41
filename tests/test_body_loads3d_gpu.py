"""3D body loads on the GPU (include/fluidsim.h "3D body loads").  The checker is tests/body_loads3d_ref.py: the
restated operator and exact Python-int sums of Q over its hits.  Integer equality throughout, and particles byte for byte: no
tolerance in this file.  The shapes and the shared states are those of tests/test_bodies3d_gpu.py (16^3, 18^3, 4097 of 4200),
plus 26^3 for more workgroups than the shard table has rows."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies3d_ref as B
from tests import body_loads3d_ref as L
from tests import collide3d_ref as CR
from tests import test_bodies3d_gpu as G
from tests.handle_helpers import _add, _same, _same_but_nan_bits, _size

pytestmark = pytest.mark.gpu
f32 = np.float32
IEEE = "ieee"


def _mode(fs, mode):
    return fs.FS_MATH_IEEE if mode == IEEE else fs.FS_MATH_TOLERANCE


def _on(sim):
    sim.enable_body_loads()


def _words(sim, slots, reset=False):
    """the eight words of every slot of `slots` as Python ints modulo 2^64, and the steps"""
    got = [sim.body_loads(k, reset=reset) for k in slots]
    return [g.words() for g in got], [g.steps for g in got]


def _step_with(fs, m, bodies, prep=None, before=_on):
    """the shared jittered state, `prep`, the bodies, `before` (which turns the loads on), one step: (particles, the open handle)"""
    st, off, tick, p = G._base(fs, m, prep)[:4]
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=m)
    sim.upload_particles(p)
    if prep:
        prep(sim)
    _add(sim, bodies)
    before(sim)
    sim.tick(tick)
    return sim.download_particles(), sim


def _check(fs, mode, bodies, prep=None, before=_on, ctx=""):
    """One step of the shared jittered state with `bodies` and loads on, against the checker on the state a body-less handle
    leaves: the particles and, per slot, the words.  Returns (the checker's words, its per-body records, the still open handle)."""
    m = _mode(fs, mode)
    st, _, tick, _, after = G._base(fs, m, prep)[:5]
    want, want_words, recs = L.apply_bodies(after, bodies, _size(st), tick.damping_factor)
    got, sim = _step_with(fs, m, bodies, prep, before)
    _same(got, want, f"{ctx}: particles")
    got_words, steps = _words(sim, range(len(bodies)))
    print(f"[body_loads3d] {ctx}: {[[L.signed(x) for x in w[:6]] + w[6:] for w in want_words]}")
    assert got_words == want_words, f"{ctx}: words"
    assert steps == [1] * len(bodies)
    return want_words, recs, sim


def _scene_sim(fs, run):
    sc = run["scene"]
    sim = fs.FluidSimulation3D(sc.st, device=0, initial_offset=sc.off)
    if run["static"] is not None:
        sim.set_collider(run["static"])
    for k, (field, extent) in enumerate(zip(sc.fields, sc.extents)):
        assert sim.add_body(field, extent) == k
    return sim


def _scene_step(sim, sc, bodies, s):
    for k, b in enumerate(sc.set_motions(bodies, s)):
        sim.set_body_motion(k, *b.motion())
    sim.tick(sc.tick)


# ---- 1. the scene against the oracle plus the operators ---------------------------------------------------------------
@pytest.mark.parametrize("static", [None, "a"])
@pytest.mark.parametrize("side", [16, 18])
def test_scene_words_and_particles(fs, orc, side, static):
    """16^3 = 16 full workgroups, 18^3 = 5832: the last workgroup has three full waves and eight lanes.  Poses set before every
    step and no sync between the steps: after 1, 8 and 40 steps every slot's words are the checker's accumulated words, and the
    particles are bodies3d_ref.oracle_run's loads-off snapshots.  With the static collider 'a', v0 is taken behind C."""
    run = L.scene_run(fs, orc, side, static)
    ref = B.oracle_run(fs, orc, side, static)
    sc = run["scene"]
    sim = _scene_sim(fs, run)
    assert not sim.body_loads_enabled
    sim.enable_body_loads()
    assert sim.body_loads_enabled
    bodies = sc.bodies()
    for s in range(1, 41):
        _scene_step(sim, sc, bodies, s)
        if s in (1, 8, 40):
            got, steps = _words(sim, range(3))
            assert got == L.accumulated(run["words"], s), f"side {side} static {static}: words after {s} steps"
            assert steps == [s, s, s]
            _same(sim.download_particles(), ref["snap"][s], f"side {side} static {static} step {s} with loads on")
    sim.close()


def test_read_with_reset_after_every_step(fs, orc):
    """the words of each single step, and their Python-int sum is the accumulated run"""
    run = L.scene_run(fs, orc, 16)
    sc = run["scene"]
    sim = _scene_sim(fs, run)
    sim.enable_body_loads()
    bodies = sc.bodies()
    acc = [L.ZERO] * 3
    for s in range(1, 41):
        _scene_step(sim, sc, bodies, s)
        got, steps = _words(sim, range(3), reset=True)
        assert got == run["words"][s - 1], f"the words of step {s} alone"
        assert steps == [1, 1, 1]
        acc = [L.add_words(a, g) for a, g in zip(acc, got)]
    assert acc == L.accumulated(run["words"], 40)
    got, steps = _words(sim, range(3))
    assert got == [L.ZERO] * 3 and steps == [0, 0, 0], "the last reset left zeros"
    sim.close()


def test_same_scene_twice_gives_the_same_words(fs, orc):
    """integer sums cannot depend on the order of the reduction: this guards a float slipping in"""
    run = L.scene_run(fs, orc, 18)
    sc = run["scene"]
    seen = []
    for _ in range(2):
        sim = _scene_sim(fs, run)
        sim.enable_body_loads()
        bodies = sc.bodies()
        for s in range(1, 9):
            _scene_step(sim, sc, bodies, s)
        seen.append(_words(sim, range(3)))
        sim.close()
    assert seen[0] == seen[1] and seen[0][0] == L.accumulated(run["words"], 8)


# ---- 2. the operator alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_operator_alone_both_math_modes(fs, mode):
    body = G._moving_body(fs, CR.random_field((13, 9, 7), 3, fill=0.6, mag=0.4))
    want, recs, sim = _check(fs, mode, [body], ctx=f"operator alone, {mode}")
    sim.close()
    assert want[0][6] > 0 and recs[0]["clamped"].any() and want[0][7] == 0


# ---- 3. the edges of the reduction ------------------------------------------------------------------------------------
def test_one_voxel_body_with_exactly_one_hit(fs):
    st, _, tick, _, after = G._base(fs, fs.FS_MATH_IEEE)[:5]
    field = np.array([0.01, -0.02, 0.015], dtype=f32).reshape(1, 1, 1, 3)
    body = None
    for j in range(1500, 1600):                       # the first particle the tiny box holds alone
        centre = after["position"][j] + np.array([3e-4, -2e-4, 5e-4], dtype=f32)      # off the particle: s is not parallel to j
        cand = B.Body(field, (2e-3, 2e-3, 2e-3), centre=centre, velocity=(0.5, 0.25, -0.125), angular_velocity=(1.0, 0.5, -2.0))
        if int(L.apply_body_record(after, cand, _size(st), tick.damping_factor)[1]["hit"].sum()) == 1:
            body = cand
            break
    assert body is not None
    want, _, sim = _check(fs, IEEE, [body], ctx="one hit")
    sim.close()
    assert want[0][6:] == [1, 0] and 0 not in want[0][:3] and want[0][3:6] != [0, 0, 0]


def test_body_that_hits_nothing(fs):
    body = B.Body(CR.random_field((4, 4, 4), 1, fill=1.0), (1.0, 1.0, 1.0), centre=(50.0, 50.0, 50.0))
    want, _, sim = _check(fs, IEEE, [body], ctx="no hit")
    sim.close()
    assert want == [L.ZERO], "all words 0; steps is 1 (checked by _check)"


def _everywhere(st):
    """a one-voxel body over four times the box: every particle is a hit"""
    field = np.array([0.01, 0.02, -0.015], dtype=f32).reshape(1, 1, 1, 3)
    return B.Body(field, (4.0 * st.size.x, 4.0 * st.size.y, 4.0 * st.size.z), velocity=(0.3, -0.2, 0.1), angular_velocity=(0.5, -0.25, 0.125))


def test_body_over_the_whole_block(fs):
    """every lane of every wave"""
    st, _, _, _, after = G._base(fs, fs.FS_MATH_IEEE)[:5]
    want, _, sim = _check(fs, IEEE, [_everywhere(st)], ctx="every particle")
    sim.close()
    assert want[0][6:] == [after.shape[0], 0]


def test_more_workgroups_than_shard_rows(fs):
    """26^3 = 17 576 particles are 69 workgroups: rows 0 .. 4 of the 64-row shard table take two workgroups each.  One body over
    the whole block, two steps; the second step's words are right only if the fold left the table zero.  The state a step starts
    from comes from a handle with the body and loads off (step 1: the uploaded lattice; step 2: its state after step 1, uploaded
    into a body-less handle), and that handle's bytes are also what the loads-on handle must leave."""
    st, off, tick = fs.dam_break_3d(26 ** 3)
    body = _everywhere(st)
    assert (st.particle_count + 255) // 256 == 69

    def handle(with_body, state=None):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        if state is not None:
            sim.upload_particles(state)
        if with_body:
            _add(sim, [body])
        return sim

    kin = handle(True)
    kin.tick(tick)
    k1 = kin.download_particles()
    kin.tick(tick)
    k2 = kin.download_particles()
    kin.close()
    want_words = []
    for start, expect in ((None, k1), (k1, k2)):
        plain = handle(False, start)
        plain.tick(tick)
        after = plain.download_particles()
        plain.close()
        want, w, _ = L.apply_bodies(after, [body], _size(st), tick.damping_factor)
        _same(expect, want, "the checker on a body-less step is the kinematic handle's step")
        want_words.append(w[0])
    assert all(w[6:] == [st.particle_count, 0] for w in want_words)
    sim = handle(True)
    sim.enable_body_loads()
    sim.tick(tick)
    sim.tick(tick)
    got, steps = _words(sim, [0])
    assert got == [L.add_words(*want_words)] and steps == [2]
    _same(sim.download_particles(), k2, "69 workgroups, two steps, loads on against loads off")
    sim.close()


@pytest.mark.parametrize("prep", [G._prep_emit, G._prep_emit_remove], ids=["emit", "emit+remove"])
def test_live_count_4097_under_capacity_4200(fs, prep):
    """a count of 4097: the last particle is alone in its workgroup and inside a body of its own (slot 0, so that it is hit where
    the step left it); after a removal, the count that left"""
    st, _, tick, _, after = G._base(fs, fs.FS_MATH_IEEE, prep)[:5]
    tail = B.Body(np.array([0.01, -0.01, 0.02], dtype=f32).reshape(1, 1, 1, 3), (0.05, 0.05, 0.05), centre=after["position"][-1],
                  velocity=(0.2, 0.1, -0.3))
    body = G._moving_body(fs, np.full((2, 2, 2, 3), 0.04, dtype=f32))
    want, recs, sim = _check(fs, IEEE, [tail, body], prep=prep, ctx=f"count {after.shape[0]}")
    sim.close()
    assert want[1][6] > 0 and recs[0]["hit"][-1], "the last particle is inside the first body"
    if prep is G._prep_emit:
        assert after.shape[0] == 4097, "one lane in the last workgroup"
    else:
        assert after.shape[0] < 4097


# ---- 4. slots ---------------------------------------------------------------------------------------------------------
def _fresh_body(fs):
    return G._moving_body(fs, np.array([0.05, -0.02, 0.03], dtype=f32).reshape(1, 1, 1, 3), extent=(0.7, 0.5, 0.6), centre=(-0.9, 0.4, 0.0), seed=0.3)


def test_eight_bodies_at_once_by_slot_with_slot_1_created_again(fs):
    """[a, x, c, d, e, f, g, h]: all 64 words of a row in use; slot 1 destroyed and created again before the step; every slot's
    words are its own body's"""
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    eight = G._small_bodies(fs, 8)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    assert _add(sim, eight) == list(range(8))
    sim.enable_body_loads()
    sim.remove_body(1)
    assert _add(sim, [_fresh_body(fs)]) == [1] and sim.body_count == 8
    order = [eight[0], _fresh_body(fs)] + eight[2:]
    sim.tick(tick)
    want, want_words, _ = L.apply_bodies(after, order, _size(st), tick.damping_factor)
    assert min(w[6] for w in want_words) > 0 and len({tuple(w) for w in want_words}) == 8, "every body hits, no two alike"
    _same(sim.download_particles(), want, "eight bodies, slot 1 created again")
    assert _words(sim, range(8)) == (want_words, [1] * 8)
    sim.close()


def test_bodies_by_slot_with_a_free_slot_and_a_reused_one(fs):
    """slot 1 destroyed and created again, slot 5 destroyed and left free: kernel indices 5 and 6 are slots 6 and 7; a slot that
    is reused after a step starts at zero while the others keep their words"""
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    eight = G._small_bodies(fs, 8)
    fresh = _fresh_body(fs)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    sim.enable_body_loads()
    assert _add(sim, eight) == list(range(8))
    sim.remove_body(1)
    sim.remove_body(5)
    assert _add(sim, [fresh]) == [1]
    slots = [0, 1, 2, 3, 4, 6, 7]
    order = [eight[0], fresh] + eight[2:5] + eight[6:]
    sim.tick(tick)
    want, want_words, _ = L.apply_bodies(after, order, _size(st), tick.damping_factor)
    assert min(w[6] for w in want_words) > 0 and len({tuple(w) for w in want_words}) == 7, "every body hits, no two alike"
    _same(sim.download_particles(), want, "seven bodies in eight slots")
    got, steps = _words(sim, slots)
    assert got == want_words and steps == [1] * 7
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads(5)
    assert "holds no body" in str(e.value)
    sim.remove_body(2)
    assert _add(sim, [eight[5]]) == [2]
    got, steps = _words(sim, [0, 2])
    assert got == [want_words[0], L.ZERO] and steps == [1, 0], "the reused slot starts at zero, slot 0 keeps its words"
    sim.close()


def test_two_overlapping_bodies_in_both_slot_orders(fs):
    """v0 of the second body is the first one's output, re-clamp included: the two orders give different words, each its own
    checker's"""
    p = G._moving_body(fs, CR.random_field((6, 5, 4), 21, fill=0.7, mag=0.3))
    q = G._moving_body(fs, CR.random_field((3, 7, 5), 22, fill=0.7, mag=0.3), extent=(0.9, 1.1, 0.8), centre=(-0.6, 0.2, -0.1), seed=-1.0)
    pq, _, sim = _check(fs, IEEE, [p, q], ctx="bodies (P, Q)")
    sim.close()
    qp, _, sim = _check(fs, IEEE, [q, p], ctx="bodies (Q, P)")
    sim.close()
    assert pq[1] != qp[0] and pq[0] != qp[1], "the second body sees what the first one left"


# ---- 5. drops and ties ------------------------------------------------------------------------------------------------
def _run_pair(fs, p, tick, bodies):
    """`p` uploaded into three handles, one step of `tick`: (the body-less handle's state, the state of the handle with the
    bodies and loads on, its words); the third handle, with the bodies and loads off, must leave the second one's bytes"""
    st, off = G._base(fs, fs.FS_MATH_IEEE)[:2]
    states = []
    for with_bodies in (False, True):
        plain = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        plain.upload_particles(p)
        if with_bodies:
            _add(plain, bodies)
        plain.tick(tick)
        states.append(plain.download_particles())
        plain.close()
    after, kinematic = states
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    _add(sim, bodies)
    sim.enable_body_loads()
    sim.tick(tick)
    got = sim.download_particles()
    words, _ = _words(sim, range(len(bodies)))
    sim.close()
    _same(got, kinematic, "loads on against loads off, the same bodies")
    return after, got, words


def test_out_of_range_and_nan_hits_are_dropped(fs):
    """Body 1 spins at 3e38 rad/s about y (finite, so fs3_body_set_motion takes it) over a box of two voxels.  Where |s.z| or |s.x|
    exceeds FLT_MAX / 3e38 = 1.13 the surface velocity overflows and inf - inf makes the hit's values NaN.  Elsewhere it is finite
    and enormous: in the voxel whose push is along the spin axis, us . n = 0 and v1 = us + (v0 - us) rounds to nearly nothing, so
    the hit stays in range and is KEPT; in the voxel whose push is tilted, v1 ~ 0.9 (us . n) n is finite and far above 2^14, so the
    hit is out of range.  Body 0 is an ordinary body beside it.  dropped, hits and the six sums of both bodies are the checker's,
    and the particles are byte for byte those of a handle with the same bodies and loads off (and the checker's, up to the sign
    and payload of a NaN)."""
    st, _, tick, p = G._base(fs, fs.FS_MATH_IEEE)[:4]
    body0 = G._moving_body(fs, CR.random_field((5, 4, 3), 7, fill=0.8, mag=0.05), extent=(0.6, 0.6, 0.6), centre=(-1.0, 0.5, 0.3))
    field = np.zeros((1, 1, 2, 3), dtype=f32)
    field[0, 0, 0] = (0.0, 0.03, 0.0)
    field[0, 0, 1] = (0.003, 0.03, 0.0)
    body1 = B.Body(field, (3.0, 3.0, 3.0), centre=(-0.8, 0.4, -0.5), angular_velocity=(0.0, 3e38, 0.0))
    after, got, words = _run_pair(fs, p, tick, [body0, body1])
    want, want_words, recs = L.apply_bodies(after, [body0, body1], _size(st), tick.damping_factor)
    cs = [np.stack(L.contributions(r)) for r in recs]
    nans = [int(np.isnan(c).any(axis=0).sum()) for c in cs]
    print(f"[body_loads3d] drops: checker {[[L.signed(x) for x in w[:6]] + w[6:] for w in want_words]}, hits with a NaN {nans}")
    assert want_words[0][6] > 20 and want_words[0][7] == 0, "body 0: ordinary hits"
    hits, dropped = want_words[1][6:]
    assert 0 < nans[1] < dropped < hits, "body 1: NaN hits, out-of-range hits and kept hits"
    _same_but_nan_bits(got, want, "drops: a dropped hit's particle is moved as the operator says")
    assert words == want_words


def test_dyadic_inputs_that_make_ties(fs):
    """The uploaded velocities are multiples of 2^-21 and the step has delta 0, so it adds no acceleration to them; the body's
    velocity is such a multiple too, its normal is the unit vector (1, 0, 0) (one voxel (g, 0, 0): len = g exactly) and damping is
    0.5, so for a velocity the step left alone j.x = (v.x - u.x) / 2 is a multiple of 2^-22, and a quarter of those lie exactly
    half way between two multiples of 2^-20.  The checker counts the exact ties among the kept contributions: hundreds."""
    st, _, tick0, p = G._base(fs, fs.FS_MATH_IEEE)[:4]
    tick = fs.TickSettings3(0.0, tick0.gravity, tick0.mass, tick0.pressure_constant, tick0.rest_density, 0.5, tick0.viscosity_coefficient)
    rng = np.random.default_rng(5)
    p = p.copy()
    p["velocity"] = (rng.integers(-2 ** 22, 2 ** 22, size=p["velocity"].shape) * 2.0 ** -21).astype(f32)
    field = np.array([0.0625, 0.0, 0.0], dtype=f32).reshape(1, 1, 1, 3)
    body = B.Body(field, (1.0, 1.0, 1.0), centre=(-0.8, 0.3, 0.1), velocity=(3 * 2.0 ** -21, 0.0, 0.0))
    after, got, words = _run_pair(fs, p, tick, [body])
    want, want_words, recs = L.apply_bodies(after, [body], _size(st), tick.damping_factor)
    _, ties = L.words(recs[0], want_ties=True)
    print(f"[body_loads3d] ties: {ties} exact ties in {want_words[0][6]} hits")
    assert ties >= 100 and want_words[0][7] == 0
    _same(got, want, "ties: particles")
    assert words == want_words


# ---- 6. with the other features ---------------------------------------------------------------------------------------
def test_surface_tension_tracking_and_profiling_give_the_same_words(fs):
    body = G._moving_body(fs, CR.random_field((6, 5, 4), 41, fill=0.7, mag=0.3))
    want, _, sim = _check(fs, IEEE, [body], prep=G._prep_st_track, ctx="surface tension + tracking")
    ids = G._base(fs, fs.FS_MATH_IEEE, G._prep_st_track)[5]
    assert np.array_equal(sim.particle_ids(), ids), "ids follow the sort, loads or not"
    sim.close()
    assert want[0][6] > 0
    plain, _, sim = _check(fs, IEEE, [body], ctx="plain")
    sim.close()

    def profiled(sim):
        sim.enable_body_loads()
        sim.profile(True)

    prof, _, sim = _check(fs, IEEE, [body], before=profiled, ctx="profiled")
    ms, steps = sim.profile_read()
    assert steps == 1 and ms["force"] > 0.0
    sim.close()
    assert plain == prof


def test_timed_steps_against_three_steps(fs):
    m = fs.FS_MATH_IEEE
    st, off, tick, p = G._base(fs, m)[:4]
    body = G._moving_body(fs, CR.random_field((6, 5, 4), 61, fill=0.7, mag=0.3))
    seen = []
    for timed in (False, True):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        sim.upload_particles(p)
        _add(sim, [body])
        sim.enable_body_loads()
        if timed:
            assert sim.timed_steps(tick, 3) > 0.0
        else:
            for _ in range(3):
                sim.tick(tick)
        seen.append((_words(sim, [0]), sim.download_particles()))
        sim.close()
    assert seen[0][0] == seen[1][0] and seen[0][0][1] == [3] and seen[0][0][0][0][6] > 0
    _same(seen[1][1], seen[0][1], "timed_steps with loads on")


def test_off_is_off(fs):
    """a handle that enabled and then disabled loads leaves, over 8 steps, the bytes of one that never did"""
    st, off, tick, p = G._base(fs, fs.FS_MATH_IEEE)[:4]
    bodies = G._small_bodies(fs, 3)
    outs = []
    for variant in ("never", "on then off"):
        sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
        sim.upload_particles(p)
        _add(sim, bodies)
        if variant != "never":
            sim.enable_body_loads()
            sim.enable_body_loads(False)
            assert not sim.body_loads_enabled
        for _ in range(8):
            sim.tick(tick)
        outs.append(sim.download_particles())
        sim.close()
    _same(outs[1], outs[0], "enabled and disabled against never enabled, 8 steps")


# ---- 7. life cycle and argument checks --------------------------------------------------------------------------------
def _device_words(fs, sim, ptr=None):
    out = np.zeros(fs._abi.FS3_MAX_BODIES * 8, dtype=np.uint64)
    sim.sync()
    ptr = sim.body_loads_device_ptr() if ptr is None else ptr
    assert sim._lib.fs_import_read(C.c_void_p(ptr), 0, out.ctypes.data_as(C.c_void_p), out.nbytes) == fs._abi.FS_OK
    return [[int(x) for x in row] for row in out.reshape(-1, 8)]


def test_life_cycle(fs):
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    a, b, c = G._small_bodies(fs, 3)
    off_sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)                 # loads never enabled
    off_sim.upload_particles(p)
    _add(off_sim, [a, b])
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    _add(sim, [a, b])
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads(0)
    assert e.value.status == fs._abi.FS_ERR_INVALID and "not enabled" in str(e.value)
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads_device_ptr()
    assert "not enabled" in str(e.value)
    sim.enable_body_loads()
    assert _words(sim, [0, 1]) == ([L.ZERO, L.ZERO], [0, 0])
    sim.tick(tick)
    off_sim.tick(tick)
    _, want, _ = L.apply_bodies(after, [a, b], _size(st), tick.damping_factor)
    assert min(w[6] for w in want) > 0
    assert _words(sim, [0, 1]) == (want, [1, 1])
    # the device words, copied back after sync(), are what fs3_body_loads returns; free slots are zero
    ptr = sim.body_loads_device_ptr()
    assert _device_words(fs, sim) == want + [L.ZERO] * 6
    # a body created while loads are on starts at zero; destroying a slot zeroes it and leaves the others
    assert _add(sim, [c]) == [2] and _words(sim, [2]) == ([L.ZERO], [0])
    sim.remove_body(2)
    sim.remove_body(1)
    assert _device_words(fs, sim) == [want[0]] + [L.ZERO] * 7, "destroy zeroes the slot"
    assert _add(sim, [b]) == [1] and _words(sim, [0, 1]) == ([want[0], L.ZERO], [1, 0])
    # disabled: a step counts nothing, the words are kept but cannot be read, and the particles are the always-off handle's
    sim.enable_body_loads(False)
    assert not sim.body_loads_enabled
    sim.tick(tick)
    off_sim.tick(tick)
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads(0)
    assert "not enabled" in str(e.value)
    _same(sim.download_particles(), off_sim.download_particles(), "on for one step, off for one, against always off")
    assert _device_words(fs, sim, ptr) == [want[0]] + [L.ZERO] * 7, "the step with loads off added nothing"
    # enabling zeroes, also when already on; the address is stable
    sim.enable_body_loads()
    assert _words(sim, [0, 1]) == ([L.ZERO, L.ZERO], [0, 0]) and sim.body_loads_device_ptr() == ptr
    sim.tick(tick)
    assert _words(sim, [0, 1])[1] == [1, 1] and _words(sim, [0])[0] != [L.ZERO]
    sim.enable_body_loads()
    assert _words(sim, [0, 1]) == ([L.ZERO, L.ZERO], [0, 0])
    sim.close()
    off_sim.close()


def test_argument_checks_in_the_headers_order(fs):
    st, off, tick, p, after = G._base(fs, fs.FS_MATH_IEEE)[:5]
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(p)
    lib, h, INV, OK = sim._lib, sim._h, fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    err = lambda: lib.fs_last_error().decode()      # noqa: E731
    out = fs.Body3Load()
    out.hits = 77
    ptr = C.c_void_p(5)
    # 1. the handle
    assert lib.fs3_body_loads_enable(None, 1) == INV and "null" in err()
    assert lib.fs3_body_loads(None, 9, None, 1) == INV and "null" in err()
    assert lib.fs3_body_loads_device(None, None) == INV and "null" in err()
    assert lib.fs3_body_loads_enabled(None) == 0
    # 2. the out pointer, before the slot and before "not enabled"
    assert lib.fs3_body_loads(h, 9, None, 1) == INV and "null" in err()
    assert lib.fs3_body_loads_device(h, None) == INV and "null" in err()
    # 3. the slot, before "not enabled"
    for k in (0, 7, 8, 0xFFFFFFFF):
        assert lib.fs3_body_loads(h, k, C.byref(out), 1) == INV and "holds no body" in err()
    body = G._small_bodies(fs, 1)[0]
    assert _add(sim, [body]) == [0]
    # 4. not enabled
    assert lib.fs3_body_loads(h, 0, C.byref(out), 1) == INV and "not enabled" in err()
    assert lib.fs3_body_loads_device(h, C.byref(ptr)) == INV and "not enabled" in err()
    assert out.hits == 77 and ptr.value == 5 and lib.fs3_body_loads_enabled(h) == 0, "a refused call sets nothing"
    assert lib.fs3_body_loads_enable(h, 1) == OK and lib.fs3_body_loads_enabled(h) == 1
    sim.tick(tick)
    _, want, _ = L.apply_bodies(after, [body], _size(st), tick.damping_factor)
    assert want[0][6] > 0
    # refused calls in between change nothing: the reset of a refused read does not happen
    assert lib.fs3_body_loads(h, 1, C.byref(out), 1) == INV and lib.fs3_body_loads(h, 0, None, 1) == INV
    assert _words(sim, [0]) == (want, [1])
    assert lib.fs3_body_loads(h, 0, C.byref(out), 1) == OK and out.hits == want[0][6] and out.steps == 1
    assert _words(sim, [0]) == ([L.ZERO], [0])
    sim.close()


# ---- 8. a dynamic body ------------------------------------------------------------------------------------------------
def test_body_dynamics_box_released_onto_the_block(fs):
    """a box released onto the top of the block through BodyDynamics3D for 8 steps: its pose stays finite and changes, the fluid is
    hit, and the particles are byte for byte those of a second handle fed the same recorded poses kinematically"""
    st, off, tick = fs.dam_break_3d(G.SIDE ** 3)
    ext = (0.6, 0.4, 0.6)
    field = CR.producer_field(B.solid_except((4, 4, 4), 1, (0, -1)), ext)
    top = float(off[1]) - 0.5 * G.SIDE * 0.1               # +y is down (gravity points there): the block's top face
    start = (float(off[0]), top - 0.02, 0.0)            # its solid middle reaches the top layer of particles at once
    dyn = fs.BodyDynamics3D(40.0, (2.0, 3.0, 2.5), start, gravity=(0.0, 9.81, 0.0), particle_mass=tick.mass)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    slot = sim.add_body(field, ext)
    sim.enable_body_loads()
    sim.set_body_motion(slot, *dyn.motion())
    poses, hits = [], 0
    for _ in range(8):
        poses.append(sim.body_motion(slot))
        sim.tick(tick)
        hits += dyn.advance(sim, slot, tick).hits
    got = sim.download_particles()
    sim.close()
    assert hits > 0 and np.isfinite(dyn.centre).all() and np.isfinite(dyn.rot).all() and np.isfinite(dyn.angular_momentum).all()
    assert tuple(dyn.centre) != start and len({tuple(np.asarray(q[0]).tolist()) for q in poses}) > 1, "the pose changes"
    kin = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    slot = kin.add_body(field, ext)
    for pose in poses:
        kin.set_body_motion(slot, *pose)
        kin.tick(tick)
    _same(got, kin.download_particles(), "dynamic body against the same poses set kinematically")
    kin.close()

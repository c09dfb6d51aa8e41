"""2D body loads on the GPU (include/fluidsim.h "2D body loads").  The checker is tests/body_loads2d_ref.py: the
restated operator and exact Python-int sums of Q over its hits.  Integer equality throughout: no tolerance in this file.  The
shapes and the shared states are those of tests/test_bodies2d_gpu.py (64^2, 66^2, 4097 of 4200)."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies2d_ref as B
from tests import body_loads2d_ref as L
from tests import test_bodies2d_gpu as G
from tests.handle_helpers import _same_but_nan_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
SORTS = G.SORTS
MODES = G.MODES
IEEE = "ieee"


def _on(sim):
    sim.enable_body_loads()


def _words(sim, slots, reset=False):
    """the five words of every slot of `slots` as Python ints modulo 2^64, and the steps"""
    got = [sim.body_loads(k, reset=reset) for k in slots]
    return [g.words() for g in got], [g.steps for g in got]


def _check(fs, mode, bodies, sort="bitonic", prep=None, before=_on, ctx=""):
    """One step of the shared jittered state with `bodies` and loads on, against the checker on the state a body-less handle
    leaves: the particles and, per slot, the words.  Returns (the checker's words, its per-body records, the still open handle)."""
    m = G._mode(fs, mode)
    st, _, tick, _, after = G._base(fs, m, sort, prep)[:5]
    want, want_words, recs = L.apply_bodies(after, bodies, G._size(st), tick.damping_factor)
    got, sim = G._one_step_with(fs, m, bodies, sort, prep=prep, keep=True, before=before)
    G._same(got, want, f"{ctx}: particles")
    got_words, steps = _words(sim, range(len(bodies)))
    print(f"[body_loads2d] {ctx}: {[[L.signed(x) for x in w] for w in want_words]}")
    assert got_words == want_words, f"{ctx}: words"
    assert steps == [1] * len(bodies)
    return want_words, recs, sim


# ---- 1. the scene against the oracle plus the operators ---------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("side", [64, 66])
def test_scene_words_and_particles(fs, orc, side, sort):
    """poses set before every step and no sync between the steps: after 1, 8 and 40 steps every slot's words are the checker's
    accumulated words, and the particles are bodies2d_ref.oracle_run's snapshots — loads on changes no particle byte"""
    run = L.scene_run(fs, orc, side, sort)
    ref = B.oracle_run(fs, orc, side, sort)
    sc = run["scene"]
    sim = fs.FluidSimulation(sc.st, device=0, initial_offset=sc.off, sort_mode=G._sort(fs, sort))
    for k, (field, extent) in enumerate(zip(sc.fields, sc.extents)):
        assert sim.add_body(field, extent) == k
    assert not sim.body_loads_enabled
    sim.enable_body_loads()
    assert sim.body_loads_enabled
    bodies = sc.bodies()
    for s in range(1, 41):
        for k, b in enumerate(sc.set_motions(bodies, s)):
            sim.set_body_motion(k, *b.motion())
        sim.tick(sc.tick)
        if s in (1, 8, 40):
            got, steps = _words(sim, range(3))
            assert got == L.accumulated(run["words"], s), f"side {side} {sort}: words after {s} steps"
            assert steps == [s, s, s]
            G._same(sim.download_particles(), ref["snap"][s], f"side {side} {sort} step {s} with loads on")
    sim.close()


@pytest.mark.parametrize("sort", SORTS)
def test_read_with_reset_after_every_step(fs, orc, sort):
    """the words of each single step, and their Python-int sum is the accumulated run"""
    run = L.scene_run(fs, orc, 64, sort)
    sc = run["scene"]
    sim = fs.FluidSimulation(sc.st, device=0, initial_offset=sc.off, sort_mode=G._sort(fs, sort))
    for field, extent in zip(sc.fields, sc.extents):
        sim.add_body(field, extent)
    sim.enable_body_loads()
    bodies = sc.bodies()
    acc = [L.ZERO] * 3
    for s in range(1, 41):
        for k, b in enumerate(sc.set_motions(bodies, s)):
            sim.set_body_motion(k, *b.motion())
        sim.tick(sc.tick)
        got, steps = _words(sim, range(3), reset=True)
        assert got == run["words"][s - 1], f"{sort}: the words of step {s} alone"
        assert steps == [1, 1, 1]
        acc = [L.add_words(a, g) for a, g in zip(acc, got)]
    assert acc == L.accumulated(run["words"], 40)
    got, steps = _words(sim, range(3))
    assert got == [L.ZERO] * 3 and steps == [0, 0, 0], "the last reset left zeros"
    sim.close()


def test_same_scene_twice_gives_the_same_words(fs, orc):
    """integer sums cannot depend on the order of the reduction: this guards a float slipping in"""
    sc = L.scene_run(fs, orc, 66)["scene"]
    seen = []
    for _ in range(2):
        sim = fs.FluidSimulation(sc.st, device=0, initial_offset=sc.off)
        for field, extent in zip(sc.fields, sc.extents):
            sim.add_body(field, extent)
        sim.enable_body_loads()
        bodies = sc.bodies()
        for s in range(1, 9):
            for k, b in enumerate(sc.set_motions(bodies, s)):
                sim.set_body_motion(k, *b.motion())
            sim.tick(sc.tick)
        seen.append(_words(sim, range(3)))
        sim.close()
    assert seen[0] == seen[1] and seen[0][0] == L.accumulated(L.scene_run(fs, orc, 66)["words"], 8)


# ---- 2. the operator alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("mode", MODES)
def test_operator_alone_in_every_math_and_sort_mode(fs, mode, sort):
    body = G._moving_body(fs, B.random_field((13, 9), 3, fill=0.6, mag=0.6))
    want, recs, sim = _check(fs, mode, [body], sort, ctx=f"operator alone, {mode} {sort}")
    sim.close()
    assert want[0][3] > 0 and recs[0]["clamped"].any() and want[0][4] == 0


# ---- 3. the edges of the reduction ------------------------------------------------------------------------------------
def test_one_pixel_body_with_exactly_one_hit(fs):
    st, _, tick, _, after = G._base(fs, fs.FS_MATH_IEEE)[:5]
    field = np.array([0.01, -0.02], dtype=f32).reshape(1, 1, 2)
    for j in range(1500, 1600):                       # the first particle the tiny box holds alone
        body = B.Body(field, (2e-3, 2e-3), centre=after["position"][j], velocity=(0.5, 0.25), angular_velocity=1.0)
        if int(L.apply_body(after, body, G._size(st), tick.damping_factor)[1]["hit"].sum()) == 1:
            break
    want, _, sim = _check(fs, IEEE, [body], ctx="one hit")
    sim.close()
    assert want[0][3:] == [1, 0] and want[0][:3] != [0, 0, 0]


def test_body_that_hits_nothing(fs):
    body = B.Body(B.random_field((4, 4), 1, fill=1.0), (1.0, 1.0), centre=(50.0, 50.0))
    want, _, sim = _check(fs, IEEE, [body], ctx="no hit")
    sim.close()
    assert want == [L.ZERO]


@pytest.mark.parametrize("sort", SORTS)
def test_body_over_the_whole_block(fs, sort):
    """both particles of every lane, every lane of every wave"""
    st, _, _, _, after = G._base(fs, fs.FS_MATH_IEEE, sort)[:5]
    field = np.array([0.01, 0.02], dtype=f32).reshape(1, 1, 2)
    body = B.Body(field, (4.0 * st.size.x, 4.0 * st.size.y), velocity=(0.3, -0.2), angular_velocity=0.5)
    want, _, sim = _check(fs, IEEE, [body], sort, ctx=f"every particle, {sort}")
    sim.close()
    assert want[0][3:] == [after.shape[0], 0]


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("prep", [G._prep_emit, G._prep_emit_remove], ids=["emit", "emit+remove"])
def test_live_count_4097_under_capacity_4200(fs, prep, sort):
    """an odd count's last particle, alone in its lane, is inside a body of its own; after a removal, the count that left"""
    st, _, tick, _, after = G._base(fs, fs.FS_MATH_IEEE, sort, prep)[:5]
    body = G._moving_body(fs, np.full((2, 2, 2), 0.04, dtype=f32))
    tail = B.Body(np.array([0.01, -0.01], dtype=f32).reshape(1, 1, 2), (0.05, 0.05), centre=after["position"][-1], velocity=(0.2, 0.1))
    want, recs, sim = _check(fs, IEEE, [body, tail], sort, prep=prep, ctx=f"count {after.shape[0]}, {sort}")
    sim.close()
    assert want[0][3] > 0 and recs[1]["hit"][-1], "the last particle is inside the second body"
    if prep is G._prep_emit:
        assert after.shape[0] == 4097, "an odd count: the last lane holds one particle"


def _fresh_body(fs):
    return G._moving_body(fs, np.array([0.05, -0.02], dtype=f32).reshape(1, 1, 2), extent=(0.7, 0.5), centre=(-5.2, 3.3), seed=0.3)


def test_eight_bodies_at_once_by_slot_with_slot_1_created_again(fs):
    """[a, x, c, d, e, f, g, h]: slot 1 destroyed and created again before the step; every slot's words are its own body's"""
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    eight = G._small_bodies(fs, 8)
    sim = G._make(fs, m, "bitonic")
    sim.upload_particles(p)
    assert G._add(sim, eight) == list(range(8))
    sim.enable_body_loads()
    sim.remove_body(1)
    assert G._add(sim, [_fresh_body(fs)]) == [1] and sim.body_count == 8
    order = [eight[0], _fresh_body(fs)] + eight[2:]
    sim.tick(tick)
    want, want_words, _ = L.apply_bodies(after, order, G._size(st), tick.damping_factor)
    assert min(w[3] for w in want_words) > 0 and len({tuple(w) for w in want_words}) == 8, "every body hits, no two alike"
    G._same(sim.download_particles(), want, "eight bodies, slot 1 created again")
    assert _words(sim, range(8)) == (want_words, [1] * 8)
    sim.close()


def test_bodies_by_slot_with_a_free_slot_and_a_reused_one(fs):
    """slot 1 destroyed and created again, slot 5 destroyed and left free: kernel indices 5 and 6 are slots 6 and 7; a slot that
    is reused after a step starts at zero while the others keep their words"""
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    eight = G._small_bodies(fs, 8)
    fresh = _fresh_body(fs)
    sim = G._make(fs, m, "bitonic")
    sim.upload_particles(p)
    sim.enable_body_loads()
    assert G._add(sim, eight) == list(range(8))
    sim.remove_body(1)
    sim.remove_body(5)
    assert G._add(sim, [fresh]) == [1]
    slots = [0, 1, 2, 3, 4, 6, 7]
    order = [eight[0], fresh] + eight[2:5] + eight[6:]
    sim.tick(tick)
    want, want_words, _ = L.apply_bodies(after, order, G._size(st), tick.damping_factor)
    assert min(w[3] for w in want_words) > 0 and len({tuple(w) for w in want_words}) == 7, "every body hits, no two alike"
    G._same(sim.download_particles(), want, "seven bodies in eight slots")
    got, steps = _words(sim, slots)
    assert got == want_words and steps == [1] * 7
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads(5)
    assert "holds no body" in str(e.value)
    sim.remove_body(2)
    assert G._add(sim, [eight[5]]) == [2]
    got, steps = _words(sim, [0, 2])
    assert got == [want_words[0], L.ZERO] and steps == [1, 0], "the reused slot starts at zero, slot 0 keeps its words"
    sim.close()


def test_two_overlapping_bodies_in_both_slot_orders(fs):
    """v0 of the second body is the first one's output: the two orders give different words, each its own checker's"""
    p = G._moving_body(fs, B.random_field((6, 5), 21, fill=0.7, mag=0.3))
    q = G._moving_body(fs, B.random_field((3, 7), 22, fill=0.7, mag=0.3), extent=(1.3, 1.7), centre=(-5.6, 3.2), seed=-1.0)
    pq, _, sim = _check(fs, IEEE, [p, q], ctx="bodies (P, Q)")
    sim.close()
    qp, _, sim = _check(fs, IEEE, [q, p], ctx="bodies (Q, P)")
    sim.close()
    assert pq[1] != qp[0] and pq[0] != qp[1], "the second body sees what the first one left"


# ---- 4. drops and ties ------------------------------------------------------------------------------------------------
def _run_pair(fs, p, tick, bodies, sort="bitonic"):
    """`p` uploaded into three handles, one step of `tick`: (the body-less handle's state, the state of the handle with the
    bodies and loads on, its words); the third handle, with the bodies and loads off, must leave the second one's bytes"""
    m = fs.FS_MATH_IEEE
    states = []
    for with_bodies in (False, True):
        plain = G._make(fs, m, sort)
        plain.upload_particles(p)
        if with_bodies:
            G._add(plain, bodies)
        plain.tick(tick)
        states.append(plain.download_particles())
        plain.close()
    after, kinematic = states
    sim = G._make(fs, m, sort)
    sim.upload_particles(p)
    G._add(sim, bodies)
    sim.enable_body_loads()
    sim.tick(tick)
    got = sim.download_particles()
    words, _ = _words(sim, range(len(bodies)))
    sim.close()
    G._same(got, kinematic, "loads on against loads off, the same bodies")
    return after, got, words


def test_out_of_range_and_nan_hits_are_dropped(fs):
    """Two particles inside body 0's box are uploaded with velocity (1e6, 0) and NaN, and the step has delta 0 so that nothing
    leaves the box; what the step itself makes of such velocities is the body-less handle's business, and the checker, applied to
    the state that handle leaves, decides whether they are hit and dropped.  Body 1 spins at 3e38 rad/s (finite, so
    fs_body_set_motion takes it): near its centre the surface velocity is finite and enormous, |j| >= 2^14; further out w * s
    overflows and inf - inf makes j a NaN; a few hits beside the centre line stay in range.  dropped, hits and the three sums of
    both bodies are the checker's, so the ordinary hits' contributions are intact, and the particles are byte for byte those of
    a handle with the same bodies and loads off (and the checker's, up to the sign and payload of a NaN)."""
    st, _, _, p = G._base(fs, fs.FS_MATH_IEEE)[:4]
    tick = fs.default_tick_settings(gravity=(0.0, 9.81), delta=0.0)
    c0 = np.array([-5.0, 2.0], dtype=f32)
    inside = np.where(np.abs(p["position"] - c0).max(axis=1) < 0.4)[0]
    assert inside.shape[0] > 20
    p = p.copy()
    p["velocity"][inside[3]] = (1e6, 0.0)
    p["velocity"][inside[10]] = (np.nan, np.nan)
    body0 = B.Body(B.random_field((5, 4), 7, fill=0.8, mag=0.05), (1.0, 1.0), centre=c0, velocity=(0.25, -0.5), angular_velocity=1.0)
    body1 = B.Body(np.array([0.0, 0.03], dtype=f32).reshape(1, 1, 2), (3.0, 3.0), centre=(-2.0, 0.5), angular_velocity=3e38)
    after, got, words = _run_pair(fs, p, tick, [body0, body1])
    want, want_words, recs = L.apply_bodies(after, [body0, body1], G._size(st), tick.damping_factor)
    cs = [L.contributions(r) for r in recs]
    nans = [int(np.isnan(np.stack(c)).any(axis=0).sum()) for c in cs]
    print(f"[body_loads2d] drops: checker {[[L.signed(x) for x in w] for w in want_words]}, hits with a NaN {nans}")
    assert want_words[0][3] > 50 and want_words[0][3] > want_words[0][4], "body 0: ordinary hits"
    hits, dropped = want_words[1][3:]
    assert 0 < nans[1] < dropped < hits, "body 1: NaN hits, out-of-range hits and kept hits"
    _same_but_nan_bits(got, want, "drops: a dropped hit's particle is moved as the operator says")
    assert words == want_words


def test_dyadic_inputs_that_make_ties(fs):
    """A step of delta 0 leaves the uploaded velocities, multiples of 2^-21; the body's velocity is one too, its normal is the
    unit vector (1, 0) (one pixel (g, 0): len = g exactly) and damping is 0.5, so j.x = (v.x - u.x) / 2 is a multiple of 2^-22:
    a quarter of the hits lie exactly half way between two multiples of 2^-20."""
    st, _, _, p = G._base(fs, fs.FS_MATH_IEEE)[:4]
    tick = fs.default_tick_settings(gravity=(0.0, 9.81), delta=0.0, damping_factor=0.5)
    rng = np.random.default_rng(5)
    p = p.copy()
    p["velocity"] = (rng.integers(-2 ** 22, 2 ** 22, size=p["velocity"].shape) * 2.0 ** -21).astype(f32)
    field = np.array([0.0625, 0.0], dtype=f32).reshape(1, 1, 2)
    body = B.Body(field, (3.0, 3.0), centre=(-4.0, 1.5), velocity=(3 * 2.0 ** -21, 0.0))
    after, got, words = _run_pair(fs, p, tick, [body])
    want, want_words, recs = L.apply_bodies(after, [body], G._size(st), tick.damping_factor)
    _, ties = L.words(recs[0], want_ties=True)
    print(f"[body_loads2d] ties: {ties} exact ties in {want_words[0][3]} hits")
    assert ties > 0 and want_words[0][4] == 0
    G._same(got, want, "ties: particles")
    assert words == want_words


# ---- 5. with the other features ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", SORTS)
def test_live_aos_view_and_profiling_give_the_same_words(fs, sort):
    body = G._moving_body(fs, B.random_field((6, 5), 41, fill=0.7, mag=0.6))
    plain, _, sim = _check(fs, IEEE, [body], sort, ctx=f"plain, {sort}")
    sim.close()
    seen = {}

    def export(sim):
        sim.enable_body_loads()
        sim.export_handle()
        seen["view"] = sim.particles_device_ptr()

    aos, _, sim = _check(fs, IEEE, [body], sort, before=export, ctx=f"live AoS view, {sort}")
    out = np.empty(sim.particle_count, dtype=fs.PARTICLE_DTYPE)
    assert sim._lib.fs_import_read(C.c_void_p(seen["view"]), 0, out.ctypes.data_as(C.c_void_p), out.shape[0] * 32) == fs._abi.FS_OK
    G._same(out, sim.download_particles(), f"exported records with loads on, {sort}")
    sim.close()

    def profiled(sim):
        sim.enable_body_loads()
        sim.profile(True)

    prof, _, sim = _check(fs, IEEE, [body], sort, before=profiled, ctx=f"profiled, {sort}")
    ms, steps = sim.profile_read()
    assert steps == 1 and ms["force"] > 0.0
    sim.close()
    assert plain == aos == prof


@pytest.mark.parametrize("sort", SORTS)
def test_timed_steps_against_three_steps(fs, sort):
    m = fs.FS_MATH_IEEE
    st, off, tick, p = G._base(fs, m, sort)[:4]
    body = G._moving_body(fs, B.random_field((6, 5), 61, fill=0.7, mag=0.3))
    seen = []
    for timed in (False, True):
        sim = G._make(fs, m, sort)
        sim.upload_particles(p)
        G._add(sim, [body])
        sim.enable_body_loads()
        if timed:
            assert sim.timed_steps(tick, 3) > 0.0
        else:
            for _ in range(3):
                sim.tick(tick)
        seen.append((_words(sim, [0]), sim.download_particles()))
        sim.close()
    assert seen[0][0] == seen[1][0] and seen[0][0][1] == [3] and seen[0][0][0][0][3] > 0
    G._same(seen[1][1], seen[0][1], f"timed_steps with loads on, {sort}")


# ---- 6. life cycle and argument checks --------------------------------------------------------------------------------
def _device_words(fs, sim):
    out = np.zeros(fs._abi.FS_MAX_BODIES * 5, dtype=np.uint64)
    sim.sync()
    assert sim._lib.fs_import_read(C.c_void_p(sim.body_loads_device_ptr()), 0, out.ctypes.data_as(C.c_void_p), out.nbytes) == fs._abi.FS_OK
    return [[int(x) for x in row] for row in out.reshape(-1, 5)]


def test_life_cycle(fs):
    m = fs.FS_MATH_IEEE
    st, off, tick, p, after = G._base(fs, m)[:5]
    two_steps = G._base(fs, m, steps=2)[4]
    a, b = G._small_bodies(fs, 2)
    off_sim = G._make(fs, m, "bitonic")                 # loads never enabled
    off_sim.upload_particles(p)
    G._add(off_sim, [a, b])
    sim = G._make(fs, m, "bitonic")
    sim.upload_particles(p)
    G._add(sim, [a, b])
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
    _, want, _ = L.apply_bodies(after, [a, b], G._size(st), tick.damping_factor)
    assert min(w[3] for w in want) > 0
    assert _words(sim, [0, 1]) == (want, [1, 1])
    # the device words, copied back after sync(), are what fs_body_loads returns; free slots are zero
    ptr = sim.body_loads_device_ptr()
    assert _device_words(fs, sim) == want + [L.ZERO] * 6
    # disabled: a step counts nothing, the words cannot be read, and the particles are the always-off handle's
    sim.enable_body_loads(False)
    assert not sim.body_loads_enabled
    sim.tick(tick)
    off_sim.tick(tick)
    with pytest.raises(fs.FluidSimError) as e:
        sim.body_loads(0)
    assert "not enabled" in str(e.value)
    G._same(sim.download_particles(), off_sim.download_particles(), "on for one step, off for one, against always off")
    assert two_steps.tobytes() != off_sim.download_particles().tobytes(), "the bodies act"
    out = np.zeros(40, dtype=np.uint64)
    assert sim._lib.fs_import_read(C.c_void_p(ptr), 0, out.ctypes.data_as(C.c_void_p), out.nbytes) == fs._abi.FS_OK
    assert [[int(x) for x in row] for row in out.reshape(-1, 5)] == want + [L.ZERO] * 6, "the step with loads off added nothing"
    # enabling zeroes, also when already on
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
    sim = G._make(fs, fs.FS_MATH_IEEE, "bitonic")
    sim.upload_particles(p)
    lib, h, INV, OK = sim._lib, sim._h, fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    err = lambda: lib.fs_last_error().decode()      # noqa: E731
    out = fs.BodyLoad()
    out.hits = 77
    ptr = C.c_void_p(5)
    # 1. the handle
    assert lib.fs_body_loads_enable(None, 1) == INV and "null" in err()
    assert lib.fs_body_loads(None, 9, None, 1) == INV and "null" in err()
    assert lib.fs_body_loads_device(None, None) == INV and "null" in err()
    assert lib.fs_body_loads_enabled(None) == 0
    # 3. the out pointer, before the slot and before "not enabled"
    assert lib.fs_body_loads(h, 9, None, 1) == INV and "null" in err()
    assert lib.fs_body_loads_device(h, None) == INV and "null" in err()
    # 4. the slot, before "not enabled"
    for k in (0, 7, 8, 0xFFFFFFFF):
        assert lib.fs_body_loads(h, k, C.byref(out), 1) == INV and "holds no body" in err()
    body = G._small_bodies(fs, 1)[0]
    assert G._add(sim, [body]) == [0]
    # 5. not enabled
    assert lib.fs_body_loads(h, 0, C.byref(out), 1) == INV and "not enabled" in err()
    assert lib.fs_body_loads_device(h, C.byref(ptr)) == INV and "not enabled" in err()
    assert out.hits == 77 and ptr.value == 5 and lib.fs_body_loads_enabled(h) == 0, "a refused call sets nothing"
    assert lib.fs_body_loads_enable(h, 1) == OK and lib.fs_body_loads_enabled(h) == 1
    sim.tick(tick)
    _, want, _ = L.apply_bodies(after, [body], G._size(st), tick.damping_factor)
    assert want[0][3] > 0
    # refused calls in between change nothing: the reset of a refused read does not happen
    assert lib.fs_body_loads(h, 1, C.byref(out), 1) == INV and lib.fs_body_loads(h, 0, None, 1) == INV
    assert _words(sim, [0]) == (want, [1])
    assert lib.fs_body_loads(h, 0, C.byref(out), 1) == OK and out.hits == want[0][3] and out.steps == 1
    assert _words(sim, [0]) == ([L.ZERO], [0])
    sim.close()


def test_slab_handle_is_refused_as_unsupported(fs):
    st, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    lib, h, UNS = fs.load_library(), slab._h, fs._abi.FS_ERR_UNSUPPORTED
    out, ptr = fs.BodyLoad(), C.c_void_p()
    assert lib.fs_body_loads_enable(h, 1) == UNS and "slab" in lib.fs_last_error().decode()
    assert lib.fs_body_loads(h, 0, None, 0) == UNS and lib.fs_body_loads(h, 0, C.byref(out), 0) == UNS
    assert lib.fs_body_loads_device(h, None) == UNS and lib.fs_body_loads_device(h, C.byref(ptr)) == UNS
    assert lib.fs_body_loads_enabled(h) == 0
    slab.close()


# ---- 7. a dynamic body ------------------------------------------------------------------------------------------------
def test_body_dynamics_smoke(fs):
    """a box released onto the top of the block for 20 steps: its pose stays finite and changes, the fluid is hit, and the
    particles are those of a kinematic handle fed the same recorded poses"""
    st, off, tick = fs.dam_break_2d(G.SIDE ** 2)
    field = B.producer_field(B.solid_except((6, 6), 0, (0, -1)), (0.8, 0.8))
    start = (-3.2, -2.3)                                 # the block's top is at y = -2.4; +y: gravity points there
    dyn = fs.BodyDynamics2D(40.0, 5.0, start, gravity=(0.0, 9.81), particle_mass=tick.mass)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    slot = sim.add_body(field, (0.8, 0.8))
    sim.enable_body_loads()
    sim.set_body_motion(slot, *dyn.motion())
    poses, hits = [], 0
    for _ in range(20):
        poses.append(sim.body_motion(slot))
        sim.tick(tick)
        hits += dyn.advance(sim, slot, tick).hits
    got = sim.download_particles()
    sim.close()
    assert hits > 0 and np.isfinite(dyn.centre).all() and np.isfinite([dyn.angle, dyn.angular_velocity]).all()
    assert tuple(dyn.centre) != start and len({tuple(np.asarray(q[0]).tolist()) for q in poses}) > 1, "the pose changes"
    kin = fs.FluidSimulation(st, device=0, initial_offset=off)
    slot = kin.add_body(field, (0.8, 0.8))
    for pose in poses:
        kin.set_body_motion(slot, *pose)
        kin.tick(tick)
    G._same(got, kin.download_particles(), "dynamic body against the same poses set kinematically")
    kin.close()

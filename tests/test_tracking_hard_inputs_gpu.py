"""Particle tracking (k_track_carry behind k_reorder / k_cs_fixreorder) at the inputs at which the plain 2D step is
held: every case of tests/hard_states2d.py — operand guards, NaN and infinite velocities, coincident particles, ragged and tiny
counts, the sixteen random configurations in both sort modes, dense_scene, corner clusters, the staging scenes and the
counting-sort scenes — with four channels, at every step; the sort's other launch sequences (per-stage plan, stand-by kernel,
another fused stage, a shuffled upload mid-run) around the first certificate's sizes; capacity > n; and several steps of the
step variants the oracle cannot follow bit for bit.

The checker is tests/track_ref.TrackChecker, unchanged: the oracle stepped pass by pass and the permutation its sort applies.
Ids and channels are compared word for word (assert_track_equal) and the state exactly as the plain parity tests compare it
(assert_state_equal: keys, the four float fields on their bits, start_indices — also where the oracle's records are NaN or
infinite).  That the cases are not vacuous — most slots change occupant, the tie cases have slots where the reference network
and the stable sort disagree — is asserted without a GPU in tests/test_tracking.py."""
import numpy as np
import pytest

from tests import hard_states2d as H
from tests import parity_states as PS
from tests.bitcmp import POOL_TWELVE, assert_track_equal, bits, special_bits
from tests.test_tracking_gpu import assert_not_vacuous, assert_state_equal, make_pair

pytestmark = pytest.mark.gpu
CHANNELS = 4


class Ref:
    """one checker step in the shape assert_track_equal and assert_state_equal read"""

    def __init__(self, ids, attr, rec, start):
        self.ids, self.attr, self.channels, self.n = ids, attr, attr.shape[0], ids.shape[0]
        self._rec, self._start = rec, start

    def particles_view(self): return self._rec
    def start_indices_view(self): return self._start


def channel_values(start):
    """arange(n), the start x, NaN payloads / -0.0 / denormals / infinities, and one channel left at the enable's +0.0"""
    n = start.shape[0]
    return [np.arange(n, dtype=np.float32), np.ascontiguousarray(start["position"][:, 0]), special_bits(n, 99, POOL_TWELVE)]


def upload_channel_values(sim, start):
    vals = channel_values(start)
    for c, v in enumerate(vals):
        sim.set_attribute(c, v)
        assert np.array_equal(bits(sim.attribute(c)), bits(v)), f"channel {c}: upload / download is not a bit copy"
    assert not bits(sim.attribute(3)).any()
    return np.stack(vals + [np.zeros(start.shape[0], dtype=np.float32)])


def engine(fs, case, **kw):
    sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, ref_quirks=case.quirks,
                             sort_mode=fs.FS_SORT_COUNTING if case.stable else fs.FS_SORT_BITONIC, track=CHANNELS, **kw)
    sim.upload_particles(case.start)
    if case.start_indices is not None:
        sim.upload_start_indices(case.start_indices)
    if case.field is not None:
        sim.upload_force_field(case.field)
    return sim


# ---- 1. every registry case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.CASE_IDS)
def test_tracking_at_the_hard_inputs(fs, orc, cid):
    case = H.case_by_id(fs, orc, cid)
    ref = case.run()
    print(case.describe())
    sim = engine(fs, case)
    n = case.n
    ids, attr = np.arange(n, dtype=np.uint32), upload_channel_values(sim, case.start)
    assert np.array_equal(sim.particle_ids(), ids)
    for s, step in enumerate(ref):
        sim.tick(case.tick)
        ids, attr = ids[step.perm], attr[:, step.perm]
        got = sim.particle_ids()
        assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32)), f"{cid} step {s}: the ids are no permutation"
        want = Ref(ids, attr, step.rec, step.start)
        assert_track_equal(sim, want, f"{cid} step {s}")
        assert_state_equal(sim, want, f"{cid} step {s}")
    if n >= H.MOVED_MIN_N:
        assert max(case.moved()) > 0.5
    sim.close()


# ---- 2. the sort's launch sequences -------------------------------------------------------------------------------------------
SEQUENCES = [("default", {}), ("per_stage", {"FS_SORT_POLICY": "0", "FS_SORT_FUSE_STAGE": "0"}), ("trusted", {"FS_SORT_TRUST": "1"}),
             ("fuse13", {"FS_SORT_FUSE_STAGE": "13"})]
SEQ_STEPS, SEQ_SHUFFLE_BEFORE = 6, 3          # a shuffled upload before step 4


def _sequence_reference(fs, orc, n):
    """the jittered dam break of n particles with coincident_state's six coincident ones, on the checker with four channels:
    6 steps, the records shuffled before step 4 (ids and channels stay with the slot).  -> (settings, offset, tick, start
    records, the permutation of the shuffle, [Ref per step])"""
    from tests.track_ref import TrackChecker
    st, off, tick, p = PS.jittered_dam_break(fs, orc, n, n)
    p = PS.coincident_state(p)
    chk = TrackChecker(st, off, channels=CHANNELS)
    chk.set_particles(p)
    for c, v in enumerate(channel_values(p)):
        chk.attr[c] = v
    shuffle = np.random.default_rng(n).permutation(n)
    refs = []
    for s in range(SEQ_STEPS):
        if s == SEQ_SHUFFLE_BEFORE:
            chk.set_particles(chk.particles()[shuffle])
        chk.step(tick)
        refs.append(Ref(chk.ids.copy(), chk.attr.copy(), chk.particles(), chk.start_indices_view().copy()))
    assert_not_vacuous(chk)
    chk.close()
    return st, off, tick, p, shuffle, refs


@pytest.mark.parametrize("n", [8192, 8193, 12289, 65536])
def test_every_sort_launch_sequence_leaves_the_same_source_slots(fs, orc, monkeypatch, n):
    """The default policy, the per-stage plan, the stand-by kernel and a fused stage 13 — tests/test_sort_gpu.py shows that they
    leave the same records; here that they leave the same source-slot word for the carry pass: ids and channels are the
    checker's at every step, through a shuffled upload (after which the first kernel's tiles are unordered).  The environment
    is read at create, so it is set around the handle's creation only.  Nothing injects a time-out."""
    st, off, tick, p, shuffle, refs = _sequence_reference(fs, orc, n)
    for name, env in SEQUENCES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sim = fs.FluidSimulation(st, device=0, initial_offset=off, track=CHANNELS)
        for k in env:
            monkeypatch.delenv(k)
        sim.upload_particles(p)
        upload_channel_values(sim, p)
        for s, want in enumerate(refs):
            if s == SEQ_SHUFFLE_BEFORE:
                sim.upload_particles(sim.download_particles()[shuffle])
            sim.tick(tick)
            assert_track_equal(sim, want, f"n={n} {name} step {s}")
            assert_state_equal(sim, want, f"n={n} {name} step {s}")
        info = sim.sort_plan()
        print(f"[sort_plan] n={n} {name}: {info}")
        assert info["timeouts"] == 0
        if n == 65536 and name == "default":
            assert info["shifted"] > 0, info
        if n == 65536 and name == "trusted":
            assert info["standby_runs"] >= 1, info
        sim.close()


# ---- 3. capacity > n ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_capacity_above_n(fs, counting):
    """The channel stride of the 2D handle is its capacity, not n."""
    n, cap = 5000, 6000
    sim, chk, tick = make_pair(fs, n, channels=CHANNELS, sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC, capacity=cap)
    assert sim.particle_count == n
    assert sim.attribute_device_ptr(1) - sim.attribute_device_ptr(0) >= 4 * cap
    chk.attr[:] = upload_channel_values(sim, chk.particles())
    for s in range(4):
        sim.tick(tick)
        chk.step(tick, stable_sort=counting)
        assert_track_equal(sim, chk, f"capacity {cap} counting={counting} step {s}")
        assert_state_equal(sim, chk, f"capacity {cap} counting={counting} step {s}")
    assert_not_vacuous(chk)
    sim.close(); chk.close()


# ---- 4. several steps of the other step variants ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["surface_tension", "tolerance", "wgsl_ulp"])
def test_several_steps_of_the_other_step_variants(fs, variant):
    """The oracle cannot follow these modes bit for bit, so before every step the checker's records are re-seeded from the
    handle's download (ids and channels stay): the step's keys come from the downloaded positions and velocities alone — the
    argument of test_one_step_of_the_other_step_variants — and so does the permutation.  The handle is never re-uploaded."""
    n = 16384
    kw = {"surface_tension": dict(surface_tension=True), "tolerance": dict(math_mode=fs.FS_MATH_TOLERANCE),
          "wgsl_ulp": dict(math_mode=fs.FS_MATH_WGSL_ULP)}[variant]
    sim, chk, tick = make_pair(fs, n, channels=CHANNELS, **kw)
    if variant == "surface_tension":
        tick.surface_tension_coefficient = 35.0
    chk.attr[:] = upload_channel_values(sim, chk.particles())
    moved = []
    for s in range(6):
        chk.set_particles(sim.download_particles())
        sim.tick(tick)
        perm = chk.step(tick)
        moved.append(float((perm != np.arange(n)).mean()))
        assert np.array_equal(sim.download_particles()["grid"], chk.particles_view()["grid"]), f"{variant} step {s}: cell keys differ"
        assert_track_equal(sim, chk, f"{variant} step {s}")
    print(f"[moved] {variant}: {moved}")
    assert max(moved) > 0.5, moved                 # the registry's condition: a step in which most slots change occupant
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(n, dtype=np.uint32))
    sim.close(); chk.close()

"""The slab step on the hard inputs of tests/slab_scenes.py (whose paths, travel and tolerances tests/test_slab_scenes.py proves on
the CPU), against the CPU ORACLE — the reference shares no kernel with the code under test:

  (a) test_single_slab_equals_the_oracle       one slab over the whole domain (no neighbours, counting sort, reference layout): every
                                               field of every owned record bit for bit, 4 steps — with an uploaded force field and
                                               with the field generate_force_field makes of an obstacle image;
  (b) test_serial_and_edge_first_leave_the_same_bytes
                                               two runs side by side with real messages, serial and edge-first, default and
                                               FS_SLAB_ROWMAJOR layout: owned masks, owned records, counters and outgoing messages
                                               byte-equal after every one of 8 steps — with both deferred-wave lists non-empty in
                                               both launches of the overlapped step;
  (c) test_every_mode_matches_the_oracle       serial, edge, strips, bitonic, serial and edge with FS_SLAB_ROWMAJOR: steps 1 and 2
                                               within match_and_compare's tolerances, cell keys exact, finite after 8 steps;
  (d) test_nothing_disappears_silently         walls_and_bad_values in every mode: owned + lost == n, and finite wherever the
                                               oracle is.

What the timing of an overlapped step makes of the two launches' shared lists cannot be forced from here: (b) makes the
interleaving possible (close pairs on both sides of adv_lo / adv_hi in one 256-slot block), it does not prove it happened."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import slab_scenes as S
from tests.test_multi_gpu import InProcessSlabs
from tests.test_parity_gpu import assert_particles_equal

pytestmark = pytest.mark.gpu
RECV = 4096
MODES = {"serial": dict(serial=True), "edge": dict(), "strips": dict(strips=True), "bitonic": dict(serial=True, sort_mode="bitonic"),
         "serial_rowmajor": dict(serial=True, rowmajor=True), "edge_rowmajor": dict(rowmajor=True)}
SCENES = [(name, world) for name in S.FIXED for world in (2, 3)] + [("obstacle_on_seam", 2)] + [("random", k) for k in range(S.RANDOM_CASES)]
ALL_SCENES = SCENES[:2] + [("cluster_with_coincident", 2), ("cluster_with_coincident", 3)] + SCENES[2:]
ORACLE_STEPS = 4


def get_scene(name, world):
    """-> (settings, tick, particles, bounds, boundary_cols, field)"""
    if name == "random":
        st, tick, p, bounds, field, z = S.random_settings(world)
        return st, tick, p, bounds, z, field
    return S.scene(name, world) + (S.scene_field(name),)


@functools.lru_cache(maxsize=None)
def oracle_states(name, world):
    """The oracle's states after steps 1 .. ORACLE_STEPS: computed once per scene, shared by every mode, never written to."""
    st, tick, p, bounds, z, field = get_scene(name, world)
    return S.step_oracle(st, tick, p, ORACLE_STEPS, field)


@functools.lru_cache(maxsize=None)
def engine_obstacle_field(fs):
    made = fs.generate_force_field(S.obstacle_image())
    assert np.array_equal(made.view(np.uint32), S.obstacle_field().view(np.uint32)), "generate_force_field differs from the oracle's field"
    return made


def make_slabs(fs, name, world, mode=None, bounds=None, **kw):
    st, tick, p, b, z, field = get_scene(name, world)
    kw = dict(MODES[mode] if mode else {}, **kw)
    if name == "obstacle_on_seam":          # the field the oracle was given (orc_gradient_field), produced by the engine
        field = engine_obstacle_field(fs)
    if kw.get("sort_mode") == "bitonic":
        kw["sort_mode"] = fs.FS_SORT_BITONIC
    n = p.shape[0]
    bounds = list(b if bounds is None else bounds)
    slabs = InProcessSlabs(fs, st, (0.0, 0.0), len(bounds) - 1, cap=n + 4 * RECV, recv=RECV, particles=p, bounds=bounds,
                           boundary_cols=z, field=field, **kw)
    return slabs, st, tick, p


def close(slabs):
    for s in slabs.sims:
        s.close()
    for b in slabs.bufs:
        for x in b.values():
            x.close()


def match_to_oracle(got, want):
    """`want` in the order of `got`: records with a finite predicted position by the nearest one (a bijection, asserted), the others
    (a NaN velocity leaves a NaN prediction for one step; the particle itself stays where it was) by the bits of their position."""
    from scipy.spatial import cKDTree
    assert got.shape[0] == want.shape[0], (got.shape, want.shape)
    fg, fw = np.isfinite(got["predicted_position"]).all(axis=1), np.isfinite(want["predicted_position"]).all(axis=1)
    assert fg.sum() == fw.sum()
    out = np.empty_like(want)
    wf = want[fw]
    _, idx = cKDTree(wf["predicted_position"].astype(np.float64)).query(got["predicted_position"][fg].astype(np.float64))
    assert np.unique(idx).shape[0] == idx.shape[0], "matching is not a bijection"
    out[fg] = wf[idx]
    bits = lambda a: np.ascontiguousarray(a["position"]).view(np.uint64).reshape(-1)
    gb, wb = got[~fg], want[~fw]
    og, ow = np.argsort(bits(gb)), np.argsort(bits(wb))
    assert np.array_equal(bits(gb)[og], bits(wb)[ow]), "records with a NaN prediction are not where the oracle's are"
    tmp = np.empty_like(wb)
    tmp[og] = wb[ow]
    out[~fg] = tmp
    return out


def compare_with_oracle(got, want, h, **tol):
    """match_and_compare on the records with a finite prediction, cell keys exact; the records with a NaN prediction (step 1 of
    walls_and_bad_values) must equal the oracle's: same key, zero velocity, NaN density."""
    from tests.slab_oracle import match_and_compare
    fg, fw = np.isfinite(got["predicted_position"]).all(axis=1), np.isfinite(want["predicted_position"]).all(axis=1)
    match_and_compare(got[fg], want[fw], h, max_key_flips=0.0, **tol)
    if (~fg).any() or (~fw).any():
        w = match_to_oracle(got, want)
        a, b = got[~fg], w[~fg]
        assert np.array_equal(a["grid"], b["grid"])
        np.testing.assert_array_equal(a["velocity"], b["velocity"])
        np.testing.assert_array_equal(a["density"], b["density"])


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", [("cluster_with_coincident", 2), ("mouse_and_field_on_seam", 2), ("obstacle_on_seam", 2),
                                        ("walls_and_bad_values", 2), ("random", 0), ("random", 3)])
def test_single_slab_equals_the_oracle(fs, orc, name, world):
    """engine_slab.hip: a slab without neighbours keeps the reference layout and is bit-identical to the plain counting engine —
    here against the oracle itself (stable sort, quirks off), through pack and step with null buffers."""
    st, tick, p, b, z, field = get_scene(name, world)
    slabs, st, tick, p = make_slabs(fs, name, world, bounds=[0, S.grid_width(st)])
    want = oracle_states(name, world)
    sim = slabs.sims[0]
    assert not sim.cfg.has_left and not sim.cfg.has_right
    for step in range(ORACLE_STEPS):
        sim.pack(tick, None, None)
        sim.step(None, None)
        sim.sync()
        rec, own = sim.download()
        assert own.all() and rec.shape[0] == p.shape[0]
        assert_particles_equal(rec, want[step], f"single slab {name}/{world} step {step + 1}")
    slabs.assert_clean()
    close(slabs)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def step_and_capture(slabs, tick):
    """InProcessSlabs.step, returning every rank's outgoing messages as they were when the exchange copied them."""
    P = lambda b: C.c_void_p(b.device_ptr)
    for r, s in enumerate(slabs.sims):
        s.pack(tick, P(slabs.bufs[r]["sl"]), P(slabs.bufs[r]["sr"]))
    for s in slabs.sims:
        s.wait_packed()
    sent = [(slabs.bufs[r]["sl"].read() if r > 0 else None, slabs.bufs[r]["sr"].read() if r < slabs.world - 1 else None)
            for r in range(slabs.world)]
    for r in range(slabs.world):
        if r > 0:
            slabs.bufs[r]["rl"].write(0, sent[r - 1][1])
        if r < slabs.world - 1:
            slabs.bufs[r]["rr"].write(0, sent[r + 1][0])
    for r, s in enumerate(slabs.sims):
        s.step(P(slabs.bufs[r]["rl"]) if r > 0 else None, P(slabs.bufs[r]["rr"]) if r < slabs.world - 1 else None)
    for s in slabs.sims:
        s.sync()
    return sent


def assert_messages_equal(a, b, ctx):
    for side, (x, y) in zip(("left", "right"), zip(a, b)):
        assert (x is None) == (y is None)
        if x is None:
            continue
        cnt = int(x[:16].view(np.uint32)[0])
        assert np.array_equal(x[:16], y[:16]), f"{ctx} {side}: headers {x[:16].view(np.uint32)} {y[:16].view(np.uint32)}"
        assert cnt <= RECV and np.array_equal(x[16:16 + 16 * cnt], y[16:16 + 16 * cnt]), f"{ctx} {side}: records differ"


@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("name,world", ALL_SCENES + [("rebalanced", 2)])
def test_serial_and_edge_first_leave_the_same_bytes(fs, name, world, rowmajor):
    """test_edge_first_prebuilt_messages_equal_a_full_pack's invariant with ghosts and migrants actually arriving and the deferred-wave
    lists non-empty: after every step the serial and the edge-first run of the same ranks agree in every byte they expose.  The
    `rebalanced` case moves the seam by one column after step 3 (set_window in both runs, late_list_on_both_sides)."""
    rebalanced = name == "rebalanced"
    name = "late_list_on_both_sides" if rebalanced else name
    ser, st, tick, p = make_slabs(fs, name, world, serial=True, rowmajor=rowmajor)
    edg, _, _, _ = make_slabs(fs, name, world, rowmajor=rowmajor)
    assert [s.step_mode for s in ser.sims] == [0] * ser.world and [s.step_mode for s in edg.sims] == [1] * edg.world
    for step in range(1, S.STEPS + 1):
        ma, mb = step_and_capture(ser, tick), step_and_capture(edg, tick)
        for r in range(ser.world):
            ctx = f"{name}/{world} rowmajor={rowmajor} step {step} rank {r}"
            assert_messages_equal(ma[r], mb[r], ctx)
            (ra, oa), (rb, ob) = ser.sims[r].download(), edg.sims[r].download()
            assert np.array_equal(oa, ob), f"{ctx}: owned masks differ"
            assert np.array_equal(ra[oa].view(np.uint8), rb[ob].view(np.uint8)), f"{ctx}: owned records differ"
            assert ser.sims[r].counters() == edg.sims[r].counters(), ctx
        if rebalanced and step == 3:
            for slabs in (ser, edg):
                new = list(slabs.bounds)
                new[1] += 1
                for r, sim in enumerate(slabs.sims):
                    sim.set_window(new[r], new[r + 1])
                slabs.bounds = new
    for slabs in (ser, edg):
        for s in slabs.sims:
            c = s.counters()
            assert c["far_halo"] == 0 and c["overflow"] == 0, c
        assert sum(s.download()[1].sum() for s in slabs.sims) + sum(s.counters()["lost"] for s in slabs.sims) == p.shape[0]
        close(slabs)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,world", SCENES)
def test_every_mode_matches_the_oracle(fs, orc, name, world, mode):
    slabs, st, tick, p = make_slabs(fs, name, world, mode)
    want = oracle_states(name, world)
    tol = S.tolerances(name)
    for step in range(1, S.STEPS + 1):
        slabs.step(tick)
        if step in S.COMPARED:
            slabs.assert_clean()
            own = slabs.owned()
            assert own.shape[0] == p.shape[0]
            with np.errstate(invalid="ignore"):
                compare_with_oracle(own, want[step - 1], st.smoothing_radius, **tol)
    slabs.assert_clean()
    own = slabs.owned()
    assert own.shape[0] == p.shape[0]
    for f in ("position", "predicted_position", "velocity", "density"):
        assert np.isfinite(own[f]).all(), f
    close(slabs)


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", [2, 3])
def test_nothing_disappears_silently(fs, orc, world, mode):
    """Particles beyond the four walls, two NaN velocities in rank 0 and a speed ten times the clamp: after each of 4 steps every
    particle is owned by some rank or counted in `lost`, and an owned record is finite wherever the oracle's record of the same
    particle is.  What the code does with the NaN velocities today is the reference's outcome: the prediction is
    NaN, which is keyed to column 1 — rank 0 owns it out to the wall, so the particle stays owned (lost == 0), its velocity is
    reset to zero and it stays where it was."""
    name = "walls_and_bad_values"
    slabs, st, tick, p = make_slabs(fs, name, world, mode)
    want = oracle_states(name, world)
    n = p.shape[0]
    for step in range(1, ORACLE_STEPS + 1):
        slabs.step(tick)
        counters = [s.counters() for s in slabs.sims]
        own = slabs.owned()
        lost = sum(c["lost"] for c in counters)
        print(f"{mode}/{world} step {step}: owned {own.shape[0]} lost {lost}", counters)
        assert all(c["overflow"] == 0 for c in counters)
        assert own.shape[0] + lost == n
        assert lost == 0
        w = match_to_oracle(own, want[step - 1])
        for f in ("position", "predicted_position", "velocity", "density"):
            fin = np.isfinite(w[f])
            assert np.isfinite(own[f][fin]).all(), f"step {step}: {f} not finite where the oracle's is"
            assert not np.isfinite(own[f][~fin]).any(), f"step {step}: {f} finite where the oracle's is not"
    close(slabs)

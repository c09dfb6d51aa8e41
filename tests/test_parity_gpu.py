"""GPU parity tests: the HIP engine, called through the C ABI, against the CPU oracle on
identical inputs.  Bar: integer artefacts (cell keys, sort permutation, start_indices incl.
stale entries) bit-exact; floats bit-exact where asserted so, otherwise within
rtol 1e-5 / atol 1e-4*h — the engine is built without FMA contraction, with
IEEE divide/sqrt, so in practice every test here asserts bit equality."""
import os

import numpy as np
import pytest

from tests import parity_states as PS
from tests.bitcmp import assert_records_equal as assert_particles_equal      # the name its importers know
from tests.dense_scene import dense_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")


def make_pair(fs, orc, n, size=None, off=None, seed=None, vel=1.0, jitter=0.025, quirks=True, **tick_over):
    st, off, tick = PS.pair_settings(fs, n, size, off, **tick_over)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=quirks)
    ref = orc.OracleSim(st, off, ref_quirks=quirks)
    if seed is not None:
        p = PS.jitter(ref.particles(), seed, vel, jitter)
        ref.set_particles(p)
        sim.upload_particles(p)
    return sim, ref, st, tick


def run_and_compare(sim, ref, tick, steps, ctx):
    for s in range(steps):
        sim.tick(tick)
        ref.step(tick)
        sim.sync()
        assert_particles_equal(sim.download_particles(), ref.particles(), f"{ctx} step {s}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices()), f"{ctx} step {s}: start_indices"
    assert sim.tick_count == ref.tick_count == steps


def test_initial_state_is_reference_lattice(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096)
    assert_particles_equal(sim.download_particles(), ref.particles(), "lattice")
    assert not sim.download_start_indices().any()
    assert sim.grid_dims == ref.grid_dims == (66, 42)


def test_dam_break_4096_steps(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096)
    run_and_compare(sim, ref, tick, 12, "dam4096")


def test_golden_dam_break_4096(fs):
    z = np.load(os.path.join(GOLD, "dam_break_4096.npz"))
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    for s in range(int(z["steps"])):
        sim.tick(tick)
        assert_particles_equal(sim.download_particles(), z[f"particles_{s}"], f"golden step {s}")
        assert np.array_equal(sim.download_start_indices(), z[f"start_indices_{s}"])


def test_golden_jitter_mouse_field(fs):
    z = np.load(os.path.join(GOLD, "jitter_mouse_field_3000.npz"))
    n = int(z["n"])
    st, off, tick = fs.dam_break_2d(n)
    tick.mouse_state = 1
    tick.mouse_pos = fs.Vec2(-3.0, 2.0)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    sim.upload_particles(z["initial"])
    field = np.zeros((st.texture_size.y, st.texture_size.x, 2), dtype=np.float32)
    y0, y1, x0, x1 = z["field_box"]
    field[y0:y1, x0:x1] = z["field_value"]
    sim.upload_force_field(field)
    for s in range(int(z["steps"])):
        sim.tick(tick)
        assert_particles_equal(sim.download_particles(), z[f"particles_{s}"], f"golden-jitter step {s}")
        assert np.array_equal(sim.download_start_indices(), z[f"start_indices_{s}"])


@pytest.mark.parametrize("n", PS.RAGGED_DAM_N)
def test_ragged_counts(fs, orc, n):
    sim, ref, st, tick = make_pair(fs, orc, n, size=PS.RAGGED_BOX, seed=n)
    run_and_compare(sim, ref, tick, 4, f"ragged{n}")


def test_default_scene_100k(fs, orc):
    # the reference's own operating point: 100 000 particles, 53x53 (src/main.rs:48-54), gravity 0
    sim, ref, st, tick = make_pair(fs, orc, 100_000, size=(53.0, 53.0), seed=5, gravity=(0.0, 0.0))
    run_and_compare(sim, ref, tick, 3, "default100k")


def test_dam_break_1m(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 1 << 20, seed=21)
    run_and_compare(sim, ref, tick, 2, "dam1M")


def test_long_run_exercises_stale_quirk(fs, orc):
    # SURVEY A.6a fires from step ~130 on in this scene; compare every 10th step bit-exactly
    sim, ref, st, tick = make_pair(fs, orc, 4096)
    hits = 0
    for s in range(260):
        sim.tick(tick)
        ref.step(tick)
        if s % 10 == 9 or s > 250:
            assert_particles_equal(sim.download_particles(), ref.particles(), f"long step {s}")
            si = ref.start_indices()
            assert np.array_equal(sim.download_start_indices(), si)
            hits += int(si[ref.particles()["grid"][0]] != 0)
    assert hits > 0, "the stale-min-cell quirk never fired; the test lost its point"


def test_quirks_off_clean_cell_starts(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096, quirks=False)
    for s in range(160):
        sim.tick(tick)
        ref.step(tick)
    assert_particles_equal(sim.download_particles(), ref.particles(), "noquirk")
    assert np.array_equal(sim.download_start_indices(), ref.start_indices())


def test_poisoned_stale_start(fs, orc):
    """Force the quirk: give the minimum cell a non-zero stale start on both sides."""
    sim, ref, st, tick = make_pair(fs, orc, 4096, seed=9)
    sim.tick(tick); ref.step(tick)
    cmin = ref.particles()["grid"][0]
    si = ref.start_indices()
    for v in (1, 2, 1000):
        si[cmin] = v
        ref.start_indices_view()[:] = si
        sim.upload_start_indices(si)
        sim.tick(tick); ref.step(tick)
        assert_particles_equal(sim.download_particles(), ref.particles(), f"poison {v}")
        si = ref.start_indices()
        assert np.array_equal(sim.download_start_indices(), si)
        cmin = ref.particles()["grid"][0]


def test_mouse_and_force_field(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096, **PS.MOUSE_FIELD)
    field = PS.mouse_field()
    sim.upload_force_field(field)
    ref.texture_view()[:] = field
    run_and_compare(sim, ref, tick, 5, "mouse+field")


def test_coincident_particles_prng_path(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096, **PS.COINCIDENT)
    p = PS.coincident_state(ref.particles())
    ref.set_particles(p); sim.upload_particles(p)
    run_and_compare(sim, ref, tick, 3, "coincident")


def test_nan_reset_speed_clamp_and_walls(fs, orc):
    sim, ref, st, tick = make_pair(fs, orc, 4096, **PS.NAN_CLAMP)
    p = PS.nan_clamp_state(ref.particles())
    ref.set_particles(p); sim.upload_particles(p)
    run_and_compare(sim, ref, tick, 4, "nan/clamp")


@pytest.mark.parametrize("math_mode", ["ieee", "tolerance"])
def test_partial_upload_after_steps_keeps_the_rest(fs, math_mode):
    """A step no longer writes separate copies of the keys / densities (they live in the sorted pairs and in the force
    pass's {rho, 1/rho} array); an upload of the first k records must still leave the other records' keys and
    densities as the last step produced them (ResizableBuffer::write semantics, src/buffer.rs:61-87)."""
    n, k = 8192, 1000
    st, off, tick = fs.dam_break_2d(n)
    mm = fs.FS_MATH_IEEE if math_mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=mm)
    for _ in range(5):
        sim.tick(tick)
    before = sim.download_particles()
    assert before["density"].min() > 0 and np.all(before["grid"][:-1] <= before["grid"][1:])
    rng = np.random.default_rng(3)
    head = before[:k].copy()
    head["density"] = rng.uniform(1, 2, size=k).astype(np.float32)
    head["grid"] = rng.integers(0, 2**32, size=k, dtype=np.uint32)
    sim.upload_particles(head)
    after = sim.download_particles()
    assert np.array_equal(after[:k].view(np.uint8), head.view(np.uint8))
    assert np.array_equal(after[k:].view(np.uint8), before[k:].view(np.uint8))
    sim.tick(tick)                                   # and the engine carries on from the mixed state
    assert np.isfinite(sim.download_particles()["position"]).all()


def test_upload_download_roundtrip(fs):
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    rng = np.random.default_rng(0)
    p = np.zeros(4096, dtype=fs.PARTICLE_DTYPE)
    for f in FLOAT_FIELDS:
        p[f] = rng.standard_normal(p[f].shape).astype(np.float32)
    p["grid"] = rng.integers(0, 2**32, size=4096, dtype=np.uint32)
    sim.upload_particles(p)
    assert np.array_equal(sim.download_particles().view(np.uint8), p.view(np.uint8))
    u = sim.uniform()
    assert u.particle_count == 4096 and (u.grid_w, u.grid_h) == (66, 42)


def test_resizable_buffer_semantics(fs):
    # src/buffer.rs:46-87: grow-only resize keeping contents; oversize writes trimmed
    b = fs.ResizableBuffer("t", np.float32, 8)
    b.write(0, np.arange(8, dtype=np.float32))
    assert not b.resize(4) and len(b) == 8
    assert b.resize(16) and len(b) == 16
    got = b.read()
    assert np.array_equal(got[:8], np.arange(8)) and not got[8:].any()
    b.write(12, np.ones(100, dtype=np.float32))      # trimmed to the buffer
    assert np.array_equal(b.read()[12:], np.ones(4))
    b.close()


def test_sort_permutation_16m_matches_network(fs, orc):
    """Full-size (configs[2]) sort: the permutation of the first step equals the reference
    network run on the same keys by the oracle."""
    n = 1 << 24
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    p0 = sim.download_particles()
    sim.tick(tick)
    p1 = sim.download_particles()
    # keys of the unsorted particles: recompute from the lattice through a zero-velocity predict
    assert np.all(p1["grid"][:-1] <= p1["grid"][1:])
    # identify sources by their (unique) initial positions
    gw, gh = sim.grid_dims
    bx, by = np.float32(st.size.x) * np.float32(0.5), np.float32(st.size.y) * np.float32(0.5)
    cx = np.floor((p0["position"][:, 0] + bx) / np.float32(0.2)).astype(np.uint32) + 1
    cy = np.floor((p0["position"][:, 1] + by) / np.float32(0.2)).astype(np.uint32) + 1
    keys = cy * np.uint32(gw) + cx
    sorted_keys, perm = orc.bitonic_keys(keys)
    assert np.array_equal(sorted_keys, p1["grid"])
    assert np.array_equal(p0["position"][perm].view(np.uint32), p1["predicted_position"].view(np.uint32))


def test_16m_full_state_matches_oracle(fs, orc):
    """BASELINE configs[2] at its full size: two steps of the 16M dam break on the GPU, EVERY field of EVERY particle
    and the whole start_indices table bit for bit against the oracle (run on all host cores; its results do not
    depend on the thread count) — compute.wgsl:45-157, sort.wgsl:27-51 at the headline size, not a property check."""
    import bench
    n = 1 << 24
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    orc.set_threads(min(bench.usable_cores(), orc.max_threads()))
    try:
        ref = orc.OracleSim(st, off)
        for step in (1, 2):
            sim.tick(tick)
            ref.step(tick)
            got, want = sim.download_particles(), ref.particles_view()
            assert_particles_equal(got, want, f"16M step {step}")
            assert np.array_equal(sim.download_start_indices(), ref.start_indices_view()), f"16M step {step}: start_indices"
            del got
    finally:
        orc.set_threads(1)
    sim.close()


def test_shuffled_upload_on_a_large_grid_takes_the_wide_tile_path(fs, orc):
    """the packed first sort kernel (k_bitonic_local32) leaves a 4096-element tile whose keys span >= 2^20 - 1 cells to
    the 64-bit kernel that follows (FS_TILE_WIDE).  That needs a grid of more than a million cells AND an unordered state — an
    fs_upload_particles of a permuted state at 4M particles (2050 x 1282 = 2.6M cells).  Every tile is then wide; the step must
    still be bit for bit the oracle's (keys, every field, start_indices), also in the step after."""
    import bench
    n = 1 << 22
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    orc.set_threads(min(bench.usable_cores(), orc.max_threads()))
    try:
        ref = orc.OracleSim(st, off)
        for _ in range(2):
            sim.tick(tick); ref.step(tick)
        assert sim.sort_plan()["wide_tiles"] == 0                # a state in cell order: no tile spans that much
        p = sim.download_particles()
        p = p[np.random.default_rng(5).permutation(n)]
        sim.upload_particles(p); ref.set_particles(p)
        for step in (1, 2):
            sim.tick(tick); ref.step(tick)
            got, want = sim.download_particles(), ref.particles_view()
            assert_particles_equal(got, want, f"step {step} after the shuffled upload")
            assert np.array_equal(sim.download_start_indices(), ref.start_indices_view())
            if step == 1:
                assert sim.sort_plan()["wide_tiles"] >= n // 4096 // 2, sim.sort_plan()
    finally:
        orc.set_threads(1)
    sim.close()


def test_counting_sort_orders_a_cell_of_5000_particles_like_the_stable_sort(fs, orc):
    """The counting sort's order inside a cell is the source order — the oracle's std::stable_sort — whatever order the histogram
    atomics were served in, for a cell of ANY size: up to CS_RANK_MAX = 2048 particles by the serial rank loop, beyond by sorting
    the cell's segment in place (kernels_csort.hip cs_sort_segment).  5000 particles in one cell (tools/fuzz_parity.py case 15
    found that such cells were left in arrival order), bit-exact over two steps.
    The bound itself, the network's other sizes and the segment's placement: tests/test_csort_gpu.py."""
    n = 16384
    st = fs.SimulationSettings(n, 0.1, 0.2, (40.0, 30.0))
    tick = fs.default_tick_settings(gravity=(0.0, 9.81))
    sim = fs.FluidSimulation(st, device=0, sort_mode=fs.FS_SORT_COUNTING)
    ref = orc.OracleSim(st)
    rng = np.random.default_rng(23)
    p = ref.particles()
    idx = rng.choice(n, 5000, replace=False)
    p["position"][idx] = rng.uniform(0.01, 0.19, size=(5000, 2)).astype(np.float32) + np.float32([4.0, -3.0])   # inside one cell
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-0.05, 0.05, size=(n, 2)).astype(np.float32)
    ref.set_particles(p); sim.upload_particles(p)
    for s in range(2):
        sim.tick(tick)
        ref.step(tick, stable_sort=True)
        want = ref.particles()
        if s == 0:
            assert np.unique(want["grid"], return_counts=True)[1].max() >= 4000
        assert_particles_equal(sim.download_particles(), want, f"big cell step {s}")
    sim.close(); ref.close()


def test_counting_sort_survives_a_cell_with_30k_particles(fs):
    """k_cs_fixreorder ranks a slot inside its cell segment with a serial loop — O(m^2) for a cell of m particles, on top
    of the m^2 pairs the force pass must visit anyway (which is why this test stops at 30 000 coincident particles, ~1e9 pairs).
    Segments above CS_RANK_MAX are sorted in place by one workgroup (O(m log^2 m)).  The step must finish with a valid arrangement (keys sorted, nothing lost,
    finite predicted positions)."""
    import time
    n = 1 << 18
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=fs.FS_SORT_COUNTING, ref_quirks=False)
    p = sim.download_particles()
    p["position"][:30_000] = p["position"][0]
    p["predicted_position"][:30_000] = p["position"][0]
    sim.upload_particles(p)
    t0 = time.perf_counter()
    sim.tick(tick)
    q = sim.download_particles()
    assert time.perf_counter() - t0 < 30.0
    assert np.all(q["grid"][:-1] <= q["grid"][1:])
    cell, cnt = np.unique(q["grid"], return_counts=True)
    assert cnt.max() >= 30_000 and q.shape[0] == n
    assert np.isfinite(q["predicted_position"]).all()
    sim.close()


def test_16m_properties(fs):
    """Size-independent properties at the headline size: sortedness, start_indices
    consistency, permutation (multiset of lattice x-coordinates preserved), finite state."""
    n = 1 << 24
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    for _ in range(3):
        sim.tick(tick)
    p = sim.download_particles()
    si = sim.download_start_indices()
    assert np.all(p["grid"][:-1] <= p["grid"][1:])
    occupied, first = np.unique(p["grid"], return_index=True)
    assert np.array_equal(si[occupied[1:]], first[1:].astype(np.uint32))
    assert np.isfinite(p["position"]).all() and np.isfinite(p["velocity"]).all()
    interior = np.median(p["density"])
    assert interior == pytest.approx(101.46, rel=1e-3)
    assert np.abs(p["position"][:, 0]).max() <= st.size.x / 2 and np.abs(p["position"][:, 1]).max() <= st.size.y / 2


@pytest.mark.parametrize("n,seed,steps", [(4096, None, 20), (5000, 3, 5), (100_000, 8, 3), (1 << 20, None, 2)])
def test_counting_sort_mode_matches_stable_oracle(fs, orc, n, seed, steps):
    """FS_SORT_COUNTING is a stable cell sort: bit-exact against the oracle run
    with std::stable_sort in place of the network (keys, start_indices and floats)."""
    if seed is None:
        st, off, tick = fs.dam_break_2d(n)
    else:
        side = float(np.ceil(np.sqrt(n))) * 0.1
        st = fs.SimulationSettings(n, 0.1, 0.2, (2.0 * side, 1.5 * side))      # roomy box: no wall pile-up
        off, tick = (0.0, 0.0), fs.default_tick_settings(gravity=(0.0, 9.81))
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=fs.FS_SORT_COUNTING)
    ref = orc.OracleSim(st, off)
    if seed is not None:
        rng = np.random.default_rng(seed)
        p = ref.particles()
        p["position"] += rng.uniform(-0.025, 0.025, size=(n, 2)).astype(np.float32)
        p["predicted_position"] = p["position"]
        p["velocity"] = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        ref.set_particles(p); sim.upload_particles(p)
    for s in range(steps):
        sim.tick(tick)
        ref.step(tick, stable_sort=True)
        assert_particles_equal(sim.download_particles(), ref.particles(), f"counting n={n} step {s}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices())


def test_counting_vs_bitonic_within_tolerance(fs):
    """The two sort modes differ only in the order inside a cell -> summation order -> ULPs."""
    from tests.slab_oracle import match_and_compare
    st, off, tick = fs.dam_break_2d(16384)
    a = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=fs.FS_SORT_BITONIC)
    b = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=fs.FS_SORT_COUNTING)
    for _ in range(4):
        a.tick(tick); b.tick(tick)
    # step 4: lattice columns that sit exactly on a cell boundary may flip with 1-ulp x differences (slab_oracle.py)
    match_and_compare(b.download_particles(), a.download_particles(), st.smoothing_radius, max_key_flips=0.02)


@pytest.mark.parametrize("sort_mode", ["bitonic", "counting"])
def test_dense_cluster_exercises_overflow_paths(fs, orc, sort_mode):
    """3000 of 8192 particles squeezed into ~3x3 cells: hundreds of in-radius neighbours per particle
    (neighbour-list flushes), candidate ranges longer than the LDS tiles (global fallback path), plus
    empty space (long cell-table gaps).  Still bit-exact against the oracle."""
    n = 8192
    st = fs.SimulationSettings(n, 0.1, 0.2, (40.0, 30.0))
    tick = fs.default_tick_settings(gravity=(0.0, 9.81))
    mode = fs.FS_SORT_BITONIC if sort_mode == "bitonic" else fs.FS_SORT_COUNTING
    sim = fs.FluidSimulation(st, device=0, sort_mode=mode)
    ref = orc.OracleSim(st)
    rng = np.random.default_rng(17)
    p = ref.particles()
    idx = rng.choice(n, 3000, replace=False)
    p["position"][idx] = rng.uniform(-0.3, 0.3, size=(3000, 2)).astype(np.float32) + np.float32([5.0, -4.0])
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-0.5, 0.5, size=(n, 2)).astype(np.float32)
    ref.set_particles(p); sim.upload_particles(p)
    for s in range(3):
        sim.tick(tick)
        ref.step(tick, stable_sort=(sort_mode == "counting"))
        got, want = sim.download_particles(), ref.particles()
        assert_particles_equal(got, want, f"cluster/{sort_mode} step {s}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices())
    cells, cnt = np.unique(want["grid"], return_counts=True)
    assert cnt.max() > 150          # the scene really has hot cells


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["ieee", "ulp"])
def test_force_quad_kernel_changes_no_bit(fs, orc, monkeypatch, math):
    """k_force_quad (a short list of deferred waves: four lanes per particle, the four terms of a round added in lane order by quad
    broadcasts) must leave every bit where the lane-per-particle general kernel leaves it — dense clusters, rows of hundreds of
    candidates, coincident pairs (which it hands to the general kernel), both math modes that use it; strict math also against
    the oracle.  FS_FORCE_QUAD_ALWAYS=1 puts it into every step (otherwise the host picks it from the list length a few steps ago)."""
    st, tick, p = dense_scene(fs)
    mm = fs.FS_MATH_IEEE if math == "ieee" else fs.FS_MATH_WGSL_ULP
    monkeypatch.setenv("FS_FORCE_QUAD_ALWAYS", "1")
    quad = fs.FluidSimulation(st, device=0, math_mode=mm)
    monkeypatch.delenv("FS_FORCE_QUAD_ALWAYS"); monkeypatch.setenv("FS_FORCE_QUAD_MAX", "0")
    plain = fs.FluidSimulation(st, device=0, math_mode=mm)
    monkeypatch.delenv("FS_FORCE_QUAD_MAX")
    ref = orc.OracleSim(st) if math == "ieee" else None
    quad.upload_particles(p); plain.upload_particles(p)
    if ref: ref.set_particles(p)
    for s in range(6):
        quad.tick(tick); plain.tick(tick)
        a, b = quad.download_particles(), plain.download_particles()
        assert a.tobytes() == b.tobytes(), f"{math} step {s}: the quad kernel changed the state"
        if ref:
            ref.step(tick)
            assert_particles_equal(a, ref.particles(), f"quad/{math} step {s}")
    quad.close(); plain.close()
    if ref: ref.close()


def test_wgsl_ulp_math_mode_within_tolerance(fs, orc):
    """FS_MATH_WGSL_ULP (native rcp/sqrt in the force pass) is not bit-exact; it must stay within the
    stated tolerance of the IEEE oracle: one step from identical state — keys and density exact (density
    has no division), velocity rtol 1e-5 / position atol 1e-4*h; a few steps — matched."""
    from tests.slab_oracle import match_and_compare
    st, off, tick = fs.dam_break_2d(16384)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_WGSL_ULP)
    ref = orc.OracleSim(st, off)
    rng = np.random.default_rng(4)
    p = ref.particles()
    p["position"] += rng.uniform(-0.02, 0.02, size=p["position"].shape).astype(np.float32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-1, 1, size=p["velocity"].shape).astype(np.float32)
    ref.set_particles(p); sim.upload_particles(p)
    sim.tick(tick); ref.step(tick)
    got, want = sim.download_particles(), ref.particles()
    assert np.array_equal(got["grid"], want["grid"])
    assert np.array_equal(got["density"].view(np.uint32), want["density"].view(np.uint32))
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32))
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * 0.2)
    assert not np.array_equal(got["velocity"].view(np.uint32), want["velocity"].view(np.uint32))   # really a different mode
    for _ in range(4):
        sim.tick(tick); ref.step(tick)
    match_and_compare(sim.download_particles(), ref.particles(), st.smoothing_radius, max_key_flips=0.02)   # step 5


def test_64m_properties(fs):
    """Largest BASELINE size (configs[4], here on one GPU): S = 26 sort stages, 42 M cells — no 32-bit
    overflow anywhere: sortedness, start_indices consistency, permutation, analytic interior density."""
    n = 1 << 26
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    assert sim.grid_dims == (8194, 5122)
    for _ in range(2):
        sim.tick(tick)
    p = sim.download_particles()
    assert np.all(p["grid"][:-1] <= p["grid"][1:])
    si = sim.download_start_indices()
    occ, first = np.unique(p["grid"], return_index=True)
    assert np.array_equal(si[occ[1:]], first[1:].astype(np.uint32))
    assert np.isfinite(p["position"]).all() and np.isfinite(p["velocity"]).all()
    assert np.unique(p["position"].view(np.uint64)).shape[0] == n          # nobody lost or duplicated
    assert np.median(p["density"]) == pytest.approx(101.46, rel=1e-3)


@pytest.mark.parametrize("case", range(PS.RANDOM_CASES))
def test_random_configurations(fs, orc, case):
    """Seeded random settings (smoothing radius, spacing, domain aspect, dt, mass, stiffness, rest density,
    damping, viscosity, gravity sign, texture size, mouse) and particle counts: bit-exact in both sort modes."""
    st, off, tick, runs = PS.random_configuration(fs, orc, case)
    for sort, p, field in runs:
        mode, stable = (fs.FS_SORT_BITONIC, False) if sort == "bitonic" else (fs.FS_SORT_COUNTING, True)
        sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=mode)
        ref = orc.OracleSim(st, off)
        ref.set_particles(p); sim.upload_particles(p)
        if field is not None:
            sim.upload_force_field(field); ref.texture_view()[:] = field
        for s in range(4):
            sim.tick(tick); ref.step(tick, stable_sort=stable)
            assert_particles_equal(sim.download_particles(), ref.particles(), f"random case {case} mode {mode} step {s}")
            assert np.array_equal(sim.download_start_indices(), ref.start_indices())
        sim.close(); ref.close()


# ---- operands at and beyond the guards of the shared-denominator quotients ----------
# The force pass forms a/b from one reciprocal only inside proven ranges; everything else must take the
# true-division body.  These scenes put numerators and denominators on both sides of every guard.
@pytest.mark.parametrize("case", PS.GUARD_CASES)
def test_force_quotient_guards(fs, orc, case):
    sim, ref, st, tick = make_pair(fs, orc, 4096, seed=PS.GUARD_SEED, **PS.guard_overrides(case))
    p = PS.guard_state(orc, st, ref.particles(), case)
    n = p.shape[0]
    ref.set_particles(p); sim.upload_particles(p)
    with np.errstate(all="ignore"):
        run_and_compare(sim, ref, tick, 3, f"guards/{case}")
    assert n == 4096


def test_true_division_path_without_shared_reciprocals(fs):
    """FS_NO_SHAREDIV=1 keeps every `/` a true IEEE division (the pre-proof body).  It is read once per
    process, so the check runs in a child: same scene, bit-compared with the oracle there."""
    import subprocess, sys
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gpu_fluid_simulation_amd as fs
from oracle import oracle as orc
st, off, tick = fs.dam_break_2d(4096)
sim = fs.FluidSimulation(st, device=0, initial_offset=off)
assert fs.load_library().fs_constdiv_status(sim._h) & 12 == 0, "shared path should be off"
ref = orc.OracleSim(st, off)
for s in range(5):
    sim.tick(tick); ref.step(tick)
a, b = sim.download_particles(), ref.particles()
for f in ("position", "predicted_position", "velocity", "density"):
    assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f
print("ok")
'''
    env = dict(os.environ, FS_NO_SHAREDIV="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------
# FS_MATH_TOLERANCE: re-associated density / force terms (FMA, one rsqrt per pair).  north_star's float contract:
# positions / velocities within a stated tolerance, cell indices bit-exact.  Stated tolerance,
# one step from an identical state: density rtol 1e-5; velocity rtol 1e-5 + atol 2e-5; position atol 1e-4 * h.
def _tolerance_one_step(fs, orc, n, seed, steps_before=0):
    st, off, tick = fs.dam_break_2d(n)
    ref = orc.OracleSim(st, off)
    rng = np.random.default_rng(seed)
    p = ref.particles()
    p["position"] += rng.uniform(-0.03, 0.03, size=p["position"].shape).astype(np.float32)
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-2, 2, size=p["velocity"].shape).astype(np.float32)
    ref.set_particles(p)
    for _ in range(steps_before):                    # let the oracle disorder the scene first (strict arithmetic)
        ref.step(tick)
    start = ref.particles()
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_TOLERANCE)
    sim.upload_particles(start)
    sim.upload_start_indices(ref.start_indices())
    for _ in range(steps_before):                    # same tick counter (PRNG seed) as the oracle
        pass
    ref.step(tick)
    # the engine's tick counter only seeds the coincident-particle PRNG; align it by stepping a scratch handle is not
    # needed here: no coincident particles in these scenes
    sim.tick(tick)
    got, want = sim.download_particles(), ref.particles()
    h = st.smoothing_radius
    assert np.array_equal(got["grid"], want["grid"]), "cell keys must stay bit-exact"
    assert np.array_equal(sim.download_start_indices(), ref.start_indices()), "start_indices must stay bit-exact"
    assert np.array_equal(got["predicted_position"].view(np.uint32), want["predicted_position"].view(np.uint32))
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * h)
    assert not np.array_equal(got["velocity"].view(np.uint32), want["velocity"].view(np.uint32))   # really another mode
    sim.close(); ref.close()


@pytest.mark.parametrize("n,seed,before", [(4096, 1, 0), (4096, 2, 40), (102400, 3, 3), (1 << 20, 4, 1)])
def test_tolerance_mode_one_step_within_stated_tolerance(fs, orc, n, seed, before):
    _tolerance_one_step(fs, orc, n, seed, steps_before=before)


def test_tolerance_mode_several_steps_and_coincident_particles(fs, orc):
    """Five steps (matched comparison: ULP-level differences move particles across cell boundaries and change the
    within-cell order) and a scene with coincident particles (the PRNG direction, r == 0 viscosity constant)."""
    from tests.slab_oracle import match_and_compare
    st, off, tick = fs.dam_break_2d(16384)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=fs.FS_MATH_TOLERANCE)
    ref = orc.OracleSim(st, off)
    rng = np.random.default_rng(9)
    p = ref.particles()
    p["position"] += rng.uniform(-0.02, 0.02, size=p["position"].shape).astype(np.float32)
    p["position"][101] = p["position"][100]
    p["position"][5001] = p["position"][5000]; p["position"][5002] = p["position"][5000]
    p["predicted_position"] = p["position"]
    p["velocity"] = rng.uniform(-1, 1, size=p["velocity"].shape).astype(np.float32)
    ref.set_particles(p); sim.upload_particles(p)
    sim.tick(tick); ref.step(tick)
    got, want = sim.download_particles(), ref.particles()
    assert np.array_equal(got["grid"], want["grid"])
    np.testing.assert_allclose(got["density"], want["density"], rtol=1e-5)
    np.testing.assert_allclose(got["velocity"], want["velocity"], rtol=2e-5, atol=5e-5)     # incl. the PRNG-direction pairs
    np.testing.assert_allclose(got["position"], want["position"], rtol=0, atol=1e-4 * 0.2)
    for _ in range(4):
        sim.tick(tick); ref.step(tick)
    match_and_compare(sim.download_particles(), ref.particles(), st.smoothing_radius, max_key_flips=0.02)


def test_tolerance_mode_mouse_field_and_guards(fs, orc):
    """Mouse impulse, obstacle push-out, NaN reset and the speed clamp behave as in the strict mode."""
    n = 4096
    st = fs.SimulationSettings(n, 0.1, 0.2, (12.8, 8.0), (64, 48))
    tick = fs.default_tick_settings(gravity=(0.0, 9.81), mouse_state=1, mouse_pos=(0.5, 0.5), mouse_force_radius=2.0)
    sim = fs.FluidSimulation(st, device=0, math_mode=fs.FS_MATH_TOLERANCE)
    ref = orc.OracleSim(st)
    rng = np.random.default_rng(12)
    field = rng.uniform(-0.01, 0.01, size=(48, 64, 2)).astype(np.float32)
    field[:24] = 0
    sim.upload_force_field(field); ref.texture_view()[:] = field
    p = ref.particles()
    p["velocity"] = rng.uniform(-1, 1, size=p["velocity"].shape).astype(np.float32)
    p["velocity"][7] = (np.nan, 0.0)
    p["velocity"][9] = (4000.0, 3000.0)
    ref.set_particles(p); sim.upload_particles(p)
    sim.tick(tick); ref.step(tick)
    got, want = sim.download_particles(), ref.particles()
    assert np.array_equal(got["grid"], want["grid"])
    ok = np.isfinite(want["velocity"]).all(axis=1)
    assert np.isfinite(got["velocity"]).all()
    np.testing.assert_allclose(got["velocity"][ok], want["velocity"][ok], rtol=2e-5, atol=1e-4)
    np.testing.assert_allclose(got["position"][ok], want["position"][ok], rtol=0, atol=1e-4 * 0.2 + 1e-5)


@pytest.mark.parametrize("cells_side", [127, 128, 129, 255, 640])
def test_counting_sort_scan_tile_boundaries(fs, orc, cells_side):
    """k_scan_lookback scans 16 384 cells per workgroup: grids whose cell count sits just below / on / above tile
    multiples (127^2 < 16 384 = 128^2 < 129^2, ...) must give the same cell table as the oracle's stable sort."""
    h = 0.2
    size = (cells_side - 2) * h - 0.01            # grid_w = grid_h = ceil(size / h) + 2 = cells_side
    n = 20000
    st = fs.SimulationSettings(n, 0.05, h, (size, size))
    tick = fs.default_tick_settings(gravity=(0.0, 9.81))
    sim = fs.FluidSimulation(st, device=0, sort_mode=fs.FS_SORT_COUNTING)
    assert sim.grid_dims == (cells_side, cells_side)
    ref = orc.OracleSim(st, (0.0, 0.0))
    rng = np.random.default_rng(cells_side)
    p = ref.particles()
    p["position"] = rng.uniform(-size / 2, size / 2, size=(n, 2)).astype(np.float32)
    p["predicted_position"] = p["position"]
    ref.set_particles(p); sim.upload_particles(p)
    for s in range(2):
        sim.tick(tick); ref.step(tick, stable_sort=True)
        got, want = sim.download_particles(), ref.particles()
        assert_particles_equal(got, want, f"step {s}")
        assert np.array_equal(sim.download_start_indices(), ref.start_indices()), f"step {s}: start_indices"
    sim.close()

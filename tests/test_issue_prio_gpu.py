"""The load phase of the density, force and sort tile kernels, where their waves run at a raised priority (csrc/fs_device.h
wave_prio_raise / wave_prio_lower; the density pass lowers inside csrc/fs_neighbours.h walk_rows), and the density pass's read of its "safe operand" word (density_block): three steps from a
fresh handle against the oracle, bit for bit — every field of every record (position, predicted position, velocity, density,
key) and start_indices — in both sort modes.  The stored reciprocal {rho, +-RN(1/rho)} is not downloadable; its value and its
sign (the safe bit) are seen through the force pass that reads it: a pair with an unsafe particle that took the
shared-reciprocal quotient would miss the oracle's bits (tests/parity_states.py guard_state).

Where it can go wrong                                                               test
dead lanes in the last wave / the last block (they shadow particle n - 1 and        test_ragged_last_wave
return without lowering): n = 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097
safe and unsafe particles next to each other inside one 64-lane word and across a   test_unsafe_operands_mixed_in_a_word
word boundary (asserted on the oracle's sorted state)
blocks whose rows do not fit the LDS tile: the unstaged paths lower the priority    test_unstaged_blocks"""
import numpy as np
import pytest

from tests import parity_states as PS
from tests import prologue_scenes as S
from tests.bitcmp import assert_records_equal, expect_invalid

pytestmark = pytest.mark.gpu
STEPS = 3
SORTS = ("bitonic", "counting")
LAST_WAVE_N = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097)
UNSAFE_SCENE = "tiny_velocities"          # two particles in three carry velocities of 1e-30 .. 1e-45: below 2^-53 and not zero
UNSTAGED_SCENES = ("force_unstaged", "both_unstaged")


def sort_mode(fs, sort):
    return fs.FS_SORT_BITONIC if sort == "bitonic" else fs.FS_SORT_COUNTING


def assert_step_equal(sim, ref, ctx):
    assert_records_equal(sim.download_particles(), ref.particles(), ctx)
    assert np.array_equal(sim.download_start_indices(), ref.start_indices()), f"{ctx}: start_indices"


def oracle_step(ref, tick, stable):
    """one oracle step pass by pass (as orc_step / orc_step_stable run it: tests/track_ref.py); returns the records as the sort
    left them — predicted positions and velocities in sorted order, before the force pass changes the velocities"""
    ref.begin_tick(tick)
    ref.predict()
    ref.spatial_lookup()
    if stable:
        ref.L.orc_sort_stable(ref.h)
    else:
        ref.sort()
    srt = ref.particles()
    ref.cell_starts()
    ref.density(1)
    ref.move()
    return srt


def kin_safe(pred, vel):
    """fs_device.h kin_safe on arrays: every component 0 or at least 2^-53 in magnitude, velocities at most 2^59"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        lo = lambda c: (c == 0) | (np.abs(c) >= f32(2.0 ** -53))
        return (lo(pred[:, 0]) & lo(pred[:, 1]) & lo(vel[:, 0]) & lo(vel[:, 1]) &
                (np.abs(vel[:, 0]) <= f32(2.0 ** 59)) & (np.abs(vel[:, 1]) <= f32(2.0 ** 59)))


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("n", LAST_WAVE_N)
def test_ragged_last_wave(fs, orc, n, sort):
    if n == 1:      # no handle and no oracle holds fewer than two particles (the reference panics): both must refuse, neither steps
        st, off, _ = PS.pair_settings(fs, n, size=PS.RAGGED_BOX)
        expect_invalid(fs, lambda: fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=sort_mode(fs, sort)))
        with pytest.raises(ValueError):
            orc.OracleSim(st, off)
        return
    st, off, tick, p = PS.jittered_dam_break(fs, orc, n, 100 + n, size=PS.RAGGED_BOX)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=sort_mode(fs, sort))
    ref = orc.OracleSim(st, off)
    sim.upload_particles(p); ref.set_particles(p)
    for s in range(STEPS):
        sim.tick(tick)
        ref.step(tick, stable_sort=sort == "counting")
        assert_step_equal(sim, ref, f"n {n} {sort} step {s}")
    sim.close(); ref.close()


@pytest.mark.parametrize("sort", SORTS)
def test_unsafe_operands_mixed_in_a_word(fs, orc, sort):
    st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.GUARD_SEED, **PS.guard_overrides(UNSAFE_SCENE))
    p = PS.guard_state(orc, st, p, UNSAFE_SCENE)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=sort_mode(fs, sort))
    ref = orc.OracleSim(st, off)
    sim.upload_particles(p); ref.set_particles(p)
    mixed_word = boundary = False
    for s in range(STEPS):
        sim.tick(tick)
        srt = oracle_step(ref, tick, sort == "counting")
        safe = kin_safe(srt["predicted_position"], srt["velocity"])
        words = safe.reshape(-1, 64)
        mixed_word |= bool(np.any(words.any(axis=1) & ~words.all(axis=1)))
        boundary |= bool(np.any(words[:-1, 63] != words[1:, 0]))
        assert_step_equal(sim, ref, f"{UNSAFE_SCENE} {sort} step {s}")
    assert mixed_word, "no 64-lane word holds both a safe and an unsafe particle"
    assert boundary, "no word boundary separates a safe from an unsafe particle"
    sim.close(); ref.close()


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", UNSTAGED_SCENES)
def test_unstaged_blocks(fs, orc, name, sort):
    """force_unstaged: block 0's longest row is 573 candidates (density stages it, the lean force kernel does not and defers);
    both_unstaged: 713 (neither stages)."""
    st, tick, p = S.staging_scene(name)
    sim = fs.FluidSimulation(st, device=0, sort_mode=sort_mode(fs, sort))
    ref = orc.OracleSim(st)
    sim.upload_particles(p); ref.set_particles(p)
    for s in range(STEPS):
        sim.tick(tick)
        ref.step(tick, stable_sort=sort == "counting")
        assert_step_equal(sim, ref, f"{name} {sort} step {s}")
    sim.close(); ref.close()

"""Fluid diagnostics on the GPU (include/fluidsim.h "fluid diagnostics" / "3D fluid diagnostics"; k_stats, k3_stats,
k_stats_fold).  Every comparison is integer and bit equality of the WHOLE record with tests/stats_ref.py, the numpy statement of
the header, run on what download_particles() and the tracking downloads return in the same state: counts at the kernel's edges,
the crafted records of tests/test_stats.py, the hard states after every step in every sort and math mode, every state a handle
can be in, that the calls only observe, the device form, the refusals, and two tie-ins with the step.  The cases' conditions (a
non-finite record, a dropped record, a dropped channel value) are asserted without a GPU in tests/test_stats.py."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import stats_cases as SC
from tests import stats_ref as R
from tests.layers import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
DIMS = [2, 3]
CHANNELS = {2: 4, 3: 2}            # channels of the tracked uploads (beside none): every channel row in 2D, two in 3D


def dtype_of(fs, dim):
    return fs.PARTICLE_DTYPE if dim == 2 else fs.PARTICLE3_DTYPE


def make(fs, dim, rec, channels=None, **kw):
    """a handle whose live records are `rec`, in upload order; no step.  A 3D handle is created with a cube count, so it starts
    with 8 particles and is brought to len(rec) by reserve + emit or by a removal."""
    n = rec.shape[0]
    if dim == 2:
        st = fs.SimulationSettings(n, 0.1, 0.2, (40.0, 30.0))
        sim = fs.FluidSimulation(st, device=0, **kw)
    else:
        sim = fs.FluidSimulation3D(fs.Settings3(8, 0.1, 0.2, fs.Vec3(8.0, 6.0, 4.0)), device=0, **kw)
        if n > 8:
            sim.reserve(n)
            sim.emit(rec[8:])
        elif n < 8:
            assert sim.remove(np.arange(8) >= n) == 8 - n
    assert sim.particle_count == n
    sim.upload_particles(rec)
    if channels is not None:
        sim.track(channels)
        for c, a in enumerate(SC.channel_values(n, channels)):
            sim.set_attribute(c, a)
    return sim


def reference(sim):
    ch = max(sim.track_channels, 0)
    return R.stats(sim.download_particles(), [sim.attribute(c) for c in range(ch)], tick=sim.tick_count)


def check(sim, ctx):
    """the engine's record against the reference on the downloads of the same state; returns the words"""
    got = R.words_of(sim.stats().raw)
    R.assert_same(got, reference(sim), ctx)
    return got


# ---- 1. counts at the kernel's edges, no step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", SC.COUNTS + SC.BIG_COUNTS)
def test_counts_at_the_kernels_edges(fs, dim, n):
    rec = SC.random_records(dtype_of(fs, dim), n)
    for channels in (None, CHANNELS[dim]):
        sim = make(fs, dim, rec, channels)
        got = check(sim, f"{dim}D n {n} channels {channels}")
        assert got["count"] == n and got["nonfinite"] == 0 and got["dropped"] == 0 and got["channels"] == (channels or 0)
        if channels:
            assert got["attr_dropped"][1] > 0 and got["attr_q"][0] != 0
        sim.close()


# ---- 2. the crafted records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_crafted_records(fs, dim):
    for name, craft in (("crafted", R.crafted), ("zeros", R.crafted_zeros), ("empty", R.crafted_empty)):
        rec, attrs, want = craft(dtype_of(fs, dim))
        sim = make(fs, dim, rec)
        if attrs:
            sim.track(len(attrs))
            for c, a in enumerate(attrs):
                sim.set_attribute(c, a)
        got = R.words_of(sim.stats().raw)
        R.assert_same(got, want, f"{dim}D {name}: the words by hand")
        check(sim, f"{dim}D {name}")
        sim.close()


# ---- 3. after steps --------------------------------------------------------------------------------------------------------------------
def math_modes(fs, dim):
    return [fs.FS_MATH_IEEE, fs.FS_MATH_WGSL_ULP, fs.FS_MATH_TOLERANCE] if dim == 2 else [fs.FS_MATH_IEEE, fs.FS_MATH_TOLERANCE]


@pytest.mark.parametrize("cid", SC.CASES_2D)
def test_after_steps_2d(fs, orc, cid):
    """both sort modes and all three math modes: the density in rho2 (strict, ulp), in rho (tolerance; every upload)"""
    from tests import hard_states2d as H2
    case = H2.case_by_id(fs, orc, cid)
    seen = []
    for sort in (fs.FS_SORT_BITONIC, fs.FS_SORT_COUNTING):
        for mode in math_modes(fs, 2):
            sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, ref_quirks=case.quirks, sort_mode=sort, math_mode=mode, track=4)
            sim.upload_particles(case.start)
            if case.start_indices is not None:
                sim.upload_start_indices(case.start_indices)
            if case.field is not None:
                sim.upload_force_field(case.field)
            for c, a in enumerate(SC.channel_values(case.n, 4)):
                sim.set_attribute(c, a)
            for step in range(SC.STEPS + 1):
                if step:
                    sim.tick(case.tick)
                seen.append(check(sim, f"{cid} sort {sort} math {mode} step {step}"))
                assert seen[-1]["tick"] == step
            sim.close()
    if cid == SC.NONFINITE_2D:
        assert max(w["nonfinite"] for w in seen if w["tick"]) > 0
    if cid == SC.DROPPED_2D:
        assert max(w["dropped"] for w in seen if w["tick"]) > 0


def _cases_3d():
    from tests import hard_states3d as H3
    return H3.CASE_IDS


@pytest.mark.parametrize("cid", _cases_3d())
def test_after_steps_3d(fs, orc, cid):
    from tests import hard_states3d as H3
    case = H3.case_by_id(fs, orc, cid)
    seen = []
    for mode in math_modes(fs, 3):
        sim = fs.FluidSimulation3D(case.st, device=0, initial_offset=case.off, math_mode=mode, track=2)
        sim.upload_particles(case.start)
        for c, a in enumerate(SC.channel_values(case.n, 2)):
            sim.set_attribute(c, a)
        for step in range(SC.STEPS + 1):
            if step:
                sim.tick(case.tick)
            seen.append(check(sim, f"{cid} math {mode} step {step}"))
        sim.close()
    if cid == SC.NONFINITE_3D:
        assert max(w["nonfinite"] for w in seen if w["tick"]) > 0
    if cid == SC.DROPPED_3D:
        assert max(w["dropped"] for w in seen if w["tick"]) > 0


# ---- 4. every state ----------------------------------------------------------------------------------------------------------------------
def dam(fs, dim, **kw):
    """(handle, tick settings) of a small dam break: 4096 particles in 2D, 12^3 in 3D"""
    if dim == 2:
        st, off, tick = fs.dam_break_2d(4096)
        return fs.FluidSimulation(st, device=0, initial_offset=off, **kw), tick
    st, off, tick = fs.dam_break_3d(1728)
    return fs.FluidSimulation3D(st, device=0, initial_offset=off, **kw), tick


@pytest.mark.parametrize("dim", DIMS)
def test_before_the_first_step(fs, dim):
    sim, _ = dam(fs, dim)
    got = check(sim, f"{dim}D lattice")
    assert got["tick"] == 0 and got["momentum_q"] == (0,) * dim and got["speed2_max"] == 0 and R.kept(got) == got["count"]
    sim.close()


@pytest.mark.parametrize("dim", DIMS)
def test_after_a_partial_upload(fs, dim):
    """after steps the 2D densities live in rho2; a partial upload brings them home and overwrites the first records only"""
    sim, tick = dam(fs, dim)
    for _ in range(2):
        sim.tick(tick)
    before = check(sim, f"{dim}D before the upload")
    part = SC.random_records(dtype_of(fs, dim), 100)
    part["density"][3] = np.nan
    sim.upload_particles(part)
    got = check(sim, f"{dim}D after a partial upload")
    assert got["nonfinite"] == 1 and got["count"] == before["count"] and got["momentum_q"] != before["momentum_q"]
    sim.tick(tick)
    check(sim, f"{dim}D a step after the partial upload")
    sim.close()


def test_with_a_renderer_hand_off_live(fs):
    sim, tick = dam(fs, 2)
    sim.export_handle()                          # switches the live 32-byte view on: the force pass writes the records too
    for step in range(3):
        sim.tick(tick)
        got = check(sim, f"hand-off step {step + 1}")
    assert got["tick"] == 3 and got["momentum_q"] != (0, 0)
    sim.close()


@pytest.mark.parametrize("dim", DIMS)
def test_after_reserve_emit_and_remove(fs, dim):
    """count is the live count, and the channels' stride the new capacity (odd here: the rows are not 8-byte aligned)"""
    sim, tick = dam(fs, dim, track=CHANNELS[dim])
    n0 = sim.particle_count
    for c, a in enumerate(SC.channel_values(n0, CHANNELS[dim])):
        sim.set_attribute(c, a)
    sim.tick(tick)
    sim.reserve(n0 + 1001)
    assert sim.capacity == n0 + 1001
    check(sim, f"{dim}D after reserve")
    extra = SC.random_records(dtype_of(fs, dim), 700)
    extra["position"] *= f32(0.01)
    extra["predicted_position"] = extra["position"]
    sim.emit(extra)
    got = check(sim, f"{dim}D after emit")
    assert got["count"] == n0 + 700 < sim.capacity
    rec = sim.download_particles()
    lo = np.median(rec["position"], axis=0).astype(f32)
    gone = sim.remove_box(lo, (1e9,) * dim)
    got = check(sim, f"{dim}D after remove_box")
    assert 0 < gone < n0 + 700 and got["count"] == n0 + 700 - gone == sim.particle_count
    sim.tick(tick)
    check(sim, f"{dim}D a step later")
    sim.close()


@pytest.mark.parametrize("dim", DIMS)
def test_tracking_enabled_after_some_steps(fs, dim):
    sim, tick = dam(fs, dim)
    for _ in range(2):
        sim.tick(tick)
    assert check(sim, f"{dim}D tracking off")["channels"] == 0
    sim.track(3)
    got = check(sim, f"{dim}D tracking on, channels at the enable's +0")
    assert got["channels"] == 3 and got["attr_min"][:3] == (0, 0, 0) and got["attr_max"][:3] == (0, 0, 0) and got["attr_min"][3] == R.POS_INF
    for c, a in enumerate(SC.channel_values(sim.particle_count, 3)):
        sim.set_attribute(c, a)
    sim.tick(tick)
    assert check(sim, f"{dim}D a step with channels")["attr_dropped"][1] > 0
    sim.untrack()
    assert check(sim, f"{dim}D tracking off again")["channels"] == 0
    sim.close()


# ---- 5. observing only ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_the_calls_only_observe(fs, orc, dim):
    """download, stats twice, download: the same bytes and two equal records; and the steps around them match the oracle exactly
    as the plain parity tests compare them"""
    sim, tick = dam(fs, dim, track=1)
    if dim == 2:
        st, off, _ = fs.dam_break_2d(4096)
        ref = orc.OracleSim(st, off)
    else:
        st, off, _ = fs.dam_break_3d(1728)
        ref = orc.OracleSim3D(st, off)
    fields = ("position", "predicted_position", "velocity", "density")
    for step in range(3):
        sim.tick(tick)
        ref.step(tick)
        a = sim.download_particles()
        ids = sim.particle_ids()
        s1, s2 = sim.stats(), sim.stats()
        b = sim.download_particles()
        assert a.tobytes() == b.tobytes() and s1.to_bytes() == s2.to_bytes() and np.array_equal(ids, sim.particle_ids())
        want = ref.particles()
        assert np.array_equal(b["grid"], want["grid"])
        for fld in fields:
            assert np.array_equal(b[fld].view(np.uint32), want[fld].view(np.uint32)), f"{dim}D step {step + 1}: {fld} differs from the oracle"
        R.assert_same(R.words_of(s1.raw), R.stats(want, [sim.attribute(0)], tick=step + 1), f"{dim}D step {step + 1}: stats of the oracle's records")
    ref.close(); sim.close()


# ---- 6. the device form ------------------------------------------------------------------------------------------------------------------
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
dev = torch.device("cuda", 0)
for dim, size in ((2, 208), (3, 232)):
    if dim == 2:
        st, off, tick = g.dam_break_2d(4096)
        sim = g.FluidSimulation(st, device=0, initial_offset=off, track=2)
    else:
        st, off, tick = g.dam_break_3d(1728)
        sim = g.FluidSimulation3D(st, device=0, initial_offset=off, track=2)
    sim.set_attribute(1, np.linspace(-3.0, 3.0, sim.particle_count).astype(np.float32))
    ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
    with torch.cuda.stream(ext):
        bufs = [torch.full((size // 8,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        for buf in bufs:                       # step, stats, step, stats: no host synchronisation in between
            sim.tick(tick)
            sim.tick(tick)
            sim.stats_device_ptr(buf.data_ptr())
    sim.sync()
    got = [g.Stats.from_bytes(b.cpu().numpy().tobytes()) if dim == 2 else g.Stats3D.from_bytes(b.cpu().numpy().tobytes()) for b in bufs]
    assert [s.tick for s in got] == [2, 4, 6] and got[0].to_bytes() != got[1].to_bytes()
    assert got[2].to_bytes() == sim.stats().to_bytes(), "the device form differs from the blocking form"
    assert got[2].channels == 2 and got[2].count == sim.particle_count
    sim.close()
print("DEVICE_OK")
"""


def test_device_form_into_a_torch_buffer(fs):
    out = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT % {"root": ROOT}], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(fs):
    lib = fs.load_library()
    inv, uns = fs._abi.FS_ERR_INVALID, fs._abi.FS_ERR_UNSUPPORTED
    raw2, raw3 = fs._abi.Stats(), fs._abi.Stats3()
    # 1. NULL handle, whatever else is wrong
    assert lib.fs_stats_read(None, C.byref(raw2)) == inv and lib.fs_stats_read(None, None) == inv
    assert lib.fs_stats_device(None, None) == inv
    assert lib.fs3_stats_read(None, C.byref(raw3)) == inv and lib.fs3_stats_device(None, None) == inv
    # 2. a slab handle, before the NULL out
    st, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    assert lib.fs_stats_read(slab._h, C.byref(raw2)) == uns and lib.fs_stats_read(slab._h, None) == uns
    assert lib.fs_stats_device(slab._h, None) == uns
    assert b"slab" in lib.fs_last_error()
    slab.close()
    # 3. NULL out; a refused call changes nothing
    for dim in DIMS:
        sim, tick = dam(fs, dim)
        sim.tick(tick)
        before = sim.download_particles().tobytes()
        assert sim._fn("stats_read")(sim._h, None) == inv and sim._fn("stats_device")(sim._h, None) == inv
        assert b"null" in lib.fs_last_error()
        assert sim.download_particles().tobytes() == before and sim.tick_count == 1
        check(sim, f"{dim}D after the refusals")
        sim.close()


# ---- 8. tie-ins with the step -------------------------------------------------------------------------------------------------------------
DENSITY_FLOOR = f32(0.1)           # oracle/sph_oracle.cpp: density = max(rho, 0.1) (compute.wgsl:70); sph_oracle3d.cpp likewise


@pytest.mark.parametrize("dim", DIMS)
def test_density_min_is_at_least_the_steps_floor(fs, dim):
    """after an IEEE step from a finite state every density is max(rho, 0.1): density_min cannot be below the floor"""
    sim, tick = dam(fs, dim)
    for _ in range(3):
        sim.tick(tick)
        got = check(sim, f"{dim}D floor")
        assert got["nonfinite"] == 0
        assert np.array([got["density_min"]], dtype=np.uint32).view(f32)[0] >= DENSITY_FLOOR
    sim.close()


def test_diffusion_keeps_the_channel_sum_within_rounding(fs):
    """One channel diffuses over S steps of the 4096-particle dam break.  The exact update conserves sum A where the neighbour
    relation is symmetric (header, "channel diffusion"; ref_quirks = 0 here, so that it is); what the engine adds is rounding.  Per particle and step the update
    A' = A + (g * acc) * u is a sum of at most K <= 64 products accumulated in f32: with |A| <= M every partial sum is below
    K * w * 2M <= 2M in magnitude for a convex update (the conductivity is a quarter of diffusion_limit), so each of the K + 3 roundings errs by
    at most ulp(2M) / 2 = M * 2^-23, and Q adds 2^-21 per value.  The drift of attr_q * 2^-20 is therefore bounded by
        S * n * ((K + 3) * M * 2^-23) + 2 * n * 2^-21.
    With n = 4096, S = 4, M = 100, K = 64: 4 * 4096 * 67 * 100 * 2^-23 + 0.004 < 13.1, against a sum of order n * M / 2.  The
    drift is printed before it is asserted."""
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=False, track=1)
    n, steps, big, k = 4096, 4, 100.0, 64
    rng = np.random.default_rng(4)
    a = rng.uniform(0.0, big, size=n).astype(f32)
    sim.set_attribute(0, a)
    sim.tick(tick)                                # the channel rides along; diffusion off: the sum is exactly the uploaded one
    first = check(sim, "diffusion off")
    assert first["attr_q"][0] == R.q_sum(a)
    rho = float(np.median(sim.download_particles()["density"]))
    sim.set_diffusion(0, 0.25 * fs.FluidSimulation.diffusion_limit(st, tick, rho))
    for _ in range(steps):
        sim.tick(tick)
    got = check(sim, "diffusion on")
    assert (got["attr_min"][0], got["attr_max"][0]) != (first["attr_min"][0], first["attr_max"][0]), "the channel did not diffuse"
    assert got["attr_dropped"][0] == 0
    drift = abs(got["attr_q"][0] - first["attr_q"][0]) * 2.0 ** -20
    bound = steps * n * (k + 3) * big * 2.0 ** -23 + 2 * n * 2.0 ** -21
    print(f"[stats] diffusion: sum {first['attr_q'][0] * 2.0 ** -20:.6f} -> {got['attr_q'][0] * 2.0 ** -20:.6f}, drift {drift:.6f}, bound {bound:.3f}")
    assert drift <= bound
    sim.close()

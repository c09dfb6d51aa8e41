"""CPU companions of tests/test_emit2d_gpu.py (a 2D particle count that changes at run time): the checker of
tests/emit2d_ref.py alone, and the two places where the feature shows without a GPU — the library's exports and the Python
class.  The numpy restatement of the nozzle agrees with a float64 evaluation, removing records from a sorted state leaves it
sorted, the tick alignment and the carried start_indices table each decide a result, and the hard emissions do what they say."""
import numpy as np
import pytest

from tests import emit2d_ref as ER

f32 = np.float32
NEW_SYMBOLS = ["fs_reserve", "fs_capacity", "fs_emit_particles", "fs_emit_nozzle", "fs_remove_in_box", "fs_remove_flagged",
               "fs_track_next_id"]


def test_library_exports_every_new_symbol(fs):
    lib = fs.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libfluidsim_hip.so does not export {name}"
        assert name in fs._abi.PROTOTYPES, f"{name} has no ctypes prototype"


def test_python_class_has_the_new_methods(fs):
    import ctypes as C
    for cls in (fs.FluidSimulation, fs.FluidSimulation3D):       # one mixin serves both handles
        for name in ("reserve", "emit", "emit_nozzle", "remove_box", "remove"):
            assert callable(getattr(cls, name, None)), f"{cls.__name__}.{name}"
        for name in ("capacity", "next_id"):
            assert isinstance(getattr(cls, name, None), property), f"{cls.__name__}.{name}"
    assert C.sizeof(fs.Nozzle) == 40 and C.sizeof(fs.Nozzle3) == 56
    assert fs.FluidSimulation._nozzle is fs.Nozzle and fs.FluidSimulation3D._nozzle is fs.Nozzle3


@pytest.mark.parametrize("nu,nv", [(1, 1), (15, 1), (17, 16), (64, 64)])
def test_nozzle_restatement_agrees_with_float64(nu, nv):
    args = dict(origin=(0.13, -0.21), u=(0.045, 0.004), v=(-0.003, 0.026))
    rec = ER.nozzle_records(velocity=(0.5, 2.0), nu=nu, nv=nv, **args)
    want = ER.nozzle_positions_f64(nu=nu, nv=nv, **args)
    got = rec["position"].astype(np.float64)
    # 2 ulp of the largest magnitude the sum passes through (the two products, the partial sum and the result)
    sa = np.abs((np.arange(nu * nv) % nu + 0.5) - 0.5 * nu)[:, None]
    sb = np.abs((np.arange(nu * nv) // nu + 0.5) - 0.5 * nv)[:, None]
    scale = np.abs(f32(args["origin"]).astype(np.float64))[None, :] + sa * np.abs(f32(args["u"]).astype(np.float64))[None, :] \
        + sb * np.abs(f32(args["v"]).astype(np.float64))[None, :]
    ulp = np.spacing(scale.astype(f32)).astype(np.float64)
    assert (np.abs(got - want) <= 2.0 * ulp).all(), float((np.abs(got - want) / ulp).max())
    assert rec.shape[0] == nu * nv and rec["predicted_position"].tobytes() == rec["position"].tobytes()
    assert (rec["velocity"] == f32([0.5, 2.0])).all() and not rec["density"].any() and not rec["grid"].any()
    assert not np.signbit(rec["density"]).any()


@pytest.mark.parametrize("sort", ER.SORTS)
def test_removal_leaves_a_sorted_state_sorted(fs, sort):
    chk, tick, st, off = ER.jittered_scene(fs, 1764, sort=sort)
    chk.step(tick)
    kill = np.random.default_rng(2).random(chk.n) < 0.4
    ids = np.arange(chk.n)[~kill]
    before = chk.rec.copy()
    assert (np.diff(before["grid"].astype(np.int64)) >= 0).all()
    assert chk.remove(kill) == int(kill.sum())
    assert (np.diff(chk.rec["grid"].astype(np.int64)) >= 0).all()
    assert chk.rec.tobytes() == before[ids].tobytes(), "survivors keep their relative order"
    chk.close()


def test_box_edges_are_inclusive_and_nan_is_kept():
    rec = np.zeros(4, dtype=ER.DTYPE)
    rec["position"] = f32([[0, 0], [1, 1], [0.5, np.nan], [1, np.nextafter(f32(1), f32(2))]])
    assert ER.kill_box(rec, (0, 0), (1, 1)).tolist() == [True, True, False, False]


def test_the_tick_alignment_decides_the_coincident_pair(fs):
    """The same state stepped on an oracle whose tick counter was not advanced differs: the alignment is not vacuous."""
    from oracle import oracle as O
    chk, tick, st, off = ER.jittered_scene(fs, 1764)
    chk.step(tick)
    chk.emit(ER.hard_records("coincident", chk.rec, st))
    start, table = chk.rec.copy(), chk.start.copy()
    aligned = chk.step(tick)
    fresh = O.OracleSim(chk.settings(start.shape[0]), off)
    fresh.set_particles(start)
    fresh.start_indices_view()[:] = table
    fresh.step(tick)
    assert fresh.tick_count == 1 and chk.ticks == 2
    assert fresh.particles()["velocity"].tobytes() != aligned["velocity"].tobytes()
    fresh.close(); chk.close()


def quirk_case(fs, sort="bitonic", ref_quirks=True):
    """-> (checker one step in, tick, the kill flags): the first 60 % of the cell-sorted state, i.e. every low cell.  The cell
    that then holds slot 0 had its start written at an index >= 0.6 n by the step before; the table is never cleared and the
    reference never writes the start of slot 0's cell, so the next step walks that cell from a start >= the new count."""
    chk, tick, st, off = ER.jittered_scene(fs, 1764, sort=sort, ref_quirks=ref_quirks)
    chk.step(tick)
    kill = np.arange(chk.n) < (chk.n * 6) // 10
    return chk, tick, kill


def test_the_carried_start_table_decides_a_density(fs):
    from oracle import oracle as O
    chk, tick, kill = quirk_case(fs)
    chk.remove(kill)
    start, table = chk.rec.copy(), chk.start.copy()
    carried = chk.step(tick).copy()
    cell0 = carried["grid"][0]                       # the cell of sorted slot 0 in the step after the removal
    assert table[cell0] >= chk.n, "the stale start of slot 0's cell names a slot behind the live count"
    assert chk.start[cell0] == table[cell0], "and the step did not write it (compute.wgsl:50)"
    fresh = O.OracleSim(chk.settings(chk.n), chk.offset)                 # a zeroed table: what not carrying it would mean
    fresh.step(tick)
    fresh.set_particles(start)
    fresh.step(tick)
    clean = fresh.particles()
    assert clean["grid"].tobytes() == carried["grid"].tobytes()
    differ = np.flatnonzero(clean["density"] != carried["density"])
    assert differ.shape[0] > 0, "the stale start hides the cell's particles from the walk: densities change"
    assert (carried["density"][differ] < clean["density"][differ]).all(), "hidden neighbours only lower a density"
    fresh.close(); chk.close()


def test_without_the_quirk_the_table_carries_nothing(fs):
    from oracle import oracle as O
    chk, tick, kill = quirk_case(fs, ref_quirks=False)
    chk.remove(kill)
    start = chk.rec.copy()
    carried = chk.step(tick)
    fresh = O.OracleSim(chk.settings(chk.n), chk.offset, ref_quirks=False)
    fresh.step(tick)
    fresh.set_particles(start)
    fresh.step(tick)
    assert fresh.particles().tobytes() == carried.tobytes()
    fresh.close(); chk.close()


# ---- the hard emissions do what they say -------------------------------------------------------------------------------------
def emitted_case(fs, name):
    """-> (checker one step after the emission, the emitted records, the state they met, tick, settings)"""
    chk, tick, st, off = ER.jittered_scene(fs, 1764)
    chk.step(tick)
    before = chk.rec.copy()
    rec = ER.hard_records(name, before, st)
    chk.emit(rec)
    chk.step(tick)
    return chk, rec, before, tick, st


def half_box(st):
    return f32([st.size.x, st.size.y]) * f32(0.5)


def test_coincident_emission_is_a_pair_at_distance_zero(fs):
    chk, rec, before, tick, st = emitted_case(fs, "coincident")
    k = before.shape[0] // 2
    assert rec["position"].tobytes() == before["position"][k].tobytes() and rec["velocity"].tobytes() == before["velocity"][k].tobytes()
    pred = chk.rec["predicted_position"]
    _, inverse, counts = np.unique(pred, axis=0, return_inverse=True, return_counts=True)
    assert (counts == 2).sum() == 1 and counts.max() == 2, "exactly one pair shares its predicted position: dst == 0"
    chk.close()


def test_emission_outside_the_box_takes_the_clamp(fs):
    chk, rec, before, tick, st = emitted_case(fs, "outside")
    half = half_box(st)
    assert all(abs(rec["position"][a, a]) > half[a] for a in range(2))
    assert (np.abs(chk.rec["position"]) <= half[None, :]).all()
    chk.close()


def test_emission_on_plus_b_is_on_the_wall(fs):
    chk, rec, before, tick, st = emitted_case(fs, "on_plus_b")
    assert rec["position"][0].tobytes() == half_box(st).tobytes()
    gw, gh = chk.grid_dims
    assert chk.rec["grid"].max() < gw * gh, "the cell of +b lies inside the grid"
    chk.close()


def test_emission_with_a_nan_velocity_meets_the_nan_reset(fs):
    chk, rec, before, tick, st = emitted_case(fs, "nan_velocity")
    assert np.isnan(rec["velocity"]).sum() == 1
    assert np.isfinite(chk.rec["velocity"]).all(), "the step's NaN reset cleared the velocity"
    chk.close()


def test_emission_into_the_extreme_cells_is_alone_there(fs):
    chk, rec, before, tick, st = emitted_case(fs, "extreme_cells")
    grid = chk.rec["grid"]
    assert (np.diff(grid.astype(np.int64)) >= 0).all()
    assert grid[-1] > grid[-2] and grid[0] < grid[1], "alone in the highest and in the lowest occupied cell"
    assert grid[-1] > before["grid"].max() and grid[0] < before["grid"].min()
    chk.close()


# ---- the counting sort's scratch layout, on the CPU under the host sanitizers ------------------------------------------------
def test_scratch_layout_by_the_capacity_under_the_host_sanitizers(tmp_path):
    """tests/emit2d_host_check.cpp: a stand-alone program over the product's csrc/fs_csort_layout.h, built with AddressSanitizer
    and UBSan.  Every region inside the allocated words, none overlapping; laid out by the capacity the histogram, the ticket
    and the look-back words keep the state DESIGN.md §22 argues for across count changes and a reserve; laid out by the count
    the next step's ticket word holds former sort data."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "emit2d_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "emit2d_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "emit2d host check ok" in out.stdout

"""The 2D moving bodies and their loads (k_bodies, k_bodies_loads, both with and without the AOS store) at the
hard inputs of the plain 2D step and at the operator's own operand guards.  The cases and their reference are those of
tests/body_cases2d.py; tests/test_bodies_hard_inputs.py shows without a GPU that the cases reach what they name.  Every
comparison is of bytes or of integers.  Where the reference's records hold a NaN the comparison is
handle_helpers._same_but_nan_bits: a NaN in the same component (inf - inf has no defined sign or payload), exact everywhere else."""
import ctypes as C

import numpy as np
import pytest

from tests import body_cases2d as BC
from tests import body_loads2d_ref as L
from tests.handle_helpers import _add, _same, _same_but_nan_bits, _size

pytestmark = pytest.mark.gpu
MODES = {"ieee": "FS_MATH_IEEE", "ulp": "FS_MATH_WGSL_ULP", "tolerance": "FS_MATH_TOLERANCE"}


def _sort(fs, name):
    return fs.FS_SORT_COUNTING if name == "counting" else fs.FS_SORT_BITONIC


def _words(sim, count):
    return [sim.body_loads(k).words() for k in range(count)]


def _compare(got, want, ctx):
    (_same_but_nan_bits if BC.has_nan(want) else _same)(got, want, ctx)


def _exported(fs, sim, view):
    out = np.empty(sim.particle_count, dtype=fs.PARTICLE_DTYPE)
    assert sim._lib.fs_import_read(C.c_void_p(view), 0, out.ctypes.data_as(C.c_void_p), out.shape[0] * 32) == fs._abi.FS_OK
    return out


# ---- a. the registry --------------------------------------------------------------------------------------------------------
def _engine(fs, run, loads, aos):
    """(handle, the exported view's device address or None) of a case with the run's bodies, poses not yet set"""
    case = run.case
    sim = fs.FluidSimulation(case.st, device=0, initial_offset=case.off, ref_quirks=case.quirks, sort_mode=_sort(fs, case.sort))
    sim.upload_particles(case.start)
    if case.start_indices is not None:
        sim.upload_start_indices(case.start_indices)
    if case.field is not None:
        sim.upload_force_field(case.field)
    for k, (field, extent) in enumerate(zip(run.fields, run.extents)):
        assert sim.add_body(field, extent) == k
    if loads:
        sim.enable_body_loads()
    view = None
    if aos:
        sim.export_handle()
        view = sim.particles_device_ptr()
    return sim, view


def _step(sim, run, k):
    for slot, b in enumerate(run.steps[k].bodies):
        sim.set_body_motion(slot, *b.motion())
    sim.tick(run.case.tick)


def _run_registry(fs, orc, cid, aos):
    run = BC.registry_run(fs, orc, cid)
    count = len(run.names)
    seen = {}
    for loads in (False, True):
        sim, view = _engine(fs, run, loads, aos)
        seen[loads] = []
        for k, step in enumerate(run.steps):
            ctx = f"{cid} step {k + 1} loads {int(loads)} aos {int(aos)}"
            _step(sim, run, k)
            got = sim.download_particles()
            _compare(got, step.rec, ctx)
            assert np.array_equal(sim.download_start_indices(), step.start), f"{ctx}: start_indices"
            if loads:
                assert _words(sim, count) == step.acc, f"{ctx}: words"
            if aos:
                # the download reads this same view, so _compare above saw the AoS stores; the next step reads the SoA stores,
                # and those of the last step are read at the end
                assert _exported(fs, sim, view).tobytes() == got.tobytes(), f"{ctx}: the exported records"
            seen[loads].append(got)
        sim.close()
    for k, (a, b) in enumerate(zip(seen[False], seen[True])):
        assert a.tobytes() == b.tobytes(), f"{cid} step {k + 1} aos {int(aos)}: loads on against loads off"
    # once more with loads on and nothing read between the steps
    sim, view = _engine(fs, run, True, aos)
    for k in range(len(run.steps)):
        _step(sim, run, k)
    assert _words(sim, count) == run.steps[-1].acc, f"{cid}: words, nothing read between the steps"
    assert sim.download_particles().tobytes() == seen[True][-1].tobytes(), f"{cid}: nothing read between the steps"
    sim.close()
    if aos:
        # the SoA stores of the AOS instantiations after the last step: one more plain step of every handle reads them
        for loads in (False, True):
            outs = []
            for with_view in (False, True):
                sim, _ = _engine(fs, run, loads, with_view)
                for k in range(len(run.steps)):
                    _step(sim, run, k)
                for slot in range(count):
                    sim.remove_body(slot)
                sim.tick(run.case.tick)
                outs.append(sim.download_particles().tobytes())
                sim.close()
            assert outs[0] == outs[1], f"{cid} loads {int(loads)}: a body-less step after the last one, with and without the view"


@pytest.mark.parametrize("cid", BC.CASE_IDS)
def test_registry(fs, orc, cid):
    _run_registry(fs, orc, cid, False)


@pytest.mark.parametrize("cid", BC.AOS_IDS)
def test_registry_with_the_live_aos_view(fs, orc, cid):
    _run_registry(fs, orc, cid, True)


# ---- b. the operator's own guards -------------------------------------------------------------------------------------------
def _one_step(fs, st, off, mode, p, tick, bodies=(), loads=False, aos=False):
    """one step of the uploaded state: (records, words or None, start_indices, the records after a second step).  With the view
    exported a download reads the AoS records; the second step reads what the first one stored in the SoA arrays."""
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, math_mode=getattr(fs, MODES[mode]))
    sim.upload_particles(p)
    _add(sim, bodies)
    if loads:
        sim.enable_body_loads()
    view = None
    if aos:
        sim.export_handle()
        view = sim.particles_device_ptr()
    sim.tick(tick)
    got = sim.download_particles()
    words = _words(sim, len(bodies)) if loads else None
    starts = sim.download_start_indices()
    if aos:
        assert _exported(fs, sim, view).tobytes() == got.tobytes(), "the exported records"
    sim.tick(tick)
    again = sim.download_particles()
    sim.close()
    return got, words, starts, again


def _all_forms(fs, st, off, mode, p, tick, make, ctx, check=None):
    """the body-less handle's step, the reference on it, and the four forms of the pass against that reference"""
    after, _, starts, _ = _one_step(fs, st, off, mode, p, tick)
    with np.errstate(all="ignore"):
        bodies, want, want_words, recs = make(after)
        if check:
            print(f"[bodies2d hard inputs] {ctx}: {check(after, want, want_words, recs)}")
    outs, second = [], []
    for loads in (False, True):
        for aos in (False, True):
            got, words, st_idx, again = _one_step(fs, st, off, mode, p, tick, bodies, loads, aos)
            second.append(again.tobytes())
            _compare(got, want, f"{ctx} loads {int(loads)} aos {int(aos)}")
            assert np.array_equal(st_idx, starts), f"{ctx}: start_indices is not touched"
            if loads:
                assert words == want_words, f"{ctx} aos {int(aos)}: words"
            outs.append(got.tobytes())
    assert len(set(outs)) == 1, f"{ctx}: the four forms agree on every byte"
    assert len(set(second)) == 1, f"{ctx}: and after a second step, which reads the SoA arrays the first one stored"


@pytest.mark.parametrize("name", BC.GUARD_IDS)
def test_guard(fs, orc, name):
    st, off, tick, base = BC.guard_base(fs, orc)
    g = BC.GUARDS[name]
    tk = g.tick(tick)
    _all_forms(fs, st, off, "ieee", g.upload(base), tk, lambda after: g.reference(after, _size(st), tk), f"guard {name}", g.check)


@pytest.mark.parametrize("mode", ["ulp", "tolerance"])
def test_guard_in_the_other_math_modes(fs, orc, mode):
    """the operator is the same IEEE operator there: B of that mode's own body-less step"""
    st, off, tick, base = BC.guard_base(fs, orc)
    g = BC.GUARDS[BC.MODE_GUARD]
    tk = g.tick(tick)
    _all_forms(fs, st, off, mode, g.upload(base), tk, lambda after: g.reference(after, _size(st), tk), f"guard {g.name} {mode}", g.check)


# ---- c. the loads over more than 64 workgroups ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BC.MANY_WORKGROUPS)
def test_more_workgroups_than_shard_rows(fs, orc, n):
    """k_bodies_loads folds blockIdx % 64 rows: 66 and 130 workgroups, so a row receives two and three of them, and the odd
    count's last particle sits alone in the last one"""
    st, off, tick, p = BC.many_state(fs, orc, n)

    def make(after):
        bodies = BC.many_bodies(_size(st))
        want, words, recs = L.apply_bodies(after, bodies, _size(st), tick.damping_factor)
        assert words[0][3] == n and recs[0]["clamped"].any()
        return bodies, want, words, recs

    _all_forms(fs, st, off, "ieee", p, tick, make, f"{n} particles")

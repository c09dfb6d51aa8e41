"""The 3D moving bodies and their loads (k3_bodies, k3_bodies_loads) at the hard inputs of the plain 3D step
and at the operator's own operand guards.  The cases and their reference are those of tests/body_cases3d.py;
tests/test_bodies_hard_inputs.py shows without a GPU that the cases reach what they name.  Every comparison is of bytes or of
integers.  Where the reference's records hold a NaN the comparison is handle_helpers._same_but_nan_bits: a NaN in the same
component (inf - inf has no defined sign or payload), exact everywhere else."""
import numpy as np
import pytest

from tests import body_cases3d as BC
from tests.handle_helpers import _add, _same, _same_but_nan_bits, _size

pytestmark = pytest.mark.gpu
MODES = {"ieee": "FS_MATH_IEEE", "tolerance": "FS_MATH_TOLERANCE"}


def _words(sim, count):
    return [sim.body_loads(k).words() for k in range(count)]


def _compare(got, want, ctx):
    (_same_but_nan_bits if BC.has_nan(want) else _same)(got, want, ctx)


def _bytes(rec):
    """the compared fields of 3D records (`pad` is not defined)"""
    return b"".join(np.ascontiguousarray(rec[name]).tobytes() for name in rec.dtype.names if name != "pad")


# ---- a. the registry --------------------------------------------------------------------------------------------------------
def _engine(fs, run, loads):
    case = run.case
    sim = fs.FluidSimulation3D(case.st, device=0, initial_offset=case.off)
    sim.upload_particles(case.start)
    for k, (field, extent) in enumerate(zip(run.fields, run.extents)):
        assert sim.add_body(field, extent) == k
    if loads:
        sim.enable_body_loads()
    return sim


def _step(sim, run, k):
    for slot, b in enumerate(run.steps[k].bodies):
        sim.set_body_motion(slot, *b.motion())
    sim.tick(run.case.tick)


@pytest.mark.parametrize("cid", BC.CASE_IDS)
def test_registry(fs, orc, cid):
    run = BC.registry_run(fs, orc, cid)
    count = len(run.names)
    seen = {}
    for loads in (False, True):
        sim = _engine(fs, run, loads)
        seen[loads] = []
        for k, step in enumerate(run.steps):
            ctx = f"{cid} step {k + 1} loads {int(loads)}"
            _step(sim, run, k)
            got = sim.download_particles()
            _compare(got, step.rec, ctx)
            if loads:
                assert _words(sim, count) == step.acc, f"{ctx}: words"
            seen[loads].append(got)
        sim.close()
    for k, (a, b) in enumerate(zip(seen[False], seen[True])):
        assert _bytes(a) == _bytes(b), f"{cid} step {k + 1}: loads on against loads off"
    # once more with loads on and nothing read between the steps
    sim = _engine(fs, run, True)
    for k in range(len(run.steps)):
        _step(sim, run, k)
    assert _words(sim, count) == run.steps[-1].acc, f"{cid}: words, nothing read between the steps"
    assert _bytes(sim.download_particles()) == _bytes(seen[True][-1]), f"{cid}: nothing read between the steps"
    sim.close()


# ---- b. the operator's own guards -------------------------------------------------------------------------------------------
def _one_step(fs, st, off, mode, p, tick, bodies=(), loads=False):
    sim = fs.FluidSimulation3D(BC.guard_engine_settings(fs), device=0, initial_offset=off, math_mode=getattr(fs, MODES[mode]))
    sim.reserve(BC.GUARD_CAPACITY)
    sim.upload_particles(p[:-1])
    sim.emit(p[-1:])                                                   # 4097: one lane in the last workgroup
    assert sim.particle_count == p.shape[0] == BC.GUARD_N
    _add(sim, bodies)
    if loads:
        sim.enable_body_loads()
    sim.tick(tick)
    got = sim.download_particles()
    words = _words(sim, len(bodies)) if loads else None
    sim.close()
    return got, words


def _both_forms(fs, orc, name, mode, check):
    st, off, tick, base = BC.guard_base(fs, orc)
    g = BC.GUARDS[name]
    tk = g.tick(tick)
    p = g.upload(base)
    ctx = f"guard {name} {mode}"
    after, _ = _one_step(fs, st, off, mode, p, tk)
    with np.errstate(all="ignore"):
        bodies, want, want_words, recs = g.reference(after, _size(st), tk)
        if check:
            print(f"[bodies3d hard inputs] {ctx}: {g.check(after, want, want_words, recs)}")
    outs = []
    for loads in (False, True):
        got, words = _one_step(fs, st, off, mode, p, tk, bodies, loads)
        _compare(got, want, f"{ctx} loads {int(loads)}")
        if loads:
            assert words == want_words, f"{ctx}: words"
        outs.append(_bytes(got))
    assert outs[0] == outs[1], f"{ctx}: the two forms agree on every byte"


@pytest.mark.parametrize("name", BC.GUARD_IDS)
def test_guard(fs, orc, name):
    _both_forms(fs, orc, name, "ieee", True)


def test_guard_in_tolerance_mode(fs, orc):
    """the operator is the same IEEE operator there: B of that mode's own body-less step"""
    _both_forms(fs, orc, BC.MODE_GUARD, "tolerance", True)

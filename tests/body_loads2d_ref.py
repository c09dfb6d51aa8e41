"""CPU statement of the 2D body loads (include/fluidsim.h "2D body loads"), written from the header's text and
from nothing in the kernel: on the operator B of "2D moving bodies" (tests/bodies2d_ref.apply_body_record: its one statement,
with v0, v1, s, the hit mask and the re-clamp mask of every hit) the header's three lines per hit, the fixed-point Q, the five checker words as exact
Python-int sums modulo 2^64, and the run of the shared scene (tests/bodies2d_ref.Scene) with its words per step.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import bodies2d_ref as B
from tests.bodies2d_ref import apply_body_record as apply_body      # (new records, rec)

f32 = np.float32
SHIFT = 20
MOD = 1 << 64
LIMIT = f32(16384.0)


def contributions(rec):
    """(j.x, j.y, tz) of every hit, float32 [hits]: the header's three lines"""
    with np.errstate(all="ignore"):
        jx = rec["v0"][:, 0] - rec["v1"][:, 0]
        jy = rec["v0"][:, 1] - rec["v1"][:, 1]
        t0 = rec["s"][:, 0] * jy
        t1 = rec["s"][:, 1] * jx
        tz = t0 - t1
    return jx.astype(f32), jy.astype(f32), tz.astype(f32)


def in_range(x):
    """the drop rule's test of one value: not NaN and fabsf(x) < 2^14"""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(x, dtype=f32)) < LIMIT            # NaN: False


def Q(x):
    """the integers nearest to x * 2^20, ties to even, as a list of Python ints; x float32, every value in range"""
    x = np.asarray(x, dtype=f32).reshape(-1)
    assert in_range(x).all()
    return [int(y) for y in np.rint(x.astype(np.float64) * 2 ** SHIFT)]


def is_tie(x):
    """values whose x * 2^20 lies exactly half way between two integers"""
    y = np.asarray(x, dtype=f32).astype(np.float64) * 2 ** SHIFT
    return np.abs(y - np.trunc(y)) == 0.5


def words(rec, want_ties=False):
    """The five checker words of one body and one step, Python ints modulo 2^64: sum Q(j.x), sum Q(j.y), sum Q(tz), hits,
    dropped.  With want_ties also the number of contributions (of kept hits) that are exact ties."""
    jx, jy, tz = contributions(rec)
    keep = in_range(jx) & in_range(jy) & in_range(tz)
    out = [sum(Q(a[keep])) % MOD for a in (jx, jy, tz)] + [int(jx.shape[0]), int((~keep).sum())]
    if want_ties:
        return out, int(sum(is_tie(a[keep]).sum() for a in (jx, jy, tz)))
    return out


def signed(word):
    """a word modulo 2^64 as the int64 it stands for"""
    return word - MOD if word >= MOD // 2 else word


def add_words(a, b):
    return [(x + y) % MOD for x, y in zip(a, b)]


ZERO = [0, 0, 0, 0, 0]


def apply_bodies(records, bodies, size, damping):
    """B_last(... B_first(records)) in the order given: (new records, the five words per body, the per-body records)"""
    out_words, recs = [], []
    for body in bodies:
        records, rec = apply_body(records, body, size, damping)
        out_words.append(words(rec))
        recs.append(rec)
    return records, out_words, recs


_RUNS = {}


def scene_run(fs, orc, side, sort="bitonic", steps=40, keep=(1, 2, 3, 4, 5, 6, 7, 8, 40)):
    """bodies2d_ref.oracle_run's scene with the restated operator: {"snap": {step: records}, "words": [steps][3] lists of five
    ints (per step, not accumulated), and for the kept steps "before": {step: the oracle's records before the bodies} and "recs":
    {step: the three per-body records}, "scene"}; computed once."""
    key = (side, sort, steps, tuple(keep))
    if key not in _RUNS:
        sc = B.Scene(fs, side)
        bodies = sc.bodies()
        ref = orc.OracleSim(sc.st, initial_offset=sc.off)
        snap, per_step, recs, before = {}, [], {}, {}
        for s in range(1, steps + 1):
            ref.step(sc.tick, stable_sort=sort == "counting")
            if s in keep:
                before[s] = ref.particles().copy()
            rec, w, rr = apply_bodies(ref.particles(), sc.set_motions(bodies, s), sc.size, sc.tick.damping_factor)
            ref.set_particles(rec)
            per_step.append(w)
            if s in keep:
                snap[s] = rec
                recs[s] = rr
        ref.close()
        for r in list(snap.values()) + list(before.values()):
            r.setflags(write=False)
        _RUNS[key] = {"snap": snap, "words": per_step, "recs": recs, "before": before, "scene": sc}
    return _RUNS[key]


def accumulated(per_step, upto):
    """the words of each body summed over steps 1 .. upto"""
    acc = [ZERO] * len(per_step[0])
    for w in per_step[:upto]:
        acc = [add_words(a, b) for a, b in zip(acc, w)]
    return acc

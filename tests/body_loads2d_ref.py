"""CPU statement of the 2D body loads (include/fluidsim.h "2D body loads"), written from the header's text and
from nothing in the kernel: the operator B of "2D moving bodies" restated in numpy float32, one f32 operation per line, with what
the loads need of every hit (v0, v1, s, the hit mask, the re-clamp mask), the fixed-point Q, the five checker words as exact
Python-int sums modulo 2^64, and the run of the shared scene (tests/bodies2d_ref.Scene) with its words per step.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import bodies2d_ref as B
from tests import collide3d_ref as CR

f32 = np.float32
SHIFT = 20
MOD = 1 << 64
LIMIT = f32(16384.0)


def apply_body(records, body, size, damping):
    """B(records) with the load outputs: (new records, rec) — rec["hit"]: bool per particle; per HIT, in particle order:
    rec["v0"], rec["v1"], rec["s"] float32 [hits, 2] and rec["clamped"] bool [hits]."""
    field = body.field
    H, W = field.shape[:2]
    out = records.copy()
    p = out["position"].astype(f32)
    v = out["velocity"].astype(f32)
    b = np.array([f32(s) for s in size], dtype=f32) * f32(0.5)
    damping = f32(damping)
    c, r, u, w, ext = body.centre, body.rot, body.velocity, body.angular_velocity, body.extent
    r00, r01, r10, r11 = (f32(x) for x in r)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = p[:, 0] - c[0]
        dy = p[:, 1] - c[1]
        t0 = r00 * dx
        t1 = r10 * dy
        qx = t0 + t1
        t0 = r01 * dx
        t1 = r11 * dy
        qy = t0 + t1
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1])
        idx = []
        for a, (q, wa) in enumerate(((qx, W), (qy, H))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            idx.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
        g = field[idx[1], idx[0]]
        nz = (g[:, 0] != 0) | (g[:, 1] != 0)
        t0 = g[:, 0] * g[:, 0]
        t1 = g[:, 1] * g[:, 1]
        ln = np.sqrt(t0 + t1)
        hit = inside & nz & (ln > f32(0))
        g, ln, ph, vh = g[hit], ln[hit], p[hit], v[hit]
        v0 = vh.copy()                                  # the velocity on entry to this operator
        t0 = r00 * g[:, 0]
        t1 = r01 * g[:, 1]
        fx = t0 + t1
        t0 = r10 * g[:, 0]
        t1 = r11 * g[:, 1]
        fy = t0 + t1
        nx = fx / ln
        ny = fy / ln
        px = ph[:, 0] + fx
        py = ph[:, 1] + fy
        sx = px - c[0]
        sy = py - c[1]
        t0 = w * sy
        usx = u[0] - t0
        t0 = w * sx
        usy = u[1] + t0
        rx = vh[:, 0] - usx
        ry = vh[:, 1] - usy
        t0 = rx * nx
        t1 = ry * ny
        rn = t0 + t1
        k = (f32(1.0) - damping) * rn
        t0 = k * nx
        t0 = rx - t0
        vx = usx + t0
        t0 = k * ny
        t0 = ry - t0
        vy = usy + t0
        ph = np.stack([px, py], axis=1).astype(f32).reshape(-1, 2)
        vh = np.stack([vx, vy], axis=1).astype(f32).reshape(-1, 2)
        v1 = vh.copy()                                  # before the wall re-clamp
        s = np.stack([sx, sy], axis=1).astype(f32).reshape(-1, 2)
        clamped = np.zeros(ph.shape[0], dtype=bool)
        for a in range(2):
            over = np.abs(ph[:, a]) > b[a]
            ph[over, a] = b[a] * np.sign(ph[over, a])
            vh[over, a] = vh[over, a] * (f32(-1.0) * damping)
            clamped |= over
    p[hit] = ph
    v[hit] = vh
    out["position"] = p
    out["velocity"] = v
    return out, {"hit": hit, "v0": v0, "v1": v1, "s": s, "clamped": clamped}


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

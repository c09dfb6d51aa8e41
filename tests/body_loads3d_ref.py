"""CPU statement of the 3D body loads (include/fluidsim.h "3D body loads"), written from the header's text and
from nothing in the kernel: the operator B of "3D moving bodies" restated so that it also returns v0, v1, s, the hit mask and the
re-clamp mask of every hit (pinned against tests/bodies3d_ref.apply_body by tests/test_body_loads3d.py), the header's lines per
hit, the eight checker words as exact Python-int sums modulo 2^64, and the run of the shared scene (tests/bodies3d_ref.Scene)
with its words per step.  Q, the drop rule's test and the word arithmetic are the dimension-free helpers of
tests/body_loads2d_ref.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import bodies3d_ref as B
from tests import collide3d_ref as CR
from tests.body_loads2d_ref import MOD, Q, add_words, in_range, is_tie, signed  # noqa: F401

f32 = np.float32
ZERO = [0] * 8


def apply_body_record(records, body, size, damping):
    """B(records) as bodies3d_ref.apply_body computes it, one f32 operation per line: (new records, rec) with rec = {"hit": bool
    [n], "v0", "v1", "s": float32 [hits, 3], "clamped": bool [hits]} — the velocity on entry, the velocity the operator computed
    before its wall re-clamp, the pushed position relative to the centre before the re-clamp."""
    field = body.field
    D, H, W = field.shape[:3]
    out = records.copy()
    p = out["position"].astype(f32)
    v = out["velocity"].astype(f32)
    b = np.array([f32(s) for s in size], dtype=f32) * f32(0.5)
    damping = f32(damping)
    c, r, u, w, ext = body.centre, body.rot, body.velocity, body.angular_velocity, body.extent
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (f32(x) for x in r)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = p[:, 0] - c[0]
        dy = p[:, 1] - c[1]
        dz = p[:, 2] - c[2]
        qx = (r00 * dx + r10 * dy) + r20 * dz
        qy = (r01 * dx + r11 * dy) + r21 * dz
        qz = (r02 * dx + r12 * dy) + r22 * dz
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1]) & (np.abs(qz) <= hb[2])
        idx = []
        for a, (q, wa) in enumerate(((qx, W), (qy, H), (qz, D))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            idx.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
        g = field[idx[2], idx[1], idx[0]]
        nz = (g[:, 0] != 0) | (g[:, 1] != 0) | (g[:, 2] != 0)
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        hit = inside & nz & (ln > f32(0))
        g, ln, ph, v0 = g[hit], ln[hit], p[hit], v[hit].copy()
        fx = (r00 * g[:, 0] + r01 * g[:, 1]) + r02 * g[:, 2]
        fy = (r10 * g[:, 0] + r11 * g[:, 1]) + r12 * g[:, 2]
        fz = (r20 * g[:, 0] + r21 * g[:, 1]) + r22 * g[:, 2]
        nx = fx / ln
        ny = fy / ln
        nz_ = fz / ln
        px = ph[:, 0] + fx
        py = ph[:, 1] + fy
        pz = ph[:, 2] + fz
        sx = px - c[0]
        sy = py - c[1]
        sz = pz - c[2]
        usx = u[0] + (w[1] * sz - w[2] * sy)
        usy = u[1] + (w[2] * sx - w[0] * sz)
        usz = u[2] + (w[0] * sy - w[1] * sx)
        rx = v0[:, 0] - usx
        ry = v0[:, 1] - usy
        rz = v0[:, 2] - usz
        rn = (rx * nx + ry * ny) + rz * nz_
        k = (f32(1.0) - damping) * rn
        vx = usx + (rx - k * nx)
        vy = usy + (ry - k * ny)
        vz = usz + (rz - k * nz_)
        ph = np.stack([px, py, pz], axis=1).astype(f32).reshape(-1, 3)
        v1 = np.stack([vx, vy, vz], axis=1).astype(f32).reshape(-1, 3)
        s = np.stack([sx, sy, sz], axis=1).astype(f32).reshape(-1, 3)
        vh = v1.copy()
        clamped = np.zeros(ph.shape[0], dtype=bool)
        for a in range(3):
            over = np.abs(ph[:, a]) > b[a]
            ph[over, a] = b[a] * np.sign(ph[over, a])
            vh[over, a] = vh[over, a] * (f32(-1.0) * damping)
            clamped |= over
    p[hit] = ph
    v[hit] = vh
    out["position"] = p
    out["velocity"] = v
    return out, {"hit": hit, "v0": v0.astype(f32).reshape(-1, 3), "v1": v1, "s": s, "clamped": clamped}


apply_body = apply_body_record


def contributions(rec):
    """(j.x, j.y, j.z, t.x, t.y, t.z) of every hit, float32 [hits] each: the header's lines, two products then one subtraction"""
    v0, v1, s = (np.asarray(rec[k], dtype=f32).reshape(-1, 3) for k in ("v0", "v1", "s"))
    with np.errstate(all="ignore"):
        jx = v0[:, 0] - v1[:, 0]
        jy = v0[:, 1] - v1[:, 1]
        jz = v0[:, 2] - v1[:, 2]
        a0 = s[:, 1] * jz
        a1 = s[:, 2] * jy
        tx = a0 - a1
        b0 = s[:, 2] * jx
        b1 = s[:, 0] * jz
        ty = b0 - b1
        c0 = s[:, 0] * jy
        c1 = s[:, 1] * jx
        tz = c0 - c1
    return tuple(a.astype(f32) for a in (jx, jy, jz, tx, ty, tz))


def words(rec, want_ties=False):
    """The eight checker words of one body and one step, Python ints modulo 2^64: sum Q(j.x), sum Q(j.y), sum Q(j.z), sum Q(t.x),
    sum Q(t.y), sum Q(t.z), hits, dropped.  With want_ties also the number of contributions (of kept hits) that are exact ties."""
    six = contributions(rec)
    keep = np.ones(six[0].shape[0], dtype=bool)
    for a in six:
        keep &= in_range(a)
    out = [sum(Q(a[keep])) % MOD for a in six] + [int(six[0].shape[0]), int((~keep).sum())]
    if want_ties:
        return out, int(sum(is_tie(a[keep]).sum() for a in six))
    return out


def apply_bodies(records, bodies, size, damping):
    """B_last(... B_first(records)) in the order given: (new records, the eight words per body, the per-body records)"""
    out_words, recs = [], []
    for body in bodies:
        records, rec = apply_body_record(records, body, size, damping)
        out_words.append(words(rec))
        recs.append(rec)
    return records, out_words, recs


_RUNS = {}


def scene_run(fs, orc, side, static=None, steps=40, keep=(1, 2, 3, 4, 5, 6, 7, 8, 40)):
    """bodies3d_ref.oracle_run's scene with the restated operator over the unchanged OracleSim3D: {"snap": {step: records},
    "words": [steps][3] lists of eight ints (per step, not accumulated), and for the kept steps "before": {step: the records the
    bodies start from — after C when `static` is 'a'} and "recs": {step: the three per-body records}, "scene", "static": the
    static field or None}; computed once."""
    key = (side, static, steps, tuple(keep))
    if key not in _RUNS:
        sc = B.Scene(fs, side)
        field = CR.scene_box_on_floor(sc.size) if static == "a" else None
        bodies = sc.bodies()
        ref = orc.OracleSim3D(sc.st, initial_offset=sc.off)
        snap, per_step, recs, before = {}, [], {}, {}
        for s in range(1, steps + 1):
            ref.step(sc.tick)
            rec = ref.particles()
            if field is not None:
                rec = CR.apply_collider(rec, field, sc.size, sc.tick.damping_factor)[0]
            if s in keep:
                before[s] = rec.copy()
            rec, w, rr = apply_bodies(rec, sc.set_motions(bodies, s), sc.size, sc.tick.damping_factor)
            ref.set_particles(rec)
            per_step.append(w)
            if s in keep:
                snap[s] = rec
                recs[s] = rr
        ref.close()
        for r in list(snap.values()) + list(before.values()):
            r.setflags(write=False)
        _RUNS[key] = {"snap": snap, "words": per_step, "recs": recs, "before": before, "scene": sc, "static": field}
    return _RUNS[key]


def accumulated(per_step, upto):
    """the words of each body summed over steps 1 .. upto"""
    acc = [ZERO] * len(per_step[0])
    for w in per_step[:upto]:
        acc = [add_words(a, b) for a, b in zip(acc, w)]
    return acc
